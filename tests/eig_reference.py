"""The eigen-reference of the block tests of trx_eig (tests/test_eig_blocks.py); also exported as tests.helpers.eig_hp, next to solve_hp."""
import numpy as np


def eig_hp(A, steps=3):
    """Eigenpairs of A beyond complex128: numpy.linalg.eig of the complex128 rounding of A, then every pair on its own by `steps` of Newton's
    method on  F(x, lam) = [A x - lam x; x_k - 1] = 0  (k = index of the largest component of the start vector), whose Jacobian is the bordered
    matrix [[A - lam I, -x], [e_k^T, 0]].  The residual and the iterate are held in np.clongdouble (eps 1.1e-19); the complex128 bordered matrix
    of the start pair, factored once per pair, only preconditions.  No Schur form and no step on all pairs at once: other algebra than the
    library's.  Returns (lam [n], X [n, n]) in clongdouble, X[k_j, j] = 1; validated against mpmath in
    tests/test_eig_blocks.py::test_eig_hp_against_mpmath.  Limiting accuracy ~ 1e-19 ||A|| / gap; needs simple eigenvalues."""
    from scipy.linalg import lu_factor, lu_solve
    Al = np.asarray(A, dtype=np.clongdouble)
    Ad = Al.astype(np.complex128)
    n = Ad.shape[0]
    w, V = np.linalg.eig(Ad)
    lam, X = w.astype(np.clongdouble), V.astype(np.clongdouble)
    M = np.zeros((n + 1, n + 1), dtype=np.complex128)
    rhs = np.empty(n + 1, dtype=np.clongdouble)
    for j in range(n):
        k = int(np.argmax(np.abs(V[:, j])))
        x, l = X[:, j] / X[k, j], lam[j]
        M[:n, :n] = Ad
        M[np.arange(n), np.arange(n)] -= complex(l)
        M[:n, n] = -x.astype(np.complex128)
        M[n, :] = 0
        M[n, k] = 1
        lu = lu_factor(M, check_finite=False)
        for _ in range(steps):
            rhs[:n] = l * x - Al @ x
            rhs[n] = 1 - x[k]
            d = lu_solve(lu, rhs.astype(np.complex128), check_finite=False).astype(np.clongdouble)
            x, l = x + d[:n], l + d[n]
        X[:, j], lam[j] = x, l
    return lam, X
