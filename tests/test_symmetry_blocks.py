"""trx_sym_fold / trx_sym_unfold through the C ABI (emulator + MI355X), DESIGN.md section 7 block-test policy.

Reference: T^H A T and T blockdiag(W_k) in numpy clongdouble from a DENSE T (the kernel never forms T: it gathers rows, then columns).  That T is the
plan's, and the plan itself is held to the definition of the mirrors by test_plan_is_symmetry_basis: the dense R_x = diag(-J_x, +J_x),
R_y = diag(+J_y, -J_y) are built here from their definition (J_x e_(m,n) = exp(+2 pi i m c / nx) e_(-m,n)), independently of the plan.

Bound:  max |out - ref| <= 16 max(e_plain, n eps) max |ref|, e_plain the error of the same dense formulas in the kernel's dtype through numpy
relative to max |ref|, eps = 2^-53 / the fp32 eps.  resid is a modulus of an entry of T^H A T divided by max |A|, so its error is held to the same
bound times max |T^H A T| / max |A|.

Shapes: order [3,2] (n = 70: blocks 35/35 for one mirror, 17/18/18/17 for two -- unequal sizes, m = 0 columns with a single entry) and a circular
order set on L = [300, 200] (unequal x / y extent); batch 1 and 3; c = n - 1 (complex weights) and c = 0 (real weights); both dtypes.
"""
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import crandn

LD = np.clongdouble
NX, NY = 40, 36
SHAPES = [("rect32", "x"), ("rect32", "y"), ("rect32", "xy"), ("circ", "x"), ("circ", "xy")]
GUARD = complex(-7.25, 3.5)


def _eps(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else float(np.finfo(np.float32).eps)


def _orders(kind):
    from torcwa_amd import lattice
    if kind == "rect32":
        return lattice.rect_orders(3, 2)
    mn = lattice.circular_orders([300., 200.], n_harmonics=20)
    assert np.abs(mn[:, 0]).max() != np.abs(mn[:, 1]).max()                          # unequal extent along x and y
    return mn


@functools.lru_cache(maxsize=None)
def _case(kind, sym, c):
    """(plan, T dense clongdouble, [R_x, R_y] dense clongdouble)."""
    from torcwa_amd.symmetry import build_plan
    mn = _orders(kind)
    cx, cy = (NX - 1, NY - 1) if c == "half" else (0, 0)
    plan = build_plan(mn, sym, cx if "x" in sym else 0, NX, cy if "y" in sym else 0, NY)
    N = len(mn)
    pos = {(int(p), int(q)): i for i, (p, q) in enumerate(mn)}
    Jx, Jy = np.zeros((N, N), dtype=LD), np.zeros((N, N), dtype=LD)
    two_pi = 2 * np.arccos(np.longdouble(-1))
    for (m, q), i in pos.items():
        Jx[pos[(-m, q)], i] = np.exp(1j * two_pi * np.longdouble((m * cx) % NX) / NX)
        Jy[pos[(m, -q)], i] = np.exp(1j * two_pi * np.longdouble((q * cy) % NY) / NY)
    Z = np.zeros((N, N), dtype=LD)
    Rx, Ry = np.block([[-Jx, Z], [Z, Jx]]), np.block([[Jy, Z], [Z, -Jy]])
    return plan, plan.dense(LD), (Rx, Ry)


def _commutant(A, Rs):
    """Average of A over the group {I, R_x, R_y, R_x R_y} (clongdouble)."""
    Rx, Ry = Rs
    Rxy = Rx @ Ry
    return (A + Rx @ A @ Rx + Ry @ A @ Ry + Rxy @ A @ Rxy.conj().T) / 4


def _pack(per_block, plan, B):
    """[per block k: [B, ...]] -> the packed flat array of include/trx.h (groups of equal size, block-major, then batch)."""
    return np.concatenate([np.concatenate([per_block[k].reshape(B, -1) for k in ks]).ravel() for _, ks in plan.groups])


def _unpack(flat, plan, B, square):
    out, at = [None] * plan.nblk, 0
    for s, ks in plan.groups:
        u = s * s if square else s
        for k in ks:
            out[k] = flat[at:at + B * u].reshape((B, s, s) if square else (B, s))
            at += B * u
    assert at == len(flat)
    return out


def _plan_dev(be, plan, dtype):
    """Plan arrays with guard words behind them: (idx, wt, off) handles and a check that the call left them alone."""
    idx = np.concatenate([plan.idx.ravel(), np.full(4, -99, dtype=np.int32)])
    wt = np.concatenate([plan.wt.ravel().astype(dtype), np.full(4, GUARD, dtype=dtype)])
    off = np.concatenate([np.asarray(plan.off, dtype=np.int32), np.full(4, -99, dtype=np.int32)])
    hs = [be.dev(a) for a in (idx, wt, off)]

    def untouched():
        return all(np.array_equal(be.host(h), a) for h, a in zip(hs, (idx, wt, off)))
    return hs, untouched


def _fold(be, A, plan, dtype):
    B, n, _ = A.shape
    tot = B * sum(s * s for s in plan.sizes)
    (idx, wt, off), untouched = _plan_dev(be, plan, dtype)
    dA = be.dev(A)
    blocks = be.dev(np.full(tot + 4, GUARD, dtype=dtype))
    resid = be.dev(np.full(B + 2, -3.5, dtype=np.float64))
    nws = be.lib.sym_fold_ws_bytes(dtcode(dtype), n, B)
    assert nws == -(-(16 * -(-n // 8) * B) // 16) * 16 + np.dtype(dtype).itemsize * n * n * B
    ws = be.dev(np.full(nws + 64, 0xA5, dtype=np.uint8))
    rc = be.lib.sym_fold(dtcode(dtype), be.ptr(dA), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, be.ptr(blocks), be.ptr(resid),
                         be.ptr(ws), nws, be.stream)
    assert rc == 0
    o, r, w = be.host(blocks), be.host(resid), be.host(ws)
    assert (o[tot:] == GUARD).all() and (r[B:] == -3.5).all() and (w[nws:] == 0xA5).all()
    assert untouched() and np.array_equal(be.host(dA), A)                            # the plan and A are inputs
    # argument checks
    args = [be.ptr(dA), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off)]
    tail = [be.ptr(blocks), be.ptr(resid), be.ptr(ws)]
    assert be.lib.sym_fold(dtcode(dtype), *args, plan.nblk, *tail, nws - 16, be.stream) == -3
    assert be.lib.sym_fold(dtcode(dtype), *args, 5, *tail, nws, be.stream) == -2
    assert be.lib.sym_fold(7, *args, plan.nblk, *tail, nws, be.stream) == -1
    assert be.lib.sym_fold(dtcode(dtype), None, n, 0, None, None, None, plan.nblk, None, None, None, 0, be.stream) == 0     # batch = 0
    return _unpack(o[:tot], plan, B, True), r[:B]


def _unfold(be, Wk, lamk, plan, B, dtype):
    n = plan.n
    (idx, wt, off), untouched = _plan_dev(be, plan, dtype)
    dW, dl = be.dev(_pack(Wk, plan, B).astype(dtype)), be.dev(_pack(lamk, plan, B).astype(dtype))
    W = be.dev(np.full(B * n * n + 4, GUARD, dtype=dtype))
    lam = be.dev(np.full(B * n + 4, GUARD, dtype=dtype))
    rc = be.lib.sym_unfold(dtcode(dtype), be.ptr(dW), be.ptr(dl), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, be.ptr(W), be.ptr(lam),
                           be.stream)
    assert rc == 0
    w, l = be.host(W), be.host(lam)
    assert (w[B * n * n:] == GUARD).all() and (l[B * n:] == GUARD).all() and untouched()
    assert be.lib.sym_unfold(dtcode(dtype), be.ptr(dW), be.ptr(dl), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off), 0, be.ptr(W), be.ptr(lam), be.stream) == -2
    return w[:B * n * n].reshape(B, n, n), l[:B * n].reshape(B, n)


@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("kind,sym", SHAPES)
def test_plan_is_symmetry_basis(kind, sym, c):
    """The plan's T is unitary, every column is a joint eigenvector of the claimed mirrors with one eigenvalue pair per block, a column has at most
    four entries and the columns of one block have disjoint supports (what trx_sym_unfold relies on)."""
    plan, T, (Rx, Ry) = _case(kind, sym, c)
    n = plan.n
    assert np.abs(T.conj().T @ T - np.eye(n)).max() < 1e-15
    if kind == "rect32":
        assert plan.sizes == ([35, 35] if len(sym) == 1 else [17, 18, 18, 17])
    else:
        assert sum(plan.sizes) == n and (len(sym) == 2 or plan.sizes[0] == plan.sizes[1])
    assert ((plan.wt != 0).sum(axis=1) <= (2 if len(sym) == 1 else 4)).all()
    assert ((plan.wt != 0).sum(axis=1) == 1).any()                                    # the self-paired m = 0 / n = 0 harmonics
    assert (np.iscomplex(plan.wt).any()) == (c == "half")
    for R, name in ((Rx, "x"), (Ry, "y")):
        if name not in sym:
            continue
        RT = R @ T
        for k in range(plan.nblk):
            cols = slice(plan.off[k], plan.off[k + 1])
            ev = {int(np.rint((T[:, j].conj() @ RT[:, j]).real)) for j in range(plan.off[k], plan.off[k + 1])}
            assert len(ev) == 1 and ev <= {1, -1}
            assert np.abs(RT[:, cols] - ev.pop() * T[:, cols]).max() < 1e-15
    for k in range(plan.nblk):
        assert ((np.abs(T[:, plan.off[k]:plan.off[k + 1]]) > 0).sum(axis=1) <= 1).all()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("kind,sym", SHAPES)
@pytest.mark.parametrize("projected", [True, False])
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_fold(backend, projected, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T, Rs = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(100 * n + 10 * B + len(sym) + (c == "half"))
    A = crandn(rng, (B, n, n)).astype(LD)
    if projected:
        A = np.stack([_commutant(a, Rs) for a in A])
    A = A.astype(dtype)                                                               # what the kernel is given
    got, resid = _fold(be, A, plan, dtype)
    Tp = T.astype(dtype)
    worst = 0.0
    for b in range(B):
        D = T.conj().T @ A[b].astype(LD) @ T
        Dp = Tp.conj().T @ A[b] @ Tp
        scale = float(np.abs(D).max())
        tol = 16 * max(float(np.abs(Dp - D).max()) / scale, n * _eps(dtype))
        mask = np.ones((n, n), dtype=bool)
        for k in range(plan.nblk):
            sl = slice(plan.off[k], plan.off[k + 1])
            mask[sl, sl] = False
            err = float(np.abs(got[k][b] - D[sl, sl]).max()) / scale
            worst = max(worst, err / tol)
            assert err <= tol, (b, k, err, tol)
        amax = float(np.abs(A[b]).max())
        ref = float(np.abs(D[mask]).max()) / amax
        print(f"b={b}: resid {resid[b]:.3e}, reference {ref:.3e}, tol {tol:.2e}")
        assert abs(resid[b] - ref) * amax <= tol * scale, (b, resid[b], ref)
        if projected:
            assert resid[b] <= tol, (b, resid[b], tol)                                 # A commutes with the mirrors: nothing is discarded
        else:
            assert resid[b] > 0.1                                                     # a random A does not: the diagnostic measures it
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: worst block error / bound = {worst:.2f}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("kind,sym", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_unfold(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T, _ = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(200 * n + 10 * B + len(sym) + (c == "half"))
    Wk = [crandn(rng, (B, s, s)).astype(dtype) for s in plan.sizes]
    lamk = [crandn(rng, (B, s)).astype(dtype) for s in plan.sizes]
    W, lam = _unfold(be, Wk, lamk, plan, B, dtype)
    assert np.array_equal(lam, np.concatenate(lamk, axis=1))                          # a copy: exact
    Tp = T.astype(dtype)
    for b in range(B):
        bd = np.zeros((n, n), dtype=LD)
        for k in range(plan.nblk):
            sl = slice(plan.off[k], plan.off[k + 1])
            bd[sl, sl] = Wk[k][b]
        ref = T @ bd
        plain = Tp @ bd.astype(dtype)
        scale = float(np.abs(ref).max())
        tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
        err = float(np.abs(W[b] - ref).max()) / scale
        assert err <= tol, (b, err, tol)
        assert (W[b][np.abs(ref) == 0] == 0).all()                                    # rows a block does not reach are exactly zero


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("kind,sym", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_fold_eig_unfold(backend, kind, sym, c, B, dtype):
    """fold -> numpy eig of every block -> unfold gives eigenpairs of A in the original basis: max |A W - W diag(lam)| is held to the residual
    of numpy's eig(A) on the whole matrix under the same policy, and the columns of W keep their unit 2-norm."""
    be = get_backend(backend)
    plan, T, Rs = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(300 * n + 10 * B + len(sym) + (c == "half"))
    A = np.stack([_commutant(a, Rs) for a in crandn(rng, (B, n, n)).astype(LD)]).astype(dtype)
    blocks, _ = _fold(be, A, plan, dtype)
    lamk, Wk = [], []
    for k in range(plan.nblk):
        ev = [np.linalg.eig(blocks[k][b]) for b in range(B)]                          # numpy keeps the dtype and returns unit columns
        lamk.append(np.stack([e[0] for e in ev]).astype(dtype))
        Wk.append(np.stack([e[1] for e in ev]).astype(dtype))
    W, lam = _unfold(be, Wk, lamk, plan, B, dtype)
    for b in range(B):
        Al, Wl = A[b].astype(LD), W[b].astype(LD)
        w, V = np.linalg.eig(A[b])
        amax = float(np.abs(A[b]).max())
        e_plain = float(np.abs(Al @ V.astype(LD) - V.astype(LD) * w.astype(LD)[None, :]).max()) / amax
        tol = 16 * max(e_plain, n * _eps(dtype))
        res = float(np.abs(Al @ Wl - Wl * lam[b].astype(LD)[None, :]).max()) / amax
        print(f"b={b}: residual {res:.2e}, numpy eig(A) {e_plain:.2e}, tol {tol:.2e}")
        assert res <= tol, (b, res, tol)
        norms = np.sqrt((np.abs(Wl) ** 2).sum(axis=0)).astype(np.float64)
        assert np.abs(norms - 1).max() <= tol, (b, np.abs(norms - 1).max())
