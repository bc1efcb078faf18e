"""trx_eig / trx_eig_opts under the block-test policy ("Block tests"): eigenvalues AND eigenvectors against a reference beyond
complex128, with a bound derived from LAPACK's own error against that reference.

Reference: helpers.eig_hp (LAPACK start, then each pair refined by Newton's method on the bordered system with clongdouble residuals; checked
against 40-digit mpmath below), computed from the matrix AS HANDED TO THE KERNEL in its dtype.  Metrics, all evaluated in clongdouble:
  R  max over columns of ||A v - w v||_2 / (||A||_F ||v||_2);
  E  max |w_j - lam_j| / ||A||_F after a one-to-one matching of the computed with the reference eigenvalues (linear_sum_assignment on
     |w_i - lam_j|: optimal, not greedy);
  X  after the same matching, both vectors scaled to 1 at the index of the reference vector's largest entry: max ||v - x||_2 / ||x||_2;
  unit norm  | ||v_j||_2 - 1 | <= 16 n eps(dtype).
Bound: err <= 16 * max(e_plain, eps(dtype)) for each of R, E, X, e_plain being the same metric of torch.linalg.eig in the kernel's own dtype
(cgeev for complex64; numpy would compute it in double) against the same reference.  The floor is eps, not n eps: LAPACK's own R is a few eps
at every n, and n eps would be looser than the fixed gates of tests/test_eig.py.
Guards on the reference data (asserted, never skipped): the smallest pairwise distance of the reference eigenvalues is
>= 2 * 16 * e_plain(E) * ||A||_F (the kernel within its bound and LAPACK then match unambiguously; a duplicated eigenpair cannot pass), and
cond(X) <= 1e4.  A, w, V, info and the workspace (exactly trx_eig_ws_bytes_opts bytes of the call's own opts) carry guard words.
Every test prints its worst err / max(e_plain, eps) with `-s`; the recorded figures are in WORST_EMU / WORST_MI355X at the end of the file.
That the suite bites (emulator, scratch build, nothing committed): with the deflation criterion of the QR / AED scan (qr_prepare_kernel's ulp)
loosened 1e3-fold, test_eig_tile_edges[65-complex128] fails with ratios R 6.5, E 7.5, X 23.3 (unmutated: 0.9, 1.3, 1.5) and
test_eig_fallback_subbatch with R 32.9, E 43.6, X 36.7 (0.1, 0.2, 0.4), while test_eig_random, test_eig_degenerate_and_structured,
test_eig_two_iteration_groups and test_eig_tuning_knobs of tests/test_eig.py (n = 70 ... 76 included) all still pass their fixed gates.  Up
to n = 64 (QNMIN) the whole matrix is finished by the in-LDS QR with a criterion of its own, which the mutation left alone.
"""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests.backends import BACKENDS, dtcode, get_backend
from tests.eig_reference import eig_hp
from tests.helpers import crandn
from tests.test_smatrix_blocks import LD, MARGIN, Guarded, _eps

ROUTE1 = 1 << 4                  # trx_eig_opts: one-precision pipeline with Schur vectors
MIXED3 = 3 | (3 << 4)            # mixed-precision route, three Newton steps
AUTO = None                      # plain trx_eig: the knobs' defaults


# ---- the reference --------------------------------------------------------------------------------------------------------------------

def test_eig_hp_against_mpmath():
    """helpers.eig_hp against a 40-digit mpmath.eig, n = 5, 16, 24: eigenvalues (relative to ||A||_F) and eigenvectors (normalised to 1 at the
    reference's largest entry) are at least 1e3 times closer than plain LAPACK's.  Fails loudly where long double is not the 80-bit extended
    type: the complex128 cases of this file would silently lose their reference."""
    import mpmath
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not extended precision here: no reference beyond complex128"
    mpmath.mp.dps = 40
    rng = np.random.default_rng(32)

    def to_mp(z):          # exact: a long double is the sum of two doubles
        def r(x):
            hi = float(x)
            return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))
        return mpmath.mpc(r(z.real), r(z.imag))

    for n in (5, 16, 24):
        A = crandn(rng, (n, n))
        nf = mpmath.mpf(float(np.linalg.norm(A)))
        Em, ERm = mpmath.eig(mpmath.matrix(A.tolist()))
        lam, X = eig_hp(A)
        assert lam.dtype == LD and X.dtype == LD
        wd, Vd = np.linalg.eig(A)

        def errors(w, V, conv):
            ew = ev = mpmath.mpf(0)
            used = set()
            for j in range(n):
                wj = conv(w[j])
                i = min(range(n), key=lambda q: abs(Em[q] - wj))
                assert i not in used
                used.add(i)
                ew = max(ew, abs(Em[i] - wj) / nf)
                k = max(range(n), key=lambda q: abs(ERm[q, i]))
                d = sum(abs(conv(V[q, j]) / conv(V[k, j]) - ERm[q, i] / ERm[k, i]) ** 2 for q in range(n))
                s = sum(abs(ERm[q, i] / ERm[k, i]) ** 2 for q in range(n))
                ev = max(ev, mpmath.sqrt(d / s))
            return ew, ev

        ew_hp, ev_hp = errors(lam, X, to_mp)
        ew_pl, ev_pl = errors(wd, Vd, lambda z: mpmath.mpc(complex(z)))
        print(f"eig_hp n={n}: eigenvalues {float(ew_hp):.2e} (LAPACK {float(ew_pl):.2e}), eigenvectors {float(ev_hp):.2e} (LAPACK {float(ev_pl):.2e})")
        assert ew_hp < 1e-3 * ew_pl, (n, float(ew_hp), float(ew_pl))
        assert ev_hp < 1e-3 * ev_pl, (n, float(ev_hp), float(ev_pl))


# ---- matrix classes -------------------------------------------------------------------------------------------------------------------

_RCWA_ORDERS = {50: (2, 2), 98: (3, 3), 162: (4, 4), 286: (5, 6)}


def _rcwa_matrix(n, lossy, seed):
    """A = P Q of torcwa/rcwa.py:1226-1232 with mu = 1, from a numpy Laurent convolution matrix: an L-shaped inclusion (no mirror symmetry) of
    eps = 12 + 0.4j (lossless: 12) in eps = 1 on a 96 x 120 grid, cell 0.4 x 0.52 at wavelength 0.55, kx0 = 0.31, ky0 = 0.17 (nothing is
    degenerate); seed s > 0 moves the incidence by (0.013 s, 0.007 s) for a second batch member."""
    ox, oy = _RCWA_ORDERS[n]
    nx, ny = 96, 120
    gx, gy = np.meshgrid((np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny, indexing="ij")
    mask = ((gx > 0.13) & (gx < 0.61) & (gy > 0.2) & (gy < 0.47)) | ((gx > 0.13) & (gx < 0.35) & (gy > 0.2) & (gy < 0.83))
    eps = np.where(mask, 12.0 + (0.4j if lossy else 0.0), 1.0 + 0.0j)
    m, q = [a.reshape(-1) for a in np.meshgrid(np.arange(-ox, ox + 1), np.arange(-oy, oy + 1), indexing="ij")]
    c = np.fft.fft2(eps) / (nx * ny)
    E = c[(m[:, None] - m[None, :]) % nx, (q[:, None] - q[None, :]) % ny]
    Kx, Ky = np.diag(0.31 + 0.013 * seed + m * 0.55 / 0.4), np.diag(0.17 + 0.007 * seed + q * 0.55 / 0.52)
    KK, N = np.vstack([Kx, Ky]), len(m)
    I, Z = np.eye(N), np.zeros((N, N))
    P = np.block([[Z, I], [-I, Z]]) + KK @ np.linalg.inv(E) @ np.hstack([Ky, -Kx])
    Q = np.block([[Z, -E], [E, Z]]) + KK @ np.hstack([-Ky, Kx])
    return P @ Q


def _matrix(cls, n, seed):
    if cls in ("rcwa", "rcwa_lossless"):
        return _rcwa_matrix(n, cls == "rcwa", seed)
    G = crandn(np.random.default_rng([20270, ["gauss", "nonnormal", "neardiag"].index(cls), n, seed]), (n, n))
    if cls == "gauss":
        return G
    if cls == "nonnormal":
        return 3 * np.triu(G, 1) + np.tril(G) / np.sqrt(n) + np.diag(np.linspace(-4, 4, n) * (1 + 0.5j))
    return 1e-3 * G + np.diag(np.arange(1.0, n + 1))           # neardiag


def _cluster_matrix(n):
    """The recipe of tests/test_eig.py::test_eig_partial_fallback_is_per_matrix: a normal matrix with a 36-fold eigenvalue (exactly equal at the
    emulator's size, 3e-9 apart on the GPU's), beyond the refinement's exact cluster treatment."""
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(crandn(rng, (n, n)))
    lam = 2.0 * crandn(rng, (n,))
    lam[:36] = (1.5 - 0.5j) + (0.0 if n < 100 else 3e-9) * np.arange(36)
    return (Q * lam[None, :]) @ Q.conj().T


# ---- metrics --------------------------------------------------------------------------------------------------------------------------

def _norm2(M):
    """Column 2-norms of a clongdouble matrix, in long double."""
    return np.sqrt((M.real * M.real + M.imag * M.imag).sum(axis=0))


def _residual(Al, nf, w, V):
    w, V = np.asarray(w, dtype=LD), np.asarray(V, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((_norm2(Al @ V - V * w[None, :]) / (nf * _norm2(V))).max())


def _metrics(Al, nf, lam, X, w, V):
    """(R, E, X) of the computed pairs (w, V) against the reference (lam, X) of the clongdouble matrix Al; NaN anywhere counts as inf."""
    n = Al.shape[0]
    w, V = np.asarray(w, dtype=LD), np.asarray(V, dtype=LD)
    if not (np.isfinite(w).all() and np.isfinite(V).all()):
        return np.inf, np.inf, np.inf
    R = _residual(Al, nf, w, V)
    rows, cols = linear_sum_assignment(np.abs(w[:, None] - lam[None, :]).astype(np.float64))          # w[i] <-> lam[cols[i]]
    assert (rows == np.arange(n)).all()
    E = float(np.abs(w - lam[cols]).max() / nf)
    Xr = X[:, cols]
    k = np.argmax(np.abs(Xr), axis=0)
    j = np.arange(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        Vs, Xs = V / V[k, j][None, :], Xr / Xr[k, j][None, :]
        ex = float((_norm2(Vs - Xs) / _norm2(Xs)).max())
    return R, E, (ex if np.isfinite(ex) else np.inf)


@functools.lru_cache(maxsize=None)
def _point(cls, n, dtname, seed):
    """Matrix in the kernel's dtype, reference pairs, ||A||_F, e_plain of (R, E, X), the eigenvalue gap and cond(X) of one (class, n, dtype,
    seed); cached and never modified: route and batch parameters reuse matrices."""
    dtype = np.dtype(dtname)
    A = np.ascontiguousarray(_matrix(cls, n, seed).astype(dtype))
    A.setflags(write=False)
    Al = A.astype(LD)
    nf = np.sqrt((np.abs(Al) ** 2).sum())
    lam, X = eig_hp(A)
    wp, Vp = torch.linalg.eig(torch.from_numpy(A.copy()))
    e_plain = _metrics(Al, nf, lam, X, wp.numpy(), Vp.numpy())
    d = np.abs(lam[:, None] - lam[None, :]).astype(np.float64) + np.diag(np.full(n, np.inf))
    Xd = X.astype(np.complex128)
    return A, Al, nf, lam, X, e_plain, float(d.min()), float(np.linalg.cond(Xd / np.linalg.norm(Xd, axis=0)[None, :]))


def _assert_reference_guards(pt):
    A, Al, nf, lam, X, e_plain, gap, condX = pt
    assert gap >= 2 * MARGIN * e_plain[1] * float(nf), (gap, e_plain[1], float(nf))
    assert condX <= 1e4, condX


# ---- the call -------------------------------------------------------------------------------------------------------------------------

def _call_eig(be, A, opts):
    """One trx_eig (opts None) or trx_eig_opts call with A, w, V, info and the exactly sized workspace guarded; all five guards checked."""
    batch, n, _ = A.shape
    dtype = A.dtype
    gA = Guarded(be, batch * n * n, dtype, body=A)
    gw, gV = Guarded(be, batch * n, dtype), Guarded(be, batch * n * n, dtype)
    info = Guarded(be, batch, np.int32, body=np.full(batch, -7))
    if opts is None:
        nws = be.lib.eig_ws_bytes(dtcode(dtype), n, batch)
    else:
        nws = be.lib.eig_ws_bytes_opts(dtcode(dtype), n, batch, opts)
    assert nws > 0
    ws = Guarded(be, nws, np.uint8)
    if opts is None:
        rc = be.lib.eig(dtcode(dtype), gA.ptr(), gw.ptr(), gV.ptr(), n, batch, info.ptr(), ws.ptr(), nws, be.stream)
    else:
        rc = be.lib.eig_opts(dtcode(dtype), gA.ptr(), gw.ptr(), gV.ptr(), n, batch, info.ptr(), ws.ptr(), nws, be.stream, opts)
    be.sync()
    fallback = be.lib.eig_last_fallback()
    assert rc == 0
    gA.host()                                                # A is destroyed; the words behind it are not
    ws.host()
    return gw.host((batch, n)), gV.host((batch, n, n)), info.host(), fallback


RATIOS = {}                      # (test, backend) -> worst err / max(e_plain, eps) of R, E, X over the cases run so far


def _record(test, backend, ratios):
    r = RATIOS.setdefault((test, backend), [0.0, 0.0, 0.0])
    for i in range(3):
        r[i] = max(r[i], ratios[i])
    print(f"{test}[{backend}] this case R {ratios[0]:.2f} E {ratios[1]:.2f} X {ratios[2]:.2f} | worst so far R {r[0]:.2f} E {r[1]:.2f} X {r[2]:.2f}  "
          f"(err / max(e_plain, eps); bound {MARGIN:g})")


def _unit_norm(V, n, dtype):
    nrm = _norm2(np.asarray(V, dtype=LD))
    assert np.abs(nrm - 1).max() <= 16 * n * _eps(dtype), float(np.abs(nrm - 1).max())


def _check_batch(test, backend, pts, w, V, info, dtype, bounds=None):
    """Every member against its own point.  bounds: None -> 16 * max(e_plain, eps) of the member's own point for R, E and X; else a function
    point index -> (bound R, bound E, bound X).  Ratios are always err / max(e_plain, eps) of the member's own point."""
    n = pts[0][0].shape[0]
    eps = _eps(dtype)
    worst = [0.0, 0.0, 0.0]
    fails = []
    for b, pt in enumerate(pts):
        A, Al, nf, lam, X, e_plain, gap, condX = pt
        assert info[b] == 0, (b, info)
        err = _metrics(Al, nf, lam, X, w[b], V[b])
        bound = [MARGIN * max(e, eps) for e in e_plain] if bounds is None else bounds(b)
        for i, name in enumerate("REX"):
            worst[i] = max(worst[i], err[i] / max(e_plain[i], eps))
            if not err[i] <= bound[i]:
                fails.append(f"{name}[{b}]: err {err[i]:.3e}  e_plain {e_plain[i]:.3e}  eps {eps:.3e}  err/max(e_plain, eps) "
                             f"{err[i] / max(e_plain[i], eps):.2f}  bound {bound[i]:.3e}")
        _unit_norm(V[b], n, dtype)
    _record(test, backend, worst)
    assert not fails, "\n".join(fails)


def _stack(pts):
    return np.stack([p[0] for p in pts])


# ---- 1. tile edges, one-precision route -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 257])
def test_eig_tile_edges(backend, dtype, n):
    """Route 1 (Hessenberg - QR - Schur vectors in the dtype's own precision), Gaussian matrices, batch 2, at the tile edges of EigPlan: HNB =
    VNB = 32, QW = QNMIN = QAED = 64, HGK = 128; 160 = HGK + HNB, 257 = two Hessenberg groups plus one row; n = 1 and 2, which the ABI accepts.
    n = 1: w = a11 exactly, v a unit-modulus scalar."""
    if backend == "emu" and (n > 65 if dtype == np.complex128 else n not in (1, 2, 3, 33)):
        pytest.skip("emulator: n <= 65 in complex128 and n = 1, 2, 3, 33 in complex64 (the CPU suite stays within minutes); the GPU runs all")
    be = get_backend(backend)
    pts = [_point("gauss", n, np.dtype(dtype).name, s) for s in range(2)]
    for pt in pts:
        _assert_reference_guards(pt)
    w, V, info, _ = _call_eig(be, _stack(pts), ROUTE1)
    if n == 1:
        for b, pt in enumerate(pts):
            assert w[b, 0] == pt[0][0, 0] and abs(abs(V[b, 0, 0]) - 1) <= 16 * _eps(dtype), (w[b], pt[0], V[b])
    _check_batch("test_eig_tile_edges", backend, pts, w, V, info, dtype)


# ---- 2. matrix classes, one-precision route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("cls,n", [("nonnormal", 64), ("nonnormal", 129), ("rcwa", 50), ("rcwa", 162), ("rcwa", 286), ("rcwa_lossless", 98)])
def test_eig_classes(backend, dtype, cls, n):
    """Route 1, batch 2, on a strongly non-normal matrix (upper triangle 3 sqrt(n) times the lower, spread diagonal) and on the solver's real
    input, A = P Q of a patterned layer (L-shaped inclusion, lossy and lossless) at Fourier orders [2,2] ... [5,6]."""
    if backend == "emu" and (cls, n) != ("rcwa", 50):
        pytest.skip("emulator: the patterned-layer matrix at n = 50 (the CPU suite stays within minutes); the GPU runs all")
    be = get_backend(backend)
    pts = [_point(cls, n, np.dtype(dtype).name, s) for s in range(2)]
    for pt in pts:
        _assert_reference_guards(pt)
    w, V, info, _ = _call_eig(be, _stack(pts), ROUTE1)
    _check_batch(f"test_eig_classes:{cls}", backend, pts, w, V, info, dtype)


# ---- 3. batch-selected paths --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("batch", [1, 3, 8, 9, 49, 64, 65])
def test_eig_batch_paths(backend, batch):
    """complex128, route 1: the batch size selects the bulge chains per sweep (3 / 2 / 1, one above batch 48) and the iteration groups
    (1 / 2 / 4 at batch < 8 / >= 8 / >= 64).  Five distinct matrices (three Gaussian, one non-normal, one nearly diagonal: members of very
    different convergence speed) repeated cyclically, every member checked.  n = 129 on the GPU, 33 on the emulator."""
    if backend == "emu" and batch not in (1, 3, 9):
        pytest.skip("emulator: batch 1, 3 and 9 at n = 33 (the CPU suite stays within minutes); the GPU runs all at n = 129")
    be = get_backend(backend)
    n = 33 if backend == "emu" else 129
    five = [("gauss", 0), ("gauss", 1), ("gauss", 2), ("nonnormal", 0), ("neardiag", 0)]
    pts = [_point(five[b % 5][0], n, "complex128", five[b % 5][1]) for b in range(batch)]
    for pt in pts[:5]:
        _assert_reference_guards(pt)
    w, V, info, _ = _call_eig(be, _stack(pts), ROUTE1)
    _check_batch("test_eig_batch_paths", backend, pts, w, V, info, np.complex128)


# ---- 4. mixed-precision route -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("cls,n", [("gauss", 8), ("gauss", 33), ("gauss", 65), ("gauss", 129), ("rcwa", 286)])
def test_eig_mixed_route(backend, batch, cls, n):
    """complex128 through the mixed-precision route (opts route 3) with three Newton steps: fp32 eigendecomposition refined to fp64.  Held to
    the SAME bound as the all-fp64 route; nothing falls back.  Gaussian members: three seeds repeated cyclically; patterned layer: two."""
    if backend == "emu" and n not in (8, 33):
        pytest.skip("emulator: n = 8 and 33 (the CPU suite stays within minutes); the GPU runs all")
    be = get_backend(backend)
    nd = 3 if cls == "gauss" else 2
    pts = [_point(cls, n, "complex128", b % nd) for b in range(batch)]
    for pt in pts[:nd]:
        _assert_reference_guards(pt)
    w, V, info, fallback = _call_eig(be, _stack(pts), MIXED3)
    assert fallback == 0
    _check_batch(f"test_eig_mixed_route:{cls}", backend, pts, w, V, info, np.complex128)


@pytest.mark.parametrize("backend", BACKENDS)
def test_eig_automatic_route(backend):
    """Plain trx_eig at n = 257, batch 8: the automatic choice is the mixed route with the knob's default of two Newton steps.  R is held to
    the 1e-11 ||A|| that include/trx.h documents for two steps, E and X to the complex64 bound of the same matrix (what a complex64 caller's
    problem is worth); nothing falls back."""
    if backend == "emu":
        pytest.skip("emulator: the mixed route runs at n = 8 and 33 in test_eig_mixed_route (the CPU suite stays within minutes); the GPU runs this")
    be = get_backend(backend)
    n, batch = 257, 8
    pts = [_point("gauss", n, "complex128", b % 2) for b in range(batch)]
    pts32 = [_point("gauss", n, "complex64", b % 2) for b in range(batch)]
    for pt in pts[:2] + pts32[:2]:
        _assert_reference_guards(pt)
    assert be.lib.eig_ws_bytes(1, n, batch) == be.lib.eig_ws_bytes_opts(1, n, batch, 3 << 4)          # the automatic choice IS the mixed route
    w, V, info, fallback = _call_eig(be, _stack(pts), AUTO)
    assert fallback == 0
    eps32 = _eps(np.complex64)

    def bounds(b):
        e32 = pts32[b][5]
        return 1e-11, MARGIN * max(e32[1], eps32), MARGIN * max(e32[2], eps32)

    _check_batch("test_eig_automatic_route", backend, pts, w, V, info, np.complex128, bounds)


# ---- 5. the fallback sub-batch under guards -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
def test_eig_fallback_subbatch(backend):
    """Route 3, three Newton steps, batch 9, one member (index 4) with a 36-fold eigenvalue: the mixed route redoes that one in fp64 as a
    compact sub-batch carved from the tail of the caller's workspace (eig_redo_subset), which here has exactly trx_eig_ws_bytes_opts bytes and
    guard words behind it.  The eight others get the full metrics; the clustered one R and unit norm only (its vectors are not unique).
    n = 65 on the emulator, 300 on the GPU."""
    be = get_backend(backend)
    n, batch, hard = (65 if backend == "emu" else 300), 9, 4
    pts = [_point("gauss", n, "complex128", b % 3) for b in range(batch)]
    for pt in pts[:3]:
        _assert_reference_guards(pt)
    A = _stack(pts)
    A[hard] = _cluster_matrix(n)
    w, V, info, fallback = _call_eig(be, A, MIXED3)
    assert fallback == 1
    keep = [b for b in range(batch) if b != hard]
    _check_batch("test_eig_fallback_subbatch", backend, [pts[b] for b in keep], w[keep], V[keep], info[keep], np.complex128)
    assert info[hard] == 0
    Al = A[hard].astype(LD)
    nf = np.sqrt((np.abs(Al) ** 2).sum())
    wp, Vp = torch.linalg.eig(torch.from_numpy(A[hard].copy()))
    e_plain = _residual(Al, nf, wp.numpy(), Vp.numpy())
    R = _residual(Al, nf, w[hard], V[hard])
    eps = _eps(np.complex128)
    print(f"test_eig_fallback_subbatch[{backend}] clustered member R {R / max(e_plain, eps):.2f} (err / max(e_plain, eps); bound {MARGIN:g})")
    assert R <= MARGIN * max(e_plain, eps), (R, e_plain)
    _unit_norm(V[hard], n, np.complex128)


# Worst err / max(e_plain, eps) of (R, E, X) per test and route over all the cases the backend runs, rounded up (the bound is 16; no class needed
# a margin of its own).  Route 1 = one precision with Schur vectors, route 3 = mixed precision with three Newton steps, auto = plain trx_eig
# (mixed, two steps; its E and X are far inside their complex64 bound, the ratios below are against the complex128 e_plain like the others).
# "clustered": R of the member with the 36-fold eigenvalue that the fallback sub-batch redoes in fp64.
WORST_EMU = {
    "test_eig_tile_edges (route 1)": (1.5, 1.6, 1.8),
    "test_eig_classes:rcwa (route 1)": (1.6, 1.2, 0.7),
    "test_eig_batch_paths (route 1)": (1.3, 1.5, 1.5),
    "test_eig_mixed_route:gauss (route 3)": (0.2, 0.2, 0.3),
    "test_eig_fallback_subbatch (route 3)": (0.1, 0.2, 0.4),
    "test_eig_fallback_subbatch clustered (fp64 redo)": (0.8,),
}
WORST_MI355X = {
    "test_eig_tile_edges (route 1)": (2.4, 3.1, 2.6),
    "test_eig_classes:nonnormal (route 1)": (1.3, 2.9, 1.9),
    "test_eig_classes:rcwa (route 1)": (1.1, 1.1, 1.1),
    "test_eig_classes:rcwa_lossless (route 1)": (0.6, 1.7, 1.7),
    "test_eig_batch_paths (route 1)": (1.1, 2.9, 2.8),
    "test_eig_mixed_route:gauss (route 3)": (0.2, 0.4, 0.7),
    "test_eig_mixed_route:rcwa (route 3)": (0.2, 0.4, 0.3),
    "test_eig_automatic_route (auto)": (3.6, 0.9, 2.2),
    "test_eig_fallback_subbatch (route 3)": (0.1, 0.3, 0.5),
    "test_eig_fallback_subbatch clustered (fp64 redo)": (1.3,),
}
