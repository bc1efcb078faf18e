"""trx_hmodes, trx_inverse and trx_lu_solve at block level, under the policy of tests/test_smatrix_blocks.py ("Block tests"):

  * reference: complex128 LAPACK for a complex64 kernel; clongdouble products and helpers.solve_hp for a complex128 kernel.  hmodes: the
    dense 2N x 2N matrix P = mu J + [Kx; Ky] E^-1 [Ky, -Kx] with E^-1 formed explicitly and one 2N x 2N solve (the kernel: one N x N LU of
    E - (Kx^2 + Ky^2)/mu and the Woodbury correction);
  * bound: err <= 16 * max(e_plain, n eps) in the relmax metric, e_plain = the same formulas through LAPACK in the kernel's dtype;
  * guards on the data, asserted on every case: every inverted matrix has cond <= 1e4 and the matrix the kernel factorises interchanges
    rows at >= half of the steps of a plain partial-pivot LU (n >= 33; a 1 x 1 or 2 x 2 matrix has too few steps to ask);
  * A / B / V, piv, info (pre-filled with -7) and the exactly sized workspace carry guard words; the workspace body is 0xFF bytes (a NaN in
    every float or double), so workspace that is read before it is written shows; the inputs are bit-identical after the call.
Data: hmodes E = 2 x complex normal (unscaled, not diagonally dominant: 26/33 ... 249/257 interchanges, where the E = 0.2 x normal + 3 I of
tests/test_blocks.py::test_hmodes_structured interchanges 0 of 41), kx, ky, W, kz complex normal, mu = 1, 1.3 - 0.2j, 0.7 + 0.1j per
point; inverse / lu_solve A = complex normal / sqrt(n) with column 0 of point 0 scaled by 1e-3 (1e-2 from n = 258 on, see _matrix).
Every point draws from a generator of its own.

At N = 257 the complex128 hmodes reference is a 16-column sample (the 514-column clongdouble solve would take most of a minute): the
sampled columns are held to the bound against the sample, every column to 17 * max(e_plain, n eps) against the complex128 LAPACK
restatement (the triangle inequality of the two errors, 16 + 1).

MUTATIONS (each built for the emulator from a scratch copy of the sources, nothing of it committed; `old` = the tests of the entry in
tests/test_blocks.py):
  1. hmodes_t without the row permutation (rhs_permute_kernel left out of this call's lu_solve): all nine test_hmodes cases with N >= 33
     that the emulator runs fail, both dtypes, and so does test_hmodes_singular_member (N = 1 passes: nothing to permute).  old:
     test_hmodes_structured fails in complex128 and PASSES in complex64, alone and within its file: E = 0.2 x normal + 3 I is diagonally
     dominant, and whether a diagonal entry 3 - (kx^2 + ky^2)/mu comes close enough to 0 for an interchange is left to the draw of the
     shared generator.  Half of this was a gap.
  2. hm_rhs_kernel without the blockIdx.x * blockDim.x term of its column index: test_hmodes fails at N = 129 (columns 256, 257 of the
     workspace D are never written, and its 0xFF fill arrives in V as NaN); N <= 41 and old (n = 82 < 256) pass.  This was a gap.
     (The same term of bd_rowcomb_kernel, probe_col_kernel and bd_colcomb_kernel: tests/test_halfspace_blocks.py.)
WORST ratios err / max(e_plain, n eps): at the end of this file.
"""
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import crandn, lu_interchanges, relmax
from tests.test_smatrix_blocks import Guarded, _arith, _bound, _check, _eps

MUS = (1.0 + 0.0j, 1.3 - 0.2j, 0.7 + 0.1j)
HM_SAMPLE_FROM = 257            # complex128 hmodes: column sample from this N on
ERR_DTYPE, ERR_ARG, ERR_WORKSPACE = -1, -2, -3          # include/trx.h


def _ws(be, nbytes):
    return Guarded(be, nbytes, np.uint8, body=np.full(nbytes, 0xFF, dtype=np.uint8))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. trx_hmodes ----------------------------------------------------------------------------------------------------------------------

def _hm_inputs(N, b, dtype, zero_at=None):
    """Inputs of one point, rounded to the kernel's dtype.  zero_at = r: row and column r of E - (Kx^2 + Ky^2)/mu are exactly zero."""
    n = 2 * N
    rng = np.random.default_rng([20271, N, b])
    inp = {"E": 2.0 * crandn(rng, (N, N)), "kx": crandn(rng, (N,)), "ky": crandn(rng, (N,)), "W": crandn(rng, (n, n)), "kz": crandn(rng, (n,)),
           "mu": np.array(MUS[b % len(MUS)])}
    if zero_at is not None:
        inp["E"][zero_at, :] = 0.0
        inp["E"][:, zero_at] = 0.0
        inp["kx"][zero_at] = inp["ky"][zero_at] = 0.0
    return {k: v.astype(dtype) for k, v in inp.items()}


def _hm_formulas(inp, wd, solve, cols=None):
    """torcwa/rcwa.py:1226-1228, 1248, 1264 with a scalar mu: V = P^-1 W diag(kz), P = mu J + [Kx; Ky] E^-1 [Ky, -Kx] dense, E^-1 explicit.
    The products with Kx, Ky are row / column scalings.  Columns `cols` of V (all by default); also returns the three inverted matrices."""
    E, kx, ky, W, kz = [np.asarray(inp[k], dtype=wd) for k in ("E", "kx", "ky", "W", "kz")]
    mu = np.asarray(inp["mu"], dtype=wd)
    N = E.shape[0]
    I = np.eye(N, dtype=wd)
    Ei = solve(E, I)
    P = np.block([[kx[:, None] * Ei * ky[None, :], mu * I - kx[:, None] * Ei * kx[None, :]],
                  [ky[:, None] * Ei * ky[None, :] - mu * I, -ky[:, None] * Ei * kx[None, :]]])
    cols = np.arange(2 * N) if cols is None else np.asarray(cols)
    V = solve(P, W[:, cols] * kz[cols][None, :])
    return V, (E, E - np.diag((kx * kx + ky * ky) / mu), P)


@functools.lru_cache(maxsize=8)
def _hm_point(N, b, dtname):
    """Inputs, reference columns, the complex-LAPACK restatement of every column, e_plain and the guards of one point."""
    dtype = np.dtype(dtname).type
    n = 2 * N
    inp = _hm_inputs(N, b, dtype)
    cols = None
    if dtype == np.complex128 and N >= HM_SAMPLE_FROM:        # 16 columns: both ends, the edges of the 256-wide x-blocks, N - 1, N, 9 drawn
        fixed = [0, 255, 256, 257, 511, 512, n - 1, N - 1, N]
        drawn = np.random.default_rng([20272, N, b]).choice(np.setdiff1d(np.arange(n), fixed), size=16 - len(set(fixed)), replace=False)
        cols = np.array(sorted(set(fixed) | set(drawn.tolist())))
    ref, inverted = _hm_formulas(inp, *_arith(dtype, True), cols=cols)
    ref = ref.astype(np.complex128)
    plain, _ = _hm_formulas(inp, *_arith(dtype, False))
    plain = plain.astype(np.complex128)
    e_plain = relmax(plain if cols is None else plain[:, cols], ref)
    conds = [float(np.linalg.cond(np.asarray(M, dtype=np.complex128))) for M in inverted]
    swaps = lu_interchanges(inverted[1])
    return inp, cols, ref, plain, e_plain, conds, swaps


def _call_hmodes(be, dtype, inps, N, ws_short=0, null=None, code=None):
    """One call through the C ABI with guarded V, piv, info and an exactly sized guarded workspace.  Returns (rc, V, info)."""
    B, n = len(inps), 2 * N
    names = ("E", "mu", "kx", "ky", "W", "kz")
    st = {k: np.stack([p[k] for p in inps]) for k in names}
    d = {k: be.dev(st[k]) for k in names}
    V = Guarded(be, B * n * n, dtype)
    piv, info = Guarded(be, B * N, np.int32), Guarded(be, B, np.int32, body=np.full(B, -7))
    nws = be.lib.hmodes_ws_bytes(dtcode(dtype), N, B)
    assert nws == np.dtype(dtype).itemsize * 3 * B * N * N                       # include/trx.h: Mi [B,N,N] and D [B,N,2N]
    ws = _ws(be, nws)
    p = {k: (None if k == null else be.ptr(d[k])) for k in names}
    rc = be.lib.hmodes(dtcode(dtype) if code is None else code, p["E"], p["mu"], p["kx"], p["ky"], p["W"], p["kz"], N, B,
                       None if null == "V" else V.ptr(), None if null == "piv" else piv.ptr(), None if null == "info" else info.ptr(),
                       None if null == "ws" else ws.ptr(), nws - ws_short, be.stream)
    be.sync()
    ws.host()
    piv.host()
    for k in names:                                                              # the inputs are not modified
        assert _same_bits(be.host(d[k]), st[k]), k
    return rc, V.host((B, n, n)), info.host()


def _hm_cases():
    return [pytest.param(dtype, N, batch, id=f"{np.dtype(dtype).name}-N{N}-b{batch}")
            for dtype in (np.complex128, np.complex64) for N in (1, 33, 41, 129, 257) for batch in (3, 1)]


def _hm_compare(what, got, pt, N, dtype, ratios):
    inp, cols, ref, plain, e_plain, conds, swaps = pt
    n = 2 * N
    _check(what, got if cols is None else got[:, cols], ref, e_plain, n, dtype, ratios)
    if cols is not None:                                     # the columns outside the sample: against the LAPACK restatement, 16 + 1
        err = relmax(got, plain)
        assert err <= 17.0 / 16.0 * _bound(e_plain, n, dtype), (what, err, e_plain)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,batch", _hm_cases())
def test_hmodes(backend, dtype, N, batch):
    """trx_hmodes against the dense 2N x 2N restatement: N = 1, 33, 41 (one x-block, ragged panels), 129 (n = 258: two columns in the second
    256-thread x-block of hm_rhs_kernel / hm_finish_kernel and of the 258-column solve), 257 (one column in the second x-block of
    hm_inner_kernel, a second LU outer block of one column); batch 1 / 3 with a different mu per point; both dtypes."""
    be = get_backend(backend)
    if backend == "emu" and (N > 129 or (N == 129 and (dtype == np.complex64 or batch > 1))):
        pytest.skip("emulator: N = 129, batch 1 in complex128 covers the second x-block (the CPU suite stays within minutes); the GPU runs all")
    pts = [_hm_point(N, b, np.dtype(dtype).name) for b in range(batch)]
    for inp, cols, ref, plain, e_plain, conds, swaps in pts:
        assert max(conds) <= 1e4, conds
        assert N == 1 or swaps >= N // 2, (swaps, N)
    rc, V, info = _call_hmodes(be, dtype, [p[0] for p in pts], N)
    assert rc == 0 and (info == 0).all(), (rc, info)
    ratios = []
    for b, pt in enumerate(pts):
        _hm_compare(f"V[{b}]", V[b], pt, N, dtype, ratios)
    print(f"hmodes worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_hmodes_singular_member(backend, dtype):
    """Point 1 of 3 has row and column 9 of E - (Kx^2 + Ky^2)/mu exactly zero: info[1] > 0, info of the other two is 0 and their V is held to
    the bound."""
    be = get_backend(backend)
    N = 41
    pts = [_hm_point(N, b, np.dtype(dtype).name) for b in range(3)]
    inps = [pts[0][0], _hm_inputs(N, 1, dtype, zero_at=9), pts[2][0]]
    rc, V, info = _call_hmodes(be, dtype, inps, N)
    assert rc == 0 and info[1] > 0 and info[0] == 0 and info[2] == 0, (rc, info)
    ratios = []
    for b in (0, 2):
        assert max(pts[b][5]) <= 1e4 and pts[b][6] >= N // 2
        _hm_compare(f"V[{b}]", V[b], pts[b], N, dtype, ratios)
    print(f"hmodes_singular_member worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_hmodes_refusals(backend):
    """A workspace one byte short, a dtype code that is neither, every NULL argument: refused with the code of include/trx.h, V and info
    untouched."""
    be, dtype, N = get_backend(backend), np.complex128, 33
    inps = [_hm_inputs(N, b, dtype) for b in range(2)]
    cases = [(dict(ws_short=1), ERR_WORKSPACE), (dict(code=2), ERR_DTYPE), (dict(code=-1), ERR_DTYPE)]
    cases += [(dict(null=k), ERR_ARG) for k in ("E", "mu", "kx", "ky", "W", "kz", "V", "piv", "info", "ws")]
    for kw, want in cases:
        rc, V, info = _call_hmodes(be, dtype, inps, N, **kw)
        assert rc == want, (kw, rc)
        assert np.isnan(V).all() and (info == -7).all(), kw


# ---- 2. trx_inverse ---------------------------------------------------------------------------------------------------------------------

SEEDS = {33: 20278, 97: 20510}          # sizes whose point 0 exceeded cond 1e4 under the default seed (searched on the CPU)


def _matrix(n, b, dtype):
    """A = complex normal / sqrt(n); column 0 of point 0 is scaled by 1e-3 (n < 258) or 1e-2 (n >= 258), so that the first pivot search must
    look below the diagonal.  The scaled column alone puts cond at about 1e3 * 2 sqrt(n): 5e3 ... 7.6e3 at n = 33 ... 97 with the seeds
    above, but 1.1e4 at best over 6000 seeds at n = 258 -- hence 1e-2 there (cond 1.6e3 ... 2.1e3).  The other points: cond 9e1 ... 8e2."""
    rng = np.random.default_rng([SEEDS.get(n, 20273), n, b])
    A = crandn(rng, (n, n)) / np.sqrt(n)
    if b == 0:
        A[:, 0] *= 1e-3 if n < 258 else 1e-2
    return A.astype(dtype), rng


@functools.lru_cache(maxsize=8)
def _inv_point(n, b, dtname):
    dtype = np.dtype(dtname).type
    A, _ = _matrix(n, b, dtype)
    wd, solve = _arith(dtype, True)
    ref = np.asarray(solve(A.astype(wd), np.eye(n, dtype=wd)), dtype=np.complex128)
    wp, solvep = _arith(dtype, False)
    e_plain = relmax(solvep(A, np.eye(n, dtype=wp)), ref)
    return A, ref, e_plain, float(np.linalg.cond(A.astype(np.complex128))), lu_interchanges(A)


def _call_inverse(be, dtype, As, ws_short=0):
    B, n = len(As), As[0].shape[0]
    A = Guarded(be, B * n * n, dtype, body=np.stack(As))
    piv, info = Guarded(be, B * n, np.int32), Guarded(be, B, np.int32, body=np.full(B, -7))
    nws = be.lib.inverse_ws_bytes(dtcode(dtype), n, B)
    assert nws == np.dtype(dtype).itemsize * B * n * n                           # include/trx.h: batch * n * n elements
    ws = _ws(be, nws)
    rc = be.lib.inverse(dtcode(dtype), A.ptr(), n, B, piv.ptr(), info.ptr(), ws.ptr(), nws - ws_short, be.stream)
    be.sync()
    ws.host()
    piv.host()
    return rc, A.host((B, n, n)), info.host()


def _inv_cases():
    return [pytest.param(dtype, n, batch, id=f"{np.dtype(dtype).name}-n{n}-b{batch}")
            for dtype in (np.complex128, np.complex64) for n in (1, 2, 33, 45, 258, 300) for batch in (3, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,n,batch", _inv_cases())
def test_inverse(backend, dtype, n, batch):
    """trx_inverse against solve(A, I): n = 1, 2, 33 (one row beyond a 32-row tile), 45, 258 (two columns in the second x-block of
    set_identity_kernel and of the solve, a second outer block of two columns), 300; batch 1 / 3; both dtypes."""
    be = get_backend(backend)
    if backend == "emu" and n >= 258 and (dtype == np.complex64 or batch > 1):
        pytest.skip("emulator: n = 258 and 300 run with batch 1 in complex128 (the CPU suite stays within minutes); the GPU runs all")
    pts = [_inv_point(n, b, np.dtype(dtype).name) for b in range(batch)]
    for A, ref, e_plain, cond, swaps in pts:
        assert cond <= 1e4, cond
        assert n < 33 or swaps >= n // 2, (swaps, n)
    rc, got, info = _call_inverse(be, dtype, [p[0] for p in pts])
    assert rc == 0 and (info == 0).all(), (rc, info)
    ratios = []
    for b, (A, ref, e_plain, cond, swaps) in enumerate(pts):
        _check(f"inverse[{b}]", got[b], ref, e_plain, n, dtype, ratios)
    print(f"inverse worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_inverse_singular_member(backend, dtype):
    """Point 1 of 3 has a zero row and column: info[1] > 0; the other two are inverted to the bound."""
    be, n = get_backend(backend), 45
    pts = [_inv_point(n, b, np.dtype(dtype).name) for b in range(3)]
    As = [p[0] for p in pts]
    As[1] = As[1].copy()
    As[1][9, :] = 0.0
    As[1][:, 9] = 0.0
    rc, got, info = _call_inverse(be, dtype, As)
    assert rc == 0 and info[1] > 0 and info[0] == 0 and info[2] == 0, (rc, info)
    ratios = []
    for b in (0, 2):
        A, ref, e_plain, cond, swaps = pts[b]
        assert cond <= 1e4 and swaps >= n // 2
        _check(f"inverse[{b}]", got[b], ref, e_plain, n, dtype, ratios)
    print(f"inverse_singular_member worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_inverse_short_workspace(backend):
    """One byte less than trx_inverse_ws_bytes is refused; A and info are untouched."""
    be, dtype, n = get_backend(backend), np.complex128, 33
    As = [_matrix(n, b, dtype)[0] for b in range(2)]
    rc, got, info = _call_inverse(be, dtype, As, ws_short=1)
    assert rc == ERR_WORKSPACE
    assert _same_bits(got, np.stack(As)) and (info == -7).all()


# ---- 3. trx_lu_solve --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _lu_point(n, nrhs, b, dtname):
    dtype = np.dtype(dtname).type
    A, rng = _matrix(n, b, dtype)
    Bm = crandn(rng, (n, nrhs)).astype(dtype)
    wd, solve = _arith(dtype, True)
    ref = np.asarray(solve(A.astype(wd), Bm.astype(wd)), dtype=np.complex128)
    _, solvep = _arith(dtype, False)
    e_plain = relmax(solvep(A, Bm), ref)
    return A, Bm, ref, e_plain, float(np.linalg.cond(A.astype(np.complex128))), lu_interchanges(A)


def _call_lu_solve(be, dtype, As, Bs):
    B, n, nrhs = len(As), As[0].shape[0], Bs[0].shape[1]
    A, Bm = Guarded(be, B * n * n, dtype, body=np.stack(As)), Guarded(be, B * n * nrhs, dtype, body=np.stack(Bs))
    piv, info = Guarded(be, B * n, np.int32), Guarded(be, B, np.int32, body=np.full(B, -7))
    rc = be.lib.lu_solve(dtcode(dtype), A.ptr(), n, Bm.ptr(), nrhs, B, piv.ptr(), info.ptr(), be.stream)
    be.sync()
    return rc, A.host((B, n, n)), Bm.host((B, n, nrhs)), piv.host((B, n)), info.host()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n,nrhs", [(1, 1), (33, 7), (97, 130), (258, 1), (258, 257), (300, 16)])
def test_lu_solve(backend, dtype, n, nrhs):
    """trx_lu_solve, batch 2: X against the policy bound (tests/test_blocks.py::test_lu_solve gates complex64 at 2e-3, about 100 x LAPACK's
    own error on its data), the factors by || L U - P A || with piv a valid LAPACK interchange sequence.  nrhs = 257: one column in the second
    x-block of rhs_permute_kernel / trsm_kernel; n = 258, 300: a second outer block of 2 / 44 columns; nrhs = 1: ldb = 1."""
    be = get_backend(backend)
    batch = 2
    pts = [_lu_point(n, nrhs, b, np.dtype(dtype).name) for b in range(batch)]
    for A, Bm, ref, e_plain, cond, swaps in pts:
        assert cond <= 1e4, cond
        assert n < 33 or swaps >= n // 2, (swaps, n)
    rc, LU, X, pv, info = _call_lu_solve(be, dtype, [p[0] for p in pts], [p[1] for p in pts])
    assert rc == 0 and (info == 0).all(), (rc, info)
    ratios = []
    for b, (A, Bm, ref, e_plain, cond, swaps) in enumerate(pts):
        _check(f"X[{b}]", X[b], ref, e_plain, n, dtype, ratios)
        assert ((pv[b] >= np.arange(n)) & (pv[b] < n)).all()
        PA = A.astype(np.complex128)
        for r in range(n):
            if pv[b][r] != r:
                PA[[r, pv[b][r]]] = PA[[pv[b][r], r]]
        LUb = LU[b].astype(np.complex128)
        Lm, Um = np.tril(LUb, -1) + np.eye(n), np.triu(LUb)
        assert np.abs(Lm).max() <= 2 ** 0.5 + 1e-6           # partial pivoting by |re| + |im| (LAPACK cabs1): moduli up to sqrt(2)
        assert np.abs(Lm @ Um - PA).max() / np.abs(PA).max() < 50 * n * _eps(dtype)
    print(f"lu_solve worst err/max(e_plain, n eps) = {max(ratios):.3f}")


# ---- 4. the same call twice ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_solve_entries_repeat_bit_identical(backend, dtype):
    """trx_hmodes, trx_inverse and trx_lu_solve called twice on the same inputs give the same bits (V; the inverse; factors, X and piv)."""
    be = get_backend(backend)
    inps = [_hm_inputs(41, b, dtype) for b in range(3)]
    first, second = _call_hmodes(be, dtype, inps, 41), _call_hmodes(be, dtype, inps, 41)
    assert first[0] == 0 and second[0] == 0 and _same_bits(first[1], second[1]) and _same_bits(first[2], second[2])
    As = [_matrix(45, b, dtype)[0] for b in range(3)]
    first, second = _call_inverse(be, dtype, As), _call_inverse(be, dtype, As)
    assert first[0] == 0 and second[0] == 0 and _same_bits(first[1], second[1]) and _same_bits(first[2], second[2])
    pts = [_lu_point(97, 130, b, np.dtype(dtype).name) for b in range(2)]
    first = _call_lu_solve(be, dtype, [p[0] for p in pts], [p[1] for p in pts])
    second = _call_lu_solve(be, dtype, [p[0] for p in pts], [p[1] for p in pts])
    assert first[0] == 0 and second[0] == 0
    for x, y in zip(first[1:], second[1:]):
        assert _same_bits(x, y)


# Worst err / max(e_plain, n eps) per test over all its cases (the bound is 16); no entry needed a margin of its own.
# Emulator: every case it runs; MI355X: all 129 cases of the two files, from a `-m gpu -s` run, rounded up.
WORST_EMU = {"test_hmodes": 0.6, "test_inverse": 1.4, "test_lu_solve": 2.0}
WORST_MI355X = {"test_hmodes": 0.9, "test_inverse": 2.5, "test_lu_solve": 2.0}
