"""trx_redheffer_halfspace (its three algebra branches) and trx_redheffer_halfspace_columns at block level, under the policy of
tests/test_smatrix_blocks.py ("Block tests"):

  * different algebra: the reference forms BOTH inverses, t1 = (I - Sm12 Sn21)^-1 and t2 = (I - Sn21 Sm12)^-1 (the kernels: one LU of K and
    the push-through identity, or right solves with K^T in the lean branch);
  * reference precision: complex128 LAPACK for a complex64 kernel (the full products, at every N); clongdouble products and
    helpers.solve_hp for a complex128 kernel -- helpers.star_full at N = 37, and at N = 129, 257 PER COLUMN on a sample of 12 - 14 columns
    (the full clongdouble product takes 7 s / 38 s per point there): for column c, v = Sm11 e_c or Sm12 Sn22 e_c, u = t1 v, and S21 / S22 / Y
    through the other inverse, w = t2 (Sn21 Sm11 e_c) or t2 (Sn22 e_c); products with the block-diagonal operand are row / column
    combinations, so a point costs O(n^2 * sample).  The sample: columns 0, 255, 256, 257, N - 1, N, N + 255, N + 256 (where < 2N), 2N - 1
    and 8 drawn; every row of a sampled column is compared under the bound, and the columns outside the sample against the complex128
    LAPACK restatement under 17 * max(e_plain, n eps) (the triangle inequality of the two errors, 16 + 1);
  * bound: err <= 16 * max(e_plain, n eps) per output tensor in the relmax metric, e_plain = the same formulas through LAPACK in the
    kernel's dtype on the same columns, n = 2N;
  * guards on the data, asserted on every case: cond(I - Sm12 Sn21) and cond(I - Sn21 Sm12) <= 1e4; a plain partial-pivot LU of K
    interchanges rows at >= n/2 steps, and so does K^T for the lean branch, which factors K^T;
  * the four Sout blocks (four separate allocations, none aliasing S), XY, out, piv, info (pre-filled with -7) and the exactly sized
    workspace carry guard words; the workspace body is 0xFF bytes (NaN in every float or double); S and bd are bit-identical afterwards.
Data: S[k] = complex normal / sqrt(n), bd = 1.5 x complex normal, every point from its own default_rng([seed, N, side, b]).

MUTATIONS (each built for the emulator from a scratch copy of the sources, nothing of it committed; `old` = the tests of the entry in
tests/test_blocks.py and tests/test_redheffer_columns.py):
  2a. bd_rowcomb_kernel without the blockIdx.x * blockDim.x term of its column index: the three test_halfspace branches and
      test_halfspace_columns side 0 fail at N = 129; every N = 37 case and all 28 old tests pass (n = 74 < 256).  This was a gap.
  2b. probe_col_kernel, the same term of its row index: test_halfspace_columns fails at N = 129 on both sides; N = 37 and all 22 tests of
      tests/test_redheffer_columns.py pass.  This was a gap.
  3.  bd_colcomb_kernel, the same term (N = 257, which the suite runs on the GPU only: the emulator skip was lifted in the scratch copy for
      this note, complex128, batch 1): test_halfspace xy1 and test_halfspace_columns side 1 fail at N = 257; N = 37, 129 and all 28 old
      tests pass.  This was a gap.
  4.  Lean branch with M = D12 Sn22 written before the solve, over the factors of K^T: every lean case of test_halfspace and
      test_halfspace_lean_info_of_singular_K fail -- and so does old, tests/test_blocks.py::test_redheffer_halfspace[0-0] in both dtypes.
      That line was never a gap.
  (1, and hm_rhs_kernel of 2: tests/test_solve_blocks.py.)
WORST ratios err / max(e_plain, n eps): at the end of this file.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, crandn, lu_interchanges, relmax, star_full
from tests.test_smatrix_blocks import Guarded, _arith, _bound, _check

SEED = 20281
NS = (37, 129, 257)
SAMPLE_FROM = 129               # complex128: per-column reference from this N on
NAMES = ("S11", "S21", "S12", "S22", "X", "Y")
ERR_DTYPE, ERR_ARG, ERR_WORKSPACE = -1, -2, -3          # include/trx.h


def _ws(be, nbytes):
    return Guarded(be, nbytes, np.uint8, body=np.full(nbytes, 0xFF, dtype=np.uint8))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _arr(ptrs):
    return (ctypes.c_void_p * 4)(*ptrs)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------

class _BD:
    """A 2x2-block-diagonal operator [[d0, d1], [d2, d3]] kept as its four diagonals d [4, N]."""

    def __init__(self, d):
        self.d = d


def _mul(A, B):
    """A @ B where at most one factor is a _BD: rows i, i + N of B (or columns j, j + N of A) combine."""
    if isinstance(A, _BD):
        d, N = A.d, A.d.shape[1]
        return np.concatenate([d[0][:, None] * B[:N] + d[1][:, None] * B[N:], d[2][:, None] * B[:N] + d[3][:, None] * B[N:]])
    if isinstance(B, _BD):
        d, N = B.d, B.d.shape[1]
        return np.concatenate([A[:, :N] * d[0][None, :] + A[:, N:] * d[2][None, :], A[:, :N] * d[1][None, :] + A[:, N:] * d[3][None, :]], axis=1)
    return A @ B


def _cols(A, C):
    """Columns C of A."""
    if not isinstance(A, _BD):
        return A[:, C]
    d, N = A.d, A.d.shape[1]
    out = np.zeros((2 * N, len(C)), dtype=d.dtype)
    for q, c in enumerate(C):
        j = c % N
        out[j, q], out[j + N, q] = (d[0][j], d[2][j]) if c < N else (d[1][j], d[3][j])
    return out


def _column_formulas(Sm, Sn, C, wd, solve):
    """Columns C of [S11, S21, S12, S22] and columns C | n + C of X, Y of the star product Sm * Sn (include/trx.h), both inverses explicit,
    in the working dtype `wd` with `solve`.  One of Sm, Sn is a list of _BD."""
    n = 2 * Sm[0].d.shape[1] if isinstance(Sm[0], _BD) else Sm[0].shape[0]
    I = np.eye(n, dtype=wd)
    K, K2 = I - _mul(Sm[2], Sn[1]), I - _mul(Sn[1], Sm[2])
    V1 = _cols(Sm[0], C)
    U = solve(K, np.hstack([V1, _mul(Sm[2], _cols(Sn[3], C))]))
    W = solve(K2, np.hstack([_mul(Sn[1], V1), _cols(Sn[3], C)]))
    U1, U2, W1, W2 = U[:, :len(C)], U[:, len(C):], W[:, :len(C)], W[:, len(C):]
    return [_mul(Sn[0], U1), _cols(Sm[1], C) + _mul(Sm[3], W1), _cols(Sn[2], C) + _mul(Sn[0], U2), _mul(Sm[3], W2), U, W]


def _inputs(N, side, b, dtype):
    n = 2 * N
    rng = np.random.default_rng([SEED, N, side, b])
    S = [(crandn(rng, (n, n)) / np.sqrt(n)).astype(dtype) for _ in range(4)]
    bd = (1.5 * crandn(rng, (4, 4, N))).astype(dtype)
    return bd, S


def _sample(N):
    """The column sample of size N (one for all points, so that a column list shared by a batch lies inside it)."""
    n = 2 * N
    fixed = sorted({c for c in (0, 255, 256, 257, N - 1, N, N + 255, N + 256, n - 1) if c < n})
    drawn = np.random.default_rng([SEED + 1, N]).choice(np.setdiff1d(np.arange(n), fixed), size=8, replace=False)
    return np.array(sorted(fixed + drawn.tolist()))


class _Point:
    """Inputs, reference, e_plain and guards of one (N, side, b, dtype).  cols = None: ref[k] and plain[k] are the full tensors; else
    ref[k] and plain[k] hold the sampled columns (X, Y: columns cols | n + cols) and plain_full[k] the complex128 restatement of all."""

    def index(self, k, columns=None):
        """Positions inside ref[k] / plain[k] of `columns` of block k (default: everything the reference holds), and inside the output."""
        n, two = 2 * self.N, k >= 4
        if columns is None:
            if self.cols is None:
                return slice(None), slice(None)
            return slice(None), (np.concatenate([self.cols, n + self.cols]) if two else self.cols)
        columns = np.asarray(columns)
        if self.cols is None:
            return columns, columns
        pos = np.searchsorted(self.cols, columns)
        assert (self.cols[pos] == columns).all(), "column outside the sample of the reference"
        return pos, columns


@functools.lru_cache(maxsize=3)
def _point(N, side, b, dtname):
    dtype = np.dtype(dtname).type
    n = 2 * N
    pt = _Point()
    pt.N, pt.side, pt.dtype = N, side, dtype
    pt.bd, pt.S = _inputs(N, side, b, dtype)
    dense = lambda wd: ([_bd_dense(pt.bd[k].astype(wd)) for k in range(4)], [x.astype(wd) for x in pt.S])
    order = (lambda D, S: (D, S)) if side == 0 else (lambda D, S: (S, D))
    pt.cols = _sample(N) if dtype == np.complex128 and N >= SAMPLE_FROM else None
    wp, solvep = _arith(dtype, False)
    Ip = np.eye(n, dtype=wp)
    full_plain = [np.asarray(x, dtype=np.complex128) for x in star_full(*order(*dense(wp)), lambda M: solvep(M, Ip))]
    if pt.cols is None:
        wd, solve = _arith(dtype, True)
        I = np.eye(n, dtype=wd)
        pt.ref = [np.asarray(x, dtype=np.complex128) for x in star_full(*order(*dense(wd)), lambda M: solve(M, I))]
        pt.plain = full_plain
        pt.plain_full = None
    else:
        ops = lambda wd: order([_BD(pt.bd[k].astype(wd)) for k in range(4)], [x.astype(wd) for x in pt.S])
        wd, solve = _arith(dtype, True)
        pt.ref = [np.asarray(x, dtype=np.complex128) for x in _column_formulas(*ops(wd), pt.cols, wd, solve)]
        pt.plain = [np.asarray(x, dtype=np.complex128) for x in _column_formulas(*ops(wp), pt.cols, wp, solvep)]
        pt.plain_full = full_plain
    pt.e_plain = [relmax(p, r) for p, r in zip(pt.plain, pt.ref)]
    Dm, Sd = dense(np.complex128)
    Sm, Sn = order(Dm, Sd)
    K, K2 = np.eye(n) - Sm[2] @ Sn[1], np.eye(n) - Sn[1] @ Sm[2]
    pt.conds = (float(np.linalg.cond(K)), float(np.linalg.cond(K2)))
    pt.swaps = lu_interchanges(K)
    pt.swaps_t = lu_interchanges(K.T)
    return pt


def _assert_guards(pt, lean=False):
    n = 2 * pt.N
    assert max(pt.conds) <= 1e4, pt.conds
    assert pt.swaps >= n // 2, (pt.swaps, n)
    if lean:
        assert pt.swaps_t >= n // 2, (pt.swaps_t, n)


def _compare(k, got, pt, b, ratios):
    """Output tensor k of point b against the reference: sampled (or all) columns under the bound, the rest against LAPACK under 16 + 1."""
    n = 2 * pt.N
    _, sel = pt.index(k)
    _check(f"{NAMES[k]}[{b}]", got[:, sel], pt.ref[k], pt.e_plain[k], n, pt.dtype, ratios)
    if pt.plain_full is not None:
        err = relmax(got, pt.plain_full[k])
        assert err <= 17.0 / 16.0 * _bound(pt.e_plain[k], n, pt.dtype), (NAMES[k], b, err, pt.e_plain[k])


def _emu_skip(backend, N, dtype, batch):
    if backend == "emu" and (N > 129 or (N == 129 and (dtype == np.complex64 or batch > 1))):
        pytest.skip("emulator: N = 37 in full and N = 129 with batch 1 in complex128 (the CPU suite stays within minutes); the GPU runs all")


# ---- 1. trx_redheffer_halfspace -----------------------------------------------------------------------------------------------------------

def _call_halfspace(be, dtype, side, bds, Ss, N, want_xy, **kw):
    """One call through the C ABI; bds / Ss: the inputs of the B points.  kw: tell_side, tell_N, tell_batch, code (dtype code), nws (workspace size
    passed), null_S (index of a NULL S[k]) override what the call is told.  Returns (rc, [S11, S21, S12, S22], XY or None, info)."""
    B, n = len(bds), 2 * N
    nn, esz = n * n, np.dtype(dtype).itemsize
    bd = np.stack(bds, axis=2)                                                   # [4, 4, B, N]
    S = [np.stack([s[k] for s in Ss]) for k in range(4)]
    dbd, dS = be.dev(bd), [be.dev(x) for x in S]
    out = [Guarded(be, B * nn, dtype) for _ in range(4)]
    XY = Guarded(be, 2 * B * n * 2 * n, dtype) if want_xy else None
    piv, info = Guarded(be, B * n, np.int32), Guarded(be, B, np.int32, body=np.full(B, -7))
    nws = be.lib.redheffer_halfspace_ws_bytes(dtcode(dtype), N, B, side, want_xy)
    assert nws == esz * B * nn * (4 if side == 0 and not want_xy else 1)         # include/trx.h: K alone, or the lean branch's two solve buffers
    ws = _ws(be, nws)
    for o in out:                                                                # four separate allocations, none aliasing an input
        for x in dS:
            assert o.ptr() + (B * nn + 64) * esz <= be.ptr(x) or be.ptr(x) + B * nn * esz <= o.ptr()
    ps = _arr([None if k == kw.get("null_S") else be.ptr(x) for k, x in enumerate(dS)])
    po = _arr([x.ptr() for x in out])
    rc = be.lib.redheffer_halfspace(kw.get("code", dtcode(dtype)), kw.get("tell_side", side), be.ptr(dbd), ctypes.addressof(ps), ctypes.addressof(po),
                                    XY.ptr() if XY else None, kw.get("tell_N", N), kw.get("tell_batch", B), piv.ptr(), info.ptr(), ws.ptr(),
                                    kw.get("nws", nws), be.stream)
    be.sync()
    ws.host()
    piv.host()
    assert _same_bits(be.host(dbd), bd)
    for x, h in zip(dS, S):
        assert _same_bits(be.host(x), h)
    return rc, [o.host((B, n, n)) for o in out], XY.host((2, B, n, 2 * n)) if XY else None, info.host()


BRANCHES = {"xy0": (0, 1), "lean": (0, 0), "xy1": (1, 1)}          # (side, want_xy)


def _full_cases():
    return [pytest.param(dtype, N, batch, br, id=f"{np.dtype(dtype).name}-N{N}-b{batch}-{br}")
            for dtype in (np.complex128, np.complex64) for N in NS for side in (0, 1) for batch in (3, 1)
            for br in BRANCHES if BRANCHES[br][0] == side]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,batch,branch", _full_cases())
def test_halfspace(backend, dtype, N, batch, branch):
    """The four blocks, and X | Y where produced, of the three branches (side 0 with XY, side 0 lean, side 1): N = 37; N = 129 (n = 258: two
    columns in the second 256-thread x-block of bd_rowcomb / bd_dense / block_copy and of the transposes, a second LU outer block of two
    columns); N = 257 (one column in the second x-block of bd_colcomb_kernel, n = 514: three outer blocks, gemm_big in complex128);
    batch 1 / 3; both dtypes."""
    be = get_backend(backend)
    _emu_skip(backend, N, dtype, batch)
    side, want_xy = BRANCHES[branch]
    pts = [_point(N, side, b, np.dtype(dtype).name) for b in range(batch)]
    for pt in pts:
        _assert_guards(pt, lean=branch == "lean")
    rc, out, XY, info = _call_halfspace(be, dtype, side, [p.bd for p in pts], [p.S for p in pts], N, want_xy)
    assert rc == 0 and (info == 0).all(), (rc, info)
    ratios = []
    for b, pt in enumerate(pts):
        for k in range(4):
            _compare(k, out[k][b], pt, b, ratios)
        if want_xy:
            _compare(4, XY[0, b], pt, b, ratios)
            _compare(5, XY[1, b], pt, b, ratios)
    print(f"halfspace {branch} worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_halfspace_refusals(backend):
    """Every refusal of include/trx.h leaves the outputs and info untouched: side outside {0, 1}; XY = NULL with side 1; a NULL S[k]; a
    workspace one byte short, and in particular the lean call (XY = NULL) offered the one matrix of the other branches; a dtype code that is
    neither; N = 0; batch = 0."""
    be, dtype, N, B = get_backend(backend), np.complex128, 37, 2
    esz, nn = 16, 4 * N * N
    for side in (0, 1):
        ins = [_inputs(N, side, b, dtype) for b in range(B)]
        bds, Ss = [i[0] for i in ins], [i[1] for i in ins]
        cases = [(1, dict(tell_side=2), ERR_ARG), (1, dict(tell_side=-1), ERR_ARG), (1, dict(null_S=0), ERR_ARG), (1, dict(null_S=3), ERR_ARG),
                 (1, dict(nws=esz * B * nn - 1), ERR_WORKSPACE), (1, dict(code=2), ERR_DTYPE), (1, dict(tell_N=0), ERR_ARG), (1, dict(tell_batch=0), ERR_ARG)]
        if side == 1:
            cases += [(0, dict(), ERR_ARG)]                                      # XY = NULL with side 1
        if side == 0:
            cases += [(0, dict(nws=4 * esz * B * nn - 1), ERR_WORKSPACE), (0, dict(nws=esz * B * nn), ERR_WORKSPACE), (0, dict(null_S=1), ERR_ARG)]
        for want_xy, kw, want in cases:
            rc, out, XY, info = _call_halfspace(be, dtype, side, bds, Ss, N, want_xy, **kw)
            assert rc == want, (side, want_xy, kw, rc)
            assert all(np.isnan(o).all() for o in out) and (XY is None or np.isnan(XY).all()) and (info == -7).all(), (side, kw)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_halfspace_lean_info_of_singular_K(backend, dtype):
    """The lean branch with K = I - D12 Sn21 = 0 exactly at point 1 of 3 (tests/test_redheffer_columns.py::test_columns_info_of_singular_K
    for the full product): info[1] reports it, info[0] = info[2] = 0 and those two points are held to the bound."""
    be, N = get_backend(backend), 37
    n = 2 * N
    pts = [_point(N, 0, b, np.dtype(dtype).name) for b in range(3)]
    bds, Ss = [p.bd for p in pts], [list(p.S) for p in pts]
    bds[1] = bds[1].copy()
    bds[1][2] = 0                                                                # D12 = I
    bds[1][2, 0] = bds[1][2, 3] = 1
    Ss[1][1] = np.eye(n, dtype=dtype)                                            # Sn21 = I
    rc, out, XY, info = _call_halfspace(be, dtype, 0, bds, Ss, N, 0)
    assert rc == 0 and info[1] != 0 and info[0] == 0 and info[2] == 0, (rc, info)
    ratios = []
    for b in (0, 2):
        _assert_guards(pts[b], lean=True)
        for k in range(4):
            _compare(k, out[k][b], pts[b], b, ratios)
    print(f"halfspace_lean_singular worst err/max(e_plain, n eps) = {max(ratios):.3f}")


# ---- 2. trx_redheffer_halfspace_columns -------------------------------------------------------------------------------------------------------

def _column_lists(N):
    """m = 16, 3, 1.  Together: columns 0, N - 1, N, 2N - 1, at N >= 129 also 255, 256, 257, and columns given twice; all inside the column
    sample, so that the per-column reference of the complex128 cases holds them.  m = 16: the 12 - 14 columns of the sample in descending
    order, then its first ones again."""
    n, sample = 2 * N, _sample(N).tolist()
    long = (sample[::-1] + sample)[:16]
    assert {0, N - 1, N, n - 1} <= set(long) and (N < 129 or {255, 256, 257} <= set(long)) and len(set(long)) < 16
    return [long, [n - 1, 0, N], [N - 1]]


def _call_columns(be, dtype, side, bds, Ss, N, block, cols):
    B, n, m = len(bds), 2 * N, len(cols)
    bd = np.stack(bds, axis=2)
    S = [np.stack([s[k] for s in Ss]) for k in range(4)]
    dbd, dS = be.dev(bd), [be.dev(x) for x in S]
    out = Guarded(be, B * n * m, dtype)
    piv, info = Guarded(be, B * n, np.int32), Guarded(be, B, np.int32, body=np.full(B, -7))
    nws = be.lib.redheffer_halfspace_columns_ws_bytes(dtcode(dtype), N, B, m)
    assert nws == np.dtype(dtype).itemsize * B * (n * n + 3 * n * m)             # include/trx.h: K and three [B,n,m] column blocks
    ws = _ws(be, nws)
    ps = _arr([be.ptr(x) for x in dS])
    pc = (ctypes.c_int * m)(*cols)
    rc = be.lib.redheffer_halfspace_columns(dtcode(dtype), side, be.ptr(dbd), ctypes.addressof(ps), block, ctypes.addressof(pc), m, out.ptr(), N, B,
                                            piv.ptr(), info.ptr(), ws.ptr(), nws, be.stream)
    be.sync()
    ws.host()
    piv.host()
    assert _same_bits(be.host(dbd), bd)
    for x, h in zip(dS, S):
        assert _same_bits(be.host(x), h)
    return rc, out.host((B, n, m)), info.host()


def _column_cases():
    return [pytest.param(dtype, N, side, batch, id=f"{np.dtype(dtype).name}-N{N}-side{side}-b{batch}")
            for dtype in (np.complex128, np.complex64) for N in NS for side in (0, 1) for batch in (3, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,side,batch", _column_cases())
def test_halfspace_columns(backend, dtype, N, side, batch):
    """m = 16, 3, 1 columns of every block of both sides against the same columns of the reference: first / last column of both halves, the
    columns around the edge of probe_col_kernel's 256-thread x-block, one column twice; the m-column solve (ldb = m) across a second
    (N = 129) and a third (N = 257) outer block; batch 1 / 3; both dtypes."""
    be = get_backend(backend)
    _emu_skip(backend, N, dtype, batch)
    n = 2 * N
    pts = [_point(N, side, b, np.dtype(dtype).name) for b in range(batch)]
    for pt in pts:
        _assert_guards(pt)
    ratios = []
    for block in range(4):
        for cols in _column_lists(N):
            rc, got, info = _call_columns(be, dtype, side, [p.bd for p in pts], [p.S for p in pts], N, block, cols)
            assert rc == 0 and (info == 0).all(), (rc, info)
            for b, pt in enumerate(pts):
                pos, _ = pt.index(block, cols)
                ref, plain = pt.ref[block][:, pos], pt.plain[block][:, pos]
                _check(f"side {side} block {block} cols {cols} point {b}", got[b], ref, relmax(plain, ref), n, dtype, ratios)
    print(f"halfspace_columns side {side} worst err/max(e_plain, n eps) = {max(ratios):.3f}")


# ---- 3. the same call twice -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_halfspace_entries_repeat_bit_identical(backend, dtype):
    """Both entries called twice on the same inputs give the same bits: the three branches of the full product (blocks, XY, info) and the
    columns of a block of each side."""
    be, N, B = get_backend(backend), 37, 2
    for side in (0, 1):
        ins = [_inputs(N, side, b, dtype) for b in range(B)]
        bds, Ss = [i[0] for i in ins], [i[1] for i in ins]
        for want_xy in ((1, 0) if side == 0 else (1,)):
            first, second = [_call_halfspace(be, dtype, side, bds, Ss, N, want_xy) for _ in range(2)]
            assert first[0] == 0 and second[0] == 0 and _same_bits(first[3], second[3])
            assert all(_same_bits(x, y) for x, y in zip(first[1], second[1]))
            assert not want_xy or _same_bits(first[2], second[2])
        for block in (1, 2):
            first, second = [_call_columns(be, dtype, side, bds, Ss, N, block, [N, 0, 2 * N - 1]) for _ in range(2)]
            assert first[0] == 0 and second[0] == 0 and _same_bits(first[1], second[1]) and _same_bits(first[2], second[2])


# Worst err / max(e_plain, n eps) per test over all its cases (the bound is 16); no entry needed a margin of its own.
# Emulator: every case it runs; MI355X: all cases, from a `-m gpu -s` run, rounded up.  The largest ratios all belong to complex128 at N = 257
# (n = 514: three LU outer blocks, gemm_big; batch 3 above batch 1, which stays below 4.2); every case of the other sizes and of complex64 is
# below 3.  The e_plain of a columns case is that of the 1 - 16 columns compared and so varies more than a whole block's.
WORST_EMU = {"test_halfspace[xy0]": 3.4, "test_halfspace[lean]": 2.8, "test_halfspace[xy1]": 2.1, "test_halfspace_columns[side0]": 2.5,
             "test_halfspace_columns[side1]": 1.9}
WORST_MI355X = {"test_halfspace[xy0]": 4.5, "test_halfspace[lean]": 6.2, "test_halfspace[xy1]": 6.2, "test_halfspace_columns[side0]": 8.3,
                "test_halfspace_columns[side1]": 10.2}
