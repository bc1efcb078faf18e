"""trx_redheffer_halfspace_columns (include/trx.h): m columns of one block of a half-space star product, against the same columns of the
full products of the library (trx_redheffer_halfspace, and trx_redheffer on the densified half-space) and of the reference's formulas.

Sizes, data scales and per-dtype tolerances are those of tests/test_blocks.py::test_redheffer_halfspace (N = 37, batch 2, blocks 0.3 x and
diagonals 0.4 x complex normal; 1e-11 for complex128, 2e-4 for complex64, max-abs error over max-abs of the reference BLOCK).  Every buffer
the call writes carries guard words behind the size the header states, and the workspace has exactly *_ws_bytes (tests/test_smatrix_blocks.py).
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, _star, crandn
from tests.test_smatrix_blocks import Guarded

N, BATCH = 37, 2
TOLS = [(np.complex128, 1e-11), (np.complex64, 2e-4)]
# (column lists) m = 1 and m = 2, indices in both halves (c < N and c >= N), first / last column, a repeated column
COLS = [[0], [N + 5], [2 * N - 1], [3, N + 3], [N + 20, 11], [N, N]]


def _inputs(dtype, seed=0):
    rng = np.random.default_rng([777, seed, np.dtype(dtype).itemsize])
    bd = (0.4 * crandn(rng, (4, 4, BATCH, N))).astype(dtype)
    S = [(0.3 * crandn(rng, (BATCH, 2 * N, 2 * N))).astype(dtype) for _ in range(4)]
    return bd, S


def _arr(ptrs):
    return (ctypes.c_void_p * 4)(*ptrs)


def _full_halfspace(be, dtype, side, bd, S):
    """The four blocks of trx_redheffer_halfspace (with coupling factors: the path both sides share) and its info."""
    n = 2 * N
    dbd, dS = be.dev(bd), [be.dev(x) for x in S]
    out = [be.empty((BATCH, n, n), dtype) for _ in range(4)]
    XY = be.empty((2, BATCH, n, 2 * n), dtype)
    piv, info = be.empty((BATCH, n), np.int32), be.dev(np.full((BATCH,), -7, dtype=np.int32))
    nws = be.lib.redheffer_halfspace_ws_bytes(dtcode(dtype), N, BATCH, side, 1)
    ws = be.empty((nws,), np.uint8)
    ps, po = _arr([be.ptr(x) for x in dS]), _arr([be.ptr(x) for x in out])
    rc = be.lib.redheffer_halfspace(dtcode(dtype), side, be.ptr(dbd), ctypes.addressof(ps), ctypes.addressof(po), be.ptr(XY), N, BATCH,
                                    be.ptr(piv), be.ptr(info), be.ptr(ws), nws, be.stream)
    assert rc == 0
    return [be.host(x) for x in out], be.host(info)


def _full_dense(be, dtype, side, bd, S):
    """The four blocks of the dense trx_redheffer with the half-space densified."""
    n = 2 * N
    D = [np.stack([_bd_dense(bd[k, :, b]) for b in range(BATCH)]).astype(dtype) for k in range(4)]
    Sm, Sn = (D, S) if side == 0 else (S, D)
    dm, dn = [be.dev(x) for x in Sm], [be.dev(x) for x in Sn]
    out = [be.empty((BATCH, n, n), dtype) for _ in range(4)]
    XY = be.empty((2, BATCH, n, 2 * n), dtype)
    piv, info = be.empty((BATCH, n), np.int32), be.dev(np.full((BATCH,), -7, dtype=np.int32))
    nws = be.lib.redheffer_ws_bytes(dtcode(dtype), n, BATCH)
    ws = be.empty((nws,), np.uint8)
    pm, pn, po = _arr([be.ptr(x) for x in dm]), _arr([be.ptr(x) for x in dn]), _arr([be.ptr(x) for x in out])
    rc = be.lib.redheffer(dtcode(dtype), ctypes.addressof(pm), ctypes.addressof(pn), ctypes.addressof(po), be.ptr(XY), n, BATCH, be.ptr(piv),
                          be.ptr(info), be.ptr(ws), nws, be.stream)
    assert rc == 0 and (be.host(info) == 0).all()
    return [be.host(x) for x in out]


@functools.lru_cache(maxsize=None)
def _references(backend, dtname, side):
    be, dtype = get_backend(backend), np.dtype(dtname).type
    bd, S = _inputs(dtype)
    half, info = _full_halfspace(be, dtype, side, bd, S)
    assert (info == 0).all()
    dense = _full_dense(be, dtype, side, bd, S)
    formulas = []
    for b in range(BATCH):
        D = [_bd_dense(bd[k, :, b].astype(np.complex128)) for k in range(4)]
        Sd = [x[b].astype(np.complex128) for x in S]
        formulas.append(_star(D, Sd) if side == 0 else _star(Sd, D))
    formulas = [np.stack([formulas[b][k] for b in range(BATCH)]) for k in range(4)]
    return half, dense, formulas


def _call(be, dtype, side, bd, S, block, cols, ws_short=0, m=None):
    """One call through the C ABI with guarded output, piv, info and an exactly sized guarded workspace.  Returns (rc, out, info)."""
    n, m = 2 * N, len(cols) if m is None else m
    dbd, dS = be.dev(bd), [be.dev(x) for x in S]
    out = Guarded(be, BATCH * n * max(m, 1), dtype)
    piv, info = Guarded(be, BATCH * n, np.int32), Guarded(be, BATCH, np.int32, body=np.full(BATCH, -7))
    nws = be.lib.redheffer_halfspace_columns_ws_bytes(dtcode(dtype), N, BATCH, max(m, 1))
    assert nws == np.dtype(dtype).itemsize * BATCH * (n * n + 3 * n * max(m, 1))
    ws = Guarded(be, nws, np.uint8)
    ps = _arr([be.ptr(x) for x in dS])
    pc = (ctypes.c_int * max(len(cols), 1))(*cols)
    rc = be.lib.redheffer_halfspace_columns(dtcode(dtype), side, be.ptr(dbd), ctypes.addressof(ps), block, ctypes.addressof(pc), m, out.ptr(),
                                            N, BATCH, piv.ptr(), info.ptr(), ws.ptr(), nws - ws_short, be.stream)
    be.sync()
    ws.host()
    piv.host()
    for x, ref in zip(dS, S):                                    # the inputs are not modified
        assert (be.host(x) == ref).all()
    return rc, out.host((BATCH, n, max(m, 1))), info.host()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", TOLS)
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("block", [0, 1, 2, 3])
def test_columns_against_full_products(backend, dtype, tol, side, block):
    be = get_backend(backend)
    bd, S = _inputs(dtype)
    half, dense, formulas = _references(backend, np.dtype(dtype).name, side)
    for cols in COLS:
        rc, got, info = _call(be, dtype, side, bd, S, block, cols)
        assert rc == 0 and (info == 0).all()
        for name, ref in (("trx_redheffer_halfspace", half), ("trx_redheffer", dense), ("formulas", formulas)):
            for b in range(BATCH):
                scale = np.abs(formulas[block][b]).max()
                for q, c in enumerate(cols):
                    err = np.abs(got[b, :, q].astype(np.complex128) - ref[block][b][:, c]).max() / scale
                    print(f"side {side} block {block} cols {cols} point {b} column {c} vs {name}: {err:.3e}")
                    assert err < tol, (name, side, block, cols, b, c, err)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("side", [0, 1])
def test_columns_workspace_and_arguments(backend, side):
    """One byte less than *_ws_bytes is refused (and nothing is written); so are a block, a column index or a column count out of range."""
    be, dtype = get_backend(backend), np.complex128
    bd, S = _inputs(dtype)
    n = 2 * N
    for kw, want in ((dict(cols=[1, N + 1], ws_short=1), -3), (dict(cols=[n]), -2), (dict(cols=[-1]), -2), (dict(cols=[0], block=4), -2),
                     (dict(cols=[0], block=-1), -2), (dict(cols=[0], m=0), -2), (dict(cols=list(range(17))), -2)):
        kw.setdefault("block", 1)
        rc, got, info = _call(be, dtype, side, bd, S, **kw)
        assert rc == want, (kw, rc)
        assert np.isnan(got).all() and (info == -7).all()        # untouched
    rc, got, info = _call(be, dtype, side, bd, S, 1, list(range(16)))          # the largest column count
    assert rc == 0 and (info == 0).all() and np.isfinite(got).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", TOLS)
@pytest.mark.parametrize("side", [0, 1])
def test_columns_info_of_singular_K(backend, dtype, tol, side):
    """Point 1 of 2 has K = I - Sm12 Sn21 = 0 exactly (the coupled half-space block is the identity, the dense one too): info[1] reports it, with the
    value the full product reports for the same inputs; point 0 has info 0 and correct columns."""
    be = get_backend(backend)
    bd, S = _inputs(dtype, seed=1)
    n = 2 * N
    kb, ks = (2, 1) if side == 0 else (1, 2)                     # side 0: K = I - D12 S21;  side 1: K = I - S12 D21
    bd[kb, :, 1] = 0
    bd[kb, 0, 1] = bd[kb, 3, 1] = 1
    S[ks][1] = np.eye(n)
    _, info_full = _full_halfspace(be, dtype, side, bd, S)
    rc, got, info = _call(be, dtype, side, bd, S, 1, [2, N + 2])
    assert rc == 0
    assert info[0] == 0 and info[1] != 0 and (info == info_full).all(), (info, info_full)
    D = [_bd_dense(bd[k, :, 0].astype(np.complex128)) for k in range(4)]
    Sd = [x[0].astype(np.complex128) for x in S]
    ref = (_star(D, Sd) if side == 0 else _star(Sd, D))[1]
    for q, c in enumerate([2, N + 2]):
        assert np.abs(got[0, :, q] - ref[:, c]).max() / np.abs(ref).max() < tol
