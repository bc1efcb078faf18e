"""trx_sym_fold_backward / trx_sym_unfold_backward through the C ABI (emulator + MI355X), DESIGN.md section 7 block-test policy.

Reference: gA = sum_k T_k gB_k T_k^H and gW_k = T_k^H gW[:, block k] in numpy clongdouble from the DENSE T of plan.dense() (the kernels never form
T: the first gathers through the row plan, the second combines rows).  The row plan itself is held to plan.dense() by
test_row_plan_reproduces_dense.

Bound:  max |out - ref| <= 16 max(e_plain, n eps) max |ref|, e_plain the error of the same dense formulas in the kernel's dtype through numpy
relative to max |ref|, eps = 2^-53 / the fp32 eps -- the bound of the forward kernels (tests/test_symmetry_blocks.py).  glam_k is a copy: exact.

Dot-product tests tie each backward to the forward kernel that exists already: <L x, y> = <x, L^H y> with <a, b> = sum conj(a) b.  Both sides
are summed in clongdouble from the kernels' outputs, so what separates them is the element error of the two kernels, each within the bound
above with e_plain <= n eps (a kernel sums at most 16 products per element): 16 n eps (max |L x| sum |y| + max |L^H y| sum |x|).

Shapes: those of tests/test_symmetry_blocks.py -- order [3,2] (n = 70: blocks 35/35 and 17/18/18/17) and the circular order set; symmetries x, y,
xy; c = n - 1 (complex weights) and c = 0; batch 1 and 3; both dtypes.
"""
import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import crandn
from tests.test_symmetry_blocks import GUARD, LD, SHAPES, _case, _eps, _fold, _pack, _plan_dev, _unfold, _unpack

PARAMS = [pytest.mark.parametrize("dtype", [np.complex64, np.complex128]), pytest.mark.parametrize("B", [1, 3]),
          pytest.mark.parametrize("c", ["half", "zero"]), pytest.mark.parametrize("kind,sym", SHAPES),
          pytest.mark.parametrize("backend", BACKENDS)]


def _all(fn):
    for p in PARAMS:
        fn = p(fn)
    return fn


def _rows_dev(be, plan, dtype):
    """Row plan and off with guard words behind them, and a check that the call left them alone."""
    ridx, rwt = plan.rows()
    arrs = (np.concatenate([ridx.ravel(), np.full(4, -99, dtype=np.int32)]), np.concatenate([rwt.ravel().astype(dtype), np.full(4, GUARD, dtype=dtype)]),
            np.concatenate([np.asarray(plan.off, dtype=np.int32), np.full(4, -99, dtype=np.int32)]))
    hs = [be.dev(a) for a in arrs]

    def untouched():
        return all(np.array_equal(be.host(h), a) for h, a in zip(hs, arrs))
    return hs, untouched


def _fold_backward(be, G, plan, B, dtype, off_override=None):
    """gA [B,n,n] of the per-block gradients G (list of [B,s,s]); guards, inputs unchanged, argument checks."""
    n = plan.n
    (ridx, rwt, off), untouched = _rows_dev(be, plan, dtype)
    if off_override is not None:
        off = be.dev(np.asarray(off_override, dtype=np.int32))
    Gp = _pack(G, plan, B).astype(dtype)
    dG = be.dev(Gp)
    gA = be.dev(np.full(B * n * n + 4, GUARD, dtype=dtype))
    dt = dtcode(dtype)
    rc = be.lib.sym_fold_backward(dt, be.ptr(dG), n, B, be.ptr(ridx), be.ptr(rwt), be.ptr(off), plan.nblk, be.ptr(gA), be.stream)
    assert rc == 0
    o = be.host(gA)
    assert (o[B * n * n:] == GUARD).all() and untouched() and np.array_equal(be.host(dG), Gp)
    args = [be.ptr(dG), n, B, be.ptr(ridx), be.ptr(rwt), be.ptr(off)]
    assert be.lib.sym_fold_backward(dt, *args, 5, be.ptr(gA), be.stream) == -2
    assert be.lib.sym_fold_backward(dt, *args, 0, be.ptr(gA), be.stream) == -2
    assert be.lib.sym_fold_backward(7, *args, plan.nblk, be.ptr(gA), be.stream) == -1
    assert be.lib.sym_fold_backward(dt, *args, plan.nblk, None, be.stream) == -2
    assert be.lib.sym_fold_backward(dt, be.ptr(dG), n, 65536, *args[3:], plan.nblk, be.ptr(gA), be.stream) == -2
    assert be.lib.sym_fold_backward(dt, None, n, 0, None, None, None, plan.nblk, None, be.stream) == 0                      # batch = 0
    assert be.host(gA).tobytes() == o.tobytes()                                        # none of the refused calls wrote
    return o[:B * n * n].reshape(B, n, n)


def _unfold_backward(be, gW, glam, plan, dtype, off_override=None):
    """(gWk, glamk) per block from gW [B,n,n], glam [B,n]; guards, inputs unchanged, argument checks."""
    B, n, _ = gW.shape
    tot = B * sum(s * s for s in plan.sizes)
    (idx, wt, off), untouched = _plan_dev(be, plan, dtype)
    if off_override is not None:
        off = be.dev(np.asarray(off_override, dtype=np.int32))
    dW, dl = be.dev(gW), be.dev(glam)
    gWk = be.dev(np.full(tot + 4, GUARD, dtype=dtype))
    glamk = be.dev(np.full(B * n + 4, GUARD, dtype=dtype))
    dt = dtcode(dtype)
    rc = be.lib.sym_unfold_backward(dt, be.ptr(dW), be.ptr(dl), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, be.ptr(gWk), be.ptr(glamk),
                                    be.stream)
    assert rc == 0
    w, l = be.host(gWk), be.host(glamk)
    assert (w[tot:] == GUARD).all() and (l[B * n:] == GUARD).all() and untouched()
    assert np.array_equal(be.host(dW), gW) and np.array_equal(be.host(dl), glam)
    args = [be.ptr(dW), be.ptr(dl), n, B, be.ptr(idx), be.ptr(wt), be.ptr(off)]
    assert be.lib.sym_unfold_backward(dt, *args, 5, be.ptr(gWk), be.ptr(glamk), be.stream) == -2
    assert be.lib.sym_unfold_backward(7, *args, plan.nblk, be.ptr(gWk), be.ptr(glamk), be.stream) == -1
    assert be.lib.sym_unfold_backward(dt, *args, plan.nblk, be.ptr(gWk), None, be.stream) == -2
    assert be.lib.sym_unfold_backward(dt, None, None, n, 0, None, None, None, plan.nblk, None, None, be.stream) == 0       # batch = 0
    assert be.host(gWk).tobytes() == w.tobytes() and be.host(glamk).tobytes() == l.tobytes()     # none of the refused calls wrote
    if off_override is not None:
        return w[:tot], l[:B * n]
    return _unpack(w[:tot], plan, B, True), _unpack(l[:B * n], plan, B, False)


def _dot(a, b):
    return complex(np.sum(np.conj(a.astype(LD)) * b.astype(LD)))


@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("kind,sym", SHAPES)
def test_row_plan_reproduces_dense(kind, sym, c):
    """T rebuilt from the row plan alone equals plan.dense(): slot k of row r names a column of block k, a slot without a column has weight 0,
    and a row lies in at most four columns in all."""
    plan, T, _ = _case(kind, sym, c)
    ridx, rwt = plan.rows()
    n = plan.n
    assert ridx.shape == (n, 4) and rwt.shape == (n, 4) and ridx.dtype == np.int32 and ridx.flags.c_contiguous
    R = np.zeros((n, n), dtype=np.complex128)
    for r in range(n):
        for k in range(4):
            if rwt[r, k] != 0:
                assert k < plan.nblk and plan.off[k] <= ridx[r, k] < plan.off[k + 1]
                R[r, ridx[r, k]] = rwt[r, k]
    assert np.array_equal(R, plan.dense(np.complex128))
    assert ((np.abs(T) > 0).sum(axis=1) <= 4).all() and ((rwt != 0).sum(axis=1) == (np.abs(T) > 0).sum(axis=1)).all()
    assert plan.rows()[0] is ridx                                                     # built once


@_all
def test_sym_fold_backward(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T, _ = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(400 * n + 10 * B + len(sym) + (c == "half"))
    G = [crandn(rng, (B, s, s)).astype(dtype) for s in plan.sizes]
    got = _fold_backward(be, G, plan, B, dtype)
    Tp = T.astype(dtype)
    worst = 0.0
    for b in range(B):
        ref = np.zeros((n, n), dtype=LD)
        plain = np.zeros((n, n), dtype=dtype)
        for k in range(plan.nblk):
            sl = slice(plan.off[k], plan.off[k + 1])
            ref += T[:, sl] @ G[k][b].astype(LD) @ T[:, sl].conj().T
            plain += Tp[:, sl] @ G[k][b] @ Tp[:, sl].conj().T
        scale = float(np.abs(ref).max())
        tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
        err = float(np.abs(got[b] - ref).max()) / scale
        worst = max(worst, err / tol)
        assert err <= tol, (b, err, tol)
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: worst error / bound = {worst:.3f}")


@_all
def test_sym_unfold_backward(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T, _ = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(500 * n + 10 * B + len(sym) + (c == "half"))
    gW, glam = crandn(rng, (B, n, n)).astype(dtype), crandn(rng, (B, n)).astype(dtype)
    gWk, glamk = _unfold_backward(be, gW, glam, plan, dtype)
    assert np.array_equal(np.concatenate(glamk, axis=1), glam)                         # a copy: exact
    Tp = T.astype(dtype)
    worst = 0.0
    for b in range(B):
        for k in range(plan.nblk):
            sl = slice(plan.off[k], plan.off[k + 1])
            ref = T[:, sl].conj().T @ gW[b][:, sl].astype(LD)
            plain = Tp[:, sl].conj().T @ gW[b][:, sl]
            scale = float(np.abs(ref).max())
            tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
            err = float(np.abs(gWk[k][b] - ref).max()) / scale
            worst = max(worst, err / tol)
            assert err <= tol, (b, k, err, tol)
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: worst error / bound = {worst:.3f}")


@_all
def test_fold_dot_product(backend, kind, sym, c, B, dtype):
    """<sym_fold(A), G> = <A, sym_fold_backward(G)> for a random A (no mirror: the fold drops its off-block part, and so does the adjoint)."""
    be = get_backend(backend)
    plan, _, _ = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(600 * n + 10 * B + len(sym) + (c == "half"))
    A = crandn(rng, (B, n, n)).astype(dtype)
    G = [crandn(rng, (B, s, s)).astype(dtype) for s in plan.sizes]
    blocks, _ = _fold(be, A, plan, dtype)
    gA = _fold_backward(be, G, plan, B, dtype)
    lhs = sum(_dot(blocks[k], G[k]) for k in range(plan.nblk))
    rhs = _dot(A, gA)
    tol = 16 * n * _eps(dtype) * (max(float(np.abs(x).max()) for x in blocks) * sum(float(np.abs(g).sum()) for g in G)
                                  + float(np.abs(gA).max()) * float(np.abs(A).sum()))
    print(f"<fold A, G> = {lhs:.6g}, <A, fold^H G> = {rhs:.6g}, |difference| {abs(lhs - rhs):.2e}, bound {tol:.2e}")
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= tol


@_all
def test_unfold_dot_product(backend, kind, sym, c, B, dtype):
    """<sym_unfold(Wk, lamk), (gW, glam)> = <(Wk, lamk), sym_unfold_backward(gW, glam)>."""
    be = get_backend(backend)
    plan, _, _ = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(700 * n + 10 * B + len(sym) + (c == "half"))
    Wk = [crandn(rng, (B, s, s)).astype(dtype) for s in plan.sizes]
    lamk = [crandn(rng, (B, s)).astype(dtype) for s in plan.sizes]
    gW, glam = crandn(rng, (B, n, n)).astype(dtype), crandn(rng, (B, n)).astype(dtype)
    W, lam = _unfold(be, Wk, lamk, plan, B, dtype)
    gWk, glamk = _unfold_backward(be, gW, glam, plan, dtype)
    lhs = _dot(W, gW) + _dot(lam, glam)
    rhs = sum(_dot(Wk[k], gWk[k]) + _dot(lamk[k], glamk[k]) for k in range(plan.nblk))
    tol = 16 * n * _eps(dtype) * (float(np.abs(W).max()) * float(np.abs(gW).sum())
                                  + max(float(np.abs(x).max()) for x in gWk) * sum(float(np.abs(w).sum()) for w in Wk))
    print(f"<unfold x, y> = {lhs:.6g}, <x, unfold^H y> = {rhs:.6g}, |difference| {abs(lhs - rhs):.2e}, bound {tol:.2e}")
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= tol


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("backend", BACKENDS)
def test_malformed_off(backend, dtype):
    """An off that is not monotone from 0 to n: gA is NaN throughout; glamk (batch n elements whatever the blocks) is NaN throughout and gWk,
    whose packing off would define, is left alone.  Nothing is written behind an output."""
    be = get_backend(backend)
    plan, _, _ = _case("rect32", "xy", "half")
    n, B = plan.n, 2
    rng = np.random.default_rng(8)
    bad = [0, 40, 20, 50, n]
    gA = _fold_backward(be, [crandn(rng, (B, s, s)).astype(dtype) for s in plan.sizes], plan, B, dtype, off_override=bad)
    assert np.isnan(gA.real).all() and np.isnan(gA.imag).all()
    w, l = _unfold_backward(be, crandn(rng, (B, n, n)).astype(dtype), crandn(rng, (B, n)).astype(dtype), plan, dtype, off_override=bad)
    assert np.isnan(l.real).all() and np.isnan(l.imag).all() and (w == GUARD).all()
