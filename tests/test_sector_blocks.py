"""trx_sym_fold_pair / trx_sym_fold_pair_bd through the C ABI (emulator + MI355X), DESIGN.md section 7 block-test policy.

Reference: T_kl^H M T_kr in numpy clongdouble from the DENSE T of the plan (plan.dense(); the plan itself is held to the definition of the mirrors
by tests/test_symmetry_blocks.py::test_plan_is_symmetry_basis).  The kernel never forms T: it gathers at most 16 elements of M per output element.
M is a random matrix, NOT one that commutes with the mirrors, so the blocks off the diagonal of T^H M T are as large as those on it.

Bound:  max |out - ref| <= 16 max(e_plain, n eps) max |ref|, e_plain the error of the same dense formula in the kernel's dtype through numpy
relative to max |ref|, eps = 2^-53 / the fp32 eps.  Every output carries guard words behind it.

Shapes: order [0,0] (n = 2: two of the four "xy" blocks are empty), [1,0] (n = 6: unequal extent, small), [3,2] (n = 70: blocks 17/18/18/17 under
"xy", the singleton m = 0 / n = 0 orbits) and the circular order set of test_symmetry_blocks.py; symmetry x, y, xy; c = n - 1 (complex weights)
and c = 0; batch 1 and 3; both dtypes.  Pairs: every (k, k), every (k, k'), and (0, 1), (2, 0) under two mirrors (rectangular where the sizes
differ, an empty side at [0,0]).
"""
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, crandn

LD = np.clongdouble
NX, NY = 40, 36
KINDS = ["rect00", "rect10", "rect32", "circ"]
GUARD = complex(-7.25, 3.5)


def _eps(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def _case(kind, sym, c):
    """(plan, T dense clongdouble)."""
    from torcwa_amd import lattice
    from torcwa_amd.symmetry import build_plan
    mn = lattice.circular_orders([300., 200.], n_harmonics=20) if kind == "circ" else lattice.rect_orders(int(kind[4]), int(kind[5]))
    cx, cy = (NX - 1, NY - 1) if c == "half" else (0, 0)
    plan = build_plan(mn, sym, cx if "x" in sym else 0, NX, cy if "y" in sym else 0, NY)
    return plan, plan.dense(LD)


def _pairs(plan):
    from torcwa_amd.symmetry import opposite_block
    nb = plan.nblk
    pairs = [(k, k) for k in range(nb)] + [(k, opposite_block(nb, k)) for k in range(nb)]
    if nb == 4:
        pairs += [(0, 1), (2, 0)]
    return pairs


def _plan_dev(be, plan, dtype, off=None):
    idx = np.concatenate([plan.idx.ravel(), np.full(4, -99, dtype=np.int32)])
    wt = np.concatenate([plan.wt.ravel().astype(dtype), np.full(4, GUARD, dtype=dtype)])
    off = np.concatenate([np.asarray(plan.off if off is None else off, dtype=np.int32), np.full(4, -99, dtype=np.int32)])
    hs = [be.dev(a) for a in (idx, wt, off)]

    def untouched():
        return all(np.array_equal(be.host(h), a) for h, a in zip(hs, (idx, wt, off)))
    return hs, untouched


def _call(be, entry, src, lead, plan, B, kl, kr, dtype, off=None):
    """One call of `entry` (sym_fold_pair: lead = n; sym_fold_pair_bd: lead = N).  Returns (rc, out [B, n_kl, n_kr])."""
    nl, nr = plan.sizes[kl], plan.sizes[kr]
    (idx, wt, offd), untouched = _plan_dev(be, plan, dtype, off)
    dsrc = be.dev(src)
    out = be.dev(np.full(B * nl * nr + 4, GUARD, dtype=dtype))
    rc = getattr(be.lib, entry)(dtcode(dtype), be.ptr(dsrc), lead, B, be.ptr(idx), be.ptr(wt), be.ptr(offd), plan.nblk, kl, kr, be.ptr(out), be.stream)
    o = be.host(out)
    assert (o[B * nl * nr:] == GUARD).all(), "guard words behind out"
    assert untouched() and np.array_equal(be.host(dsrc), src)                         # the plan and the operand are inputs
    return rc, o[:B * nl * nr].reshape(B, nl, nr)


def _check(got, M, T, plan, kl, kr, dtype, what):
    """got [B, n_kl, n_kr] against T_kl^H M T_kr in clongdouble under the block-test bound."""
    n = plan.n
    Tp = T.astype(dtype)
    sl, sr = slice(plan.off[kl], plan.off[kl + 1]), slice(plan.off[kr], plan.off[kr + 1])
    worst = 0.0
    for b in range(M.shape[0]):
        ref = T[:, sl].conj().T @ M[b].astype(LD) @ T[:, sr]
        assert got[b].shape == ref.shape
        if ref.size == 0:
            continue
        plain = Tp[:, sl].conj().T @ M[b] @ Tp[:, sr]
        scale = float(np.abs(ref).max())
        if scale == 0.0:
            assert (got[b] == 0).all(), (what, kl, kr, b)
            continue
        tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
        err = float(np.abs(got[b] - ref).max()) / scale
        worst = max(worst, err / tol)
        assert err <= tol, (what, kl, kr, b, err, tol)
    return worst


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("sym", ["x", "y", "xy"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_fold_pair(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T = _case(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(1000 * n + 10 * B + len(sym) + (c == "half"))
    M = crandn(rng, (B, n, n)).astype(dtype)
    if kind == "rect00" and sym == "xy":
        assert plan.sizes == [0, 1, 1, 0]
    if kind == "rect32" and sym == "xy":
        assert plan.sizes == [17, 18, 18, 17]
    worst = 0.0
    for kl, kr in _pairs(plan):
        rc, got = _call(be, "sym_fold_pair", M, n, plan, B, kl, kr, dtype)
        assert rc == 0
        worst = max(worst, _check(got, M, T, plan, kl, kr, dtype, "dense"))
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: sizes {plan.sizes}, worst error / bound = {worst:.2f}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c", ["half", "zero"])
@pytest.mark.parametrize("sym", ["x", "y", "xy"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_fold_pair_bd(backend, kind, sym, c, B, dtype):
    """Random diagonals [4, B, N] against the same reference on the dense 2x2-block-diagonal matrix; zeros of the result are written."""
    be = get_backend(backend)
    plan, T = _case(kind, sym, c)
    n = plan.n
    N = n // 2
    rng = np.random.default_rng(2000 * n + 10 * B + len(sym) + (c == "half"))
    bd = crandn(rng, (4, B, N)).astype(dtype)
    M = np.stack([_bd_dense(bd[:, b]) for b in range(B)]).astype(dtype)
    worst = 0.0
    for kl, kr in _pairs(plan):
        rc, got = _call(be, "sym_fold_pair_bd", bd, N, plan, B, kl, kr, dtype)
        assert rc == 0
        worst = max(worst, _check(got, M, T, plan, kl, kr, dtype, "bd"))
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: worst error / bound = {worst:.2f}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("sym", ["x", "xy"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_malformed_plan_and_bad_arguments(backend, sym, dtype):
    """A malformed off (its last entry is not n) fills out with NaN and nothing else; a block index outside [0, nblk), nblk outside [1, 4], an
    unknown dtype and a negative batch are refused; batch = 0 touches nothing."""
    be = get_backend(backend)
    plan, _ = _case("rect32", sym, "half")
    n, B = plan.n, 2
    N = n // 2
    rng = np.random.default_rng(7)
    M = crandn(rng, (B, n, n)).astype(dtype)
    bd = crandn(rng, (4, B, N)).astype(dtype)
    bad_off = np.array(plan.off, dtype=np.int32)
    bad_off[-1] = n - 1
    for entry, src, lead in (("sym_fold_pair", M, n), ("sym_fold_pair_bd", bd, N)):
        rc, got = _call(be, entry, src, lead, plan, B, 0, 0, dtype, off=bad_off)
        assert rc == 0 and got.size > 0 and np.isnan(got.real).all() and np.isnan(got.imag).all(), entry
        for kl, kr in ((plan.nblk, 0), (0, plan.nblk), (-1, 0), (0, -1)):
            fn = getattr(be.lib, entry)
            (idx, wt, off), _ = _plan_dev(be, plan, dtype)
            dsrc, out = be.dev(src), be.dev(np.full(B * n * n, GUARD, dtype=dtype))
            assert fn(dtcode(dtype), be.ptr(dsrc), lead, B, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, kl, kr, be.ptr(out), be.stream) == -2
            assert (be.host(out) == GUARD).all()
        fn = getattr(be.lib, entry)
        (idx, wt, off), _ = _plan_dev(be, plan, dtype)
        dsrc, out = be.dev(src), be.dev(np.full(B * n * n, GUARD, dtype=dtype))
        args = [be.ptr(dsrc), lead, B, be.ptr(idx), be.ptr(wt), be.ptr(off)]
        assert fn(dtcode(dtype), *args, 5, 0, 0, be.ptr(out), be.stream) == -2
        assert fn(dtcode(dtype), *args, 0, 0, 0, be.ptr(out), be.stream) == -2
        assert fn(7, *args, plan.nblk, 0, 0, be.ptr(out), be.stream) == -1
        assert fn(dtcode(dtype), be.ptr(dsrc), lead, -1, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, 0, 0, be.ptr(out), be.stream) == -2
        assert fn(dtcode(dtype), None, lead, 0, None, None, None, plan.nblk, 0, 0, None, be.stream) == 0                 # batch = 0
        assert fn(dtcode(dtype), None, lead, B, be.ptr(idx), be.ptr(wt), be.ptr(off), plan.nblk, 0, 0, be.ptr(out), be.stream) == -2
        assert (be.host(out) == GUARD).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_engine_wrappers(backend):
    """Engine.sym_fold_pair / sym_fold_pair_bd return [B, n_kl, n_kr] tensors equal to the C ABI's output, and refuse a foreign plan or block."""
    import torch
    from tests.test_pipeline import make_engine
    eng = make_engine(backend)
    plan, T = _case("rect32", "xy", "half")
    n, B = plan.n, 2
    rng = np.random.default_rng(11)
    M = crandn(rng, (B, n, n))
    bd = crandn(rng, (4, B, n // 2))
    got = eng.sym_fold_pair(torch.from_numpy(M).to(eng.device), plan, 0, 3).cpu().numpy()
    assert got.shape == (B, 17, 17)
    _check(got, M, T, plan, 0, 3, np.complex128, "engine")
    got = eng.sym_fold_pair_bd(torch.from_numpy(bd).to(eng.device), plan, 1, 2).cpu().numpy()
    Md = np.stack([_bd_dense(bd[:, b]) for b in range(B)])
    _check(got, Md, T, plan, 1, 2, np.complex128, "engine bd")
    with pytest.raises(ValueError):
        eng.sym_fold_pair(torch.from_numpy(M).to(eng.device), plan, 0, 4)
    with pytest.raises(ValueError):
        eng.sym_fold_pair(torch.from_numpy(M[:, :10, :10].copy()).to(eng.device), plan, 0, 0)
    with pytest.raises(ValueError):
        eng.sym_fold_pair_bd(torch.from_numpy(bd[:3].copy()).to(eng.device), plan, 0, 0)
