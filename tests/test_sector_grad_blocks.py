"""trx_sym_fold_pairs_backward / trx_sym_fold_pair_bd_backward through the C ABI (emulator + MI355X), DESIGN.md section 7 block-test policy.

Reference: gM = sum_p T_kl_p G_p T_kr_p^H, and the four diagonals of T_kl G T_kr^H, in numpy clongdouble from the DENSE T of plan.dense() (the
kernels never form T: they gather through the row plan, which tests/test_symmetry_grad_blocks.py::test_row_plan_reproduces_dense holds to
plan.dense()).

Bound (that of tests/test_symmetry_grad_blocks.py):  max |out - ref| <= 16 max(e_plain, n eps) max |ref|, e_plain the error of the same dense
formula in the kernel's dtype through numpy relative to max |ref|, eps = 2^-53 / the fp32 eps.  A reference that is 0 throughout (no pair, or
only null pointers) is met exactly.

Dot-product tests tie each adjoint to its forward kernel: <fold_pair(M), G> = <M, backward(G)> with <a, b> = sum conj(a) b, both sides summed in
clongdouble from the kernels' outputs, tolerance 16 n eps (max |L x| sum |y| + max |L^H y| sum |x|) as in that file.

Shapes: the SHAPES of tests/test_symmetry_blocks.py -- order [3,2] (n = 70: nine row groups, the last ragged) and the circular order set (blocks
of different sizes, rectangular pairs), symmetries x, y, xy; c = n - 1 and c = 0; batch 1 and 3; both dtypes; and order [6,5] (n = 286 > the 256
threads of a workgroup: the column loop takes a second trip) once per symmetry.  Pair sets: one (rectangular where sizes differ) pair, the P
pattern (k, k') of all k, the Q pattern (k', k), all nblk^2 pairs, that set with every other pointer null (bit-equal to the same set with those
G zero-filled) and all pointers null (exact zeros).
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, crandn
from tests.test_sector_blocks import _call as _fold_pair_call
from tests.test_sector_blocks import _case as _case_rect
from tests.test_sector_blocks import _pairs as _bd_pairs
from tests.test_symmetry_blocks import GUARD, LD, NX, NY, SHAPES, _case, _eps
from tests.test_symmetry_grad_blocks import _dot, _rows_dev

PARAMS = [pytest.mark.parametrize("dtype", [np.complex64, np.complex128]), pytest.mark.parametrize("B", [1, 3]),
          pytest.mark.parametrize("c", ["half", "zero"]), pytest.mark.parametrize("kind,sym", SHAPES),
          pytest.mark.parametrize("backend", BACKENDS)]


def _all(fn):
    for p in PARAMS:
        fn = p(fn)
    return fn


def _plan(kind, sym, c):
    """(plan, T dense clongdouble) of a SHAPES kind, or of "rect65" (order [6,5], n = 286)."""
    return _case_rect(kind, sym, c) if kind == "rect65" else _case(kind, sym, c)[:2]


@functools.lru_cache(maxsize=None)
def _wide_plan(sym):
    """(plan, T dense clongdouble) of order [12,5]: N = 275 > 256."""
    from torcwa_amd import lattice
    from torcwa_amd.symmetry import build_plan
    plan = build_plan(lattice.rect_orders(12, 5), sym, NX - 1 if "x" in sym else 0, NX, NY - 1 if "y" in sym else 0, NY)
    return plan, plan.dense(LD)


def _pair_sets(plan):
    from torcwa_amd.symmetry import opposite_block
    nb = plan.nblk
    opp = [opposite_block(nb, k) for k in range(nb)]
    return {"single": [(0, 1)], "P": [(k, opp[k]) for k in range(nb)], "Q": [(opp[k], k) for k in range(nb)],
            "all": [(kl, kr) for kl in range(nb) for kr in range(nb)]}


def _table(be, G, pairs):
    """Host arrays of the pair table: device pointers (None for a null pair), kl, kr; and the device buffers, guard words behind each."""
    m = len(pairs)
    bufs = [None if g is None else np.concatenate([g.ravel(), np.full(4, GUARD, dtype=g.dtype)]) for g in G]
    devs = [None if a is None else be.dev(a) for a in bufs]
    pg = (ctypes.c_void_p * max(m, 1))(*[None if d is None else be.ptr(d) for d in devs])
    pl = (ctypes.c_int * max(m, 1))(*[p[0] for p in pairs])
    pr = (ctypes.c_int * max(m, 1))(*[p[1] for p in pairs])

    def untouched():
        return all(d is None or np.array_equal(be.host(d), a) for d, a in zip(devs, bufs))
    return (pg, pl, pr), devs, untouched


def _pairs_backward(be, G, pairs, plan, B, dtype, off_override=None, refusals=False):
    """gM [B,n,n] of the per-pair gradients G (list of [B, n_kl, n_kr] or None); guards, inputs unchanged and, with `refusals`, every
    refused-argument return code and that none of those calls wrote."""
    n, m = plan.n, len(pairs)
    (ridx, rwt, off), plan_untouched = _rows_dev(be, plan, dtype)
    if off_override is not None:
        off = be.dev(np.asarray(off_override, dtype=np.int32))
    (pg, pl, pr), devs, g_untouched = _table(be, G, pairs)
    gM = be.dev(np.full(B * n * n + 4, GUARD, dtype=dtype))
    dt = dtcode(dtype)
    fn = be.lib.sym_fold_pairs_backward
    adr = ctypes.addressof
    rc = fn(dt, adr(pg), adr(pl), adr(pr), m, n, B, be.ptr(ridx), be.ptr(rwt), be.ptr(off), plan.nblk, be.ptr(gM), be.stream)
    assert rc == 0
    o = be.host(gM)
    assert (o[B * n * n:] == GUARD).all() and plan_untouched() and g_untouched()
    if refusals:
        tab, tail = [adr(pg), adr(pl), adr(pr), m, n, B], [be.ptr(ridx), be.ptr(rwt), be.ptr(off)]
        assert fn(dt, *tab, *tail, 5, be.ptr(gM), be.stream) == -2
        assert fn(dt, *tab, *tail, 0, be.ptr(gM), be.stream) == -2
        assert fn(7, *tab, *tail, plan.nblk, be.ptr(gM), be.stream) == -1
        assert fn(dt, *tab, *tail, plan.nblk, None, be.stream) == -2
        assert fn(dt, adr(pg), adr(pl), adr(pr), m, n, 65536, *tail, plan.nblk, be.ptr(gM), be.stream) == -2
        assert fn(dt, adr(pg), adr(pl), adr(pr), 17, n, B, *tail, plan.nblk, be.ptr(gM), be.stream) == -2
        assert fn(dt, adr(pg), adr(pl), adr(pr), -1, n, B, *tail, plan.nblk, be.ptr(gM), be.stream) == -2
        assert fn(dt, None, adr(pl), adr(pr), m, n, B, *tail, plan.nblk, be.ptr(gM), be.stream) == -2
        for bad_l, bad_r in ((plan.nblk, 0), (0, plan.nblk), (-1, 0), (0, -1)):          # a block outside [0, nblk), also behind a null pointer
            bl = (ctypes.c_int * m)(*([p[0] for p in pairs[:-1]] + [bad_l]))
            br = (ctypes.c_int * m)(*([p[1] for p in pairs[:-1]] + [bad_r]))
            assert fn(dt, adr(pg), adr(bl), adr(br), m, n, B, *tail, plan.nblk, be.ptr(gM), be.stream) == -2
        assert fn(dt, None, None, None, m, n, 0, None, None, None, plan.nblk, None, be.stream) == 0                       # batch = 0
        assert be.host(gM).tobytes() == o.tobytes()                                    # none of the refused calls wrote
    return o[:B * n * n].reshape(B, n, n)


def _pair_bd_backward(be, G, plan, kl, kr, dtype, off_override=None, refusals=False):
    """gbd [4,B,N] of G [B, n_kl, n_kr]; guards, inputs unchanged, argument checks."""
    B, N = G.shape[0], plan.n // 2
    (ridx, rwt, off), plan_untouched = _rows_dev(be, plan, dtype)
    if off_override is not None:
        off = be.dev(np.asarray(off_override, dtype=np.int32))
    Gg = np.concatenate([G.ravel(), np.full(4, GUARD, dtype=dtype)])
    dG = be.dev(Gg)
    gbd = be.dev(np.full(4 * B * N + 4, GUARD, dtype=dtype))
    dt = dtcode(dtype)
    fn = be.lib.sym_fold_pair_bd_backward
    rc = fn(dt, be.ptr(dG), N, B, be.ptr(ridx), be.ptr(rwt), be.ptr(off), plan.nblk, kl, kr, be.ptr(gbd), be.stream)
    assert rc == 0
    o = be.host(gbd)
    assert (o[4 * B * N:] == GUARD).all() and plan_untouched() and np.array_equal(be.host(dG), Gg)
    if refusals:
        args = [be.ptr(dG), N, B, be.ptr(ridx), be.ptr(rwt), be.ptr(off)]
        assert fn(dt, *args, 5, kl, kr, be.ptr(gbd), be.stream) == -2
        assert fn(dt, *args, 0, 0, 0, be.ptr(gbd), be.stream) == -2
        assert fn(7, *args, plan.nblk, kl, kr, be.ptr(gbd), be.stream) == -1
        assert fn(dt, *args, plan.nblk, kl, kr, None, be.stream) == -2
        assert fn(dt, None, *args[1:], plan.nblk, kl, kr, be.ptr(gbd), be.stream) == -2
        assert fn(dt, be.ptr(dG), N, 65536, *args[3:], plan.nblk, kl, kr, be.ptr(gbd), be.stream) == -2
        assert fn(dt, be.ptr(dG), 0, B, *args[3:], plan.nblk, kl, kr, be.ptr(gbd), be.stream) == -2
        for bl, br in ((plan.nblk, 0), (0, plan.nblk), (-1, 0), (0, -1)):
            assert fn(dt, *args, plan.nblk, bl, br, be.ptr(gbd), be.stream) == -2
        assert fn(dt, None, N, 0, None, None, None, plan.nblk, kl, kr, None, be.stream) == 0                              # batch = 0
        assert be.host(gbd).tobytes() == o.tobytes()                                   # none of the refused calls wrote
    return o[:4 * B * N].reshape(4, B, N)


def _reference(G, pairs, T, plan, b, dtype):
    """(ref clongdouble, the same formula in `dtype`) of sum_p T_kl G_p[b] T_kr^H over the pairs with a gradient."""
    n = plan.n
    Tp = T.astype(dtype)
    ref, plain = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=dtype)
    for g, (kl, kr) in zip(G, pairs):
        if g is None:
            continue
        sl, sr = slice(plan.off[kl], plan.off[kl + 1]), slice(plan.off[kr], plan.off[kr + 1])
        ref += T[:, sl] @ g[b].astype(LD) @ T[:, sr].conj().T
        plain += Tp[:, sl] @ g[b] @ Tp[:, sr].conj().T
    return ref, plain


def _check_pairs(got, G, pairs, T, plan, dtype, what):
    n, worst = plan.n, 0.0
    for b in range(got.shape[0]):
        ref, plain = _reference(G, pairs, T, plan, b, dtype)
        scale = float(np.abs(ref).max())
        if scale == 0.0:
            assert (got[b] == 0).all(), (what, b)
            continue
        tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
        err = float(np.abs(got[b] - ref).max()) / scale
        worst = max(worst, err / tol)
        assert err <= tol, (what, b, err, tol)
    return worst


def _run_pair_sets(be, plan, T, B, dtype, rng, refusals):
    worst = 0.0
    for name, pairs in _pair_sets(plan).items():
        G = [crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])).astype(dtype) for kl, kr in pairs]
        got = _pairs_backward(be, G, pairs, plan, B, dtype, refusals=refusals and name == "P")
        worst = max(worst, _check_pairs(got, G, pairs, T, plan, dtype, name))
        if name == "all":
            # every other pointer null: the reference of the pairs that are left, and bit-equal to the same set with zero-filled G
            Gn = [g if p % 2 == 0 else None for p, g in enumerate(G)]
            Gz = [g if p % 2 == 0 else np.zeros_like(g) for p, g in enumerate(G)]
            got_n = _pairs_backward(be, Gn, pairs, plan, B, dtype)
            worst = max(worst, _check_pairs(got_n, Gn, pairs, T, plan, dtype, "nulls"))
            assert got_n.tobytes() == _pairs_backward(be, Gz, pairs, plan, B, dtype).tobytes()
            got_0 = _pairs_backward(be, [None] * len(pairs), pairs, plan, B, dtype)
            assert (got_0 == 0).all() and not np.signbit(got_0.real).any() and not np.signbit(got_0.imag).any()
    assert (_pairs_backward(be, [], [], plan, B, dtype) == 0).all()                     # no pair at all: zeros as well
    return worst


@_all
def test_sym_fold_pairs_backward(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T = _plan(kind, sym, c)
    rng = np.random.default_rng(1100 * plan.n + 10 * B + len(sym) + (c == "half"))
    worst = _run_pair_sets(be, plan, T, B, dtype, rng, refusals=True)
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: sizes {plan.sizes}, worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("sym", ["x", "y", "xy"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_fold_pairs_backward_second_column_trip(backend, sym, dtype):
    """Order [6,5], n = 286: the lanes of a workgroup take a second trip over the columns, the last row group holds 6 of 8 rows."""
    be = get_backend(backend)
    plan, T = _plan("rect65", sym, "half")
    assert plan.n == 286
    worst = _run_pair_sets(be, plan, T, 1, dtype, np.random.default_rng(1286 + len(sym)), refusals=False)
    print(f"rect65 {sym} {np.dtype(dtype).name}: sizes {plan.sizes}, worst error / bound = {worst:.3f}")


def _bd_reference(G, T, plan, kl, kr, b, dtype):
    """([4, N] clongdouble, the same in `dtype`): the diagonals (p N + m, q N + m) of T_kl G[b] T_kr^H."""
    N = plan.n // 2
    sl, sr = slice(plan.off[kl], plan.off[kl + 1]), slice(plan.off[kr], plan.off[kr + 1])
    Tp = T.astype(dtype)
    m = np.arange(N)

    def diagonals(U, g):                                                               # only the 4 N entries asked for, not the n x n product
        left = [U[p * N + m][:, sl] @ g for p in (0, 1)]
        return np.stack([(left[pq >> 1] * U[(pq & 1) * N + m][:, sr].conj()).sum(axis=1) for pq in range(4)])
    return diagonals(T, G[b].astype(LD)), diagonals(Tp, G[b])


def _run_bd(be, plan, T, B, dtype, rng, refusals):
    n, worst = plan.n, 0.0
    for i, (kl, kr) in enumerate(_bd_pairs(plan)):
        G = crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])).astype(dtype)
        got = _pair_bd_backward(be, G, plan, kl, kr, dtype, refusals=refusals and i == 0)
        for b in range(B):
            ref, plain = _bd_reference(G, T, plan, kl, kr, b, dtype)
            scale = float(np.abs(ref).max())
            if scale == 0.0:
                assert (got[:, b] == 0).all(), (kl, kr, b)
                continue
            tol = 16 * max(float(np.abs(plain - ref).max()) / scale, n * _eps(dtype))
            err = float(np.abs(got[:, b] - ref).max()) / scale
            worst = max(worst, err / tol)
            assert err <= tol, (kl, kr, b, err, tol)
    return worst


@_all
def test_sym_fold_pair_bd_backward(backend, kind, sym, c, B, dtype):
    be = get_backend(backend)
    plan, T = _plan(kind, sym, c)
    rng = np.random.default_rng(1200 * plan.n + 10 * B + len(sym) + (c == "half"))
    worst = _run_bd(be, plan, T, B, dtype, rng, refusals=True)
    print(f"{kind} {sym} c={c} B={B} {np.dtype(dtype).name}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("sym", ["x", "y", "xy"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_sym_fold_pair_bd_backward_two_workgroups(backend, sym, dtype):
    """Order [12,5], N = 275: one thread per diagonal entry m, so two workgroups along m, the second ragged."""
    be = get_backend(backend)
    plan, T = _wide_plan(sym)
    assert plan.n // 2 == 275
    worst = _run_bd(be, plan, T, 1, dtype, np.random.default_rng(1650 + len(sym)), refusals=False)
    print(f"order [12,5] {sym} {np.dtype(dtype).name}: worst error / bound = {worst:.3f}")


@_all
def test_pairs_dot_product(backend, kind, sym, c, B, dtype):
    """sum_p <sym_fold_pair(M, kl_p, kr_p), G_p> = <M, sym_fold_pairs_backward(G)> for a random M, over the P pattern and over all pairs."""
    be = get_backend(backend)
    plan, _ = _plan(kind, sym, c)
    n = plan.n
    rng = np.random.default_rng(1300 * n + 10 * B + len(sym) + (c == "half"))
    M = crandn(rng, (B, n, n)).astype(dtype)
    sets = _pair_sets(plan)
    for name in ("P", "all"):
        pairs = sets[name]
        G = [crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])).astype(dtype) for kl, kr in pairs]
        folds = []
        for kl, kr in pairs:
            rc, out = _fold_pair_call(be, "sym_fold_pair", M, n, plan, B, kl, kr, dtype)
            assert rc == 0
            folds.append(out)
        gM = _pairs_backward(be, G, pairs, plan, B, dtype)
        lhs = sum(_dot(f, g) for f, g in zip(folds, G))
        rhs = _dot(M, gM)
        tol = 16 * n * _eps(dtype) * (max(float(np.abs(f).max()) for f in folds) * sum(float(np.abs(g).sum()) for g in G)
                                      + float(np.abs(gM).max()) * float(np.abs(M).sum()))
        print(f"{name}: <fold M, G> = {lhs:.6g}, <M, fold^H G> = {rhs:.6g}, |difference| {abs(lhs - rhs):.2e}, bound {tol:.2e}")
        assert abs(lhs) > 1.0 and abs(lhs - rhs) <= tol


@_all
def test_pair_bd_dot_product(backend, kind, sym, c, B, dtype):
    """<sym_fold_pair_bd(bd, kl, kr), G> = <bd, sym_fold_pair_bd_backward(G)> for random diagonals, per pair."""
    be = get_backend(backend)
    plan, _ = _plan(kind, sym, c)
    n = plan.n
    N = n // 2
    rng = np.random.default_rng(1400 * n + 10 * B + len(sym) + (c == "half"))
    bd = crandn(rng, (4, B, N)).astype(dtype)
    total = 0.0
    for kl, kr in _bd_pairs(plan):
        G = crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])).astype(dtype)
        rc, out = _fold_pair_call(be, "sym_fold_pair_bd", bd, N, plan, B, kl, kr, dtype)
        assert rc == 0
        gbd = _pair_bd_backward(be, G, plan, kl, kr, dtype)
        lhs, rhs = _dot(out, G), _dot(bd, gbd)
        tol = 16 * n * _eps(dtype) * (float(np.abs(out).max()) * float(np.abs(G).sum()) + float(np.abs(gbd).max()) * float(np.abs(bd).sum()))
        assert abs(lhs - rhs) <= tol, (kl, kr, lhs, rhs, tol)
        total += abs(lhs)
    assert total > 1.0                                                                 # the pairs (k, k) reach every diagonal entry


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("backend", BACKENDS)
def test_malformed_off(backend, dtype):
    """An off that is not monotone from 0 to n: gM and gbd are NaN throughout, and nothing is written behind them."""
    be = get_backend(backend)
    plan, _ = _plan("rect32", "xy", "half")
    n, B = plan.n, 2
    rng = np.random.default_rng(9)
    for bad in ([0, 40, 20, 50, n], [0, 17, 35, 53, n - 1]):
        pairs = _pair_sets(plan)["P"]
        G = [crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])).astype(dtype) for kl, kr in pairs]
        gM = _pairs_backward(be, G, pairs, plan, B, dtype, off_override=bad)
        assert np.isnan(gM.real).all() and np.isnan(gM.imag).all()
        gbd = _pair_bd_backward(be, crandn(rng, (B, plan.sizes[1], plan.sizes[2])).astype(dtype), plan, 1, 2, dtype, off_override=bad)
        assert np.isnan(gbd.real).all() and np.isnan(gbd.imag).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_engine_wrappers_and_autograd(backend):
    """Engine.sym_fold_pairs_backward / sym_fold_pair_bd_backward return the C ABI's output, and torch.autograd through SymFoldPairsFn /
    SymFoldPairBdFn reproduces the gradient of the dense-T torch expression to the block-test bound (16 n eps of the largest entry: the
    reference is itself a complex128 product)."""
    import torch
    from tests.test_pipeline import make_engine
    from torcwa_amd import autograd_ops as ag
    eng = make_engine(backend)
    be = get_backend(backend)
    plan, T = _plan("rect32", "xy", "half")
    n, B, dtype = plan.n, 2, np.complex128
    rng = np.random.default_rng(12)
    pairs = _pair_sets(plan)["all"]
    G = [crandn(rng, (B, plan.sizes[kl], plan.sizes[kr])) if p % 3 else None for p, (kl, kr) in enumerate(pairs)]
    dev = lambda a: None if a is None else torch.from_numpy(a).to(eng.device)
    got = eng.sym_fold_pairs_backward([dev(g) for g in G], plan, pairs).cpu().numpy()
    assert got.tobytes() == _pairs_backward(be, G, pairs, plan, B, dtype).tobytes()
    zero = eng.sym_fold_pairs_backward([None] * len(pairs), plan, pairs, B=B, dtype=torch.complex128)
    assert zero.shape == (B, n, n) and not bool(zero.any())
    Gb = crandn(rng, (B, plan.sizes[1], plan.sizes[2]))
    got = eng.sym_fold_pair_bd_backward(dev(Gb), plan, 1, 2).cpu().numpy()
    assert got.shape == (4, B, n // 2) and got.tobytes() == _pair_bd_backward(be, Gb, plan, 1, 2, dtype).tobytes()
    with pytest.raises(ValueError):
        eng.sym_fold_pairs_backward([dev(G[1])], plan, [(0, 4)])
    with pytest.raises(ValueError):
        eng.sym_fold_pairs_backward([dev(G[1])], plan, [(2, 2)])                        # G[1] is the block (0, 1): 17 x 18, not 18 x 18
    with pytest.raises(ValueError):
        eng.sym_fold_pairs_backward([None], plan, [(0, 0)])                            # nothing to size the result from
    with pytest.raises(ValueError):
        eng.sym_fold_pair_bd_backward(dev(Gb), plan, 0, 0)
    # autograd: a real loss of the folded blocks, through the Functions and through dense products with T
    Tt = torch.from_numpy(T.astype(np.complex128)).to(eng.device)
    cols = lambda k: Tt[:, plan.off[k]:plan.off[k + 1]]
    sub = [(0, 3), (1, 2), (2, 0)]                                                     # outputs that take a gradient; the rest stay None
    Wt = {p: dev(crandn(rng, (B, plan.sizes[p[0]], plan.sizes[p[1]]))) for p in sub}
    loss = lambda outs: sum(torch.real((outs[p] * Wt[p]).sum()) + (torch.abs(outs[p]) ** 2).sum() for p in sub)
    M = dev(crandn(rng, (B, n, n)))
    M1, M2 = M.clone().requires_grad_(True), M.clone().requires_grad_(True)
    outs = dict(zip(pairs, ag.SymFoldPairsFn.apply(M1, plan, eng, pairs)))
    loss(outs).backward()
    loss({p: cols(p[0]).conj().T @ M2 @ cols(p[1]) for p in sub}).backward()
    ref = M2.grad.cpu().numpy()
    err = np.abs(M1.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"SymFoldPairsFn: gradient error {err:.2e}, bound {16 * n * _eps(dtype):.2e}")
    assert err <= 16 * n * _eps(dtype)
    bd = dev(crandn(rng, (4, B, n // 2)))
    b1, b2 = bd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    Wb = dev(crandn(rng, (B, plan.sizes[1], plan.sizes[2])))
    out = ag.SymFoldPairBdFn.apply(b1, plan, eng, 1, 2)
    (torch.real((out * Wb).sum()) + (torch.abs(out) ** 2).sum()).backward()
    a, b, c, d = b2
    dense = torch.cat((torch.cat((torch.diag_embed(a), torch.diag_embed(b)), dim=2), torch.cat((torch.diag_embed(c), torch.diag_embed(d)), dim=2)), dim=1)
    assert np.array_equal(dense[0].detach().cpu().numpy(), _bd_dense(bd[:, 0].cpu().numpy()))
    outd = cols(1).conj().T @ dense @ cols(2)
    (torch.real((outd * Wb).sum()) + (torch.abs(outd) ** 2).sum()).backward()
    ref = b2.grad.cpu().numpy()
    err = np.abs(b1.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"SymFoldPairBdFn: gradient error {err:.2e}, bound {16 * n * _eps(dtype):.2e}")
    assert err <= 16 * n * _eps(dtype)
