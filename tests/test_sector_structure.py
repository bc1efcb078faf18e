"""The block structure the sector solve rests on, checked in numpy on random mirror-symmetric grids (CPU only, no kernel but trx_sym_fold in the
last test): in the mirror basis T of torcwa_amd.symmetry the E -> E operators are block diagonal, the E -> H and H -> E operators (Q, Vf; P,
Vf^-1) connect block k with the opposite block k' only, and the unit vectors of order (0, 0) are single columns of T.

P, Q come from the oracle's statement of the reference's formulas (oracle.rcwa_oracle.pq_patterned on its conv_matrix), with a patterned eps AND a
patterned mu; Vf from its kvectors.  Bound on an entry that must vanish: 16 n eps max |T^H M T| -- T has unit columns of at most four entries, so
an entry of T^H M T is a sum of at most 16 entries of M, each of which carries the rounding of the O(n) sums behind P and Q.
"""
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS

ORDER, L, NX, NY = [3, 2], [300., 280.], 40, 36
EPS = 2.0 ** -53
CASES = [(sym, c) for sym in ("x", "y", "xy") for c in ("half", "zero")]


def _mirror(g, sym, c):
    """g symmetrised about the half-cell centre (c = n - 1) or about sample 0 (c = 0) along every claimed axis."""
    for ax, name in ((0, "x"), (1, "y")):
        if name in sym:
            f = np.flip(g, axis=ax)
            g = g + (f if c == "half" else np.roll(f, 1, axis=ax))
    return g


@functools.lru_cache(maxsize=None)
def _operators(sym, c):
    """(plan, T, P, Q, Vf, Vfinv) as numpy complex128 at order [3, 2], normal incidence."""
    from oracle import rcwa_oracle as orc
    from torcwa_amd import lattice
    from torcwa_amd.symmetry import build_plan
    rng = np.random.default_rng(17 + len(sym) + (c == "half"))
    eps = _mirror(1.0 + rng.random((NX, NY)) + 0.1j * rng.random((NX, NY)), sym, c)
    mu = _mirror(1.0 + 0.3 * rng.random((NX, NY)), sym, c).astype(np.complex128)
    s = orc.kvectors(orc.Setup(freq=1 / 532., order=ORDER, L=L))
    E, M = orc.conv_matrix(torch.from_numpy(eps), ORDER), orc.conv_matrix(torch.from_numpy(mu), ORDER)
    P, Q = orc.pq_patterned(E, M, s.kx, s.ky)
    cx, cy = (NX - 1, NY - 1) if c == "half" else (0, 0)
    plan = build_plan(lattice.rect_orders(*ORDER), sym, cx if "x" in sym else 0, NX, cy if "y" in sym else 0, NY)
    Vf = s.Vf.numpy()
    return plan, plan.dense(np.complex128), P.numpy(), Q.numpy(), Vf, np.linalg.inv(Vf)


def _outside(D, plan, pattern):
    """Largest |D[i, j]| over the block pairs (a, b) with pattern(a) != b, relative to max |D|."""
    worst = 0.0
    for a in range(plan.nblk):
        for b in range(plan.nblk):
            if pattern(a) != b:
                blk = D[plan.off[a]:plan.off[a + 1], plan.off[b]:plan.off[b + 1]]
                worst = max(worst, float(np.abs(blk).max()) if blk.size else 0.0)
    return worst / float(np.abs(D).max())


def test_opposite_block():
    from torcwa_amd.symmetry import _CLASS, opposite_block
    inv = {v: k for k, v in _CLASS.items()}
    for k in range(4):                                          # H carries minus the mirror eigenvalues of E
        rx, ry = inv[k]
        assert opposite_block(4, k) == _CLASS[(-rx, -ry)] == 3 - k
    assert [opposite_block(2, k) for k in range(2)] == [1, 0]
    for bad in ((3, 0), (4, 4), (2, -1)):
        with pytest.raises(ValueError):
            opposite_block(*bad)


@pytest.mark.parametrize("sym,c", CASES)
def test_operators_connect_the_expected_blocks(sym, c):
    from torcwa_amd.symmetry import opposite_block
    plan, T, P, Q, Vf, Vfinv = _operators(sym, c)
    n = plan.n
    tol = 16 * n * EPS
    opp = lambda k: opposite_block(plan.nblk, k)
    Th = T.conj().T
    for k in range(plan.nblk):
        assert plan.sizes[k] == plan.sizes[opp(k)]
    figs = {"A": _outside(Th @ (P @ Q) @ T, plan, lambda a: a), "Q": _outside(Th @ Q @ T, plan, opp), "P": _outside(Th @ P @ T, plan, opp),
            "Vf": _outside(Th @ Vf @ T, plan, opp), "Vfinv": _outside(Th @ Vfinv @ T, plan, opp)}
    print(f"{sym} c={c}: largest entry outside the pattern / max, " + ", ".join(f"{k} {v:.1e}" for k, v in figs.items()) + f" (bound {tol:.1e})")
    for name, v in figs.items():
        assert v <= tol, (name, v, tol)
    # ... and the pattern is not empty: the blocks inside it carry the operator
    assert _outside(Th @ Q @ T, plan, lambda a: a) > 0.1


@pytest.mark.parametrize("sym,c", CASES)
def test_unit_vectors_of_the_zeroth_order(sym, c):
    """Component x of order (0, 0) is one column of T with weight 1, in block 2 / 1 / 0 under "xy" / "x" / "y"; component y in block 1 / 0 / 1.  A
    general order spreads over up to four blocks with the weights conj(T[c, j])."""
    from torcwa_amd import lattice
    from torcwa_amd.symmetry import sector_coordinates
    plan, T = _operators(sym, c)[:2]
    mn = lattice.rect_orders(*ORDER)
    N = len(mn)
    pos = {(int(p), int(q)): i for i, (p, q) in enumerate(mn)}
    for comp, blocks in ((0, {"xy": 2, "x": 1, "y": 0}), (1, {"xy": 1, "x": 0, "y": 1})):
        (k, j, w), = sector_coordinates(plan, comp * N + pos[(0, 0)])
        assert k == blocks[sym] and w == 1.0
        col = T[:, plan.off[k] + j]
        assert col[comp * N + pos[(0, 0)]] == 1.0 and np.count_nonzero(col) == 1
    row = pos[(1, 1)]
    coords = sector_coordinates(plan, row)
    assert len(coords) == (4 if sym == "xy" else 2)
    e = np.zeros(plan.n)
    e[row] = 1.0
    full = T.conj().T @ e
    got = np.zeros(plan.n, dtype=np.complex128)
    for k, j, w in coords:
        got[plan.off[k] + j] = w
    assert np.abs(got - full).max() <= 4 * EPS
    with pytest.raises(ValueError):
        sector_coordinates(plan, plan.n)


@pytest.mark.parametrize("sym,c", CASES)
def test_expansion_is_T_k(sym, c):
    """SymPlan.expansion(k): x[rows] += w y[src] is x = T_k y, and the rows of one block are distinct."""
    plan, T = _operators(sym, c)[:2]
    rng = np.random.default_rng(3)
    for k in range(plan.nblk):
        rows, src, w = (t.numpy() for t in plan.expansion(k, torch.device("cpu"), torch.complex128))
        assert len(set(rows.tolist())) == len(rows)
        y = rng.standard_normal(plan.sizes[k]) + 1j * rng.standard_normal(plan.sizes[k])
        x = np.zeros(plan.n, dtype=np.complex128)
        x[rows] += w * y[src]
        assert np.abs(x - T[:, plan.off[k]:plan.off[k + 1]] @ y).max() <= 4 * EPS * np.abs(y).max()


@pytest.mark.parametrize("sym,c", CASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_pk_qk_is_the_block_of_sym_fold(backend, sym, c):
    """P_k Q_k with P_k = T_k^H P T_k', Q_k = T_k'^H Q T_k (numpy) equals the diagonal block k that trx_sym_fold gives for A = P Q."""
    from tests.test_pipeline import make_engine
    from torcwa_amd.symmetry import opposite_block
    eng = make_engine(backend)
    plan, T, P, Q = _operators(sym, c)[:4]
    n = plan.n
    blocks, resid = eng.sym_fold(torch.from_numpy((P @ Q)[None]).to(eng.device), plan)
    assert float(resid[0]) <= 16 * n * EPS
    per = {}
    for (s, ks), blk in zip(plan.groups, blocks):
        for i, k in enumerate(ks):
            per[k] = blk[i].cpu().numpy()
    for k in range(plan.nblk):
        Tk, To = T[:, plan.off[k]:plan.off[k + 1]], T[:, plan.off[opposite_block(plan.nblk, k)]:plan.off[opposite_block(plan.nblk, k) + 1]]
        ref = (Tk.conj().T @ P @ To) @ (To.conj().T @ Q @ Tk)
        assert np.abs(per[k] - ref).max() <= 16 * n * EPS * np.abs(ref).max(), k
