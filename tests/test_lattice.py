"""Oblique lattices and arbitrary Fourier-order sets: torcwa_amd.lattice, lattice_geometry, the kernels of trx_convmat_orders /
trx_normal_field_lattice / trx_convmat_nv_orders against numpy restatements, and the solver's general path (rectangular list = today's path,
basis invariance, hexagonal lattice = its rectangular supercell, physics, gradients, sweeps).

Unmarked tests are pure Python; `emu` runs the kernels and small solves through the CPU kernel-logic emulator; `gpu` runs them on MI355X.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, get_backend
from tests.helpers import load_case
from tests.test_pipeline import make_engine, run_case

S3 = math.sqrt(3.0)
HEX = [[1.0, 0.0], [0.5, S3 / 2]]
POLS = ("xx", "yx", "xy", "yy", "pp", "sp", "ps", "ss")


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- 1. pure-Python helpers -------------------------------------------------------------------------------------------------------------
def test_reciprocal_rect_orders_and_parse():
    from torcwa_amd.lattice import parse_order, reciprocal, rect_orders
    assert np.array_equal(reciprocal([2.0, 4.0]), np.diag([0.5, 0.25]))
    assert np.array_equal(reciprocal([[2.0, 0.0], [0.0, 4.0]]), np.diag([0.5, 0.25]))
    b = reciprocal(HEX)
    assert np.abs(np.array(HEX) @ b.T - np.eye(2)).max() < 1e-15
    for bad in ([[1.0, 0.0], [2.0, 1e-12]], [[1.0, 1.0], [1.0, 1.0]], [0.0, 1.0], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            reciprocal(bad)
    mn = rect_orders(2, 1)
    ox, oy = 2, 1
    assert mn.shape == (15, 2)
    for i, (m, n) in enumerate(mn):
        assert i == (m + ox) * (2 * oy + 1) + (n + oy)
    assert parse_order([3, 2]) == ("rect", (3, 2), None)
    kind, _, got = parse_order([[0, 0], [1, -1]])
    assert kind == "list" and got.tolist() == [[0, 0], [1, -1]]
    kind, _, got = parse_order([[0, 0]])
    assert kind == "list" and got.shape == (1, 2)
    for bad in ([[1, 0], [0, 1]], [[0, 0], [1, 0], [1, 0]], [[0, 0], [0.5, 1]], [1, 2, 3]):
        with pytest.raises(ValueError):
            parse_order(bad)


def _as_set(mn):
    return {(int(m), int(n)) for m, n in mn}


def test_circular_orders():
    from torcwa_amd.lattice import circular_orders, reciprocal
    for L in (HEX, [1.0, 1.0], [[1.0, 0.0], [0.3, 0.8]], [0.7, 1.3]):
        b = reciprocal(L)
        for nh in (1, 7, 19, 50, 120):
            mn = circular_orders(L, n_harmonics=nh)
            g = np.hypot(*(mn @ b).T)
            assert len(mn) >= nh and tuple(mn[0]) == (0, 0) and len(_as_set(mn)) == len(mn)
            assert (np.diff(g) > -1e-9 * g.max()).all()                         # sorted by |G|
            R = g.max()
            # complete: every harmonic of the box with |G| <= R (to the shell tolerance) is present, none beyond
            M = 40
            m, n = np.meshgrid(np.arange(-M, M + 1), np.arange(-M, M + 1), indexing="ij")
            full = np.stack((m.ravel(), n.ravel()), 1)
            gf = np.hypot(*(full @ b).T)
            assert _as_set(full[gf <= R * (1 + 1e-9)]) == _as_set(mn)
            # the smallest such set: dropping the outermost shell leaves fewer than nh
            assert (g < R * (1 - 1e-9)).sum() < nh
            # symmetric under G -> -G
            assert _as_set(-mn) == _as_set(mn)
    # whole shells of the hexagonal lattice: 1, 7, 13, 19 harmonics
    assert [len(circular_orders(HEX, n_harmonics=k)) for k in (1, 2, 8, 14, 19, 20)] == [1, 7, 13, 19, 19, 31]
    # g_max form, and basis invariance: (a1, a1 + a2) gives the same physical set, (m, n) -> (m, m + n)
    L2 = [HEX[0], [HEX[0][0] + HEX[1][0], HEX[0][1] + HEX[1][1]]]
    for kw in ({"n_harmonics": 37}, {"g_max": 2.5}):
        A, Bs = circular_orders(HEX, **kw), circular_orders(L2, **kw)
        assert _as_set(Bs) == {(m, m + n) for m, n in _as_set(A)}
    with pytest.raises(ValueError):
        circular_orders(HEX)
    with pytest.raises(ValueError):
        circular_orders(HEX, n_harmonics=3, g_max=1.0)


def test_lattice_geometry():
    import torcwa_amd
    from torcwa_amd import geometry, lattice_geometry
    # a diagonal lattice reproduces geometry's grid and shapes
    g0 = geometry(Lx=0.8, Ly=0.5, nx=40, ny=25, edge_sharpness=60.0, dtype=torch.float64, device=torch.device("cpu"))
    g1 = lattice_geometry([0.8, 0.0], [0.0, 0.5], 40, 25, 60.0, dtype=torch.float64, device=torch.device("cpu"))
    g0.grid()
    assert torch.allclose(g1.x_grid, g0.x_grid) and torch.allclose(g1.y_grid, g0.y_grid)
    for name, args in (("circle", (0.15, 0.4, 0.25)), ("ellipse", (0.2, 0.1, 0.4, 0.25, 0.3)), ("square", (0.2, 0.4, 0.25, 0.2)),
                       ("rectangle", (0.3, 0.1, 0.4, 0.25, 0.5)), ("rhombus", (0.3, 0.2, 0.4, 0.25, 0.0)),
                       ("super_ellipse", (0.3, 0.2, 0.4, 0.25, 0.1, 4.0))):
        assert torch.allclose(getattr(g1, name)(*args), getattr(g0, name)(*args), atol=1e-12), name
    # hexagonal cell: a disk on a lattice point and one on a cell edge are whole (minimum image)
    n = 96
    hexg = lattice_geometry(HEX[0], HEX[1], n, n, 2000.0, dtype=torch.float64, device=torch.device("cpu"))
    area = S3 / 2
    for c in ((0.0, 0.0), (0.5, 0.0), (0.75, S3 / 4)):
        d = hexg.circle(0.3, *c)
        frac = float(d.mean())
        assert abs(frac - math.pi * 0.09 / area) < 0.01, (c, frac)
    # the minimum image: no sample is farther from the centre than the hexagon's circumradius
    u, v = hexg._disp(0.2, 0.1)
    assert float(torch.sqrt(u * u + v * v).max()) <= 1 / S3 + 1e-12
    # set algebra and differentiability in the parameters
    a, b = hexg.circle(0.3, 0.0, 0.0), hexg.circle(0.2, 0.5, 0.0)
    assert torch.equal(hexg.union(a, b), torch.maximum(a, b)) and torch.equal(hexg.difference(a, b), torch.minimum(a, 1 - b))
    R = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    (gR,) = torch.autograd.grad(hexg.circle(R, 0.1, 0.2).sum(), R)
    assert float(gR) > 0
    assert "lattice_geometry" in torcwa_amd.__all__ and "lattice" in torcwa_amd.__all__


# ---- 2. kernels ----------------------------------------------------------------------------------------------------------------------------
def orders_ref(g, mn):
    """out[i, j] = c[m_i - m_j, n_i - n_j] of the full FFT, c = fft2(g) / (n1 n2)."""
    g = np.asarray(g, dtype=np.complex128)
    n1, n2 = g.shape
    c = np.fft.fft2(g) / (n1 * n2)
    dm = (mn[:, None, 0] - mn[None, :, 0]) % n1
    dn = (mn[:, None, 1] - mn[None, :, 1]) % n2
    return c[dm, dn]


def _run_orders(be, grids, mn, dt, mmax=None, nmax=None, ws_extra=0):
    B, n1, n2 = grids.shape
    cplx = np.iscomplexobj(grids)
    rdt = np.float64 if dt == np.complex128 else np.float32
    gin = be.dev(grids.astype(dt if cplx else rdt))
    mn32 = be.dev(np.ascontiguousarray(mn, dtype=np.int32))
    N = len(mn)
    mmax = int(np.abs(mn[:, 0]).max()) if mmax is None else mmax
    nmax = int(np.abs(mn[:, 1]).max()) if nmax is None else nmax
    out = be.empty((B, N, N), dt)
    code = 1 if dt == np.complex128 else 0
    nws = be.lib.convmat_orders_ws_bytes(code, B, n1, n2, N, mmax, nmax)
    ws = be.empty((max(nws + ws_extra, 16),), np.uint8)
    rc = be.lib.convmat_orders(code, int(cplx), be.ptr(gin), B, n1, n2, be.ptr(mn32), N, mmax, nmax, be.ptr(out), be.ptr(ws), nws + ws_extra,
                               be.stream)
    return rc, (be.host(out) if rc == 0 else None)


def _sets():
    from torcwa_amd.lattice import circular_orders
    rng = np.random.default_rng(5)
    circ = circular_orders(HEX, n_harmonics=19)
    box = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 2)
    rand = box[rng.permutation(len(box))[:17]]
    rand = np.concatenate(([[0, 0]], rand[(rand != 0).any(1)]))[:15]
    sparse = np.array([[0, 0], [3, -2], [-3, 1], [2, 2], [-1, -2], [0, 2]])      # non-contiguous, caller's order
    return {"circular": circ, "random": rand, "sparse": sparse}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dt,tol", [(np.complex128, 1e-12), (np.complex64, 2e-6)])
@pytest.mark.parametrize("cplx", [False, True])
def test_convmat_orders_matches_restatement(backend, dt, tol, cplx):
    be = get_backend(backend)
    rng = np.random.default_rng(1)
    n1, n2 = 13, 11
    grids = 1.0 + rng.random((2, n1, n2))
    if cplx:
        grids = grids + 1j * rng.random((2, n1, n2))
    for name, mn in _sets().items():
        rc, out = _run_orders(be, grids, mn, dt)
        assert rc == 0, name
        for b in range(2):
            g = grids[b] if dt == np.complex128 else grids[b].astype(np.complex64 if cplx else np.float32)
            assert _rel(out[b], orders_ref(g, mn)) < tol, name
    # a coefficient box larger than the set's own (explicit mmax / nmax) gives the same matrix
    mn = _sets()["sparse"]
    rc, out = _run_orders(be, grids, mn, dt, mmax=4, nmax=5)
    assert rc == 0 and _rel(out[0], orders_ref(grids[0], mn)) < max(tol, 1e-12) * (1 if dt == np.complex128 else 1e3)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dt", [np.complex128, np.complex64])
def test_convmat_orders_rect_bit_identical(backend, dt):
    from torcwa_amd.lattice import rect_orders
    be = get_backend(backend)
    rng = np.random.default_rng(2)
    for (n1, n2, ox, oy, cplx) in ((13, 11, 2, 1, True), (16, 20, 3, 4, False), (9, 12, 0, 3, True)):
        grids = 1.0 + rng.random((3, n1, n2)) + (1j * rng.random((3, n1, n2)) if cplx else 0)
        rdt = np.float64 if dt == np.complex128 else np.float32
        gin = be.dev(grids.astype(dt if cplx else rdt))
        N = (2 * ox + 1) * (2 * oy + 1)
        ref = be.empty((3, N, N), dt)
        code = 1 if dt == np.complex128 else 0
        nws = be.lib.convmat_ws_bytes(code, 3, n1, n2, ox, oy)
        ws = be.empty((nws,), np.uint8)
        assert be.lib.convmat(code, int(cplx), be.ptr(gin), 3, n1, n2, ox, oy, be.ptr(ref), be.ptr(ws), nws, be.stream) == 0
        rc, out = _run_orders(be, grids, rect_orders(ox, oy), dt)
        assert rc == 0 and np.array_equal(out, be.host(ref))


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_orders_errors(backend):
    be = get_backend(backend)
    grids = np.ones((1, 9, 8))
    mn = np.array([[0, 0], [1, 2], [-2, 1]])
    ERR_ARG, ERR_WS = -2, -3
    assert _run_orders(be, grids, mn, np.complex128)[0] == 0
    assert _run_orders(be, grids, mn, np.complex128, mmax=1)[0] == ERR_ARG           # |m| beyond mmax
    assert _run_orders(be, grids, mn, np.complex128, nmax=1)[0] == ERR_ARG           # |n| beyond nmax
    assert _run_orders(be, grids, mn, np.complex128, mmax=-1)[0] == ERR_ARG
    assert _run_orders(be, np.ones((1, 4, 8)), mn, np.complex128)[0] == ERR_ARG      # n1 <= 2 mmax: grid too coarse for the set
    assert _run_orders(be, np.ones((1, 9, 4)), mn, np.complex128)[0] == ERR_ARG      # n2 <= 2 nmax
    assert _run_orders(be, grids, mn, np.complex128, ws_extra=-16)[0] == ERR_WS
    out = be.empty((1, 3, 3), np.complex128)
    assert be.lib.convmat_orders(1, 0, None, 1, 9, 8, None, 3, 2, 2, be.ptr(out), be.ptr(out), 1 << 20, be.stream) == ERR_ARG
    gin, m32 = be.dev(grids), be.dev(mn.astype(np.int32))
    assert be.lib.convmat_orders(1, 0, be.ptr(gin), 1, 9, 8, be.ptr(m32), 0, 2, 2, be.ptr(out), be.ptr(out), 1 << 20, be.stream) == ERR_ARG
    assert be.lib.convmat_orders(7, 0, be.ptr(gin), 1, 9, 8, be.ptr(m32), 3, 2, 2, be.ptr(out), be.ptr(out), 1 << 20, be.stream) == -1


def field_ref_h(g, sigma, h):
    """field_ref on a cell matrix h (rows a1/n1, a2/n2): grad = h^-1 (du, dv) of the index-space central differences, blur in index space."""
    g = np.asarray(g, dtype=np.complex128)
    hi = np.linalg.inv(np.asarray(h, dtype=np.float64))
    du = (np.roll(g, -1, 0) - np.roll(g, 1, 0)) / 2
    dv = (np.roll(g, -1, 1) - np.roll(g, 1, 1)) / 2
    gx, gy = hi[0, 0] * du + hi[0, 1] * dv, hi[1, 0] * du + hi[1, 1] * dv
    J = [np.abs(gx) ** 2, np.real(gx * np.conj(gy)), np.abs(gy) ** 2]
    if sigma > 0:
        R = int(math.ceil(3 * sigma))
        k = np.arange(-R, R + 1)
        w = np.exp(-k * k / (2.0 * sigma * sigma))
        w /= w.sum()
        for ax in (1, 0):
            J = [sum(w[i] * np.roll(c, -k[i], ax) for i in range(len(k))) for c in J]
    d, o = J[0] - J[2], 2 * J[1]
    r = np.hypot(d, o)
    ok = r > 1e-3 * (J[0] + J[2])
    rs = np.where(ok, r, 1.0)
    return np.stack([np.where(ok, v, 0.0) for v in (0.5 * (1 + d / rs), 0.5 * o / rs, 0.5 * (1 - d / rs))])


def _hex_disk(n1, n2, eps=(1.5, 9.0), r=0.3, c=(0.1, 0.05), cplx=False, seed=0):
    from torcwa_amd import lattice_geometry
    geo = lattice_geometry(HEX[0], HEX[1], n1, n2, 40.0, dtype=torch.float64, device=torch.device("cpu"))
    d = geo.circle(r, *c).numpy()
    g = eps[0] + (eps[1] - eps[0]) * d + 0.05 * np.random.default_rng(seed).random((n1, n2))
    return g + (1j * (0.1 + 0.2 * np.random.default_rng(seed + 1).random((n1, n2))) if cplx else 0)


def _run_field_lattice(be, grids, sigma, h, dt):
    B, n1, n2 = grids.shape
    cplx = np.iscomplexobj(grids)
    rdt = np.float64 if dt == np.complex128 else np.float32
    gin = be.dev(grids.astype(dt if cplx else rdt))
    nn = be.empty((B, 3, n1, n2), np.float64)
    code = 1 if dt == np.complex128 else 0
    nws = be.lib.normal_field_ws_bytes(code, B, n1, n2)
    ws = be.empty((max(nws, 16),), np.uint8)
    hc = (ctypes.c_double * 4)(*np.asarray(h, dtype=np.float64).ravel().tolist())
    rc = be.lib.normal_field_lattice(code, int(cplx), be.ptr(gin), B, n1, n2, sigma, hc, be.ptr(nn), be.ptr(ws), nws, be.stream)
    return rc, (be.host(nn) if rc == 0 else None)


@pytest.mark.parametrize("backend", BACKENDS)
def test_normal_field_lattice(backend):
    from tests.test_normal_vector import _disk, _run_field
    be = get_backend(backend)
    grids = np.stack([_disk(24, 20, c, s) for s, c in ((0, False), (1, True))]).astype(np.complex128)
    # diagonal h: trx_normal_field with hx = h00, hy = h11
    rc0, nn0 = _run_field(be, grids, 2.0, 0.03, 0.05, np.complex128)
    rc1, nn1 = _run_field_lattice(be, grids, 2.0, [[0.03, 0.0], [0.0, 0.05]], np.complex128)
    assert rc0 == 0 and rc1 == 0 and np.array_equal(nn0, nn1)
    # a skewed cell against the restatement (both dtypes)
    n1, n2 = 24, 20
    h = np.array(HEX) / np.array([[n1], [n2]])
    grids = np.stack([_hex_disk(n1, n2, cplx=c, seed=s) for s, c in ((0, False), (1, True))])
    for dt in (np.complex128, np.complex64):
        rc, nn = _run_field_lattice(be, grids, 1.5, h, dt)
        assert rc == 0
        for b in range(2):
            g = grids[b] if dt == np.complex128 else grids[b].astype(np.complex64)
            assert np.abs(nn[b] - field_ref_h(g, 1.5, h)).max() < 1e-12
    assert _run_field_lattice(be, grids, 1.5, [[1.0, 0.0], [2.0, 0.0]], np.complex128)[0] == -2        # singular cell
    assert _run_field_lattice(be, grids, -1.0, h, np.complex128)[0] == -2


def nv_ref_orders(g, mn, nn):
    """(Exx, Exy, Eyy) from the definitions, every matrix the order-set restatement of the convolution matrix."""
    E = orders_ref(g, mn)
    D = E - np.linalg.inv(orders_ref(1 / np.asarray(g, dtype=np.complex128), mn))
    C = [orders_ref(p, mn) for p in nn]
    S = [(D @ c + c @ D) / 2 for c in C]
    return E - S[0], -S[1], E - S[2]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dt,tol", [(np.complex128, 1e-12), (np.complex64, 2e-6)])
def test_convmat_nv_orders_matches_restatement(backend, dt, tol):
    be = get_backend(backend)
    n1, n2 = 24, 20
    h = np.array(HEX) / np.array([[n1], [n2]])
    mn = _sets()["circular"]
    N = len(mn)
    for cplx in (False, True):
        grids = np.stack([_hex_disk(n1, n2, cplx=cplx, seed=s) for s in range(2)])
        if not cplx:
            grids = grids.real
        rdt = np.float64 if dt == np.complex128 else np.float32
        gin = be.dev(grids.astype(dt if cplx else rdt))
        m32 = be.dev(mn.astype(np.int32))
        code = 1 if dt == np.complex128 else 0
        hc = (ctypes.c_double * 4)(*h.ravel().tolist())
        for nn_in in (None, np.random.default_rng(4).random((2, 3, n1, n2))):
            outs = [be.empty((2, N, N), dt) for _ in range(3)]
            info = be.empty((2,), np.int32)
            nws = be.lib.convmat_nv_orders_ws_bytes(code, 2, n1, n2, N, 2, 2)
            ws = be.empty((nws,), np.uint8)
            nnd = be.dev(nn_in) if nn_in is not None else None
            rc = be.lib.convmat_nv_orders(code, int(cplx), be.ptr(gin), 2, n1, n2, be.ptr(m32), N, 2, 2, 1.5, hc,
                                          be.ptr(nnd) if nn_in is not None else None, *[be.ptr(o) for o in outs], be.ptr(info), be.ptr(ws),
                                          nws, be.stream)
            assert rc == 0 and not be.host(info).any()
            for b in range(2):
                g = grids[b] if dt == np.complex128 else grids[b].astype(np.complex64 if cplx else np.float32)
                nn = field_ref_h(g, 1.5, h) if nn_in is None else nn_in[b]
                for got, ref in zip(outs, nv_ref_orders(g, mn, nn)):
                    assert _rel(be.host(got)[b], ref) < tol


# ---- 3. solver: rectangular list = today's path -------------------------------------------------------------------------------------------
def _rect_list_case(eng, name):
    from torcwa_amd.lattice import rect_orders
    g = load_case(name, "c128")
    ref = run_case(eng, g, "c128")
    ox, oy = (int(v) for v in g["order"])
    Lx, Ly = (float(v) for v in g["L"])
    import torcwa_amd
    from tests.helpers import case_inputs
    ci = case_inputs(g, "c128")
    dev = eng.device
    sim = torcwa_amd.rcwa(freq=ci["freq"], order=rect_orders(ox, oy), L=[[Lx, 0.0], [0.0, Ly]], dtype=torch.complex128, engine=eng)
    if "eps_in" in ci:
        sim.add_input_layer(eps=ci["eps_in"])
    if "eps_out" in ci:
        sim.add_output_layer(eps=ci["eps_out"])
    sim.set_incident_angle(inc_ang=ci["inc_ang"], azi_ang=ci["azi_ang"], angle_layer=ci["angle_layer"])
    for (d, eps, mu) in ci["layers"]:
        sim.add_layer(thickness=d, eps=eps.to(dev) if torch.is_tensor(eps) else eps, mu=mu.to(dev) if torch.is_tensor(mu) else mu)
    sim.solve_global_smatrix()
    assert sim._b._general and sim.order_x is None and sim.Gx_norm is None and ref.Gx_norm is not None
    assert torch.equal(sim.Kx_norm_dn, ref.Kx_norm_dn) and torch.equal(sim.Ky_norm_dn, ref.Ky_norm_dn)
    assert torch.equal(sim.orders.cpu(), ref.orders.cpu()) and torch.equal(sim.G_norm, ref.G_norm)
    for k in range(4):
        assert _rel(sim.S[k].cpu().numpy(), ref.S[k].cpu().numpy()) < 1e-12
    probe = [[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]]
    for pol in POLS:
        a = sim.S_parameters(orders=probe, polarization=pol).cpu().numpy()
        b = ref.S_parameters(orders=probe, polarization=pol).cpu().numpy()
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-3), pol
    e1, m1 = sim.return_layer(0, 4 * ox + 3, 4 * oy + 3)
    e0, m0 = ref.return_layer(0, 4 * ox + 3, 4 * oy + 3)
    assert _rel(e1.cpu().numpy(), e0.cpu().numpy()) < 1e-12 and _rel(m1.cpu().numpy(), m0.cpu().numpy()) < 1e-12
    # the reference's clamping is the rectangular path's only: a harmonic outside the set raises on the general path
    with pytest.raises(ValueError):
        sim.S_parameters(orders=[[ox + 1, 0]])
    with pytest.raises(ValueError):
        sim.diffraction_angle(orders=[[0, oy + 1]])
    return sim, g


@pytest.mark.parametrize("backend", BACKENDS)
def test_rect_list_equals_rect_path(backend):
    _rect_list_case(make_engine(backend), "example1_o3")


@pytest.mark.gpu
def test_rect_list_equals_rect_path_example1_o5():
    from tests.helpers import DIRPORT, ORDERS_PROBE, POLS as GPOLS, relerr
    sim, g = _rect_list_case(make_engine("gpu"), "example1_o5")
    # and against the reference's fixture at test_pipeline's tolerance (probe orders inside the set)
    S = [s.cpu().numpy() for s in sim.S]
    assert np.allclose([np.linalg.norm(x) for x in S], g["S_fro"], rtol=1e-8, atol=1e-9)
    cidx = g["central_idx"]
    for k in range(4):
        if f"S{k}_central" in g:
            assert relerr(S[k][np.ix_(cidx, cidx)], g[f"S{k}_central"]) < 1e-9
    sp = g["sparams"]
    for a, (dr, pt) in enumerate(DIRPORT):
        for b, pol in enumerate(GPOLS):
            v = sim.S_parameters(orders=ORDERS_PROBE[:-1], direction=dr, port=pt, polarization=pol).cpu().numpy()
            assert np.abs(v - sp[a, b, :-1]).max() / max(np.abs(sp[a]).max(), 1e-3) < 1e-9


@pytest.mark.parametrize("backend", BACKENDS)
def test_diagonal_lattice_matrix_is_the_rectangle(backend):
    """L = [[Lx, 0], [0, Ly]] with [ox, oy] is the rectangle under every rule (the normal rule's derived field takes hx = Lx / nx)."""
    import torcwa_amd
    from tests.test_normal_vector import _disk
    eng = make_engine(backend)
    Lx, Ly = 0.7, 0.55
    g = torch.as_tensor(_disk(24, 20, True, 3, eps=(2.0, 9.0))).to(eng.device)
    for rule in ("laurent", "li", "normal"):
        S = []
        for L in ([Lx, Ly], [[Lx, 0.0], [0.0, Ly]], np.diag([Lx, Ly]), torch.tensor([[Lx, 0.0], [0.0, Ly]], dtype=torch.float64)):
            sim = torcwa_amd.rcwa(freq=1.0, order=[3, 2], L=L, dtype=torch.complex128, engine=eng, fourier_rule=rule, nv_sigma=2.0)
            sim.add_input_layer(eps=1.5)
            sim.set_incident_angle(inc_ang=0.3, azi_ang=0.2)
            sim.add_layer(thickness=0.3, eps=g)
            sim.solve_global_smatrix()
            assert not sim._b._general
            S.append([s.cpu() for s in sim.S])
        for other in S[1:]:
            assert all(torch.equal(a, b) for a, b in zip(S[0], other)), rule


@pytest.mark.emu
def test_bad_lattice_and_rule_values():
    import torcwa_amd
    from torcwa_amd.lattice import circular_orders
    from torcwa_amd.sweep import auto_chunk
    eng = make_engine("emu")
    with pytest.raises(ValueError):
        torcwa_amd.BatchedRCWA(1.0, [2, 2], [[1.0, 0.0], [2.0, 0.0]], engine=eng)
    with pytest.raises(ValueError):
        torcwa_amd.BatchedRCWA(1.0, [[1, 0], [0, 1]], [1.0, 1.0], engine=eng)             # no (0, 0)
    for L, order in ((HEX, [2, 2]), ([1.0, 1.0], circular_orders([1.0, 1.0], n_harmonics=9))):
        with pytest.raises(ValueError):
            torcwa_amd.BatchedRCWA(1.0, order, L, engine=eng, fourier_rule="li")
    s = torcwa_amd.BatchedRCWA(1.0, [2, 1], [[1.0, 0.0], [0.0, 2.0]], engine=eng, fourier_rule="li")     # diagonal 2 x 2 + box: today's path
    assert not s._general and s.order == [2, 1] and s.Gx_norm is not None and s.orders.shape == (15, 2)
    assert auto_chunk(5, circular_orders(HEX, n_harmonics=19), 1, "high", torch.device("cpu")) == 5


# ---- 4. basis invariance and the hexagonal lattice against its rectangular supercell -----------------------------------------------------
def _solve(eng, L, order, grid, *, lam=0.8, inc=0.2, azi=0.3, rule="laurent", field=None, d=0.5, eps_out=2.25):
    import torcwa_amd
    sim = torcwa_amd.rcwa(freq=1 / lam, order=order, L=L, dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=eps_out)
    sim.set_incident_angle(inc_ang=inc, azi_ang=azi)
    kw = {"normal_field": tuple(f.to(eng.device) for f in field)} if field is not None else {}
    sim.add_layer(thickness=d, eps=torch.as_tensor(grid).to(eng.device), **kw)
    sim.solve_global_smatrix()
    return sim


def _allS(sim, orders):
    return {(dr, pt, pol): sim.S_parameters(orders=orders, direction=dr, port=pt, polarization=pol).cpu().numpy()
            for dr, pt in (("forward", "transmission"), ("forward", "reflection")) for pol in POLS}


@pytest.mark.parametrize("backend", BACKENDS)
def test_basis_invariance(backend):
    from torcwa_amd.lattice import circular_orders
    eng = make_engine(backend)
    n = 24
    g = _hex_disk(n, n, eps=(1.0, 6.0), cplx=True)
    L2 = [HEX[0], [HEX[0][0] + HEX[1][0], HEX[0][1] + HEX[1][1]]]
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    g2 = g[(i + j) % n, j]                                     # g'[i, j] = g[(i + j) mod n, j]: the same samples in the basis (a1, a1 + a2)
    mn = circular_orders(HEX, n_harmonics=19)
    mn2 = circular_orders(L2, n_harmonics=19)
    probe = mn[:7]
    probe2 = np.stack((probe[:, 0], probe[:, 0] + probe[:, 1]), 1)
    s1, s2 = _solve(eng, HEX, mn, g), _solve(eng, L2, mn2, g2)
    A, Bm = _allS(s1, probe.tolist()), _allS(s2, probe2.tolist())
    for k in A:
        assert np.abs(A[k] - Bm[k]).max() < 1e-10, k
    # the kx, ky of a harmonic are the physical ones, whichever basis
    idx2 = [s2._b._index[(int(m), int(m + q))] for m, q in mn]
    assert torch.allclose(s1.Kx_norm_dn, s2.Kx_norm_dn[idx2], atol=1e-13) and torch.allclose(s1.Ky_norm_dn, s2.Ky_norm_dn[idx2], atol=1e-13)


def _hex_and_supercell(M, r=0.3, eps=12.0):
    """Hexagonal grid [2M, M] (disk of radius r a at the lattice point) and the a x sqrt(3) a supercell [2M, 2M] on the same samples."""
    from torcwa_amd import lattice_geometry
    geo = lattice_geometry(HEX[0], HEX[1], 2 * M, M, 200.0, dtype=torch.float64, device=torch.device("cpu"))
    gh = (1.0 + (eps - 1.0) * geo.circle(r, 0.0, 0.0)).numpy()
    i, j = np.meshgrid(np.arange(2 * M), np.arange(2 * M), indexing="ij")
    gs = gh[(i - j) % (2 * M), j % M]
    u, v = geo._disp(0.0, 0.0)
    rr = torch.sqrt(u * u + v * v)
    Nx, Ny = (u / rr).numpy(), (v / rr).numpy()
    fs = (Nx[(i - j) % (2 * M), j % M], Ny[(i - j) % (2 * M), j % M])
    return gh, gs, (Nx, Ny), fs


@pytest.mark.parametrize("backend", BACKENDS)
def test_hexagonal_equals_supercell(backend):
    from torcwa_amd.lattice import circular_orders, reciprocal
    eng = make_engine(backend)
    M = 12
    gh, gs, fh, fs = _hex_and_supercell(M)
    mh = circular_orders(HEX, n_harmonics=19)
    gmax = float(np.hypot(*(mh @ reciprocal(HEX)).T).max()) * (1 + 1e-9)
    SC = [[1.0, 0.0], [0.0, S3]]
    ms = circular_orders(SC, g_max=gmax)
    assert len(ms) > len(mh)
    probe = mh[:7]
    probe_s = np.stack((probe[:, 0], 2 * probe[:, 1] - probe[:, 0]), 1)       # hexagonal (m, n) = supercell (m, 2n - m)
    for rule, fields in (("laurent", (None, None)), ("normal", (fh, fs))):
        fh_t = tuple(torch.as_tensor(f) for f in fields[0]) if fields[0] is not None else None
        fs_t = tuple(torch.as_tensor(f) for f in fields[1]) if fields[1] is not None else None
        A = _allS(_solve(eng, HEX, mh, gh, rule=rule, field=fh_t), probe.tolist())
        Bm = _allS(_solve(eng, SC, ms, gs, rule=rule, field=fs_t), probe_s.tolist())
        for k in A:
            assert np.abs(A[k] - Bm[k]).max() < 1e-9, (rule, k)


# ---- 5. physics on the hexagonal lattice (MI355X) -----------------------------------------------------------------------------------------
def _power(sim, orders, port, a):
    """sum over the listed harmonics of the power S-parameters for p- or s-polarised incidence (a = "p" / "s").  The ps basis: the power
    normalisation of the xy basis is exact for the zeroth order only."""
    return sum(float((sim.S_parameters(orders=orders, port=port, polarization=b + a).abs() ** 2).sum()) for b in ("p", "s"))


@pytest.mark.gpu
def test_hexagonal_physics():
    from torcwa_amd.lattice import circular_orders
    eng = make_engine("gpu")
    M = 64
    gh, _, fh, _ = _hex_and_supercell(M)
    mn = circular_orders(HEX, n_harmonics=151)
    ordl = mn.tolist()
    # lossless slab: R + T = 1 over all harmonics (evanescent ones carry none), both polarisations, oblique incidence
    sim = _solve(eng, HEX, mn, gh, lam=0.8, inc=0.25, azi=0.4)
    for a in ("p", "s"):
        tot = _power(sim, ordl, "transmission", a) + _power(sim, ordl, "reflection", a)
        assert abs(tot - 1.0) < 1e-9, (a, tot)
    # a disk at normal incidence: the hexagonal lattice has no preferred in-plane axis, |t_xx| = |t_yy| (to the grid's pixelation)
    sim = _solve(eng, HEX, mn, gh, lam=1.6, inc=0.0, azi=0.0, d=0.5, eps_out=1.0)
    txx = complex(sim.S_parameters(orders=[[0, 0]], polarization="xx")[0])
    tyy = complex(sim.S_parameters(orders=[[0, 0]], polarization="yy")[0])
    print("hexagonal disk, normal incidence: |t_xx| %.6f |t_yy| %.6f" % (abs(txx), abs(tyy)))
    assert abs(abs(txx) - abs(tyy)) < 2e-3
    # an absorbing a-Si:H-like slab is passive
    lossy = np.where(gh > 6.5, (4.2 + 0.6j) ** 2, 1.0 + 0j)
    sim = _solve(eng, HEX, mn, lossy, lam=0.6, inc=0.3, azi=0.1)
    for a in ("p", "s"):
        tot = _power(sim, ordl, "transmission", a) + _power(sim, ordl, "reflection", a)
        assert tot < 1.0 + 1e-9, (a, tot)
    # the normal rule (analytic radial field) is closer than Laurent's to the converged T00 at a moderate set
    big = circular_orders(HEX, n_harmonics=475)
    ft = tuple(torch.as_tensor(f) for f in fh)
    t = lambda s: float(sum(abs(complex(s.S_parameters(orders=[[0, 0]], polarization=p)[0])) ** 2 for p in ("xx", "yx")))
    ref = t(_solve(eng, HEX, big, gh, lam=1.6, inc=0.2, azi=0.3, rule="normal", field=ft))
    e_nv = abs(t(_solve(eng, HEX, mn, gh, lam=1.6, inc=0.2, azi=0.3, rule="normal", field=ft)) - ref)
    e_la = abs(t(_solve(eng, HEX, mn, gh, lam=1.6, inc=0.2, azi=0.3)) - ref)
    print("hexagonal disk T00, %d vs %d harmonics: normal %.2e, laurent %.2e" % (len(mn), len(big), e_nv, e_la))
    assert e_nv < e_la


# ---- 6. gradients --------------------------------------------------------------------------------------------------------------------------
def _t00_of_radius(eng, R, n, mn, rule, field=None):
    from torcwa_amd import lattice_geometry
    geo = lattice_geometry(HEX[0], HEX[1], n, n, 30.0, dtype=torch.float64, device=eng.device)
    g = 1.0 + 8.0 * geo.circle(R, 0.0, 0.0)
    sim = _solve(eng, HEX, mn, g, lam=1.3, inc=0.2, azi=0.3, rule=rule, field=field)
    return (sim.S_parameters(orders=[[0, 0]], polarization="xx").abs() ** 2).sum()


@pytest.mark.parametrize("backend", BACKENDS)
def test_gradient_radius(backend):
    from torcwa_amd import lattice_geometry
    from torcwa_amd.lattice import circular_orders
    eng = make_engine(backend)
    n = 24
    mn = circular_orders(HEX, n_harmonics=13)
    geo = lattice_geometry(HEX[0], HEX[1], n, n, 30.0, dtype=torch.float64, device=torch.device("cpu"))
    u, v = geo._disp(0.0, 0.0)
    rr = torch.sqrt(u * u + v * v)
    field = (u / rr, v / rr)
    for rule, f in (("laurent", None), ("normal", field)):
        R = torch.tensor(0.27, dtype=torch.float64, device=eng.device, requires_grad=True)
        (gR,) = torch.autograd.grad(_t00_of_radius(eng, R, n, mn, rule, f), R)
        h = 1e-5
        with torch.no_grad():
            fd = (float(_t00_of_radius(eng, 0.27 + h, n, mn, rule, f)) - float(_t00_of_radius(eng, 0.27 - h, n, mn, rule, f))) / (2 * h)
        assert abs(float(gR) - fd) < 1e-6 * abs(fd), (rule, float(gR), fd)


# ---- 7. sweeps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hexagonal_sweep_matches_points():
    import torcwa_amd
    from torcwa_amd.lattice import circular_orders
    from torcwa_amd.sweep import solve_single_layer_sweep, solve_stack_sweep
    eng = make_engine("gpu")
    dev = eng.device
    M = 32
    gh, _, _, _ = _hex_and_supercell(M)
    mn = circular_orders(HEX, n_harmonics=61)
    lam = torch.linspace(0.7, 1.6, 128, dtype=torch.float64)
    orders = ((0, 0), (1, 0), (-1, -1))
    kw = dict(eps_in=1.0, eps_out=2.25, inc_ang=0.2, azi_ang=0.1, dtype=torch.complex128, engine=eng, orders=orders, chunk=128)
    g = torch.as_tensor(gh).to(dev)
    sw = solve_stack_sweep((1 / lam).to(dev), [(0.5, g)], mn, HEX, **kw).cpu()
    sw1 = solve_single_layer_sweep((1 / lam).to(dev), g[None].expand(128, -1, -1).contiguous(), 0.5, mn, HEX, **kw).cpu()
    for k in range(0, 128, 9):
        sim = _solve(eng, HEX, mn, gh, lam=float(lam[k]), inc=0.2, azi=0.1)
        ref = sim.S_parameters(orders=[list(o) for o in orders], polarization="xx").cpu()
        assert float((sw[k] - ref).abs().max()) < 1e-9 * max(float(ref.abs().max()), 1e-3), k
        assert float((sw1[k] - ref).abs().max()) < 1e-9 * max(float(ref.abs().max()), 1e-3), k
    # and the batched object itself on the general path, with G_norm [B, 2, 2]
    b = torcwa_amd.BatchedRCWA(1 / lam[:8], mn, HEX, dtype=torch.complex128, engine=eng)
    assert tuple(b.G_norm.shape) == (8, 2, 2) and b.Gx_norm is None and tuple(b.orders.shape) == (len(mn), 2)
