"""Vector-shape layers end to end (torcwa_amd.shapes, BatchedRCWA.add_layer(eps=ShapeLayer(...))), complex128, on both backends, with the
project's 1e-9 gate on values.

The oracle never sees the kernels' coefficients: E comes from the float64 closed forms of tests/shape_reference.py and goes through
oracle.rcwa_oracle on the CPU (pq_patterned -> modes_patterned -> layer_smatrix -> global_smatrix -> s_parameters).

Convergence against the grid path (test_grid_path_converges_to_the_shapes): |S_grid(n) - S_shapes| of a rasterised disk at n = 64 and 1024 is first
order in 1 / n (a factor of 16 expected, >= 4 required: staircase errors are not monotone).  Measured ratio: see MEASURED_RATIO below.
"""
import json

import numpy as np
import pytest
import torch

from oracle import rcwa_oracle as orc
from tests import shape_reference as sr
from tests.backends import BACKENDS, get_backend

MEASURED_RATIO = {"emu": 56.5, "gpu": 56.5}   # |S_grid(64) - S| / |S_grid(1024) - S| (from runs with -s)

DT = torch.complex128
FREQ, ORDER = 1 / 600., [2, 2]
RECT, OBLIQUE = [[700., 0.], [0., 660.]], [[700., 0.], [330., 640.]]
EPS_GLASS, EPS_SI = 1.46 ** 2, 12.0116 + 0.5259j
GATE = 1e-9
PROBE = [[0, 0], [1, 0], [0, -1], [-1, 1]]


def engine(backend):
    import torcwa_amd
    return torcwa_amd.Engine(lib=get_backend(backend).lib, device="cpu" if backend == "emu" else "cuda")


def layer_of(S, lattice=RECT, shift=(0., 0.), eps=EPS_SI, scale=1.0):
    """A rotated ellipse with a core nested in it, and a rotated rectangle, inside the cell."""
    a1, a2 = np.array(lattice)
    c1, c2 = 0.35 * a1 + 0.4 * a2 + shift, 0.75 * a1 + 0.7 * a2 + shift
    ell = S.ellipse(150. * scale, 90., c1[0], c1[1], eps, theta=0.3)
    return S.ShapeLayer(1.0, [ell, S.circle(40., c1[0], c1[1], 2.0, host=ell), S.rectangle(120., 80., c2[0], c2[1], 4.0 + 0.1j, theta=-0.4)])


def solver(eng, lattice, order=ORDER, freq=FREQ, **kw):
    import torcwa_amd
    f = torch.as_tensor(freq, dtype=torch.float64, device=eng.device).reshape(-1)
    sim = torcwa_amd.BatchedRCWA(f, order, lattice, dtype=DT, engine=eng, **kw)
    sim.add_input_layer(eps=EPS_GLASS)
    sim.add_output_layer(eps=1.)
    sim.set_incident_angle(0., 0.)
    return sim


def oracle_S(lattice, shapes, val, thickness):
    """The global S-matrix of glass / shape layer / air at normal incidence from the test's own E; (setup, S)."""
    mn = np.array([(m, n) for m in range(-ORDER[0], ORDER[0] + 1) for n in range(-ORDER[1], ORDER[1] + 1)])
    recip, area = sr.recip_of(*lattice)
    E = torch.from_numpy(sr.gather(sr.plain_box(shapes, np.asarray(val), recip, area, *ORDER), mn, *ORDER))
    s = orc.Setup(freq=FREQ, order=ORDER, L=[1., 1.], dtype=DT, eps_in=EPS_GLASS, eps_out=1.0, has_in=True, has_out=True)
    G = torch.from_numpy(np.linalg.inv(np.array(lattice)).T) / FREQ            # rows b1 / f, b2 / f (without 2 pi: k is in units of k0)
    m, n = torch.from_numpy(mn[:, 0]), torch.from_numpy(mn[:, 1])
    s.kx, s.ky = (m * G[0, 0] + n * G[1, 0]).to(DT), (m * G[0, 1] + n * G[1, 1]).to(DT)
    s.Vf = orc._halfspace_V(s.kx, s.ky, 1.0)
    s.Vi, s.Vo = orc._halfspace_V(s.kx, s.ky, torch.as_tensor(EPS_GLASS, dtype=DT)), orc._halfspace_V(s.kx, s.ky, torch.as_tensor(1.0, dtype=DT))
    T, D = torch.linalg.inv(s.Vf + s.Vi), s.Vf - s.Vi
    s.Sin = [2 * (T @ s.Vi), -(T @ D), T @ D, 2 * (T @ s.Vf)]
    T, D = torch.linalg.inv(s.Vf + s.Vo), s.Vf - s.Vo
    s.Sout = [2 * (T @ s.Vf), T @ D, -(T @ D), 2 * (T @ s.Vo)]
    M = torch.eye(len(mn), dtype=DT)
    P, Q = orc.pq_patterned(E, M, s.kx, s.ky)
    kz, W = orc.modes_patterned(P, Q)
    lay = orc.layer_smatrix(orc.Layer(thickness=thickness, E=E, M=M, P=P, Q=Q, kz=kz, W=W), s.Vf, s.omega)
    return s, orc.global_smatrix(s, [lay])[0]


def flat(layer, B=1):
    """[(kind, par)], val of a ShapeLayer at sweep point 0, as tests/shape_reference.py takes them."""
    p = layer.pack(np.eye(2), B, "cpu")
    voff = p.voff.tolist()
    return ([(int(k), p.par[0, voff[i]:voff[i + 1]].tolist()) for i, k in enumerate(p.kind.tolist())], p.val[0].numpy())


def close(a, b, what=""):
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    err, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
    assert err <= GATE * scale, f"{what}: |diff| {err:.3e} against the gate {GATE * scale:.1e}"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["rect", "oblique"])
def test_against_the_oracle_with_the_tests_own_E(backend, name):
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    lattice = RECT if name == "rect" else OBLIQUE
    layer = layer_of(S, lattice)
    sim = solver(engine(backend), [700., 660.] if name == "rect" else lattice, ORDER if name == "rect" else rect_orders(*ORDER).tolist())
    sim.add_layer(120., eps=layer)
    sim.solve_global_smatrix()
    shapes, val = flat(layer)
    s, Sg = oracle_S(lattice, shapes, val, 120.)
    for pol in ("xx", "yx", "xy", "yy"):
        for port in ("transmission", "reflection"):
            got = sim.S_parameters(PROBE, polarization=pol, port=port)[0]
            close(got, orc.s_parameters(s, Sg, PROBE, polarization=pol, port=port), f"{name} {pol} {port}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_full_cell_rectangle_is_the_homogeneous_layer(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    sims = []
    for eps in (S.ShapeLayer(1.0, [S.rectangle(700., 660., 350., 330., EPS_SI)]), EPS_SI):
        sim = solver(eng, [700., 660.])
        sim.add_layer(120., eps=eps)
        sim.solve_global_smatrix()
        sim.source_planewave(amplitude=[1., 0.3], direction="forward")
        sims.append(sim)
    for pol in ("xx", "yy", "pp"):
        close(sims[0].S_parameters(PROBE, polarization=pol), sims[1].S_parameters(PROBE, polarization=pol), pol)
    x, y = (torch.linspace(0., L, 7, dtype=torch.float64, device=eng.device) for L in (700., 660.))
    for a, b in zip(sum(sims[0].field_xy(0, x, y, z_prop=50.), []), sum(sims[1].field_xy(0, x, y, z_prop=50.), [])):
        close(a, b, "field_xy")


@pytest.mark.parametrize("backend", BACKENDS)
def test_translation_multiplies_order_mn_by_the_phase_of_G_dot_d(backend):
    """eps'(r) = eps(r - d) at normal incidence: the fields are those of eps shifted by d, so the amplitude of order (m, n) is multiplied by
    exp(-i G_mn . d), G_mn = m b1 + n b2 -- exact at finite truncation (E' = D E D^H with D = diag(exp(-i G . d)))."""
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    eng, d = engine(backend), np.array([37., -53.])
    out = []
    for shift in (np.zeros(2), d):
        sim = solver(eng, OBLIQUE, rect_orders(*ORDER).tolist())
        sim.add_layer(120., eps=layer_of(S, OBLIQUE, shift=shift))
        sim.solve_global_smatrix()
        out.append(torch.stack([sim.S_parameters(PROBE, polarization=pol, port=port)[0] for pol in ("xx", "yx") for port in ("t", "r")]).cpu())
    b = 2 * np.pi * np.linalg.inv(np.array(OBLIQUE)).T
    phase = torch.tensor([np.exp(-1j * (m * b[0] + n * b[1]) @ d) for m, n in PROBE])
    assert abs(phase[1] - 1) > 0.1                                         # the shift is visible in the orders it should be
    close(out[1], out[0] * phase[None, :], "shifted")
    close(out[1][:, 0], out[0][:, 0], "order (0, 0)")


@pytest.mark.parametrize("backend", BACKENDS)
def test_lossless_stack_conserves_energy(backend):
    import torcwa_amd.shapes as S
    sim = solver(engine(backend), OBLIQUE, [[m, n] for m in range(-2, 3) for n in range(-2, 3) if abs(m) + abs(n) <= 3])
    sim.add_layer(120., eps=S.ShapeLayer(1.0, [S.ellipse(150., 90., 300., 250., 12.0, theta=0.3), S.polygon([[500., 400.], [800., 450.], [640., 600.]], 4.0)]))
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1., 0.5j], direction="forward")
    ab = sim.absorption()
    assert float(ab["A"].abs().max()) <= GATE and float((ab["R"] + ab["T"] - 1).abs().max()) <= GATE


def _disk_S(eng, eps):
    sim = solver(eng, [700., 660.], keep_coupling=False)
    sim.add_layer(120., eps=eps)
    return torch.stack([sim.solve_S_parameters(PROBE, polarization=pol, port=port)[0] for pol in ("xx", "yy") for port in ("t", "r")]).cpu()


@pytest.mark.parametrize("backend", BACKENDS)
def test_grid_path_converges_to_the_shapes(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    layer = S.ShapeLayer(1.0, [S.circle(213., 341., 317., EPS_SI)])
    exact = _disk_S(eng, layer)
    err = [float((_disk_S(eng, layer.rasterise([700., 0.], [0., 660.], n, n, device=eng.device)[0]) - exact).abs().max()) for n in (64, 1024)]
    print(f"|S_grid(n) - S_shapes| at n = 64, 1024: {err[0]:.3e}, {err[1]:.3e}; ratio {err[0] / err[1]:.1f} [{backend}]")
    assert err[1] > 100 * GATE                 # the staircase error of the finest grid the kernels take in stride is far above the gate
    assert err[0] / err[1] >= 4


@pytest.mark.parametrize("backend", BACKENDS)
def test_batched_equals_single_solves_and_the_sweep_drivers(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    from torcwa_amd.sweep import solve_single_layer_sweep, solve_stack_sweep
    eng = engine(backend)
    R = torch.tensor([150., 170., 190.], dtype=torch.float64)
    freq = torch.tensor([1 / 600., 1 / 620., 1 / 640.], dtype=torch.float64, device=eng.device)
    mk = lambda r: S.ShapeLayer(1.0, [S.ellipse(r, 90., 300., 250., EPS_SI, theta=0.3), S.rectangle(100., 60., 560., 500., 3.0)])
    sim = solver(eng, [700., 660.], freq=freq, keep_coupling=False)
    sim.add_layer(120., eps=mk(R))
    got = sim.solve_S_parameters(PROBE, polarization="xx")
    for b in range(3):
        one = solver(eng, [700., 660.], freq=freq[b], keep_coupling=False)
        one.add_layer(120., eps=mk(R[b]))
        close(one.solve_S_parameters(PROBE, polarization="xx")[0], got[b], f"point {b}")
        close(mk(R).slice(b, b + 1).pack(np.eye(2), 1, "cpu").par, mk(R[b]).pack(np.eye(2), 1, "cpu").par, "slice")
    kw = dict(eps_in=EPS_GLASS, eps_out=1., dtype=DT, engine=eng, chunk=2, orders=[tuple(o) for o in PROBE])
    close(solve_stack_sweep(freq, [(120., mk(R))], ORDER, [700., 660.], **kw), got, "solve_stack_sweep")
    close(solve_single_layer_sweep(freq.cpu(), mk(R), 120., ORDER, [700., 660.], **kw), got, "solve_single_layer_sweep")
    # the drop-in is the B = 1 view
    drop = torcwa_amd.rcwa(freq=1 / 600., order=ORDER, L=[700., 660.], dtype=DT, engine=eng)
    drop.add_input_layer(eps=EPS_GLASS)
    drop.add_output_layer(eps=1.)
    drop.set_incident_angle(inc_ang=0., azi_ang=0.)
    drop.add_layer(thickness=120., eps=mk(R[0]))
    drop.solve_global_smatrix()
    close(drop.S_parameters(orders=PROBE, polarization="xx"), got[0], "rcwa drop-in")


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_shape_layer_equals_plain_solves(backend):
    import torcwa_amd.shapes as S
    from torcwa_amd.sweep import solve_thickness_sweep
    eng = engine(backend)
    layer = layer_of(S)
    ds = [100., 120., 145.]
    sim = solver(eng, [700., 660.], keep_coupling=False, fold_layers=True)
    sim.add_layer(60., eps=2.1)
    sim.add_layer(ds, eps=layer, swept=True)
    got = sim.solve_S_parameters(PROBE, polarization="xx")
    for t, d in enumerate(ds):
        one = solver(eng, [700., 660.], keep_coupling=False, fold_layers=True)
        one.add_layer(60., eps=2.1)
        one.add_layer(d, eps=layer)
        close(one.solve_S_parameters(PROBE, polarization="xx"), got[:, t], f"thickness {d}")
    f = torch.tensor([FREQ], dtype=torch.float64, device=eng.device)
    close(solve_thickness_sweep(f, [(60., 2.1), (0., layer)], ORDER, [700., 660.], layer=1, thicknesses=ds, eps_in=EPS_GLASS, eps_out=1., dtype=DT,
                                engine=eng, orders=[tuple(o) for o in PROBE]), got, "solve_thickness_sweep")


@pytest.mark.parametrize("backend", BACKENDS)
def test_keep_coupling_holds_the_layer_and_regions_take_grid_masks(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    layer = S.ShapeLayer(1.0, [S.rectangle(350., 330., 262.5, 247.5, EPS_SI)])          # edges on the pixel boundaries of a 24 x 24 grid
    sim = solver(eng, [700., 660.])
    sim.add_layer(120., eps=layer)
    assert sim.eps_grid[0] is layer
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1., 0.], direction="forward")
    inside = (layer.rasterise([700., 0.], [0., 660.], 24, 24, device=eng.device)[0].real > 2).to(torch.float64)
    reg = sim.absorption_by_region(0, masks=torch.stack([inside, 1 - inside]))
    ab = sim.absorption()
    assert float(reg[:, 1].abs().max()) == 0.0                             # air absorbs nothing
    whole = sim.absorption_by_region(0, masks=torch.ones((1, 24, 24), dtype=torch.float64, device=eng.device))
    close(reg.sum(dim=1), whole[:, 0], "regions add up")                   # Im(eps) sampled on the masks' grid, linear in the mask
    assert float(reg[0, 0]) > 0.5 * float(ab["layers"][0, 0]) > 0          # the raster's Laurent matrix, not the closed form's: same size, not equal
    with pytest.raises(ValueError, match="takes grid masks"):
        sim.absorption_by_region(0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    eng = engine(backend)
    layer = S.ShapeLayer(1.0, [S.circle(200., 350., 330., 4.0)])
    for kw, msg in ((dict(fourier_rule="li"), 'needs fourier_rule="laurent"'), (dict(fourier_rule="normal"), 'needs fourier_rule="laurent"'),
                    (dict(symmetry="xy"), "the mirror is detected from grids"),
                    (dict(symmetry="xy", symmetry_sector=True, keep_coupling=False), "the mirror is detected from grids")):
        with pytest.raises(ValueError, match=msg):
            solver(eng, [700., 660.], **kw).add_layer(120., eps=layer)
    with pytest.raises(ValueError, match="cannot be given as mu"):
        solver(eng, [700., 660.]).add_layer(120., eps=2.0, mu=layer)
    with pytest.raises(ValueError, match="normal_field"):
        solver(eng, [700., 660.]).add_layer(120., eps=layer, normal_field=(torch.zeros(8, 8), torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="non-empty list"):
        S.ShapeLayer(1.0, [])
    with pytest.raises(ValueError, match="same layer"):
        S.ShapeLayer(1.0, [S.circle(10., 1., 1., 2.0, host=S.circle(20., 1., 1., 3.0))])
    with pytest.raises(ValueError, match="sweep points"):
        solver(eng, [700., 660.]).add_layer(120., eps=S.ShapeLayer(1.0, [S.circle(torch.tensor([1., 2.]), 1., 1., 2.0)]))


def test_rasterise_samples_at_the_dft_positions():
    import torcwa_amd.shapes as S
    g = S.ShapeLayer(1.0, [S.rectangle(0.5, 0.25, 0.25, 0.125, 5.0), S.polygon([[0.5, 0.5], [1.0, 0.5], [1.0, 1.0]], 3.0)]).rasterise([1., 0.], [0., 1.], 8, 8)
    assert g.shape == (1, 8, 8) and g[0, 1, 1] == 5.0 and g[0, 0, 0] == 1.0 and g[0, 3, 1] == 5.0 and g[0, 4, 1] == 1.0     # (i / n), no half pixel
    assert g[0, 6, 5] == 3.0 and g[0, 5, 6] == 1.0
    wrap = S.ShapeLayer(1.0, [S.circle(0.2, 0.0, 0.0, 2.0)]).rasterise([1., 0.], [0., 1.], 8, 8)
    assert wrap[0, 7, 7] == 2.0 and wrap[0, 1, 7] == 2.0 and wrap[0, 4, 4] == 1.0       # a shape across the cell boundary wraps around
    cw = S.polygon([[0., 0.], [0., 1.], [1., 1.], [1., 0.]], 2.0)._row(1, "cpu").reshape(4, 2)
    assert torch.equal(cw, torch.tensor([[1., 0.], [1., 1.], [0., 1.], [0., 0.]], dtype=torch.float64))    # a clockwise list is reversed
    rh = S.rhombus(2., 1., 0.5, 0.5, 2.0)._row(1, "cpu").reshape(4, 2)
    assert torch.allclose(rh, torch.tensor([[1.5, 0.5], [0.5, 1.0], [-0.5, 0.5], [0.5, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("backend", BACKENDS)
def test_grid_layers_issue_the_recorded_calls_and_shapes_swap_one_entry(backend):
    """The grid path's libtrx call list is the one of tests/golden/call_trace.json (recorded before vector shapes existed), and the same stack
    with its patterned layers as ShapeLayers differs from it in the factorisation entry alone."""
    import torcwa_amd.shapes as S
    from tests import test_call_trace as tct
    with open(tct.FIXTURE) as f:
        want = json.load(f)["fold"]
    got, _ = tct.record(backend, "fold")
    assert json.loads(json.dumps(got)) == want
    eng, trace = tct.recording_engine(backend)
    layers = [(60., 2.1), (120., S.ShapeLayer(1.0, [S.rectangle(420., 264., 350., 330., tct.EPS_SI)])), (40., 1.9 + 0.05j),
              (90., S.ShapeLayer(1.0, [S.circle(245., 350., 330., tct.EPS_SI)]))]
    tct._two_readouts(tct._batched(eng, layers=layers, keep_coupling=False, fold_layers=True))
    names = [c[0] for c in trace]
    assert [("convmat_shapes" if c[0] == "convmat" else c[0]) for c in want] == names
    assert all(a[1:] == b[1:] for a, b in zip(json.loads(json.dumps(trace)), want) if a[0] != "convmat_shapes")
