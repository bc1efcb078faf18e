"""symmetry_sector=True end to end: only the mirror sectors a source excites are cascaded, against the REFERENCE's own fixtures (tests/golden,
never against the unfolded path of this project), at the tolerances the existing golden tests apply to the same case and dtype
(tests/test_pipeline.py): max |difference| over max(largest |S| of the (direction, port), 1e-3) below 1e-9 for complex128 and 1e-5 for
complex64 I/O on the float32-exact grids.

example1 (centred rectangle, normal incidence) has both mirrors; example2 (15 degrees in the xz plane) only the y mirror; thickness_example1_o3
adds a second frequency and four thicknesses; sector_stack_o3 (make_sector_golden.py) is a three-layer stack -- rectangle, homogeneous spacer,
circle on one grid -- between two half-spaces, with ref_order [0, 0] and [1, 0].  Every solver counts the sizes of its eigen calls: an x- or
y-polarised (0, 0) order solves ONE sector per patterned layer, the ps basis two.
"""
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import DIRPORT, GOLDEN, ORDERS_PROBE, POLS, case_inputs, load_case
from tests.test_pipeline import make_engine

GPU, EMU = pytest.mark.gpu, pytest.mark.emu
TOL = {"c128": 1e-9, "c64": 1e-5}


def _cast(v, dtype, dev):
    if not torch.is_tensor(v):
        return v
    if dtype == "c64":
        v = v.to(torch.complex64 if v.is_complex() else torch.float32)
    return v.to(dev)


def _solver(eng, freq, order, L, layers, dtype, sym, *, eps_in=None, eps_out=None, inc=0.0, azi=0.0, angle_layer="input", **kw):
    """(BatchedRCWA with symmetry_sector=True, the list its eigen calls append their sizes to)."""
    import torcwa_amd
    kw.setdefault("keep_coupling", False)
    kw.setdefault("symmetry_sector", True)
    sim = torcwa_amd.BatchedRCWA(freq, order, L, dtype=torch.complex128 if dtype == "c128" else torch.complex64, engine=eng, symmetry=sym, **kw)
    sizes, inner = [], sim._eig_call

    def counted(A, **k):
        sizes.append(int(A.shape[-1]))
        return inner(A, **k)
    sim._eig_call = counted
    if eps_in is not None:
        sim.add_input_layer(eps=eps_in)
    if eps_out is not None:
        sim.add_output_layer(eps=eps_out)
    sim.set_incident_angle(inc, azi, angle_layer)
    for (d, eps, mu) in layers:
        sim.add_layer(d, _cast(eps, dtype, eng.device), _cast(mu, dtype, eng.device))
    assert sizes == []                                                                # add_layer makes no eigen call in sector mode
    return sim, sizes


def _case_solver(eng, g, dtype, sym, **kw):
    ci = case_inputs(g, "c128")
    return _solver(eng, ci["freq"], ci["order"], ci["L"], ci["layers"], dtype, sym, eps_in=ci.get("eps_in"), eps_out=ci.get("eps_out"),
                   inc=ci["inc_ang"], azi=ci["azi_ang"], angle_layer=ci["angle_layer"], **kw)


# (backend, fixture, symmetry, dtype): the emulator runs complex128 and one symmetry of the n = 242 case; the GPU everything
GOLDEN_RUNS = [pytest.param(be, name, sym, dt, marks=GPU if be == "gpu" else EMU)
               for be in ("emu", "gpu")
               for name, syms in (("example1_o3", ("xy", "x", "y")), ("example1_o5", ("xy", "x", "y")), ("example2_o4", ("y",)))
               for sym in (syms if (be == "gpu" or name != "example1_o5") else syms[:1])
               for dt in (("c128",) if be == "emu" else ("c128", "c64"))]


@pytest.mark.parametrize("backend,name,sym,dtype", GOLDEN_RUNS)
def test_golden_sparams_in_sector_mode(backend, name, sym, dtype):
    """Every polarisation, direction and port of the fixture's `sparams` at all ORDERS_PROBE, and the two S-parameters the fixtures hold for
    another ref_order, through solve_S_parameters; the sectors that were solved are counted."""
    eng = make_engine(backend)
    tol = TOL[dtype]
    g = load_case(name, "c128" if dtype == "c128" else "c128f32")
    n = 2 * (2 * int(g["order"][0]) + 1) * (2 * int(g["order"][1]) + 1)
    nblk = 4 if sym == "xy" else 2
    # one sector for an x-polarised (0, 0) order, two for the ps basis (on fresh solvers: the sectors are cached per solver)
    sim, sizes = _case_solver(eng, g, dtype, sym)
    sim.solve_S_parameters(ORDERS_PROBE, polarization="xx")
    assert len(sizes) == 1 and abs(sizes[0] - n / nblk) <= 1, sizes
    sim.solve_S_parameters(ORDERS_PROBE, polarization="xx", direction="b", port="r")
    assert len(sizes) == 1                                                            # cached: another block of the same sector
    sim2, sizes2 = _case_solver(eng, g, dtype, sym)
    sim2.solve_S_parameters(ORDERS_PROBE, polarization="pp")
    assert len(sizes2) == 2 and all(abs(s - n / nblk) <= 1 for s in sizes2), sizes2
    assert sim.symmetry_residual == [None] * int(g["n_layers"]) and not hasattr(sim, "S") and not hasattr(sim, "C")
    sp = g["sparams"]
    worst = 0.0
    for a, (dr, pt) in enumerate(DIRPORT):
        scale = max(np.abs(sp[a]).max(), 1e-3)
        for b, pol in enumerate(POLS):
            v = sim.solve_S_parameters(ORDERS_PROBE, direction=dr, port=pt, polarization=pol, ref_order=[0, 0]).cpu().numpy()
            assert v.dtype == (np.complex128 if dtype == "c128" else np.complex64) and v.shape == (1, len(ORDERS_PROBE))
            err = np.abs(v[0] - sp[a, b]).max() / scale
            worst = max(worst, err)
            assert err < tol, (dr, pt, pol, err)
    assert len(sizes) == 2                                                            # x and y columns of (0, 0): two sectors, whatever was asked
    v = sim.solve_S_parameters(ORDERS_PROBE, direction="f", port="t", polarization="yx", ref_order=[-1, 1], power_norm=False).cpu().numpy()
    assert np.abs(v[0] - g["sparams_yx_ref_m1p1_nonorm"]).max() < tol
    v = sim.solve_S_parameters(ORDERS_PROBE, direction="f", port="r", polarization="ps", ref_order=[0, 1]).cpu().numpy()
    assert np.abs(v[0] - g["sparams_ps_ref_0p1_refl"]).max() < tol
    print(f"{name} {sym} {dtype}: worst error / scale = {worst:.2e}, eigen calls {sizes}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_thickness_fixture_as_a_batch_of_two(backend, dtype):
    """thickness_example1_o3: the two frequencies as a batch of 2, every stored thickness a solve of its own; all four (direction, port) pairs."""
    eng = make_engine(backend)
    z = np.load(os.path.join(GOLDEN, "thickness_example1_o3.npz"))
    ci = case_inputs(load_case("example1_o3", "c128f32"), "c128")
    (_, eps, mu), = ci["layers"]
    freq = torch.tensor(z["freqs"], dtype=torch.float64, device=eng.device)
    ref = z["sparams"]                                                                # [freq, T, dirport, pol, order]
    for ti, d in enumerate(z["thicknesses"]):
        sim, sizes = _solver(eng, freq, ci["order"], ci["L"], [(float(d), eps, mu)], dtype, "xy", eps_in=ci.get("eps_in"), eps_out=ci.get("eps_out"))
        for a, (dr, pt) in enumerate(DIRPORT):
            scale = max(np.abs(ref[:, :, a]).max(), 1e-3)
            for b, pol in enumerate(["xx", "yy", "xy"]):
                got = sim.solve_S_parameters(z["orders"].tolist(), direction=dr, port=pt, polarization=pol).cpu().numpy()
                err = np.abs(got - ref[:, ti, a, b]).max() / scale
                assert got.shape == (2, len(z["orders"])) and err < TOL[dtype], (float(d), dr, pt, pol, err)
        assert len(sizes) == 2


def _stack(dtype):
    z = np.load(os.path.join(GOLDEN, "sector_stack_o3.npz"))
    g = {k: z[k] for k in z.files}
    grids = [torch.from_numpy(g[k]) for k in ("eps_rect", "eps_circ")]
    if dtype == "c64":                                                                # variant 1 of the fixture: the float32-exact grids
        grids = [e.to(torch.complex64).to(torch.complex128) for e in grids]
    d = [float(v) for v in g["thicknesses"]]
    layers = [(d[0], grids[0], 1.0), (d[1], float(g["eps_spacer"]), 1.0), (d[2], grids[1], 1.0)]
    return g, layers, g["sparams"][0 if dtype == "c128" else 1]


STACK_RUNS = [pytest.param(be, sym, dt, marks=GPU if be == "gpu" else EMU)
              for be in ("emu", "gpu") for sym in ("xy", "x", "y") for dt in (("c128",) if (be == "emu" and sym != "xy") else ("c128", "c64"))]


@pytest.mark.parametrize("backend,sym,dtype", STACK_RUNS)
def test_three_layer_stack(backend, sym, dtype):
    """sector_stack_o3: rectangle / homogeneous spacer / circle between two half-spaces; xx, yy, yx, xy, both directions, both ports, for
    ref_order [0, 0] (one sector per column) and [1, 0] (two sectors per column under "xy", four in all)."""
    eng = make_engine(backend)
    g, layers, ref = _stack(dtype)
    tol = TOL[dtype]
    kw = dict(eps_in=float(g["eps_in"]), eps_out=float(g["eps_out"]))
    order, L = [int(v) for v in g["order"]], [float(v) for v in g["L"]]
    for ri, ro in enumerate(g["refs"].tolist()):
        sim, sizes = _solver(eng, float(g["freq"]), order, L, layers, dtype, sym, **kw)
        for a, (dr, pt) in enumerate(DIRPORT):
            scale = max(np.abs(ref[ri, a]).max(), 1e-3)
            for b, pol in enumerate(["xx", "yy", "yx", "xy"]):
                got = sim.solve_S_parameters(g["orders"].tolist(), direction=dr, port=pt, polarization=pol, ref_order=ro).cpu().numpy()
                err = np.abs(got[0] - ref[ri, a, b]).max() / scale
                assert err < tol, (ro, dr, pt, pol, err)
            if a == 0:                                                                # after forward transmission xx .. xy: x and y columns
                want = 2 if (ri == 0 or sym != "xy") else 4
                assert len(sizes) == 2 * want, (ro, sizes)                            # two patterned layers per sector
        assert sorted(sim._sector_S) == (list(range(4 if sym == "xy" else 2)) if ri == 1 else ([1, 2] if sym == "xy" else [0, 1]))
        assert sim.symmetry_residual == [None, None, None]


@pytest.mark.gpu
def test_config2_fullsize_sector_sweep():
    """config 2 at its real size (order [15,15], n = 1922, one sector of 481 / 480) through solve_single_layer_sweep and the mixed-precision
    eigensolver, complex64 I/O at the 1e-5 of the full-size golden test: the twin of test_symmetry.py::test_config2_fullsize_folded_sweep."""
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = make_engine("gpu")
    g = load_case("config2_o15_l532", "c128f32")
    B = 4
    grids = torch.from_numpy(g["L0_eps_grid"]).to(torch.complex64).to(eng.device)[None].expand(B, -1, -1).contiguous()
    freq = torch.full((B,), float(g["freq"]), dtype=torch.float64, device=eng.device)
    for pol, pi in (("xx", 0), ("yy", 3)):
        out = solve_single_layer_sweep(freq, grids, float(g["L0_thickness"]), [15, 15], [float(v) for v in g["L"]], eps_in=float(np.real(g["eps_in"])),
                                       dtype=torch.complex64, precision="high", engine=eng, chunk=4, eig_route="mixed", symmetry="xy",
                                       symmetry_sector=True, orders=[tuple(o) for o in ORDERS_PROBE[:7]], polarization=pol).cpu().numpy()
        ref = g["sparams"][0, pi, :7]
        err = np.abs(out - ref[None]).max() / np.abs(ref).max()
        print(f"{pol}: max error / max |ref| = {err:.2e}")
        assert out.dtype == np.complex64 and err < 1e-5, pol


@pytest.mark.parametrize("backend", BACKENDS)
def test_sweep_drivers_in_sector_mode(backend):
    """solve_single_layer_sweep on two copies of example1_o3 and solve_stack_sweep on the three-layer stack, in chunks of one point."""
    from torcwa_amd.sweep import solve_single_layer_sweep, solve_stack_sweep
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    grids = torch.from_numpy(g["L0_eps_grid"]).to(eng.device)[None].expand(2, -1, -1).contiguous()
    freq = torch.full((2,), float(g["freq"]), dtype=torch.float64, device=eng.device)
    out = solve_single_layer_sweep(freq, grids, float(g["L0_thickness"]), [3, 3], [float(v) for v in g["L"]], eps_in=float(np.real(g["eps_in"])),
                                   dtype=torch.complex128, engine=eng, symmetry="xy", symmetry_sector=True, orders=[tuple(o) for o in ORDERS_PROBE[:7]],
                                   polarization="yy").cpu().numpy()
    ref = g["sparams"][0, 3, :7]
    assert np.abs(out - ref[None]).max() / np.abs(ref).max() < 1e-9
    s, layers, sp = _stack("c128")
    freq = torch.full((2,), float(s["freq"]), dtype=torch.float64, device=eng.device)
    layers = [(d, e.to(eng.device) if torch.is_tensor(e) else e) for d, e, _ in layers]
    out = solve_stack_sweep(freq, layers, [int(v) for v in s["order"]], [float(v) for v in s["L"]], eps_in=float(s["eps_in"]), eps_out=float(s["eps_out"]),
                            dtype=torch.complex128, engine=eng, chunk=1, symmetry="xy", symmetry_sector=True, orders=[tuple(o) for o in s["orders"][:7]],
                            polarization="xx", direction="backward", port="reflection").cpu().numpy()
    ref = sp[0, 2, 0, :7]
    assert np.abs(out - ref[None]).max() / max(np.abs(sp[0, 2]).max(), 1e-3) < 1e-9
    with pytest.raises(ValueError, match="absorption"):
        solve_stack_sweep(freq, layers, [3, 2], [700., 660.], engine=eng, symmetry="xy", symmetry_sector=True, absorption=True)
    with pytest.raises(ValueError, match="needs symmetry="):
        solve_stack_sweep(freq, layers, [3, 2], [700., 660.], engine=eng, symmetry_sector=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    import torcwa_amd
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    grid = torch.from_numpy(g["L0_eps_grid"]).to(eng.device)
    base = dict(dtype=torch.complex128, engine=eng, keep_coupling=False, symmetry="xy", symmetry_sector=True)
    new = lambda **kw: torcwa_amd.BatchedRCWA(1 / 532., [3, 2], [300., 300.], **{**base, **kw})
    with pytest.raises(ValueError, match="needs symmetry="):
        new(symmetry=None)
    with pytest.raises(ValueError, match="keep_coupling=False"):
        new(keep_coupling=True)
    with pytest.raises(ValueError, match="drop-in class rcwa"):
        torcwa_amd.rcwa(freq=1 / 532., order=[3, 2], L=[300., 300.], dtype=torch.complex128, engine=eng, symmetry="xy", symmetry_sector=True)
    with pytest.raises(ValueError, match="avoid_Pinv_instability"):
        new(avoid_Pinv_instability=True)
    with pytest.raises(ValueError, match="differentiable"):
        new(symmetry_grad=True)
    sim = new()
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    with pytest.raises(ValueError, match="swept=True"):
        sim.add_layer(torch.tensor([100., 200.]), grid, swept=True)
    with pytest.raises(ValueError, match="differentiable"):
        sim.add_layer(100., grid.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="differentiable"):
        sim.add_layer(torch.tensor(100., dtype=torch.float64, device=eng.device, requires_grad=True), grid)
    simn = new(fourier_rule="normal")
    simn.set_incident_angle(0., 0.)
    with pytest.raises(ValueError, match="normal_field"):
        simn.add_layer(100., grid, normal_field=(torch.zeros_like(grid.real), torch.ones_like(grid.real)))
    assert sim.layer_N == 0
    sim.add_layer(100., grid)
    for name, call in (("solve_global_smatrix", lambda: sim.solve_global_smatrix()),
                       ("S_parameters", lambda: sim.S_parameters([[0, 0]])),
                       ("source_planewave", lambda: sim.source_planewave(amplitude=[1., 0.])),
                       ("source_fourier", lambda: sim.source_fourier(amplitude=[1., 0.], orders=[[0, 0]])),
                       ("power_flux", lambda: sim.power_flux(0)),
                       ("incident_flux", lambda: sim.incident_flux()),
                       ("absorption", lambda: sim.absorption()),
                       ("volume_integral", lambda: sim.volume_integral(0)),
                       ("absorption_by_region", lambda: sim.absorption_by_region(0))):
        with pytest.raises(ValueError, match=f"{name} is not available with symmetry_sector=True"):
            call()
    # a wave vector outside the mirror plane is refused as for symmetry= alone
    with pytest.raises(ValueError, match="kx0_norm must be exactly 0"):
        new().set_incident_angle(0.2, 0.)


@pytest.mark.parametrize("backend", BACKENDS)
def test_mismatched_centres_raise(backend):
    """One plan for the whole stack: a second layer whose grid mirrors about sample 0 while the first mirrors about the half-cell centre is
    refused, naming both; homogeneous layers before and after do not matter; the same grids are accepted by symmetry= alone."""
    import torcwa_amd
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    first = torch.from_numpy(g["L0_eps_grid"]).to(eng.device)
    nx, ny = first.shape
    r = torch.from_numpy(np.random.default_rng(5).random((nx, ny)))
    for ax in (0, 1):
        r = r + torch.roll(torch.flip(r, dims=(ax,)), 1, dims=(ax,))                   # symmetric about sample 0
    second = (1.0 + r).to(torch.complex128).to(eng.device)
    for sector in (True, False):
        sim = torcwa_amd.BatchedRCWA(1 / 532., [3, 2], [300., 300.], dtype=torch.complex128, engine=eng, keep_coupling=False, symmetry="xy",
                                     symmetry_sector=sector)
        sim.set_incident_angle(0., 0.)
        sim.add_layer(40., 2.1)
        sim.add_layer(100., first)
        sim.add_layer(40., 1.5)
        if sector:
            with pytest.raises(ValueError, match=rf"\(0, 1, 0, 1\), differ from those of the first patterned layer, \({nx - 1}, {nx}, {ny - 1}, {ny}\)"):
                sim.add_layer(80., second)
            sim.add_layer(80., first)                                                 # the stack is still usable
            assert sim.solve_S_parameters([[0, 0]]).shape == (1, 1)
        else:
            sim.add_layer(80., second)


@pytest.mark.parametrize("backend", BACKENDS)
def test_only_homogeneous_layers(backend):
    """No patterned layer: the stack's plan uses centres 0; fresnel_30 has ky0 = 0 only ("y" mirror) -- against the fixture."""
    eng = make_engine(backend)
    g = load_case("fresnel_30", "c128")
    sim, sizes = _case_solver(eng, g, "c128", "y")
    sp = g["sparams"]
    for a, (dr, pt) in enumerate(DIRPORT):
        scale = max(np.abs(sp[a]).max(), 1e-3)
        for b, pol in enumerate(POLS):
            v = sim.solve_S_parameters(ORDERS_PROBE, direction=dr, port=pt, polarization=pol).cpu().numpy()
            assert np.abs(v[0] - sp[a, b]).max() / scale < 1e-9, (dr, pt, pol)
    assert sizes == [] and sim._sector_centres is None


@pytest.mark.parametrize("backend", BACKENDS)
def test_default_leaves_symmetry_bit_identical(backend):
    """symmetry_sector=False is the default and today's symmetry= path: modes and S-parameters equal a run without the keyword bit for bit."""
    import torcwa_amd
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    ci = case_inputs(g, "c128")
    sims = []
    for kw in ({}, {"symmetry_sector": False}):
        sim = torcwa_amd.BatchedRCWA(ci["freq"], ci["order"], ci["L"], dtype=torch.complex128, engine=eng, keep_coupling=False, symmetry="xy", **kw)
        sim.add_input_layer(eps=ci["eps_in"])
        sim.set_incident_angle(ci["inc_ang"], ci["azi_ang"])
        for (d, eps, mu) in ci["layers"]:
            sim.add_layer(d, eps.to(eng.device), mu)
        sims.append(sim)
    a, b = sims
    assert a.symmetry_sector is False and b.symmetry_sector is False
    assert torch.equal(a.kz_norm[0], b.kz_norm[0]) and torch.equal(a.symmetry_residual[0], b.symmetry_residual[0])
    for pol in ("xx", "yy", "ps"):
        assert torch.equal(a.solve_S_parameters(ORDERS_PROBE, polarization=pol), b.solve_S_parameters(ORDERS_PROBE, polarization=pol))
