"""symmetry= end to end: the folded eigenproblem against the REFERENCE's own fixtures (tests/golden, never against the unfolded path of this
project), at the tolerances the existing golden tests apply to the same case and dtype (tests/test_pipeline.py, test_fields.py, test_flux.py,
test_fullsize_golden.py), and the validation errors.

example1 (centred 180 x 100 rectangle, normal incidence) has both mirrors; example2 (centred square, 15 degrees in the xz plane) only the y mirror,
because kx0 != 0; asym_o32 has none.  The reference's `rectangle` samples at (i + 1/2) h, so its grids mirror about c = n - 1; their measured
asymmetry is recorded in profiles/symmetry_timing.txt (rounding level).
"""
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import GOLDEN, ORDERS_PROBE, load_case
from tests.test_fields import SRCS
from tests.test_pipeline import check_against_golden, make_engine, run_case

GPU, EMU = pytest.mark.gpu, pytest.mark.emu
# (backend, fixture, symmetry, dtype, tolerance of tests/test_pipeline.py): the emulator runs complex128; the GPU both dtypes
GOLDEN_RUNS = [pytest.param(be, name, sym, dt, tol, marks=GPU if be == "gpu" else EMU)
               for be in ("emu", "gpu")
               for name, syms in (("example1_o3", ("xy", "x", "y")), ("example1_o5", ("xy", "x", "y")), ("example2_o4", ("y",)))
               for sym in (syms if (be == "gpu" or name != "example1_o5") else syms[:1])      # n = 242 on the emulator: one run
               for dt, tol in ((("c128", 1e-9),) if be == "emu" else (("c128", 1e-9), ("c64", 1e-5)))]


@pytest.mark.parametrize("backend,name,sym,dtype,tol", GOLDEN_RUNS)
def test_golden_with_symmetry(backend, name, sym, dtype, tol):
    """Every check of the golden parity test (full S at order 3, central S, layer spectra, P, Q, layer S-matrices, all S-parameters) with the
    eigenproblem folded."""
    eng = make_engine(backend)
    g = load_case(name, "c128" if dtype == "c128" else "c128f32")
    sim = run_case(eng, g, dtype, symmetry=sym)
    res = sim.symmetry_residual
    assert len(res) == int(g["n_layers"]) and all(r is not None for r in res)
    check_against_golden(sim, g, dtype, tol)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sym", ["x", "xy"])
def test_wavevector_outside_the_mirror_plane_raises(backend, sym):
    eng = make_engine(backend)
    g = load_case("example2_o4", "c128")
    with pytest.raises(ValueError, match="kx0_norm must be exactly 0"):
        run_case(eng, g, "c128", symmetry=sym)


@pytest.mark.gpu
def test_config2_fullsize_folded_sweep():
    """config 2 at its real size (order [15,15], n = 1922, blocks 480 / 481) through solve_single_layer_sweep and the mixed-precision eigensolver
    (4 points: the two groups of blocks are batches of 8), complex64 I/O at the 1e-5 of the full-size golden test."""
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = make_engine("gpu")
    g = load_case("config2_o15_l532", "c128f32")
    B = 4
    grids = torch.from_numpy(g["L0_eps_grid"]).to(torch.complex64).to(eng.device)[None].expand(B, -1, -1).contiguous()
    freq = torch.full((B,), float(g["freq"]), dtype=torch.float64, device=eng.device)
    for pol, pi in (("xx", 0), ("yy", 3)):
        out = solve_single_layer_sweep(freq, grids, float(g["L0_thickness"]), [15, 15], [float(v) for v in g["L"]], eps_in=float(np.real(g["eps_in"])),
                                       dtype=torch.complex64, precision="high", engine=eng, chunk=B, eig_route="mixed", symmetry="xy",
                                       orders=[tuple(o) for o in ORDERS_PROBE[:7]], polarization=pol).cpu().numpy()
        ref = g["sparams"][0, pi, :7]
        err = np.abs(out - ref[None]).max() / np.abs(ref).max()
        print(f"{pol}: max error / max |ref| = {err:.2e}")
        assert out.dtype == np.complex64 and err < 1e-5, pol


@pytest.mark.parametrize("backend", BACKENDS)
def test_sweep_driver_with_symmetry(backend):
    """solve_single_layer_sweep(symmetry="xy") on two copies of example1_o3 against the fixture's S-parameters."""
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    grids = torch.from_numpy(g["L0_eps_grid"]).to(eng.device)[None].expand(2, -1, -1).contiguous()
    freq = torch.full((2,), float(g["freq"]), dtype=torch.float64, device=eng.device)
    out = solve_single_layer_sweep(freq, grids, float(g["L0_thickness"]), [3, 3], [float(v) for v in g["L"]], eps_in=float(np.real(g["eps_in"])),
                                   dtype=torch.complex128, engine=eng, symmetry="xy", orders=[tuple(o) for o in ORDERS_PROBE[:7]],
                                   polarization="xx").cpu().numpy()
    ref = g["sparams"][0, 0, :7]
    assert np.abs(out - ref[None]).max() / np.abs(ref).max() < 1e-9


@pytest.mark.parametrize("backend", BACKENDS)
def test_fields_and_flux_with_symmetry(backend):
    """fields_example1_o3 and flux_example1_o3 (keep_coupling=True, the drop-in's default) with symmetry="xy": the unfolded W, the H modes and the
    coupling coefficients built from it serve the field maps and the power flux in the original basis.  Tolerances of test_fields.py / test_flux.py."""
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    tol = 1e-8
    sim = run_case(eng, g, "c128", symmetry="xy")
    assert sim._b.keep_coupling is True
    f = np.load(os.path.join(GOLDEN, "fields_example1_o3.npz"))
    fl = np.load(os.path.join(GOLDEN, "flux_example1_o3.npz"))
    x, y, z = (torch.from_numpy(f[k]) for k in ("x", "y", "z"))
    nl = int(g["n_layers"])
    for sname, (kind, kw) in SRCS.items():
        (sim.source_planewave if kind == "pw" else sim.source_fourier)(**kw)
        for plane, args in (("xz", (x, z, 133.0)), ("yz", (y, z, 41.0))):
            E, H = getattr(sim, "field_" + plane)(*args)
            got = np.stack([t.cpu().numpy() for t in E + H])
            ref = f[f"{sname}_{plane}"]
            assert np.abs(got - ref).max() / np.abs(ref).max() < tol, (sname, plane)
        for ln in (-1, 0, nl - 1, nl):
            key = f"{sname}_xy_L{ln}"
            if key in f:
                E, H = sim.field_xy(int(ln), x, y, float(f[key + "_zprop"]))
                got = np.stack([t.cpu().numpy() for t in E + H])
                assert np.abs(got - f[key]).max() / np.abs(f[key]).max() < tol, (sname, ln)
        inc = float(fl[f"{sname}_incident"])
        ref = fl[f"{sname}_flux"]
        got = np.array([float(sim.power_flux(int(ln), float(zp), normalize=False)[0]) for ln, zp in zip(fl["layer"], fl["z_prop"])])
        assert np.abs(got - ref).max() / abs(inc) < tol, sname
        ab = sim.absorption()
        fwd = kw["direction"] in ("f", "forward")
        r = ref[fl["layer"] == 0]
        drop = (r[0] - r[-1]) / inc if fwd else (r[-1] - r[0]) / inc
        assert abs(float(ab["layers"][0]) - drop) < tol


def _normal_incidence(eng, grid, **kw):
    import torcwa_amd
    sim = torcwa_amd.rcwa(freq=1 / 532., order=kw.pop("order", [3, 2]), L=kw.pop("L", [300., 300.]), dtype=torch.complex128, engine=eng, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(inc_ang=0., azi_ang=0.)
    return sim


@pytest.mark.parametrize("backend", BACKENDS)
def test_validation_errors(backend):
    import torcwa_amd
    eng = make_engine(backend)
    ga = load_case("asym_o32", "c128")
    asym = torch.from_numpy(ga["L0_eps_grid"]).to(eng.device)
    ge = load_case("example1_o3", "c128")
    symg = torch.from_numpy(ge["L0_eps_grid"]).to(eng.device)
    # a grid without the mirror (normal incidence, so the grid is what fails)
    sim = _normal_incidence(eng, asym, symmetry="x")
    with pytest.raises(ValueError, match="not mirror-symmetric along x"):
        sim.add_layer(thickness=100., eps=asym)
    # ... and with symmetry_tol wide open the same grid is accepted and the diagnostic reports what was discarded
    sim = _normal_incidence(eng, asym, symmetry="x", symmetry_tol=10.0)
    sim.add_layer(thickness=100., eps=asym)
    assert float(sim.symmetry_residual[0]) > 1e-6
    # an oblique lattice
    with pytest.raises(ValueError, match="rectangular lattice"):
        torcwa_amd.rcwa(freq=1 / 532., order=[[0, 0], [1, 0], [-1, 0]], L=[[300., 0.], [150., 260.]], dtype=torch.complex128, engine=eng, symmetry="x")
    # an order list that is not closed under the mirror (and one that is)
    with pytest.raises(ValueError, match="not closed under the x mirror"):
        torcwa_amd.rcwa(freq=1 / 532., order=[[0, 0], [1, 0], [0, 1], [0, -1]], L=[300., 300.], dtype=torch.complex128, engine=eng, symmetry="xy")
    torcwa_amd.rcwa(freq=1 / 532., order=[[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], L=[300., 300.], dtype=torch.complex128, engine=eng, symmetry="xy")
    # an unknown name
    with pytest.raises(ValueError, match="symmetry must be"):
        torcwa_amd.rcwa(freq=1 / 532., order=[1, 1], L=[300., 300.], engine=eng, symmetry="c4")
    # a caller-supplied normal field
    sim = _normal_incidence(eng, symg, symmetry="xy", fourier_rule="normal")
    nf = (torch.zeros_like(symg.real), torch.ones_like(symg.real))
    with pytest.raises(ValueError, match="normal_field"):
        sim.add_layer(thickness=100., eps=symg, normal_field=nf)
    # a differentiable stack
    sim = _normal_incidence(eng, symg, symmetry="xy")
    with pytest.raises(ValueError, match="differentiable"):
        sim.add_layer(thickness=100., eps=symg.clone().requires_grad_(True))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("rule", ["li", "normal"])
def test_other_fourier_rules_fold_too(backend, rule):
    """The fold acts on A whatever built it: Li's rule and the normal-vector rule (field derived from the grid) keep both mirrors of a centred
    rectangle, so the discarded part stays at rounding level (the bound of test_symmetry_residual_of_the_fixtures)."""
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    grid = torch.from_numpy(g["L0_eps_grid"]).to(eng.device)
    sim = _normal_incidence(eng, grid, order=[3, 3], symmetry="xy", fourier_rule=rule)
    sim.add_layer(thickness=100., eps=grid)
    n = 2 * sim.order_N
    assert float(sim.symmetry_residual[0]) <= 16 * n * max(2.0 ** -53, _grid_asymmetry(g["L0_eps_grid"]))


def _grid_asymmetry(grid):
    """max |g - mirror(g)| / max |g| about the half-cell centre, the larger of the two axes (a property of the input)."""
    a = np.abs(grid).max()
    return float(max(np.abs(grid - grid[::-1, :]).max(), np.abs(grid - grid[:, ::-1]).max()) / a)


@pytest.mark.parametrize("backend,name", [pytest.param("emu", "example1_o3", marks=EMU), pytest.param("gpu", "example1_o3", marks=GPU),
                                          pytest.param("gpu", "example1_o5", marks=GPU)])
def test_symmetry_residual_of_the_fixtures(backend, name):
    """sim.symmetry_residual of the example1 layer.  Bound: 16 n max(eps, delta), delta = the grid's own asymmetry measured here from the fixture
    (rounding level for the reference's `rectangle`): an entry of a convolution matrix moves by at most delta max |g| when the grid is
    symmetrised, the rows of the products that make A sum n such entries, and 16 n eps is the block tests' rounding allowance."""
    eng = make_engine(backend)
    g = load_case(name, "c128")
    delta = _grid_asymmetry(g["L0_eps_grid"])
    sim = run_case(eng, g, "c128", symmetry="xy")
    n = 2 * sim.order_N
    res = float(sim.symmetry_residual[0])
    print(f"{name}: grid asymmetry {delta:.2e}, symmetry_residual {res:.2e}, bound {16 * n * max(2.0 ** -53, delta):.2e}")
    assert delta < 1e-6 and res <= 16 * n * max(2.0 ** -53, delta)


@pytest.mark.parametrize("backend", BACKENDS)
def test_default_path_is_bit_identical(backend):
    """symmetry=None is today's path: lam, W and the S-parameters of example1_o3 equal a run without the keyword bit for bit."""
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    a, b = run_case(eng, g, "c128"), run_case(eng, g, "c128", symmetry=None)
    assert b.symmetry_residual == [None]
    assert torch.equal(a.kz_norm[0], b.kz_norm[0]) and torch.equal(a.E_eigvec[0], b.E_eigvec[0])
    for pol in ("xx", "yy", "ps"):
        assert torch.equal(a.S_parameters(ORDERS_PROBE, polarization=pol), b.S_parameters(ORDERS_PROBE, polarization=pol))
