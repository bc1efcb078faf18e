"""Thickness sweeps that reuse a layer's modes, end to end: BatchedRCWA.add_layer(..., swept=True) + solve_S_parameters and the driver
torcwa_amd.solve_thickness_sweep against the reference run once per thickness (tests/golden/thickness_*.npz, make_thickness_golden.py).

Tolerances: those tests/test_pipeline.py applies to S-parameters of the same dtype -- max |difference| over max(largest |S| of the (direction,
port), 1e-3) below 1e-9 for complex128 and 1e-5 for complex64 I/O, against the reference's complex128 output on identical
(float32-representable) grids.  Bodies run on the emulator and on the MI355X (tests/backends.py).
"""
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import DIRPORT, GOLDEN, ORDERS_PROBE, case_inputs, load_case
from tests.test_li_factorisation import LAM, LX, LY, ORD, _stack, li_oracle  # noqa: F401  (li_oracle: a fixture)
from tests.test_pipeline import make_engine

POLS = ["xx", "yy", "xy"]
TOLS = [("c128", 1e-9), ("c64", 1e-5)]


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"thickness_{name}.npz"))
    g = {k: z[k] for k in z.files}
    ci = case_inputs(load_case(name, "c128f32"), "c128")
    if name == "example1_o3":
        (_, eps, mu), = ci["layers"]
        layers, swept, inc, azi = [(None, eps, mu)], 0, 0.0, 0.0
    else:
        (_, eps0, mu0), _, (_, eps2, mu2) = ci["layers"]
        o = g["outer_thicknesses"]
        layers, swept, inc, azi = [(float(o[0]), eps2, mu2), (None, eps0, mu0), (float(o[1]), eps2, mu2)], 1, ci["inc_ang"], ci["azi_ang"]
    return g, ci, layers, swept, inc, azi


def _cast(v, dtype, dev):
    if not torch.is_tensor(v):
        return v
    if dtype == "c64":
        v = v.to(torch.complex64 if v.is_complex() else torch.float32)
    return v.to(dev)


def _solver(eng, name, dtype, thicknesses=None, **kw):
    """BatchedRCWA over the fixture's frequencies with its swept layer; thicknesses default to the fixture's [T]."""
    import torcwa_amd
    g, ci, layers, swept, inc, azi = _fixture(name)
    cdt = torch.complex128 if dtype == "c128" else torch.complex64
    freq = torch.tensor(g["freqs"], dtype=torch.float64, device=eng.device)
    sim = torcwa_amd.BatchedRCWA(freq, ci["order"], ci["L"], dtype=cdt, engine=eng, keep_coupling=False, **kw)
    if "eps_in" in ci:
        sim.add_input_layer(eps=ci["eps_in"])
    if "eps_out" in ci:
        sim.add_output_layer(eps=ci["eps_out"])
    sim.set_incident_angle(inc, azi)
    d = torch.tensor(g["thicknesses"], dtype=torch.float64) if thicknesses is None else thicknesses
    for j, (th, eps, mu) in enumerate(layers):
        if j == swept:
            sim.add_layer(d, _cast(eps, dtype, eng.device), _cast(mu, dtype, eng.device), swept=True)
        else:
            sim.add_layer(th, _cast(eps, dtype, eng.device), _cast(mu, dtype, eng.device))
    return sim, g


def _check_all(sim, g, dtype, tol, tsel=None):
    ref = g["sparams"]                                           # [freq, T, dirport, pol, order]
    for a, (dr, pt) in enumerate(DIRPORT):
        scale = max(np.abs(ref[:, :, a]).max(), 1e-3)
        for b, pol in enumerate(POLS):
            got = sim.solve_S_parameters(g["orders"].tolist(), direction=dr, port=pt, polarization=pol).cpu().numpy()
            want = ref[:, :, a, b] if tsel is None else ref[:, tsel, a, b]
            assert got.shape == want.shape and got.dtype == (np.complex128 if dtype == "c128" else np.complex64)
            err = np.abs(got - want).max() / scale
            print(f"{dr} {pt} {pol}: {err:.3e}")
            assert err < tol, (dr, pt, pol, err)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", TOLS)
@pytest.mark.parametrize("name", ["example1_o3", "asym_o32"])
def test_swept_layer_against_reference(backend, name, dtype, tol):
    """(a) one patterned layer on a substrate, two wavelengths: block-diagonal left side, nothing on the right; (b) patterned eps and mu between
    two patterned layers at oblique incidence: dense on both sides.  Thicknesses 1 ... 2000 nm, every (direction, port), xx / yy / xy."""
    sim, g = _solver(make_engine(backend), name, dtype)
    _check_all(sim, g, dtype, tol)


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_layer_streaming_cascade_and_chunks(backend):
    """fold_layers=True (the sweep drivers' streaming cascade: the layers right of the swept one fold into a product of their own) with the
    thickness axis forced into chunks of 2 (two library calls for the four thicknesses)."""
    sim, g = _solver(make_engine(backend), "asym_o32", "c128", fold_layers=True)
    sim.thickness_chunk = 2
    _check_all(sim, g, "c128", 1e-9)
    assert sim._right_running is not None and sim.layer_S11[2] is None


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_layer_per_point_thicknesses(backend):
    """A [B, T] thickness tensor: point 0 scans (50, 2000, 1), point 1 scans (300, 1, 50) nm."""
    sel = np.array([[1, 3, 0], [2, 0, 1]])
    g0 = _fixture("example1_o3")[0]
    d = torch.tensor(g0["thicknesses"][sel], dtype=torch.float64)
    sim, g = _solver(make_engine(backend), "example1_o3", "c128", thicknesses=d)
    ref = g["sparams"]
    for a, (dr, pt) in enumerate(DIRPORT):
        scale = max(np.abs(ref[:, :, a]).max(), 1e-3)
        got = sim.solve_S_parameters(g["orders"].tolist(), direction=dr, port=pt, polarization="xx").cpu().numpy()
        want = np.stack([ref[p, sel[p], a, 0] for p in range(2)])
        assert np.abs(got - want).max() / scale < 1e-9, (dr, pt)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", TOLS)
def test_swept_layer_with_symmetry(backend, dtype, tol):
    """symmetry="xy" on fixture (a): the swept layer's modes come from the four folded eigenproblems."""
    sim, g = _solver(make_engine(backend), "example1_o3", dtype, symmetry="xy")
    assert sim.symmetry_residual[0] is not None
    _check_all(sim, g, dtype, tol)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-9), (torch.complex64, 1e-5)])
def test_swept_layer_li_against_oracle(backend, dtype, tol, li_oracle):  # noqa: F811
    """fourier_rule="li": the first of two patterned layers swept, against the oracle with Li's matrices run once per thickness."""
    import torcwa_amd
    eng = make_engine(backend)
    layers = _stack(1)
    inc, azi, thick = 0.35, 0.2, [0.02, 0.31, 1.9]
    orders, pols = [[0, 0], [1, 0], [0, -1]], ("xx", "xy", "yx", "yy")
    cast = (lambda t: t.to(torch.complex64 if t.is_complex() else torch.float32)) if dtype == torch.complex64 else (lambda t: t)
    sim = torcwa_amd.BatchedRCWA(torch.tensor([1 / LAM], dtype=torch.float64, device=eng.device), ORD, [LX, LY], dtype=dtype, engine=eng,
                                 keep_coupling=False, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc, azi)
    sim.add_layer(torch.tensor(thick, dtype=torch.float64), cast(layers[0][1]).to(eng.device), swept=True)
    sim.add_layer(layers[1][0], cast(layers[1][1]).to(eng.device))
    for dr, pt in DIRPORT:
        got = torch.stack([sim.solve_S_parameters(orders, direction=dr, port=pt, polarization=p).cpu()[0] for p in pols], dim=1)      # [T, pol, order]
        ref = []
        for d in thick:
            s, _, S, _ = li_oracle.solve_stack(1 / LAM, ORD, [LX, LY], [(d, layers[0][1]), layers[1]], eps_in=1.5, eps_out=2.25, inc_ang=inc, azi_ang=azi)
            ref.append(torch.stack([li_oracle.s_parameters(s, S, orders, direction=dr, port=pt, polarization=p) for p in pols]))
        ref = torch.stack(ref)
        assert float((got.to(torch.complex128) - ref).abs().max() / max(float(ref.abs().max()), 1e-3)) < tol, (dr, pt)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", TOLS)
def test_solve_thickness_sweep_driver(backend, dtype, tol):
    """torcwa_amd.solve_thickness_sweep on both fixtures: shared [T] thicknesses, points in chunks of 1, thicknesses in chunks of 3; and a
    homogeneous spacer as the swept layer (W = I materialised) against the same stack solved per thickness by solve_stack_sweep."""
    import torcwa_amd
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    cdt = torch.complex128 if dtype == "c128" else torch.complex64
    for name in ("example1_o3", "asym_o32"):
        g, ci, layers, swept, inc, azi = _fixture(name)
        freq = torch.tensor(g["freqs"], dtype=torch.float64, device=eng.device)
        lays = [tuple(_cast(v, dtype, eng.device) for v in lay) for lay in layers]
        kw = dict(eps_in=ci.get("eps_in"), eps_out=ci.get("eps_out"), inc_ang=inc, azi_ang=azi, dtype=cdt, engine=eng,
                  orders=[tuple(o) for o in g["orders"].tolist()])
        for a, b in ((0, 0), (1, 2), (2, 1), (3, 0)):
            dr, pt = DIRPORT[a]
            got = torcwa_amd.solve_thickness_sweep(freq, lays, ci["order"], ci["L"], layer=swept, thicknesses=g["thicknesses"], chunk=1,
                                                   thickness_chunk=3, direction=dr, port=pt, polarization=POLS[b], **kw).cpu().numpy()
            want = g["sparams"][:, :, a, b]
            assert got.shape == want.shape
            assert np.abs(got - want).max() / max(np.abs(g["sparams"][:, :, a]).max(), 1e-3) < tol, (name, dr, pt)
    # a homogeneous spacer between the two patterned layers of (b)
    g, ci, layers, swept, inc, azi = _fixture("asym_o32")
    freq = torch.tensor(g["freqs"], dtype=torch.float64, device=eng.device)
    lays = [tuple(_cast(v, dtype, eng.device) for v in layers[0]), (None, 2.2, 1.0), tuple(_cast(v, dtype, eng.device) for v in layers[2])]
    kw = dict(eps_in=ci.get("eps_in"), eps_out=ci.get("eps_out"), inc_ang=inc, azi_ang=azi, dtype=cdt, engine=eng, orders=((0, 0), (1, 0)))
    thick = [20.0, 400.0]
    got = torcwa_amd.solve_thickness_sweep(freq, lays, ci["order"], ci["L"], layer=1, thicknesses=thick, direction="forward", port="reflection", **kw)
    for t, d in enumerate(thick):
        want = solve_stack_sweep(freq, [lays[0], (d, 2.2, 1.0), lays[2]], ci["order"], ci["L"], direction="forward", port="reflection", **kw)
        assert float((got[:, t] - want).abs().max() / want.abs().max()) < (1e-10 if dtype == "c128" else 1e-5)


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_layer_refusals(backend):
    """Every documented ValueError, each naming its reason."""
    import torcwa_amd
    eng = make_engine(backend)
    g, ci, layers, swept, inc, azi = _fixture("example1_o3")
    eps = layers[0][1].to(eng.device)
    d = torch.tensor([10.0, 20.0], dtype=torch.float64)

    def new(**kw):
        sim = torcwa_amd.BatchedRCWA(torch.tensor([1 / 532.], dtype=torch.float64, device=eng.device), [1, 1], ci["L"], dtype=torch.complex128,
                                     engine=eng, **dict(dict(keep_coupling=False), **kw))
        sim.add_input_layer(eps=ci["eps_in"])
        sim.set_incident_angle(0.0, 0.0)
        return sim

    sim = new()
    sim.add_layer(d, eps, swept=True)
    with pytest.raises(ValueError, match="already swept"):
        sim.add_layer(d, eps, swept=True)
    with pytest.raises(ValueError, match="keep_coupling"):
        new(keep_coupling=True).add_layer(d, eps, swept=True)
    with pytest.raises(ValueError, match="differentiable"):
        new().add_layer(d, eps.clone().requires_grad_(True), swept=True)
    with pytest.raises(ValueError, match="differentiable"):
        new().add_layer(d.clone().requires_grad_(True), eps, swept=True)
    with pytest.raises(ValueError, match="differentiable"):          # a differentiable layer after the swept one
        sim.add_layer(30.0, eps.clone().requires_grad_(True))
    sim = new()
    sim.add_layer(30.0, eps.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="differentiable"):          # ... or before it
        sim.add_layer(d, eps, swept=True)
    with pytest.raises(ValueError, match=r"\[T\] or \[1, T\]"):
        new().add_layer(torch.ones(2, 2, dtype=torch.float64), eps, swept=True)
    sim = new()
    sim.add_layer(d, eps, swept=True)
    for call in (lambda: sim.solve_global_smatrix(), lambda: sim.power_flux(0), lambda: sim.incident_flux(), lambda: sim.absorption(),
                 lambda: sim.volume_integral(0), lambda: sim.absorption_by_region(0)):
        with pytest.raises(ValueError, match="solve_S_parameters"):
            call()
    assert sim.solve_S_parameters([[0, 0]]).shape == (1, 2, 1)
    with pytest.raises(ValueError, match="thicknesses"):
        torcwa_amd.solve_thickness_sweep(torch.tensor([1 / 532.], dtype=torch.float64, device=eng.device), [(None, eps)], [1, 1], ci["L"],
                                         thicknesses=torch.ones(3, 2), engine=eng)
    with pytest.raises(TypeError):
        torcwa_amd.solve_thickness_sweep(torch.tensor([1 / 532.], dtype=torch.float64, device=eng.device), [(None, eps)], [1, 1], ci["L"],
                                         thicknesses=[1.0], engine=eng, absorption=True)


def test_unswept_solver_is_unchanged_by_default():
    """swept defaults to False and is keyword-only: a positional fifth argument is still refused, and a plain solver has no swept state."""
    import inspect
    import torcwa_amd
    p = inspect.signature(torcwa_amd.BatchedRCWA.add_layer).parameters["swept"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "solve_thickness_sweep" in torcwa_amd.__all__


@pytest.mark.gpu
def test_thickness_sweep_at_bench_order():
    """The workload's order: config 2's grid at [15,15] (n = 1922), 4 wavelengths x 3 thicknesses, complex64 I/O; the point and the thickness
    of the fixture config2_o15_l532 (the reference in complex128 on the same float32-representable grid) at the 1e-5 of
    tests/test_fullsize_golden.py, forward transmission xx and yy; the other entries finite and different per thickness."""
    import torcwa_amd
    eng = make_engine("gpu")
    g = load_case("config2_o15_l532", "c128f32")
    grid = torch.from_numpy(g["L0_eps_grid"]).to(torch.complex64).to(eng.device)
    f0, d0 = float(g["freq"]), float(g["L0_thickness"])
    freq = torch.tensor([f0, 1 / 470., 1 / 590., 1 / 655.], dtype=torch.float64, device=eng.device)
    grids = grid[None].expand(4, -1, -1).contiguous()
    for pol, pi in (("xx", 0), ("yy", 3)):
        out = torcwa_amd.solve_thickness_sweep(freq, [(None, grids)], [15, 15], [300., 300.], thicknesses=[0.5 * d0, d0, 1.5 * d0], eps_in=1.46 ** 2,
                                               dtype=torch.complex64, engine=eng, orders=[tuple(o) for o in ORDERS_PROBE[:7]],
                                               polarization=pol).cpu().numpy()
        assert out.shape == (4, 3, 7) and out.dtype == np.complex64 and np.isfinite(out).all()
        ref = g["sparams"][0, pi, :7]
        err = np.abs(out[0, 1] - ref).max() / np.abs(ref).max()
        print(f"{pol}: {err:.3e}")
        assert err < 1e-5, (pol, err)
        assert np.abs(out[0, 0] - out[0, 1]).max() > 1e-3 and np.abs(out[0, 2] - out[0, 1]).max() > 1e-3
