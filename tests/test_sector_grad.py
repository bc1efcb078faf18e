"""symmetry_sector=True, sector_grad=True end to end (complex128): the adjoint of the sector cascade.

Gates: the project's 1e-9 on values and 1e-6 on gradients (tests/test_grad.py, tests/test_symmetry_grad.py).

1. Against the REFERENCE's autograd on the symgrad fixtures (tests/golden/make_symgrad_golden.py), objective |r_(1,0),xx|^2 + 1/2 |r_(0,1),yy|^2,
   which is not mirror-invariant: FoM, d/d thickness, and the RAW per-pixel gradient against the reference's mirror-averaged one
   (`grad_rho_avg`).  A sector solve folds P and Q themselves, so its raw gradient is mirror-symmetric (asymmetry below the gradient gate) and no
   averaging is left to the caller -- where symmetry_grad=True projects the eigen-part only.
2. Against the reference's shape_grad fixtures of tests/test_grad.py (the cylinder with its degenerate mode pairs, the rectangle at theta = 0),
   re-stated on BatchedRCWA: the drop-in class is refused in sector mode.
3. Against the unfolded differentiable path of this project (symmetry=None; pinned to the reference by tests/test_grad.py), its density gradient
   mirror-averaged: the other Fourier rules, one mirror with oblique incidence, a batch with per-point thicknesses, a differentiable layer
   behind a constant patterned one, a homogeneous layer whose thickness and permittivity require grad.  The unfolded raw gradient must differ
   from its own mirror average by more than 1e-3, so the comparison is not vacuous.
4. Graph shape: one eigenproblem of about n / 4 per patterned layer for an xx objective; two read-outs of one sector share its graph; a
   read-out that no solved sector reaches gives zero gradients, not None and not an error.
5. Validation: what sector_grad needs, what stays refused, and that a plain stack on a sector_grad solver is bit-identical.
"""
import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.test_pipeline import make_engine
from tests.test_symmetry_grad import _geo, _golden, _mirror_average

GPU, EMU = pytest.mark.gpu, pytest.mark.emu
SECTOR = dict(keep_coupling=False, symmetry_sector=True, sector_grad=True)


def _count_eig(eng):
    """The sizes of every eigensolver call of `eng` from now on (Eig's forward and the plain path both go through Engine.eig)."""
    sizes, inner = [], eng.eig

    def counted(A, *a, **kw):
        sizes.append(int(A.shape[-1]))
        return inner(A, *a, **kw)
    eng.eig = counted
    return sizes


def _run(eng, g, order, *, B=1, thick=300., inc=0., rho_first=None, hom_grad=False, backward=True, **kw):
    """The stack of tests/test_symmetry_grad.py::_run_stack through solve_S_parameters: FoM [B] = |r_(1,0),xx|^2 + 1/2 |r_(0,1),yy|^2 of
    (patterned layer of differentiable thickness, homogeneous layer) behind n = 1.46.  rho_first: a constant patterned layer in front;
    hom_grad: the thickness and the permittivity of the homogeneous layer require grad too.  Returns a dict of numpy arrays and the solver."""
    import torcwa_amd
    eps_si = complex(g["eps_si"])
    dev = eng.device
    rho = torch.from_numpy(g["rho"]).to(dev)[None].repeat(B, 1, 1).requires_grad_(True)
    d = torch.as_tensor(thick, dtype=torch.float64, device=dev).expand(B).clone().requires_grad_(True)
    dh = torch.full((B,), 80., dtype=torch.float64, device=dev, requires_grad=hom_grad)
    eh = torch.full((B,), 2.25, dtype=torch.float64, device=dev, requires_grad=hom_grad)
    sim = torcwa_amd.BatchedRCWA(1 / float(g["lam0"]), order, [700., 300.], batch=B, dtype=torch.complex128, engine=eng, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(inc, 0.)
    if rho_first is not None:
        sim.add_layer(120., rho_first * 2.6 + (1. - rho_first))
        assert not sim._diff
    sim.add_layer(d, rho * eps_si + (1. - rho))
    sim.add_layer(dh, eh)
    rxx = sim.solve_S_parameters([[1, 0]], direction="forward", port="reflection", polarization="xx", ref_order=[0, 0])
    ryy = sim.solve_S_parameters([[0, 1]], direction="forward", port="reflection", polarization="yy", ref_order=[0, 0])
    fom = (torch.abs(rxx) ** 2 + 0.5 * torch.abs(ryy) ** 2).reshape(B)
    out = dict(fom=fom.detach().cpu().numpy())
    if backward:
        fom.sum().backward()
        out.update(thick=d.grad.cpu().numpy(), rho=rho.grad.cpu().numpy())
        if hom_grad:
            out.update(hom_thick=dh.grad.cpu().numpy(), hom_eps=eh.grad.cpu().numpy())
    return out, sim


# ---- 1. the reference's autograd on the symgrad fixtures -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,name,B", [pytest.param("emu", "symgrad_o32", 1, marks=EMU), pytest.param("gpu", "symgrad_o32", 1, marks=GPU),
                                            pytest.param("gpu", "symgrad_o7", 2, marks=GPU)])
def test_nonsymmetric_objective_matches_reference(backend, name, B):
    """symgrad_o32 (order [3,2], n = 70) and symgrad_o7 (order [7,7], n = 450, two points): FoM to 1e-9; d/d thickness and the RAW per-pixel
    gradient to 1e-6 of the reference's d/d thickness and mirror-averaged per-pixel gradient; the raw gradient is mirror-symmetric to 1e-6."""
    eng = make_engine(backend)
    g = _golden(name)
    r, sim = _run(eng, g, [int(v) for v in g["order"]], B=B, symmetry="xy", **SECTOR)
    ref = g["grad_rho_avg"]
    assert sim.symmetry_residual == [None, None] and not hasattr(sim, "S")
    for b in range(B):
        e_f = abs(r["fom"][b] - float(g["fom"])) / float(g["fom"])
        e_t = abs(r["thick"][b] - float(g["grad_thick"])) / abs(float(g["grad_thick"]))
        e_r = np.abs(r["rho"][b] - ref).max() / np.abs(ref).max()
        asym = np.abs(r["rho"][b] - _mirror_average(r["rho"][b], "xy")).max() / np.abs(r["rho"][b]).max()
        print(f"{name} point {b}: FoM {e_f:.2e}, d/d thickness {e_t:.2e}, RAW d/d density against the averaged reference {e_r:.2e}, "
              f"asymmetry of the raw gradient {asym:.2e}")
        assert e_f < 1e-9 and e_t < 1e-6 and e_r < 1e-6 and asym < 1e-6


# ---- 2. the reference's shape_grad fixtures, on BatchedRCWA ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("tag,stable,bp", [("exact", False, 1e-10), ("bpe-10", True, 1e-10)])
def test_cylinder_radius_gradient_sector(backend, tag, stable, bp):
    """tests/test_grad.py::test_shape_derivative_of_a_cylinder in sector mode: d|txx|^2 / dR at R = 88 and 97."""
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("shape_grad")
    old = torcwa_amd.Eig.broadening_parameter
    torcwa_amd.Eig.broadening_parameter = bp
    sizes = _count_eig(eng)
    try:
        for R0 in (88, 97):
            del sizes[:]
            R = torch.tensor(float(R0), dtype=torch.float64, device=eng.device, requires_grad=True)
            sim = torcwa_amd.BatchedRCWA(1 / 473., [3, 3], [300., 300.], dtype=torch.complex128, engine=eng, stable_eig_grad=stable, symmetry="xy",
                                         **SECTOR)
            sim.add_input_layer(eps=1.46 ** 2)
            sim.set_incident_angle(0., 0.)
            m = _geo(eng).circle(R=R, Cx=150., Cy=150.)
            sim.add_layer(600., m * 2.0709 ** 2 + (1. - m))
            txx = sim.solve_S_parameters([[0, 0]], direction="forward", port="transmission", polarization="xx", ref_order=[0, 0])
            (torch.abs(txx) ** 2).sum().backward()
            ref_t = complex(np.asarray(g[f"circle_{tag}_R{R0}_txx"]).reshape(-1)[0])
            ref_g = float(np.asarray(g[f"circle_{tag}_R{R0}_grad"]).reshape(-1)[0])
            got_t = complex(txx.detach().reshape(-1)[0])
            print(f"R = {R0} {tag}: |txx - ref| / |ref| = {abs(got_t - ref_t) / abs(ref_t):.2e}, dR {float(R.grad):.9e} reference {ref_g:.9e}, "
                  f"eigen calls {sizes}")
            assert len(sizes) == 1 and abs(sizes[0] - 98 / 4) <= 1                     # one sector of n = 98
            assert abs(got_t - ref_t) / abs(ref_t) < 1e-9
            assert abs(float(R.grad) - ref_g) < 1e-6 * max(abs(ref_g), 1e-2), (float(R.grad), ref_g)
    finally:
        torcwa_amd.Eig.broadening_parameter = old


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sym", ["xy", "x", "y"])
def test_rectangle_gradient_sector(backend, sym):
    """tests/test_grad.py::test_shape_derivative_of_a_rectangle at theta = 0 in sector mode, with both mirrors, the x mirror alone and the y
    mirror alone: d |tyy - txx| / d(Wx, Wy) against the reference's autograd."""
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("shape_grad")
    eps_si = complex(g["eps_si"])
    W = torch.tensor([180., 100.], dtype=torch.float64, device=eng.device, requires_grad=True)
    theta = torch.tensor(0.0, dtype=torch.float64, device=eng.device)
    sim = torcwa_amd.BatchedRCWA(1 / 532., [3, 3], [300., 300.], dtype=torch.complex128, engine=eng, symmetry=sym, **SECTOR)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    m = _geo(eng).rectangle(Wx=W[0], Wy=W[1], Cx=150., Cy=150., theta=theta)
    sim.add_layer(250., m * eps_si + (1. - m))
    txx = sim.solve_S_parameters([[0, 0]], direction="forward", port="transmission", polarization="xx", ref_order=[0, 0])
    tyy = sim.solve_S_parameters([[0, 0]], direction="forward", port="transmission", polarization="yy", ref_order=[0, 0])
    torch.abs(tyy - txx).sum().backward()
    for v, name in ((txx, "_txx"), (tyy, "_tyy")):
        ref = complex(np.asarray(g["rect_th0" + name]).reshape(-1)[0])
        assert abs(complex(v.detach().reshape(-1)[0]) - ref) / abs(ref) < 1e-9
    refW = np.asarray(g["rect_th0_gradW"])
    err = np.abs(W.grad.cpu().numpy() - refW).max() / np.abs(refW).max()
    print(f"{sym}: dW error {err:.2e}")
    assert err < 1e-6


# ---- 3. the unfolded differentiable path ---------------------------------------------------------------------------------------------------------
CASES = {"li": dict(fourier_rule="li"), "normal": dict(fourier_rule="normal"), "oblique_y": dict(inc=0.2, symmetry="y"),
         "batch3": dict(B=3, thick=[280., 300., 320.]), "late_layer": dict(late=True), "homogeneous": dict(hom_grad=True)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(CASES))
def test_sector_matches_unfolded_path(backend, case):
    """The symgrad_o32 stack at order [3,2] through symmetry=None and through the differentiable sector solve: FoM to 1e-9, d/d thickness to
    1e-6, the sector path's RAW d/d density to 1e-6 of the mirror average of the unfolded path's."""
    eng = make_engine(backend)
    g = _golden("symgrad_o32")
    kw = dict(CASES[case])
    sym = kw.pop("symmetry", "xy")
    if kw.pop("late", False):
        kw["rho_first"] = torch.from_numpy(g["rho"] ** 2).to(eng.device)                # another density with both mirrors
    r0, _ = _run(eng, g, [3, 2], **kw)
    r1, sim = _run(eng, g, [3, 2], symmetry=sym, **SECTOR, **kw)
    a0 = _mirror_average(r0["rho"], sym)
    nB = len(r0["fom"])
    e_f = np.abs(r1["fom"] - r0["fom"]).max() / np.abs(r0["fom"]).max()
    e_t = (np.abs(r1["thick"] - r0["thick"]) / np.abs(r0["thick"])).max()
    e_r = max(np.abs(r1["rho"][b] - a0[b]).max() / np.abs(a0[b]).max() for b in range(nB))
    own = min(np.abs(r0["rho"][b] - a0[b]).max() / np.abs(r0["rho"][b]).max() for b in range(nB))
    print(f"{case}: FoM {e_f:.2e}, d/d thickness {e_t:.2e}, raw sector d/d density against the averaged unfolded one {e_r:.2e}; "
          f"the unfolded raw gradient is {own:.2e} away from its own average")
    assert e_f < 1e-9 and e_t < 1e-6 and e_r < 1e-6
    assert own > 1e-3                                                                  # not vacuous: averaging changes the unfolded gradient
    if case == "batch3":
        assert len({float(v) for v in r1["thick"]}) == 3                               # per-point thickness gradients
    if case == "homogeneous":
        for key in ("hom_thick", "hom_eps"):
            e = (np.abs(r1[key] - r0[key]) / np.abs(r0[key])).max()
            print(f"  homogeneous layer, d/d {key[4:]}: {e:.2e}")
            assert np.abs(r0[key]).min() > 0 and e < 1e-6


# ---- 4. graph shape ------------------------------------------------------------------------------------------------------------------------------
def _xx_solver(eng, g, rho, d, **kw):
    import torcwa_amd
    eps_si = complex(g["eps_si"])
    sim = torcwa_amd.BatchedRCWA(1 / float(g["lam0"]), [3, 2], [700., 300.], dtype=torch.complex128, engine=eng, symmetry="xy", **{**SECTOR, **kw})
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(120., (rho.detach() ** 2) * 2.6 + (1. - rho.detach() ** 2))                # constant patterned layer
    sim.add_layer(d, rho * eps_si + (1. - rho))
    sim.add_layer(80., 2.25)
    return sim


@pytest.mark.parametrize("backend", BACKENDS)
def test_graph_shape(backend):
    eng = make_engine(backend)
    g = _golden("symgrad_o32")
    rho = torch.from_numpy(g["rho"]).to(eng.device).requires_grad_(True)
    d = torch.tensor(300., dtype=torch.float64, device=eng.device, requires_grad=True)
    sizes = _count_eig(eng)
    sim = _xx_solver(eng, g, rho, d)
    assert sizes == [] and sim._diff                                                   # add_layer makes no eigen call in sector mode
    # two read-outs of the same sector, summed: one sector per patterned layer is solved, and one backward() serves both
    txx = sim.solve_S_parameters([[0, 0], [1, 0]], polarization="xx")
    rxx = sim.solve_S_parameters([[0, 0], [1, 0]], polarization="xx", port="reflection")
    assert len(sizes) == 2 and all(abs(s - 70 / 4) <= 1 for s in sizes), sizes          # the constant layer and the differentiable one
    assert sorted(k for _, k in sim._sector_layer_S) == sorted(3 * list(sim._sector_S)) and len(sim._sector_S) == 1
    ((torch.abs(txx) ** 2).sum() + (torch.abs(rxx) ** 2).sum()).backward()
    assert len(sizes) == 2
    g_both, d_both = rho.grad.clone(), d.grad.clone()
    assert float(g_both.abs().max()) > 0 and float(d_both.abs()) > 0
    # ... and equals the sum of the two objectives differentiated on solvers of their own
    rho.grad = d.grad = None
    for port in ("transmission", "reflection"):
        v = _xx_solver(eng, g, rho, d).solve_S_parameters([[0, 0], [1, 0]], polarization="xx", port=port)
        (torch.abs(v) ** 2).sum().backward()
    assert float((rho.grad - g_both).abs().max()) <= 1e-9 * float(g_both.abs().max())
    assert abs(float(d.grad - d_both)) <= 1e-9 * abs(float(d_both))
    # a read-out that the solved sector does not reach -- the y component of (0, 0) for an x-polarised source -- is exactly 0, and every
    # parameter gets a zero gradient from it: a tensor, not None, and no error
    rho.grad = d.grad = None
    sim = _xx_solver(eng, g, rho, d)
    tyx = sim.solve_S_parameters([[0, 0]], polarization="yx")
    assert tyx.requires_grad and float(tyx.detach().abs().max()) == 0.0
    (torch.abs(tyx) ** 2).sum().backward()
    assert rho.grad is not None and d.grad is not None
    assert float(rho.grad.abs().max()) == 0.0 and float(d.grad.abs()) == 0.0


# ---- 5. validation -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_sector_grad_validation(backend):
    import torcwa_amd
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    g = _golden("symgrad_o32")
    rho = torch.from_numpy(g["rho"]).to(eng.device)
    base = dict(dtype=torch.complex128, engine=eng, keep_coupling=False, symmetry="xy")
    new = lambda **kw: torcwa_amd.BatchedRCWA(1 / 400., [3, 2], [700., 300.], **{**base, **kw})
    with pytest.raises(ValueError, match="sector_grad=True needs symmetry_sector=True"):
        new(sector_grad=True)
    with pytest.raises(ValueError, match="sector_grad=True needs symmetry_sector=True"):
        new(sector_grad=True, symmetry_grad=True)
    # the default stays closed
    with pytest.raises(ValueError, match="differentiable"):
        new(symmetry_sector=True, symmetry_grad=True)
    sim = new(symmetry_sector=True)
    sim.set_incident_angle(0., 0.)
    with pytest.raises(ValueError, match="differentiable"):
        sim.add_layer(100., (rho * 11. + 1.).requires_grad_(True))
    # with sector_grad either value of symmetry_grad is accepted; swept=True, the global S-matrix and the drop-in class stay refused
    for sg in (False, True):
        sim = new(symmetry_sector=True, sector_grad=True, symmetry_grad=sg)
        sim.set_incident_angle(0., 0.)
        with pytest.raises(ValueError, match="swept=True"):
            sim.add_layer(torch.tensor([100., 200.]), (rho * 11. + 1.).requires_grad_(True), swept=True)
        sim.add_layer(100., (rho * 11. + 1.).requires_grad_(True))
        assert sim._diff and sim.symmetry_residual == [None]
        with pytest.raises(ValueError, match="solve_global_smatrix is not available with symmetry_sector=True"):
            sim.solve_global_smatrix()
    with pytest.raises(TypeError):
        torcwa_amd.rcwa(freq=1 / 400., order=[3, 2], L=[700., 300.], dtype=torch.complex128, engine=eng, symmetry="xy", sector_grad=True)
    # the sweep drivers take no sector_grad, and refuse a differentiable grid in sector mode as before
    freq = torch.full((1,), 1 / 400., dtype=torch.float64, device=eng.device)
    with pytest.raises(TypeError):
        solve_stack_sweep(freq, [(100., rho * 11. + 1.)], [3, 2], [700., 300.], engine=eng, symmetry="xy", symmetry_sector=True, sector_grad=True)
    with pytest.raises(ValueError, match="differentiable"):
        solve_stack_sweep(freq, [(100., (rho * 11. + 1.).requires_grad_(True))], [3, 2], [700., 300.], dtype=torch.complex128, engine=eng,
                          symmetry="xy", symmetry_sector=True)
    # a plain stack on a sector_grad solver: the calls and the bits of sector_grad=False
    vals = []
    for kw in ({}, {"sector_grad": True}):
        sim = new(symmetry_sector=True, **kw)
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0., 0.)
        sim.add_layer(100., rho * 11. + 1.)
        sim.add_layer(80., 2.25)
        assert not sim._diff
        vals.append([sim.solve_S_parameters([[0, 0], [1, 0], [0, -1]], polarization=pol, port=port)
                     for pol in ("xx", "yy", "ps") for port in ("transmission", "reflection")])
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(*vals))
