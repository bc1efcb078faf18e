"""The normal-vector rule on vector-shape layers end to end (BatchedRCWA(fourier_rule="normal").add_layer(eps=ShapeLayer(...))), complex128,
on both backends, with the project's 1e-9 gate on values.

The oracle never sees the kernels' tensor: [eps], [1/eps] come from the float64 closed forms of tests/shape_reference.py, the field from the
float64 numpy restatement of tests/shape_nv_reference.py, the tensor from tensor_plain, and it enters Q of oracle.rcwa_oracle as in
profiles/normal_vector_study.py (pq_patterned patched around test_shapes.oracle_S).

Convergence (gpu only; n = 450 and 1458 are too slow on the emulator): the eps = 12 disk of profiles/normal_vector.txt at [7,7] against the
same method at [13,13]; the error must be at least 4 x below closed-form Laurent's at [7,7] (the CPU oracle gives 13 x; 4 is the margin
test_shapes.py uses for a non-monotone convergence ratio).  Measured ratio: MEASURED_RATIO below.
"""
import numpy as np
import pytest
import torch

from oracle import rcwa_oracle as orc
from tests import shape_nv_reference as nvr
from tests import shape_reference as sr
from tests.backends import BACKENDS
from tests.test_shapes import DT, EPS_GLASS, EPS_SI, GATE, OBLIQUE, ORDER, PROBE, RECT, close, engine, layer_of, oracle_S, solver

MEASURED_RATIO = {"gpu": 13.1}          # err_laurent[7,7] / err_nv[7,7] of the eps = 12 disk: 8.009e-02 / 6.115e-03 (from a run with -s)
GRID = (40, 36)                          # field samples of the small end-to-end cases (> 4 x the order [2,2])


def flat_b(layer, lattice, b, B):
    """[(kind, par)], val, rval of a ShapeLayer at sweep point b, as the references take them."""
    p = layer.pack(np.array(lattice), B, "cpu")
    voff = p.voff.tolist()
    shapes = [(int(k), p.par[b, voff[i]:voff[i + 1]].tolist()) for i, k in enumerate(p.kind.tolist())]
    return shapes, p.val[b].numpy(), layer.reciprocal_values(B, "cpu")[b].numpy()


def oracle_S_nv(lattice, shapes, val, rval, thickness):
    """test_shapes.oracle_S with the test's own tensor in Q (normal_vector_study.solve's patch)."""
    mn = np.array([(m, n) for m in range(-ORDER[0], ORDER[0] + 1) for n in range(-ORDER[1], ORDER[1] + 1)])
    recip, area = sr.recip_of(*lattice)
    nn = nvr.field(shapes, lattice[0], lattice[1], *GRID, dtype=np.float64)["nn"]
    Exx, Exy, Eyy = (torch.from_numpy(np.ascontiguousarray(t)) for t in nvr.tensor_plain(shapes, val, rval, recip, area, mn, *ORDER, nn))
    pq0 = orc.pq_patterned

    def pq(E, M, kx, ky):
        P, Q = pq0(E, M, kx, ky)
        N = E.shape[-1]
        Q[:N, :N] -= Exy
        Q[:N, N:] += E - Eyy
        Q[N:, :N] += Exx - E
        Q[N:, N:] += Exy
        return P, Q
    orc.pq_patterned = pq
    try:
        return oracle_S(lattice, shapes, val, thickness)
    finally:
        orc.pq_patterned = pq0


def nv_solver(eng, lattice, order=ORDER, **kw):
    kw.setdefault("shape_nv_grid", GRID)
    return solver(eng, lattice, order, fourier_rule="normal", **kw)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["rect", "oblique"])
def test_against_the_oracle_with_the_tests_own_tensor(backend, name):
    """B = 2 with a per-point radius and a host= core (layer_of), on both lattice paths."""
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    lattice = RECT if name == "rect" else OBLIQUE
    layer = layer_of(S, lattice, scale=torch.tensor([1.0, 1.1], dtype=torch.float64))
    freq = torch.full((2,), 1 / 600., dtype=torch.float64)
    sim = nv_solver(engine(backend), [700., 660.] if name == "rect" else lattice, ORDER if name == "rect" else rect_orders(*ORDER).tolist(),
                    freq=freq)
    sim.add_layer(120., eps=layer)
    sim.solve_global_smatrix()
    assert sim.eps_conv_xy[0] is not None and sim.eps_conv_xx[0].shape == sim.eps_conv[0].shape          # keep_coupling stores the tensor
    for b in range(2):
        shapes, val, rval = flat_b(layer, lattice, b, 2)
        s, Sg = oracle_S_nv(lattice, shapes, val, rval, 120.)
        for pol in ("xx", "yx", "xy", "yy"):
            for port in ("transmission", "reflection"):
                got = sim.S_parameters(PROBE, polarization=pol, port=port)[b]
                close(got, orc.s_parameters(s, Sg, PROBE, polarization=pol, port=port), f"{name} b{b} {pol} {port}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_rule_changes_the_answer(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    out = []
    for rule in ("laurent", "normal"):
        sim = solver(eng, [700., 660.], fourier_rule=rule, keep_coupling=False, shape_nv_grid=GRID)
        sim.add_layer(120., eps=layer_of(S))
        out.append(sim.solve_S_parameters(PROBE, polarization="xx").cpu())
    assert float((out[0] - out[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("backend", BACKENDS)
def test_lossless_disk_conserves_energy(backend):
    """R + T = 1 at normal incidence: the tensor is Hermitian (the symmetrised products)."""
    import torcwa_amd.shapes as S
    sim = nv_solver(engine(backend), [700., 660.])
    sim.add_layer(120., eps=S.ShapeLayer(1.0, [S.circle(213., 341., 317., 12.0)]))
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1., 0.5j], direction="forward")
    ab = sim.absorption()
    assert float(ab["A"].abs().max()) <= GATE and float((ab["R"] + ab["T"] - 1).abs().max()) <= GATE


def _S(sim):
    return torch.stack([sim.solve_S_parameters(PROBE, polarization=pol, port=port) for pol in ("xx", "yx") for port in ("t", "r")]).cpu()


@pytest.mark.parametrize("backend", BACKENDS)
def test_supplied_field_equal_to_the_derived_one(backend):
    """The derived products handed back as normal_field= give the same S bit for bit (one tensor = the products, as normal_products returns
    them); as (Nx, Ny) = (sqrt(Nx^2), sign(Nx Ny) sqrt(Ny^2)) the products are re-formed with one rounding each, so S agrees to the gate."""
    import torcwa_amd.shapes as S
    eng = engine(backend)
    layer = layer_of(S, OBLIQUE)
    derived = nv_solver(eng, OBLIQUE, keep_coupling=False)
    derived.add_layer(120., eps=layer)
    want = _S(derived)
    nn = S.normal_products(layer, OBLIQUE, *GRID, engine=eng)
    assert tuple(nn.shape) == (1, 3) + GRID and (nn != 0).any()
    for field in (nn, nn[0]):
        sim = nv_solver(eng, OBLIQUE, keep_coupling=False, shape_nv_grid=64)        # the supplied field's own grid decides, not this one
        sim.add_layer(120., eps=layer, normal_field=field)
        assert torch.equal(_S(sim), want)
    Nx, Ny = nn[0, 0].sqrt(), torch.where(nn[0, 1] < 0, -1.0, 1.0) * nn[0, 2].sqrt()
    sim = nv_solver(eng, OBLIQUE, keep_coupling=False)
    sim.add_layer(120., eps=layer, normal_field=(Nx, Ny))
    close(_S(sim), want, "(Nx, Ny)")


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_and_the_drop_in_agree_with_a_plain_solve(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    from torcwa_amd.sweep import solve_stack_sweep
    eng = engine(backend)
    R = torch.tensor([150., 170.], dtype=torch.float64)
    freq = torch.tensor([1 / 600., 1 / 620.], dtype=torch.float64, device=eng.device)
    mk = lambda r: S.ShapeLayer(1.0, [S.ellipse(r, 90., 300., 250., EPS_SI, theta=0.3), S.rectangle(100., 60., 560., 500., 3.0)])
    d = torch.tensor([100., 120.], dtype=torch.float64, device=eng.device)
    plain = []
    for t in d:
        sim = nv_solver(eng, [700., 660.], freq=freq, keep_coupling=False)
        sim.add_layer(float(t), eps=mk(R))
        plain.append(sim.solve_S_parameters(PROBE, polarization="xx"))
    sim = nv_solver(eng, [700., 660.], freq=freq, keep_coupling=False)
    sim.add_layer(d, eps=mk(R), swept=True)
    close(sim.solve_S_parameters(PROBE, polarization="xx"), torch.stack(plain, dim=1), "swept=True")
    kw = dict(eps_in=EPS_GLASS, eps_out=1., dtype=DT, engine=eng, chunk=1, orders=[tuple(o) for o in PROBE], fourier_rule="normal",
              shape_nv_grid=GRID)
    close(solve_stack_sweep(freq, [(120., mk(R))], ORDER, [700., 660.], **kw), plain[1], "solve_stack_sweep")
    drop = torcwa_amd.rcwa(freq=1 / 600., order=ORDER, L=[700., 660.], dtype=DT, engine=eng, fourier_rule="normal", shape_nv_grid=GRID)
    drop.add_input_layer(eps=EPS_GLASS)
    drop.add_output_layer(eps=1.)
    drop.set_incident_angle(inc_ang=0., azi_ang=0.)
    drop.add_layer(thickness=120., eps=mk(R[0]))
    drop.solve_global_smatrix()
    close(drop.S_parameters(PROBE, polarization="xx"), plain[1][0], "rcwa drop-in")


def _disk_errors(eng, order):
    """|S|^2 of the 8 zeroth-order pairs of the eps = 12 disk of profiles/normal_vector.txt (cell 0.5 x 0.5, lambda 1, depth 0.3, air over
    2.25, inc 0.3, azi 0.4, r 0.18) under both rules."""
    import torcwa_amd
    import torcwa_amd.shapes as S
    from torcwa_amd.batched import SHAPE_NV_GRID_DEFAULT
    out = {}
    for rule in ("laurent", "normal"):
        sim = torcwa_amd.BatchedRCWA(torch.ones(1, dtype=torch.float64, device=eng.device), order, [0.5, 0.5], dtype=DT, engine=eng,
                                     fourier_rule=rule, keep_coupling=False, shape_nv_grid=SHAPE_NV_GRID_DEFAULT)
        sim.add_input_layer(eps=1.0)
        sim.add_output_layer(eps=2.25)
        sim.set_incident_angle(0.3, 0.4)
        sim.add_layer(0.3, eps=S.ShapeLayer(1.0, [S.circle(0.18, 0.25, 0.25, 12.0)]))
        out[rule] = torch.stack([sim.solve_S_parameters([[0, 0]], polarization=pol, port=port)[0, 0].abs() ** 2
                                 for port in ("transmission", "reflection") for pol in ("xx", "xy", "yx", "yy")]).cpu()
    return out


@pytest.mark.gpu
def test_convergence_beats_laurent_by_4():
    eng = engine("gpu")
    ref = _disk_errors(eng, [13, 13])["normal"]
    at7 = _disk_errors(eng, [7, 7])
    err = {rule: float((at7[rule] - ref).abs().max()) for rule in at7}
    print(f"disk eps 12 at [7,7] against NV [13,13]: Laurent {err['laurent']:.3e}, NV {err['normal']:.3e}; ratio {err['laurent'] / err['normal']:.1f}")
    assert err["laurent"] >= 4 * err["normal"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    layer = layer_of(S)
    with pytest.raises(ValueError, match="li"):
        solver(eng, [700., 660.], fourier_rule="li").add_layer(120., eps=layer)
    with pytest.raises(ValueError, match="symmetry"):
        solver(eng, [700., 660.], fourier_rule="normal", symmetry="x").add_layer(120., eps=layer)
    with pytest.raises(ValueError, match="mu"):
        nv_solver(eng, [700., 660.]).add_layer(120., eps=2.0, mu=layer)
    with pytest.raises(ValueError, match="normal_field"):
        nv_solver(eng, [700., 660.]).add_layer(120., eps=layer, normal_field=(torch.zeros(40, 36), torch.zeros(36, 40)))
    with pytest.raises(ValueError, match="normal_field"):
        nv_solver(eng, [700., 660.]).add_layer(120., eps=layer, normal_field=(torch.zeros(3, 40, 36), torch.zeros(3, 40, 36)))     # B is 1
    with pytest.raises(ValueError, match="too small"):
        nv_solver(eng, [700., 660.]).add_layer(120., eps=layer, normal_field=(torch.zeros(4, 36), torch.zeros(4, 36)))
    with pytest.raises(ValueError, match="shape_nv_grid"):                 # opt-in: no field grid and no supplied field
        solver(eng, [700., 660.], fourier_rule="normal").add_layer(120., eps=layer)
    with pytest.raises(ValueError, match="shape_nv_grid"):
        nv_solver(eng, [700., 660.], shape_nv_grid=8).add_layer(120., eps=layer)                    # 8 <= 4 x 2
    with pytest.raises(ValueError, match="shape_nv_grid"):
        nv_solver(eng, [700., 660.], shape_nv_grid=(64, 4096))
    with pytest.raises(ValueError, match='fourier_rule="normal"'):
        solver(eng, [700., 660.]).add_layer(120., eps=layer, normal_field=(torch.zeros(40, 36), torch.zeros(40, 36)))
