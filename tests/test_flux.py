"""Per-plane power flux and per-layer absorption (torcwa_amd/flux.py, trx_layer_flux / trx_matvec).

1. Golden values: the grid mean of Ex conj(Hy) - Ey conj(Hx) of the REFERENCE's field_xy maps (tests/golden/flux_*.npz, make_flux_golden.py: an
   exact quadrature of the truncated series), tolerances of test_fields.py for the same runs, relative to the incident flux.  The generator's
   grid spans L pi / pi_ref per axis, not L: the reference's own pi is off in the 10th digit, so that is the period of ITS harmonics, and only
   over it does the grid mean pass the 1e-12 doubling check (over L it is exact to about 3e-12).  The fields are the reference's throughout.
2. Identities against the project's own S-parameters and energy conservation, complex128, 1e-9.
3. Batched against single solves (1e-12), the sweep driver, autograd against central differences (1e-6), and the full-size complex64 gate (1e-5).
"""
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import GOLDEN, load_case
from tests.test_fields import FIELD_CASES, SRCS
from tests.test_pipeline import make_engine, run_case

C128 = torch.complex128


def _set_source(sim, kind, kw):
    (sim.source_planewave if kind == "pw" else sim.source_fourier)(**kw)


# ---- 1. golden values from the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,tag,emu_ok", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_flux_against_reference_field_maps(backend, name, tag, emu_ok):
    if backend == "emu" and not emu_ok and not os.environ.get("TRX_TEST_SLOW_EMU"):
        pytest.skip("too slow for the CPU suite (validated on the emulator once, runs on the GPU)")
    eng = make_engine(backend)
    g = load_case(name, tag)
    tol = 1e-8 if emu_ok else 1e-7
    f = np.load(os.path.join(GOLDEN, f"flux_{name}.npz"))
    sim = run_case(eng, g, "c128")
    nl = int(g["n_layers"])
    for sname, (kind, kw) in SRCS.items():
        _set_source(sim, kind, kw)
        inc = float(f[f"{sname}_incident"])
        assert abs(float(sim.incident_flux()) - inc) < 1e-12 * abs(inc)
        ref = f[f"{sname}_flux"]
        got = np.array([float(sim.power_flux(int(ln), float(zp), normalize=False)[0]) for ln, zp in zip(f["layer"], f["z_prop"])])
        err = np.abs(got - ref).max() / abs(inc)
        print(f"{name} {sname}: max |flux - golden| / incident = {err:.2e}")
        assert err < tol, (sname, got, ref)
        # several planes of one layer in one call equal the single-plane calls
        for ln in range(nl):
            sel = f["layer"] == ln
            many = sim.power_flux(ln, torch.from_numpy(f["z_prop"][sel]), normalize=False).cpu().numpy()
            assert np.abs(many - ref[sel]).max() / abs(inc) < tol
        # absorption(): per-layer drops and the far-side flux of the golden planes (z = 0 and z = d are the first and last plane of a layer)
        ab = sim.absorption()
        fwd = kw["direction"] in ("f", "forward")
        drops = []
        for ln in range(nl):
            r = ref[f["layer"] == ln]
            drops.append((r[0] - r[-1]) / inc if fwd else (r[-1] - r[0]) / inc)
        assert np.abs(ab["layers"].cpu().numpy() - np.array(drops)).max() < tol
        far = ref[f["layer"] == (nl if fwd else -1)][0] / inc
        assert abs(float(ab["T"]) - far) < tol
        assert abs(float(ab["A"]) - sum(drops)) < tol


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------
def _disk(nx, ny, r):
    x = (torch.arange(nx, dtype=torch.float64) + 0.5) / nx - 0.5
    y = (torch.arange(ny, dtype=torch.float64) + 0.5) / ny - 0.5
    return ((x[:, None] ** 2 + y[None, :] ** 2) < r * r).to(torch.float64)


def _rect(nx, ny, wx, wy):
    x = (torch.arange(nx, dtype=torch.float64) + 0.5) / nx - 0.5
    y = (torch.arange(ny, dtype=torch.float64) + 0.5) / ny - 0.5
    return ((x[:, None].abs() < wx / 2) & (y[None, :].abs() < wy / 2)).to(torch.float64)


def _stack(eng, *, inc=0.0, azi=0.0, lossy=True, rule="laurent", hexagonal=False, B=None, freq=1 / 560.):
    """Glass | patterned a-Si-like layer | homogeneous layer | patterned layer | air."""
    import torcwa_amd
    from torcwa_amd import lattice
    if hexagonal:
        a = 330.0
        L = [[a, 0.0], [a / 2, a * np.sqrt(3) / 2]]
        order = lattice.circular_orders(L, n_harmonics=19)
    else:
        L, order = [300., 340.], [3, 2]
    e_core = (12.0 + 0.6j) if lossy else 12.0
    e_slab = (2.4 + 0.05j) if lossy else 2.4
    pat = _disk(40, 44, 0.3) if rule == "normal" or hexagonal else _rect(40, 44, 0.55, 0.4)
    g0 = (pat * (e_core - 1.0) + 1.0).to(eng.device)
    g2 = (_rect(40, 44, 0.3, 0.7) * (e_core - 2.0) + 2.0).to(eng.device)
    kw = dict(dtype=C128, engine=eng, fourier_rule=rule)
    sim = torcwa_amd.rcwa(freq, order, L, **kw) if B is None else torcwa_amd.BatchedRCWA(freq, order, L, batch=B, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.add_output_layer(eps=1.0)
    sim.set_incident_angle(inc, azi)
    sim.add_layer(120., g0)
    sim.add_layer(60., e_slab)
    sim.add_layer(90., g2)
    sim.solve_global_smatrix()
    return sim, order


def _all_orders(sim):
    return sim.orders.cpu().tolist()


def _RT_from_sparams(sim, src_pol, direction):
    """R, T summed over all orders from S_parameters in the pp / sp / ps / ss basis for a p- or s-polarised unit plane wave."""
    orders = _all_orders(sim)
    out = []
    for port in ("reflection", "transmission"):
        tot = 0.0
        for pol in ("p" + src_pol, "s" + src_pol):
            v = sim.S_parameters(orders, direction=direction, port=port, polarization=pol)
            tot += float((v.abs() ** 2).sum())
        out.append(tot)
    return out


IDENTITY_CASES = [("normal_incidence", dict(inc=0.0, azi=0.0)), ("oblique_azimuth", dict(inc=0.35, azi=0.6)),
                  ("li", dict(inc=0.2, azi=0.3, rule="li")), ("normal_vector_disk", dict(inc=0.2, azi=0.3, rule="normal")),
                  ("hexagonal_circular", dict(inc=0.25, azi=0.4, hexagonal=True))]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,kw", IDENTITY_CASES, ids=[c[0] for c in IDENTITY_CASES])
def test_flux_identities(backend, name, kw):
    eng = make_engine(backend)
    sim, _ = _stack(eng, **kw)
    nl = sim.layer_N
    for pol, amp in (("p", [1.0, 0.0]), ("s", [0.0, 1.0])):
        sim.source_planewave(amplitude=amp, direction="forward", notation="ps")
        R, T = _RT_from_sparams(sim, pol, "forward")
        f_in = float(sim.power_flux(-1, 0.0)[0])
        f_out = float(sim.power_flux(nl, 0.0)[0])
        assert abs(f_in - (1 - R)) < 1e-9, (pol, f_in, 1 - R)
        assert abs(f_out - T) < 1e-9, (pol, f_out, T)
        # the flux does not depend on z in the lossless half-spaces
        assert abs(float(sim.power_flux(-1, -77.0)[0]) - f_in) < 1e-9
        assert abs(float(sim.power_flux(nl, 133.0)[0]) - f_out) < 1e-9
        # continuity across every interface
        prev = f_in
        for l in range(nl):
            d = float(sim.thickness[l])
            ph = sim.power_flux(l, torch.tensor([0.0, d], dtype=torch.float64))
            assert abs(float(ph[0]) - prev) < 1e-9, (pol, l)
            prev = float(ph[1])
        assert abs(prev - f_out) < 1e-9
        ab = sim.absorption()
        assert abs(float(ab["R"]) - R) < 1e-9 and abs(float(ab["T"]) - T) < 1e-9
        assert abs(float(ab["R"] + ab["T"] + ab["A"]) - 1.0) < 1e-9
        assert float(ab["layers"].min()) > 0.0            # every layer of this stack is lossy
        assert abs(float(ab["layers"].sum()) - float(ab["A"])) < 1e-14


@pytest.mark.parametrize("backend", BACKENDS)
def test_flux_lossless_stack(backend):
    """All-real eps: nothing is absorbed and the flux is the same on 17 interior planes of every layer."""
    eng = make_engine(backend)
    sim, _ = _stack(eng, inc=0.3, azi=0.2, lossy=False)
    sim.source_planewave(amplitude=[1.0, 0.4j], direction="forward", notation="xy")
    ab = sim.absorption()
    assert float(ab["layers"].abs().max()) < 1e-9
    assert abs(float(ab["R"] + ab["T"]) - 1.0) < 1e-9
    for l in range(sim.layer_N):
        z = torch.linspace(0.03, 0.97, 17, dtype=torch.float64) * float(sim.thickness[l])
        ph = sim.power_flux(l, z)
        assert ph.shape == (17,)
        assert float((ph - float(ab["T"])).abs().max()) < 1e-9


@pytest.mark.parametrize("backend", BACKENDS)
def test_flux_backward_source(backend):
    eng = make_engine(backend)
    sim, _ = _stack(eng, inc=0.2, azi=0.5)
    nl = sim.layer_N
    sim.source_planewave(amplitude=[0.0, 1.0], direction="backward", notation="ps")
    R, T = _RT_from_sparams(sim, "s", "backward")
    assert float(sim.incident_flux()) < 0.0                                   # counted along +z
    assert float(sim.power_flux(nl, 0.0, normalize=False)[0]) < 0.0
    assert abs(float(sim.power_flux(nl, 0.0)[0]) - (1 - R)) < 1e-9                   # normalised: positive along the source's direction
    assert abs(float(sim.power_flux(-1, 0.0)[0]) - T) < 1e-9
    ab = sim.absorption()
    assert abs(float(ab["R"]) - R) < 1e-9 and abs(float(ab["T"]) - T) < 1e-9
    assert abs(float(ab["R"] + ab["T"] + ab["A"]) - 1.0) < 1e-9
    assert float(ab["layers"].min()) > 0.0
    prev = float(sim.power_flux(-1, 0.0)[0])
    for l in range(nl):
        ph = sim.power_flux(l, torch.tensor([0.0, float(sim.thickness[l])], dtype=torch.float64))
        assert abs(float(ph[0]) - prev) < 1e-9
        prev = float(ph[1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_flux_needs_coupling_solve_and_source(backend):
    import torcwa_amd
    from torcwa_amd._lib import TrxError
    eng = make_engine(backend)
    sim = torcwa_amd.BatchedRCWA(1 / 500., [1, 1], [300., 300.], dtype=C128, engine=eng, keep_coupling=False)
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(50., 2.0 + 0.1j)
    sim.source_planewave()
    with pytest.raises(TrxError, match="keep_coupling=True.*solved stack"):
        sim.absorption()
    sim.solve_global_smatrix()
    with pytest.raises(TrxError, match="keep_coupling=True"):
        sim.power_flux(0)
    sim = torcwa_amd.BatchedRCWA(1 / 500., [1, 1], [300., 300.], dtype=C128, engine=eng)
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(50., 2.0 + 0.1j)
    with pytest.raises(TrxError, match="solved stack"):
        sim.power_flux(0)
    sim.solve_global_smatrix()
    with pytest.raises(TrxError, match="source"):
        sim.power_flux(0)
    with pytest.raises(TrxError, match="source"):
        sim.incident_flux()
    sim.source_planewave()
    with pytest.raises(ValueError):
        sim.power_flux(2)
    with pytest.raises(ValueError):
        sim.power_flux(0.5)
    assert sim.power_flux(np.int64(0)).shape == (1, 1) and sim.power_flux(torch.tensor(1)).shape == (1, 1)       # integer scalars of any kind
    one = torcwa_amd.rcwa(1 / 500., [1, 1], [300., 300.], dtype=C128, engine=eng)
    one.set_incident_angle(0.0, 0.0)
    one.add_layer(50., 2.0 + 0.1j)
    one.solve_global_smatrix()
    with pytest.raises(TrxError, match="source"):
        one.incident_flux()
    assert sim.power_flux(0, [0.0, 10.0, 50.0]).shape == (1, 3)


# ---- 4. batching ----------------------------------------------------------------------------------------------------------------------
def _batched_problem(eng, B=4):
    gen = torch.Generator().manual_seed(7)
    grid = _rect(24, 20, 0.5, 0.45)
    grids = (grid[None] * (11.0 + 0.7j - 1.0) + 1.0 + 0.3 * torch.rand(B, 24, 20, generator=gen, dtype=torch.float64)).to(eng.device)
    freq = torch.tensor([1 / 480., 1 / 520., 1 / 575., 1 / 640., 1 / 700.][:B], dtype=torch.float64)
    d0 = torch.tensor([90., 105., 120., 135., 150.][:B], dtype=torch.float64)
    inc = torch.tensor([0.0, 0.15, 0.3, 0.45, 0.2][:B], dtype=torch.float64)
    return grids, freq, d0, inc


def _solve_points(eng, grids, freq, d0, inc, sl):
    import torcwa_amd
    sim = torcwa_amd.BatchedRCWA(freq[sl], [2, 2], [300., 280.], dtype=C128, engine=eng)
    sim.add_input_layer(eps=2.1)
    sim.add_output_layer(eps=1.3)
    sim.set_incident_angle(inc[sl], 0.25)
    sim.add_layer(d0[sl], grids[sl])
    sim.add_layer(45., 2.2 + 0.08j)
    sim.solve_global_smatrix()
    return sim


@pytest.mark.parametrize("backend", BACKENDS)
def test_flux_batched_equals_single(backend):
    eng = make_engine(backend)
    grids, freq, d0, inc = _batched_problem(eng)
    B = 4
    amp = torch.tensor([[1.0, 0.2j], [0.5, 1.0], [1.0, 0.0], [0.3j, 0.8]], dtype=C128)           # a source per point
    zfrac = torch.tensor([0.0, 0.25, 1.0], dtype=torch.float64)
    bs = _solve_points(eng, grids, freq, d0, inc, slice(0, B))
    bs.source_planewave(amplitude=amp, notation="ps")
    ab = bs.absorption()
    pf = bs.power_flux(0, zfrac[None, :] * d0[:, None], normalize=False)
    assert pf.shape == (B, 3) and ab["layers"].shape == (B, 2) and ab["R"].shape == (B,)
    for b in range(B):
        one = _solve_points(eng, grids, freq, d0, inc, slice(b, b + 1))
        one.source_planewave(amplitude=amp[b], notation="ps")
        ab1 = one.absorption()
        for k in ("layers", "R", "T", "A"):
            assert float((ab[k][b] - ab1[k][0]).abs().max()) < 1e-12, (b, k)
        pf1 = one.power_flux(0, zfrac * d0[b], normalize=False)
        assert float((pf[b] - pf1[0]).abs().max()) < 1e-12 * float(one.incident_flux().abs())


# ---- 5. sweep driver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_sweep_absorption(backend):
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    B = 5
    grids, freq, d0, inc = _batched_problem(eng, B)
    freq, d0, inc = freq.to(eng.device), d0.to(eng.device), inc.to(eng.device)
    layers = [(d0, grids), (45., 2.2 + 0.08j)]
    kw = dict(eps_in=2.1, eps_out=1.3, inc_ang=inc, azi_ang=0.25, dtype=C128, engine=eng, chunk=2, orders=[(0, 0), (1, 0)], polarization="xx")
    plain = solve_stack_sweep(freq, layers, [2, 2], [300., 280.], **kw)
    assert torch.is_tensor(plain) and plain.shape == (B, 2)
    S, ab = solve_stack_sweep(freq, layers, [2, 2], [300., 280.], absorption=True, **kw)
    assert float((S - plain).abs().max()) < 1e-10
    ref = _solve_points(eng, grids, freq, d0, inc, slice(0, B))
    ref.source_planewave(amplitude=[1.0, 0.0], notation="xy")
    rab = ref.absorption()
    assert ab["layers"].shape == (B, 2)
    for k in ("layers", "R", "T", "A"):
        assert float((ab[k] - rab[k]).abs().max()) < 1e-12, k
    # another source
    _, ab2 = solve_stack_sweep(freq, layers, [2, 2], [300., 280.], absorption=True, source=dict(amplitude=[0.0, 1.0], notation="ps"), **kw)
    ref.source_planewave(amplitude=[0.0, 1.0], notation="ps")
    assert float((ab2["A"] - ref.absorption()["A"]).abs().max()) < 1e-12
    # a source amplitude per sweep point is cut into the chunks like the other per-point inputs; a wrong size is refused before any solve
    amp = torch.tensor([[1.0, 0.2j], [0.5, 1.0], [1.0, 0.0], [0.3j, 0.8], [0.2, 0.9]], dtype=C128)
    _, ab3 = solve_stack_sweep(freq, layers, [2, 2], [300., 280.], absorption=True, source=dict(amplitude=amp, notation="ps"), **kw)
    ref.source_planewave(amplitude=amp, notation="ps")
    assert float((ab3["layers"] - ref.absorption()["layers"]).abs().max()) < 1e-12
    with pytest.raises(ValueError, match="amplitude"):
        solve_stack_sweep(freq, layers, [2, 2], [300., 280.], absorption=True, source=dict(amplitude=amp[:3]), **kw)


# ---- 6. gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_absorption_gradient(backend):
    """d(absorption of the patterned layer) / d(thickness) and / d(one eps pixel): autograd against central differences."""
    import torcwa_amd
    eng = make_engine(backend)
    dev = eng.device
    gen = torch.Generator().manual_seed(5)
    base = (_rect(16, 16, 0.5, 0.4) * (10.0 + 0.8j - 1.0) + 1.0 + 0.2 * torch.rand(16, 16, generator=gen, dtype=torch.float64)).to(C128).to(dev)
    px = (6, 9)

    def fom(d, delta):
        eps = base + delta * torch.nn.functional.one_hot(torch.tensor(px[0] * 16 + px[1]), 256).reshape(16, 16).to(dev)
        sim = torcwa_amd.rcwa(1 / 540., [2, 2], [300., 300.], dtype=C128, engine=eng)
        sim.add_input_layer(eps=2.1)
        sim.set_incident_angle(0.15, 0.3)
        sim.add_layer(d, eps)
        sim.add_layer(40., 2.0 + 0.05j)
        sim.solve_global_smatrix()
        sim.source_planewave(amplitude=[1.0, 0.3], notation="xy")
        return sim.absorption()["layers"][0]

    d = torch.tensor(110.0, dtype=torch.float64, device=dev, requires_grad=True)
    delta = torch.tensor(0.0, dtype=torch.float64, device=dev, requires_grad=True)
    f = fom(d, delta)
    gd, ge = torch.autograd.grad(f, (d, delta))
    with torch.no_grad():
        hd, he = 1e-3, 1e-4
        fd_d = (fom(torch.tensor(110.0 + hd, dtype=torch.float64, device=dev), 0.0) - fom(torch.tensor(110.0 - hd, dtype=torch.float64, device=dev), 0.0)) / (2 * hd)
        fd_e = (fom(torch.tensor(110.0, dtype=torch.float64, device=dev), he) - fom(torch.tensor(110.0, dtype=torch.float64, device=dev), -he)) / (2 * he)
        plain = fom(torch.tensor(110.0, dtype=torch.float64, device=dev), 0.0)
    assert abs(float(f) - float(plain)) < 1e-10                    # the differentiable path and the kernel path agree
    print(f"dA/dd autograd {float(gd):.9e} fd {float(fd_d):.9e};  dA/deps autograd {float(ge):.9e} fd {float(fd_e):.9e}")
    assert abs(float(gd) - float(fd_d)) < 1e-6 * abs(float(fd_d))
    assert abs(float(ge) - float(fd_e)) < 1e-6 * abs(float(fd_e))


# ---- 7. full size ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flux_fullsize_c64():
    """Config 2's geometry at order [15,15] (n = 1922), the wavelengths of the config2_o15_* fixtures, complex64 I/O with precision="high"."""
    import glob
    import torcwa_amd
    eng = torcwa_amd.Engine()
    files = sorted(glob.glob(os.path.join(GOLDEN, "config2_o15_*_c128f32.npz")))
    assert len(files) >= 3
    gs = [np.load(p) for p in files[:3]]
    freq = torch.tensor([float(g["freq"]) for g in gs], dtype=torch.float64, device=eng.device)
    grids = torch.stack([torch.from_numpy(g["L0_eps_grid"]) for g in gs]).to(torch.complex64).to(eng.device)
    g0 = gs[0]
    sim = torcwa_amd.BatchedRCWA(freq, [int(v) for v in g0["order"]], [float(v) for v in g0["L"]], dtype=torch.complex64, precision="high", engine=eng)
    if bool(g0["has_in"]):
        sim.add_input_layer(eps=float(np.real(g0["eps_in"])))
    if bool(g0["has_out"]):
        sim.add_output_layer(eps=float(np.real(g0["eps_out"])))
    sim.set_incident_angle(float(g0["inc"]), float(g0["azi"]))
    sim.add_layer(float(g0["L0_thickness"]), grids)
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1.0, 0.0], notation="ps")
    ab = sim.absorption()
    orders = sim.orders.cpu().tolist()
    T = sum((sim.S_parameters(orders, polarization=pol).abs().to(torch.float64) ** 2).sum(dim=1) for pol in ("pp", "sp"))
    print("R + T + A - 1 =", (ab["R"] + ab["T"] + ab["A"] - 1).tolist(), " T - sum|t|^2 =", (ab["T"] - T).tolist(), " A =", ab["A"].tolist())
    assert float((ab["R"] + ab["T"] + ab["A"] - 1).abs().max()) < 1e-5
    assert float((ab["T"] - T).abs().max()) < 1e-5
