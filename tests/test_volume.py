"""Per-layer volume integrals and absorption by region (torcwa_amd/volume.py, trx_modal_overlap) on the GPU, complex128 unless stated.

1. Poynting identity of the truncated system (Laurent's rule): regions, masks=None and depth bins sum to absorption()["layers"], and every bin is
   the difference of power_flux at its ends.
2. volume_integral against a quadrature of the solver's own field_xy maps (grid sum in xy, exact by Parseval; Gauss-Legendre in z).
3. Batched against looped solves.  4. An order-list solver on an oblique lattice.  5. A complex64 solver.  6. Li's and the normal-vector rule
   (linearity in the weight only).  7. Autograd against central differences.  8. Errors.
"""
import numpy as np
import pytest
import torch

from tests.test_flux import _batched_problem, _disk, _solve_points, _stack

pytestmark = pytest.mark.gpu
C128 = torch.complex128

# Residual of the identity of test 1 evaluated on the CPU in complex128 (the same W, V, C and formulas, torch ops and the kernel-logic
# emulator): the largest |sum - absorption()["layers"]| and |bin - flux difference| over all sources and points, relative to the incident flux.
CPU_RESIDUAL = 3.0e-14


def _engine():
    import torcwa_amd
    return torcwa_amd.Engine()


def _identity_stack(eng, *, dtype=C128, rule="laurent", precision="high", B=3):
    """Lossless superstrate | lossy disk (12 + 0.8i) in a lossy film (2.1 + 0.05i) | lossy homogeneous layer | air, B wavelengths."""
    import torcwa_amd
    nx = ny = 36
    disk = _disk(nx, ny, 0.28).to(eng.device)
    eps = disk * (12.0 + 0.8j) + (1.0 - disk) * (2.1 + 0.05j)
    freq = torch.tensor([1 / 520., 1 / 560., 1 / 610.][:B], dtype=torch.float64, device=eng.device)
    sim = torcwa_amd.BatchedRCWA(freq, [3, 3], [300., 320.], dtype=dtype, engine=eng, fourier_rule=rule, precision=precision)
    sim.add_input_layer(eps=2.1)
    sim.set_incident_angle(0.3, 0.4)
    sim.add_layer(110., eps.to(dtype))
    sim.add_layer(70., 2.4 + 0.1j)
    sim.solve_global_smatrix()
    masks = torch.stack((disk, 1.0 - disk))
    return sim, masks


def _identity_residual(sim, masks, l, patterned):
    """Largest deviation (relative to the incident flux: everything is normalised) of the region / bin sums from the layer absorption."""
    lay = sim.absorption()["layers"][:, l]
    d = sim.thickness[l]
    edges = torch.linspace(0.0, 1.0, 17, dtype=torch.float64, device=d.device)[None, :] * d[:, None]          # [B, 17]
    bins = torch.stack((edges[:, :-1], edges[:, 1:]), dim=2)                                                   # [B, 16, 2]
    res = [(sim.absorption_by_region(l)[:, 0] - lay).abs().max()]
    prof = sim.absorption_by_region(l, z_range=bins)
    assert prof.shape == (sim.B, 16)
    res.append((prof.sum(dim=1) - lay).abs().max())
    phi = sim.power_flux(l, edges)
    sign = 1.0 if sim.source_direction == "forward" else -1.0
    res.append((prof - sign * (phi[:, :-1] - phi[:, 1:])).abs().max())
    if patterned:
        reg = sim.absorption_by_region(l, masks)
        assert reg.shape == (sim.B, 2, 1)
        res.append((reg.sum(dim=1)[:, 0] - lay).abs().max())
        regp = sim.absorption_by_region(l, masks, z_range=bins)
        assert regp.shape == (sim.B, 2, 16)
        res.append((regp.sum(dim=(1, 2)) - lay).abs().max())
        assert float(reg.min()) > 0.0                     # both materials are lossy: the sign is that of absorption()["layers"]
    return float(torch.stack(res).max())


SOURCES = [([1.0, 0.0], "forward"), ([0.0, 1.0], "forward"), ([1.0, 0.0], "backward"), ([0.0, 1.0], "backward")]


def test_poynting_identity():
    """Measured on the CPU (complex128, kernel-logic emulator): residual 2.8e-14 of the incident flux on the patterned layer, 6e-16 on the
    homogeneous one (CPU_RESIDUAL = 3e-14); asserted: 100 times that,
    and no more than 1e-9."""
    sim, masks = _identity_stack(_engine())
    tol = min(100 * CPU_RESIDUAL, 1e-9)
    for amp, direction in SOURCES:
        sim.source_planewave(amplitude=amp, direction=direction, notation="ps")
        for l, patterned in ((0, True), (1, False)):
            r = _identity_residual(sim, masks, l, patterned)
            print(f"identity residual {direction} {amp} layer {l}: {r:.2e}")
            assert r < tol, (amp, direction, l, r)


def test_against_field_maps():
    import torcwa_amd
    eng = _engine()
    ox, nx, ny, d = 3, 20, 24, 40.0
    assert nx > 4 * ox and ny > 4 * ox                     # the grid sum of w |F|^2 is then exact (Parseval)
    L = [300., 320.]
    disk = _disk(nx, ny, 0.3).to(eng.device)
    eps = disk * (12.0 + 0.8j) + (1.0 - disk) * (2.1 + 0.05j)
    sim = torcwa_amd.rcwa(1 / 560., [ox, ox], L, dtype=C128, engine=eng)
    sim.add_input_layer(eps=2.1)
    sim.set_incident_angle(0.3, 0.4)
    sim.add_layer(d, eps)
    sim.add_layer(60., 2.4 + 0.1j)
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1.0, 0.5j], direction="forward", notation="xy")
    # the solver's harmonics have the period L pi / pi_ref (the reference's pi): its own grid points are i / nx of that period
    from torcwa_amd.batched import PI_REF
    per = np.pi / PI_REF
    x = torch.arange(nx, dtype=torch.float64) * (L[0] * per / nx)
    y = torch.arange(ny, dtype=torch.float64) * (L[1] * per / ny)
    gen = torch.Generator().manual_seed(3)
    wr = (0.3 + torch.rand(nx, ny, generator=gen, dtype=torch.float64)).to(eng.device)
    wc = wr + 1j * (torch.rand(nx, ny, generator=gen, dtype=torch.float64) - 0.5).to(eng.device)

    def quad(nodes):
        t, wt = np.polynomial.legendre.leggauss(nodes)
        acc = {}
        for ti, wi in zip(t, wt):
            E, H = sim.field_xy(0, x, y, z_prop=float(0.5 * d * (ti + 1)))
            for f, F in (("E", E), ("H", H)):
                for c, Fc in zip("xyz", F):
                    acc[f + c] = acc.get(f + c, 0) + 0.5 * d * wi * Fc.abs() ** 2
        return acc

    q24, q48 = quad(24), quad(48)
    for w in (wr, wc):
        for f in "EH":
            for comp in ("x", "y", "z", "xyz"):
                ref24 = sum((w * q24[f + c]).mean() for c in comp)
                ref48 = sum((w * q48[f + c]).mean() for c in comp)
                assert abs(complex(ref48 - ref24)) < 1e-11 * abs(complex(ref24))          # the z quadrature has converged
                got = sim.volume_integral(0, f, comp, weight=w)
                assert got.shape == (1,) and got.is_complex() == w.is_complex()
                err = abs(complex(got[0]) - complex(ref24)) / abs(complex(ref24))
                print(f"{f}{comp} {'complex' if w.is_complex() else 'real'} weight: rel. err {err:.2e}")
                assert err < 1e-9, (f, comp, err)
    # w = 1 is the same integral without a convolution matrix; a stack adds the region axis
    one = sim.volume_integral(0, "E", "xyz")
    assert abs(float(one[0]) - float(sum(q24["E" + c].mean() for c in "xyz"))) < 1e-9 * float(one[0])
    st = sim.volume_integral(0, "E", "xyz", weight=torch.stack((wr, 2 * wr)), z_range=[[0.0, d], [0.0, d / 2]], normalize=True)
    assert st.shape == (2, 2) and abs(float(st[1, 0]) - 2 * float(st[0, 0])) < 1e-12 * abs(float(st[1, 0]))


def test_batched_equals_looped():
    eng = _engine()
    B = 4
    grids, freq, d0, inc = _batched_problem(eng)
    amp = torch.tensor([[1.0, 0.2j], [0.5, 1.0], [1.0, 0.0], [0.3j, 0.8]], dtype=C128)
    core = (grids.real > 5.0).to(torch.float64)                                            # [B, 24, 20]: a mask per point
    masks = torch.stack((core, 1.0 - core), dim=1)
    zfr = torch.tensor([[0.0, 0.3], [0.3, 1.0], [0.9, 0.2]], dtype=torch.float64)
    bs = _solve_points(eng, grids, freq, d0, inc, slice(0, B))
    bs.source_planewave(amplitude=amp, notation="ps")
    zr = zfr[None] * d0[:, None, None]
    ab = bs.absorption_by_region(0, masks, zr)
    vi = bs.volume_integral(0, "H", "xz", weight=grids.imag, z_range=zr)
    ah = bs.absorption_by_region(1, z_range=[[0.0, 20.0], [20.0, 45.0]])
    assert ab.shape == (B, 2, 3) and vi.shape == (B, 3) and ah.shape == (B, 2)
    for b in range(B):
        one = _solve_points(eng, grids, freq, d0, inc, slice(b, b + 1))
        one.source_planewave(amplitude=amp[b], notation="ps")
        ab1 = one.absorption_by_region(0, masks[b:b + 1], zr[b:b + 1])
        vi1 = one.volume_integral(0, "H", "xz", weight=grids[b:b + 1].imag, z_range=zr[b:b + 1])
        ah1 = one.absorption_by_region(1, z_range=[[0.0, 20.0], [20.0, 45.0]])
        for got, ref in ((ab[b], ab1[0]), (vi[b], vi1[0]), (ah[b], ah1[0])):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), b


def test_order_list_solver():
    """circular_orders on a hexagonal lattice (the general path: trx_convmat_orders for the weights)."""
    sim, _ = _stack(_engine(), inc=0.25, azi=0.4, hexagonal=True)
    disk = _disk(40, 44, 0.3).to(sim._device)
    tol = min(100 * CPU_RESIDUAL, 1e-9)
    for amp, direction in SOURCES[1:3]:
        sim.source_planewave(amplitude=amp, direction=direction, notation="ps")
        lay = sim.absorption()["layers"]
        for l in (0, 1, 2):
            assert abs(float(sim.absorption_by_region(l)[0] - lay[l])) < tol
        one = sim.absorption_by_region(0, torch.ones(1, 40, 44, dtype=torch.float64))
        assert one.shape == (1, 1) and abs(float(one[0, 0] - lay[0])) < tol
        reg = sim.absorption_by_region(0, torch.stack((disk, 1.0 - disk)))
        assert abs(float(reg.sum() - lay[0])) < tol


def test_complex64_solver():
    """The identity against the complex64 solver's own absorption(); tolerance: 16 times the deviation of that absorption() from the complex128
    one on the same stack, measured here."""
    eng = _engine()
    ref, _ = _identity_stack(eng)
    sim, masks = _identity_stack(eng, dtype=torch.complex64, precision="native")
    assert sim.E_eigvec[0].dtype == torch.complex64
    for amp, direction in SOURCES[:2]:
        ref.source_planewave(amplitude=amp, direction=direction, notation="ps")
        sim.source_planewave(amplitude=amp, direction=direction, notation="ps")
        dev = float((sim.absorption()["layers"].double() - ref.absorption()["layers"]).abs().max())
        for l, patterned in ((0, True), (1, False)):
            r = _identity_residual(sim, masks, l, patterned)
            print(f"complex64 {amp} layer {l}: identity residual {r:.2e}, deviation of absorption() from complex128 {dev:.2e}")
            assert r <= 16 * dev, (amp, l, r, dev)


@pytest.mark.parametrize("rule", ["li", "normal"])
def test_other_fourier_rules(rule):
    """No physical identity here (the split sums to the layer absorption only up to truncation): finite results, and linearity in the weight."""
    sim, masks = _identity_stack(_engine(), rule=rule, B=2)
    sim.source_planewave(amplitude=[1.0, 0.3], direction="forward", notation="xy")
    zr = [[0.0, 40.0], [40.0, 110.0]]
    tot = sim.absorption_by_region(0, z_range=zr)
    reg = sim.absorption_by_region(0, masks, z_range=zr)
    assert torch.isfinite(tot).all() and torch.isfinite(reg).all()
    assert float((reg.sum(dim=1) - tot).abs().max()) <= 1e-12 * float(tot.abs().max())


def test_gradient():
    """d(absorption in the first region) / d(Re eps of 5 grid entries): autograd against central differences, 1e-6 relative (the tolerance of
    the finite-difference and golden gradient checks of tests/test_grad.py and tests/test_flux.py)."""
    import torcwa_amd
    eng = _engine()
    dev = eng.device
    gen = torch.Generator().manual_seed(11)
    disk = _disk(16, 16, 0.3)
    re0 = (disk * 9.0 + 2.0 + 0.3 * torch.rand(16, 16, generator=gen, dtype=torch.float64)).to(dev)
    im0 = (disk * 0.7 + 0.05).to(dev)
    masks = torch.stack((disk, 1.0 - disk)).to(dev)

    def fom(re):
        sim = torcwa_amd.rcwa(1 / 540., [2, 2], [300., 300.], dtype=C128, engine=eng)
        sim.add_input_layer(eps=2.1)
        sim.set_incident_angle(0.15, 0.3)
        sim.add_layer(110., torch.complex(re, im0))
        sim.add_layer(40., 2.0 + 0.05j)
        sim.solve_global_smatrix()
        sim.source_planewave(amplitude=[1.0, 0.3], notation="xy")
        return sim.absorption_by_region(0, masks)[..., 0].sum()

    re = re0.clone().requires_grad_(True)
    f = fom(re)
    (g,) = torch.autograd.grad(f, re)
    with torch.no_grad():
        assert abs(float(f) - float(fom(re0))) < 1e-10                 # the differentiable path and the kernel path agree
        h = 1e-4
        for idx in torch.randperm(256, generator=gen)[:5].tolist():
            e = torch.zeros(256, dtype=torch.float64, device=dev)
            e[idx] = h
            e = e.reshape(16, 16)
            fd = float(fom(re0 + e) - fom(re0 - e)) / (2 * h)
            ga = float(g.reshape(-1)[idx])
            print(f"entry {idx}: autograd {ga:.9e} fd {fd:.9e}")
            assert abs(ga - fd) < 1e-6 * abs(fd), (idx, ga, fd)


def test_errors():
    import torcwa_amd
    from torcwa_amd._lib import TrxError
    eng = _engine()
    grid = (_disk(16, 16, 0.3) * (9.0 + 0.5j) + 2.0).to(eng.device)

    def build(**kw):
        sim = torcwa_amd.BatchedRCWA(1 / 500., [1, 1], [300., 300.], dtype=C128, engine=eng, **kw)
        sim.set_incident_angle(0.0, 0.0)
        sim.add_layer(50., grid)
        sim.add_layer(30., 2.0 + 0.1j)
        return sim

    sim = build(keep_coupling=False)
    sim.solve_global_smatrix()
    sim.source_planewave()
    with pytest.raises(TrxError, match="keep_coupling=True"):
        sim.volume_integral(0)
    sim = build()
    with pytest.raises(TrxError, match="solved stack"):
        sim.absorption_by_region(0)
    sim.solve_global_smatrix()
    with pytest.raises(TrxError, match="source"):
        sim.volume_integral(0)
    sim.source_planewave()
    for bad in (-1, 2, 0.5):
        with pytest.raises(ValueError):
            sim.volume_integral(bad)
        with pytest.raises(ValueError):
            sim.absorption_by_region(bad)
    with pytest.raises(ValueError, match="homogeneous"):
        sim.absorption_by_region(1, torch.ones(1, 16, 16))
    with pytest.raises(ValueError, match="masks must be"):
        sim.absorption_by_region(0, torch.ones(1, 16, 12))
    with pytest.raises(ValueError):
        sim.volume_integral(0, "D")
    with pytest.raises(ValueError):
        sim.volume_integral(0, "E", "")
    with pytest.raises(ValueError):
        sim.volume_integral(0, z_range=[0.0, 1.0, 2.0])
    assert sim.volume_integral(0).shape == (1, 1) and sim.absorption_by_region(0, torch.ones(2, 16, 16)).shape == (1, 2, 1)
