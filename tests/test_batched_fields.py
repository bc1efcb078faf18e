"""BatchedRCWA.field_xy / field_xz / field_yz (torcwa_amd/batched_fields.py; trx_layer_field, trx_field_synth) end to end.

1. The reference's own field maps (tests/golden/fields_*.npz) at sweep point 0 of a B = 3 solver, and a single `rcwa` run at the frequency of
   points 1 and 2, at the gate of test_fields.py for the same runs: 1e-8 (1e-7 for the six-layer stack) relative to the largest value.
2. Independent of every field-map code path: the grid mean of Re(Ex conj(Hy) - Ey conj(Hx)) over one cell equals power_flux (Parseval), 1e-9 of
   the incident flux, the gate of test_flux.py for flux identities.  The uniform grid of 4 o + 1 samples per axis integrates every product of
   two harmonics of |order| <= o exactly; it spans L pi / PI_REF, the period of the solver's own harmonics (omega = 2 PI_REF f, test_flux.py).
3. Per-point sources and z_prop, complex64, an oblique lattice with a circular order set, symmetry=, autograd, refusals.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import GOLDEN, case_inputs, load_case
from tests.test_fields import FIELD_CASES, SRCS
from tests.test_flux import _batched_problem, _rect, _set_source, _solve_points, _stack
from tests.test_pipeline import make_engine

C128 = torch.complex128
SCALE = (1.0, 0.97, 1.04)          # sweep point 0 is the fixture's frequency


def _build(eng, g, freq, *, batched, dtype=C128, **kw):
    """The stack of golden case g at `freq` (a [B] tensor: BatchedRCWA; a float: the drop-in rcwa), solved."""
    import torcwa_amd
    ci = case_inputs(g, "c128")
    cls = torcwa_amd.BatchedRCWA if batched else torcwa_amd.rcwa
    sim = cls(freq, ci["order"], ci["L"], dtype=dtype, engine=eng, **kw)
    if "eps_in" in ci:
        sim.add_input_layer(eps=ci["eps_in"])
    if "eps_out" in ci:
        sim.add_output_layer(eps=ci["eps_out"])
    sim.set_incident_angle(ci["inc_ang"], ci["azi_ang"], ci["angle_layer"])
    for d, eps, mu in ci["layers"]:
        sim.add_layer(d, eps.to(eng.device) if torch.is_tensor(eps) else eps, mu.to(eng.device) if torch.is_tensor(mu) else mu)
    sim.solve_global_smatrix()
    return sim, ci


def _np(EH):
    E, H = EH
    return np.stack([t.detach().cpu().numpy() for t in E + H], axis=-3)          # [..., 6, n1, n2]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- 1. the reference's field maps -------------------------------------------------------------------------------------------------------
# the six-layer stack of config 3 runs on the GPU only and at 1e-7, as in test_fields.py
REFERENCE_CASES = ([pytest.param(b, name, tag, 1e-8, marks=getattr(pytest.mark, b), id=f"{name}-{b}")
                    for b in ("emu", "gpu") for name, tag, emu_ok in FIELD_CASES if emu_ok]
                   + [pytest.param("gpu", name, tag, 1e-7, marks=pytest.mark.gpu, id=f"{name}-gpu") for name, tag, emu_ok in FIELD_CASES if not emu_ok])


@pytest.mark.parametrize("backend,name,tag,tol", REFERENCE_CASES)
def test_batched_fields_against_reference(backend, name, tag, tol):
    eng = make_engine(backend)
    g = load_case(name, tag)
    f = np.load(os.path.join(GOLDEN, f"fields_{name}.npz"))
    f0 = float(g["freq"])
    freq = torch.tensor([f0 * s for s in SCALE], dtype=torch.float64)
    sim, _ = _build(eng, g, freq, batched=True)
    singles = [_build(eng, g, f0 * s, batched=False)[0] for s in SCALE[1:]]
    x, y, z = (torch.from_numpy(f[k]) for k in ("x", "y", "z"))
    nl = int(g["n_layers"])
    for sname, (kind, kw) in SRCS.items():
        for s in [sim] + singles:
            _set_source(s, kind, kw)
        for plane, args in (("xz", (x, z, 133.0)), ("yz", (y, z, 41.0))):
            got = _np(getattr(sim, "field_" + plane)(*args))
            assert got.shape == (3,) + f[f"{sname}_{plane}"].shape
            errs = [_rel(got[0], f[f"{sname}_{plane}"])] + [_rel(got[b + 1], _np(getattr(s, "field_" + plane)(*args))) for b, s in enumerate(singles)]
            print(f"{name} {sname} {plane}: rel. err per point {errs}")
            assert max(errs) < tol, (sname, plane, errs)
        for ln in (-1, 0, nl - 1, nl):
            key = f"{sname}_xy_L{ln}"
            if key not in f:
                continue
            zp = float(f[key + "_zprop"])
            got = _np(sim.field_xy(int(ln), x, y, zp))
            errs = [_rel(got[0], f[key])] + [_rel(got[b + 1], _np(s.field_xy(int(ln), x, y, zp))) for b, s in enumerate(singles)]
            print(f"{name} {sname} xy L{ln}: rel. err per point {errs}")
            assert max(errs) < tol, (sname, ln, errs)


# ---- 2. Parseval: the grid mean of the Poynting vector equals power_flux --------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_field_xy_poynting_equals_power_flux(backend):
    from torcwa_amd.batched import PI_REF
    eng = make_engine(backend)
    freq = torch.tensor([1 / 560., 1 / 610.], dtype=torch.float64)
    sim, order = _stack(eng, inc=0.35, azi=0.6, B=2, freq=freq)
    sim.source_planewave(amplitude=[1.0, 0.4j], notation="xy")
    inc = sim.incident_flux().abs().cpu().numpy()
    nx, ny = 4 * order[0] + 1, 4 * order[1] + 1
    per = math.pi / PI_REF
    x = torch.arange(nx, dtype=torch.float64) * (300. * per / nx)
    y = torch.arange(ny, dtype=torch.float64) * (340. * per / ny)
    for ln, zp in ((0, 37.0), (2, 90.0), (-1, -20.0), (sim.layer_N, 15.0)):
        (Ex, Ey, _), (Hx, Hy, _) = sim.field_xy(ln, x, y, zp)
        mean = torch.real(Ex * torch.conj(Hy) - Ey * torch.conj(Hx)).mean(dim=(1, 2)).cpu().numpy()
        pf = sim.power_flux(ln, zp, normalize=False)[:, 0].cpu().numpy()
        err = np.abs(mean - pf) / inc
        print(f"layer {ln}: |grid mean - power_flux| / incident = {err}")
        assert (err < 1e-9).all(), (ln, mean, pf)


# ---- 3. further cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_fields_per_point_source_and_zprop(backend):
    """A source amplitude [B, M, 2] and z_prop [B]: every point equals its own single solve (per-point thicknesses: field_xy has no limit)."""
    eng = make_engine(backend)
    B = 3
    grids, freq, d0, inc = _batched_problem(eng, B)
    amp = torch.tensor([[[1.0, 0.2j], [0.1, 0.3]], [[0.5, 1.0], [0.2j, 0.0]], [[0.3j, 0.8], [0.4, 0.1]]], dtype=C128)      # [B, M, 2]
    orders = [[0, 0], [1, -1]]
    zp = torch.tensor([10.0, 55.0, 120.0], dtype=torch.float64)
    x, y = torch.linspace(0., 300., 7, dtype=torch.float64), torch.linspace(-20., 250., 5, dtype=torch.float64)
    bs = _solve_points(eng, grids, freq, d0, inc, slice(0, B))
    bs.source_fourier(amplitude=amp, orders=orders)
    got = {ln: _np(bs.field_xy(ln, x, y, zp)) for ln in (-1, 0, 1, 2)}
    assert got[0].shape == (B, 6, 7, 5)
    with pytest.raises(ValueError, match="thickness of layer 0"):
        bs.field_xz(x, torch.tensor([5.0]), 10.0)
    for b in range(B):
        one = _solve_points(eng, grids, freq, d0, inc, slice(b, b + 1))
        one.source_fourier(amplitude=amp[b], orders=orders)
        for ln in got:
            ref = _np(one.field_xy(ln, x, y, float(zp[b])))[0]
            assert _rel(got[ln][b], ref) < 1e-12, (b, ln)


def _small(eng, dtype, freq, **kw):
    import torcwa_amd
    g0 = (_rect(24, 20, 0.5, 0.45) * (11.0 + 0.5j - 1.0) + 1.0).to(torch.complex64)            # float32-representable: both dtypes get the same inputs
    sim = torcwa_amd.BatchedRCWA(freq, [3, 2], [300., 280.], dtype=dtype, engine=eng, **kw)
    sim.add_input_layer(eps=2.25)
    sim.set_incident_angle(0.25, 0.5)
    sim.add_layer(110., g0.to(eng.device) if dtype == torch.complex64 else g0.to(C128).to(eng.device))
    sim.add_layer(40., 2.5)
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[0.6, 1.0], notation="ps")
    return sim


@pytest.mark.parametrize("backend", BACKENDS)
def test_fields_complex64(backend):
    eng = make_engine(backend)
    freq = torch.tensor([1 / 512., 1 / 640.], dtype=torch.float64)                              # exact in float32
    x, y, z = torch.linspace(0., 300., 9), torch.linspace(0., 280., 6), torch.tensor([-30., 0., 20., 110., 125., 150., 200.])
    s64, s128 = _small(eng, torch.complex64, freq), _small(eng, C128, freq)
    for call in (lambda s: s.field_xy(0, x, y, 60.0), lambda s: s.field_xy(2, x, y, 5.0), lambda s: s.field_xz(x, z, 100.0),
                 lambda s: s.field_yz(y, z, 30.0)):
        a, b = call(s64), call(s128)
        assert a[0][0].dtype == torch.complex64 and b[0][0].dtype == C128
        assert _rel(_np(a), _np(b)) < 1e-5


@pytest.mark.parametrize("backend", BACKENDS)
def test_fields_oblique_lattice_circular_orders(backend):
    """A hexagonal lattice with a circular order set: kx, ky per harmonic are no outer product of two axes.  Against rcwa at B = 1; both run the
    same solve in complex128, so only the two read-outs differ: 1e-10 of the largest value leaves three digits over n eps."""
    eng = make_engine(backend)
    kw = dict(inc=0.25, azi=0.4, hexagonal=True)
    one, _ = _stack(eng, **kw)
    bat, _ = _stack(eng, B=1, **kw)
    for s in (one, bat):
        s.source_planewave(amplitude=[1.0, 0.5j], notation="xy")
    x, y, z = torch.linspace(0., 330., 9, dtype=torch.float64), torch.linspace(0., 285., 7, dtype=torch.float64), \
        torch.tensor([-40., 0., 30., 120., 150., 180., 200., 270., 300.], dtype=torch.float64)
    for ln in (-1, 0, 1, 3):
        assert _rel(_np(bat.field_xy(ln, x, y, 25.0))[0], _np(one.field_xy(ln, x, y, 25.0))) < 1e-10, ln
    assert _rel(_np(bat.field_xz(x, z, 77.0))[0], _np(one.field_xz(x, z, 77.0))) < 1e-10
    assert _rel(_np(bat.field_yz(y, z, 21.0))[0], _np(one.field_yz(y, z, 21.0))) < 1e-10


@pytest.mark.parametrize("backend", BACKENDS)
def test_fields_with_symmetry(backend):
    eng = make_engine(backend)
    g = load_case("example1_o3", "c128")
    freq = torch.tensor([float(g["freq"]) * s for s in SCALE[:2]], dtype=torch.float64)
    plain, _ = _build(eng, g, freq, batched=True)
    folded, _ = _build(eng, g, freq, batched=True, symmetry="xy")
    x, y, z = torch.linspace(0., 300., 6, dtype=torch.float64), torch.linspace(0., 300., 4, dtype=torch.float64), \
        torch.tensor([-50., 10., 150., 299., 340.], dtype=torch.float64)
    for s in (plain, folded):
        s.source_planewave(amplitude=[1.0, 0.5j])
    assert _rel(_np(folded.field_xy(0, x, y, 120.0)), _np(plain.field_xy(0, x, y, 120.0))) < 1e-8
    assert _rel(_np(folded.field_xz(x, z, 133.0)), _np(plain.field_xz(x, z, 133.0))) < 1e-8
    assert _rel(_np(folded.field_yz(y, z, 41.0)), _np(plain.field_yz(y, z, 41.0))) < 1e-8


# ---- 4. gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_field_xy_gradient(backend):
    """d(sum |Ex|^2 over a field_xy map at two sweep points) / d(density of one pixel): autograd against central differences."""
    import torcwa_amd
    eng = make_engine(backend)
    dev = eng.device
    gen = torch.Generator().manual_seed(11)
    rho0 = (0.8 * _rect(16, 16, 0.5, 0.4) + 0.15 * torch.rand(16, 16, generator=gen, dtype=torch.float64)).to(dev)
    onehot = torch.nn.functional.one_hot(torch.tensor(6 * 16 + 9), 256).reshape(16, 16).to(torch.float64).to(dev)
    freq = torch.tensor([1 / 540., 1 / 600.], dtype=torch.float64)
    x, y = torch.linspace(0., 300., 7, dtype=torch.float64), torch.linspace(0., 300., 5, dtype=torch.float64)

    def fom(delta):
        rho = rho0 + delta * onehot
        eps = (1.0 + rho * (10.0 + 0.8j - 1.0)).to(C128)
        sim = torcwa_amd.BatchedRCWA(freq, [3, 2], [300., 300.], dtype=C128, engine=eng)
        sim.add_input_layer(eps=2.1)
        sim.set_incident_angle(0.15, 0.3)
        sim.add_layer(110., eps)
        sim.add_layer(40., 2.0 + 0.05j)
        sim.solve_global_smatrix()
        sim.source_planewave(amplitude=[1.0, 0.3], notation="xy")
        (Ex, _, _), _ = sim.field_xy(0, x, y, 70.0)
        return (Ex.abs() ** 2).sum()

    delta = torch.tensor(0.0, dtype=torch.float64, device=dev, requires_grad=True)
    f = fom(delta)
    (gd,) = torch.autograd.grad(f, (delta,))
    with torch.no_grad():
        h = 1e-4
        fd = (fom(torch.tensor(h, dtype=torch.float64, device=dev)) - fom(torch.tensor(-h, dtype=torch.float64, device=dev))) / (2 * h)
        plain = fom(torch.tensor(0.0, dtype=torch.float64, device=dev))
    print(f"forward: graph {float(f.detach()):.12e} kernels {float(plain):.12e};  d/d(rho) autograd {float(gd):.9e} fd {float(fd):.9e}")
    assert abs(float(f.detach()) - float(plain)) < 1e-10 * abs(float(plain))             # the differentiable path and the kernel path agree
    assert abs(float(gd) - float(fd)) < 1e-6 * abs(float(fd))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_field_refusals(backend):
    import torcwa_amd
    from torcwa_amd._lib import TrxError
    eng = make_engine(backend)
    ax = torch.zeros(1, dtype=torch.float64)

    def every(sim, exc, match):
        for call in (lambda: sim.field_xy(0, ax, ax), lambda: sim.field_xz(ax, ax, 0.0), lambda: sim.field_yz(ax, ax, 0.0)):
            with pytest.raises(exc, match=match):
                call()

    mk = lambda **kw: torcwa_amd.BatchedRCWA(1 / 500., [1, 1], [300., 300.], dtype=C128, engine=eng, **kw)
    sim = mk(keep_coupling=False)
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(50., 2.0 + 0.1j)
    sim.source_planewave()
    every(sim, TrxError, "keep_coupling=True.*solved stack")
    sim.solve_global_smatrix()
    every(sim, TrxError, "keep_coupling=True")
    sim = mk()
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(50., 2.0 + 0.1j)
    every(sim, TrxError, "solved stack")
    sim.solve_global_smatrix()
    every(sim, TrxError, "source")
    sim.source_planewave()
    for bad in (2, -2, 0.5):
        with pytest.raises(ValueError, match="layer_num"):
            sim.field_xy(bad, ax, ax)
    assert sim.field_xy(np.int64(1), ax, ax)[0][0].shape == (1, 1, 1)
    E, H = sim.field_xz(torch.zeros(3), torch.tensor([-1.0, 10.0, 60.0]), 0.0)
    assert len(E) == 3 and len(H) == 3 and E[0].shape == (1, 3, 3)
    grid = (_rect(12, 12, 0.5, 0.5) * 5.0 + 1.0).to(eng.device)
    sec = mk(keep_coupling=False, symmetry="xy", symmetry_sector=True)
    sec.set_incident_angle(0.0, 0.0)
    sec.add_layer(50., grid)
    every(sec, ValueError, "symmetry_sector=True")
    swp = mk(keep_coupling=False)
    swp.set_incident_angle(0.0, 0.0)
    swp.add_layer(torch.tensor([40., 50.]), grid, swept=True)
    every(swp, ValueError, "swept")
