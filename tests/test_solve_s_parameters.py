"""BatchedRCWA.solve_S_parameters (the read-out that probes the last half-space star product instead of forming the global S-matrix) against
solve_global_smatrix() + S_parameters(...) on the same solver inputs, and the sweep drivers against a per-chunk full solve.

Gates: the project's own -- 1e-9 for complex128, 1e-5 for complex64 I/O, max-abs difference over max(max-abs of the full-path values, 1e-3)
as in tests/test_fullsize_golden.py.  The fallback cases go through the very same full path and must agree to rounding (1e-13).
"""
import warnings

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import DIRPORT, ORDERS_PROBE, POLS
from tests.test_pipeline import make_engine

ORDER, L = [2, 1], [300., 260.]
TOL = {torch.complex128: 1e-9, torch.complex64: 1e-5}
SETUPS = ["in", "out", "both", "two_layers"]
REF_ORDERS = [[0, 0], [1, -1]]


def _grid(nx=24, ny=20, shift=0.0):
    x = (torch.arange(nx, dtype=torch.float64) + 0.5) / nx - 0.5
    y = (torch.arange(ny, dtype=torch.float64) + 0.5) / ny - 0.5
    inside = (((x[:, None] - shift) / 0.31) ** 2 + ((y[None, :] + 0.5 * shift) / 0.22) ** 2) < 1.0
    return 1.0 + (11.9 + 0.3j - 1.0) * inside.to(torch.complex128)


def _build(eng, setup, dtype, *, keep_coupling=False, fold_layers=True, diff=False, B=2):
    """A small oblique-incidence stack; setup names which half-spaces it has and how many patterned layers."""
    import torcwa_amd
    freq = torch.tensor([1 / 500., 1 / 530., 1 / 610.][:B], dtype=torch.float64, device=eng.device)
    sim = torcwa_amd.BatchedRCWA(freq, ORDER, L, dtype=dtype, engine=eng, keep_coupling=keep_coupling, fold_layers=fold_layers)
    if setup in ("in", "both", "two_layers"):
        sim.add_input_layer(eps=1.46 ** 2)
    if setup in ("out", "both", "two_layers"):
        sim.add_output_layer(eps=2.1)
    sim.set_incident_angle(0.21, 0.4)
    rdt = torch.complex128 if dtype == torch.complex128 else torch.complex64
    g = _grid().to(rdt).to(eng.device)
    if diff:
        g.requires_grad_(True)
    sim.add_layer(120., g)
    if setup == "two_layers":
        sim.add_layer(80., _grid(shift=0.12).to(rdt).to(eng.device))
    return sim


def _rel(a, ref):
    a, ref = a.detach().cpu().numpy().astype(np.complex128), ref.detach().cpu().numpy().astype(np.complex128)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-3))


def _combos():
    for (dr, pt) in DIRPORT:
        for pol in POLS:
            for ro in REF_ORDERS:
                yield dict(direction=dr, port=pt, polarization=pol, ref_order=ro)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["c128", "c64"])
@pytest.mark.parametrize("setup", SETUPS)
def test_restricted_read_out_equals_full(backend, dtype, setup):
    """Every (direction, port) x polarisation x reference order, probe orders that include clamped out-of-range ones."""
    eng = make_engine(backend)
    sim = _build(eng, setup, dtype)
    full = _build(eng, setup, dtype)
    full.solve_global_smatrix()
    assert not hasattr(sim, "S")
    worst = 0.0
    for kw in _combos():
        for pn in (True, False):
            ref = full.S_parameters([list(o) for o in ORDERS_PROBE], power_norm=pn, **kw)
            got = sim.solve_S_parameters([list(o) for o in ORDERS_PROBE], power_norm=pn, **kw)
            assert got.dtype == ref.dtype == dtype and got.shape == ref.shape == (2, len(ORDERS_PROBE))
            assert torch.isfinite(torch.view_as_real(got)).all()
            err = _rel(got, ref)
            worst = max(worst, err)
            assert err < TOL[dtype], (setup, kw, pn, err)
    assert not hasattr(sim, "S"), "the restricted path must not form the global S-matrix"
    print(f"{setup} {dtype}: worst restricted-vs-full difference {worst:.3e}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_arguments_warnings_and_clamping(backend):
    """Invalid names give the warnings and defaults of S_parameters, an order tensor is clamped in place, evanscent is passed on."""
    eng = make_engine(backend)
    sim, full = _build(eng, "both", torch.complex128), _build(eng, "both", torch.complex128)
    full.solve_global_smatrix()
    bad = dict(direction="sideways", port="window", polarization="zz")
    with warnings.catch_warnings(record=True) as w_ref:
        warnings.simplefilter("always")
        ref = full.S_parameters([[0, 0], [1, 0]], **bad)
    with warnings.catch_warnings(record=True) as w_got:
        warnings.simplefilter("always")
        got = sim.solve_S_parameters([[0, 0], [1, 0]], **bad)
    assert [str(x.message) for x in w_got] == [str(x.message) for x in w_ref] and len(w_ref) == 3
    assert _rel(got, ref) < 1e-9
    assert _rel(got, full.S_parameters([[0, 0], [1, 0]])) < 1e-9          # = forward / transmission / xx
    o_ref = torch.tensor(ORDERS_PROBE, dtype=torch.int64, device=eng.device)
    o_got = o_ref.clone()
    ref = full.S_parameters(o_ref, polarization="sp", evanscent=0.5)
    got = sim.solve_S_parameters(o_got, polarization="sp", evanscent=0.5)
    assert torch.equal(o_got, o_ref) and int(o_got[-1, 0]) == ORDER[0] and int(o_got[-1, 1]) == -ORDER[1]
    assert _rel(got, ref) < 1e-9


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["keep_coupling", "differentiable", "no_halfspace", "homogeneous_only"])
def test_fallback_cases_take_the_full_path(backend, case):
    import torcwa_amd
    eng = make_engine(backend)
    dt = torch.complex128

    def build():
        if case == "keep_coupling":
            return _build(eng, "both", dt, keep_coupling=True, fold_layers=False)
        if case == "differentiable":
            return _build(eng, "both", dt, diff=True)
        if case == "no_halfspace":
            return _build(eng, "none", dt)
        sim = torcwa_amd.BatchedRCWA(torch.tensor([1 / 500., 1 / 530.], dtype=torch.float64, device=eng.device), ORDER, L, dtype=dt, engine=eng,
                                     keep_coupling=False, fold_layers=True)
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0.21, 0.4)
        sim.add_layer(90., 2.3)
        return sim

    sim, full = build(), build()
    full.solve_global_smatrix()
    for kw in list(_combos())[::5]:
        ref = full.S_parameters([list(o) for o in ORDERS_PROBE], **kw)
        got = sim.solve_S_parameters([list(o) for o in ORDERS_PROBE], **kw)
        assert _rel(got, ref) < 1e-13, (case, kw)
        assert hasattr(sim, "S") and all(_rel(a, b) < 1e-13 for a, b in zip(sim.S, full.S))          # the full path sets S (and C)
        assert len(sim.C[0]) == len(full.C[0])
    if case == "differentiable":
        assert got.requires_grad


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["c128", "c64"])
@pytest.mark.parametrize("layers", [1, 2])
def test_sweep_drivers_equal_per_chunk_full_solve(backend, dtype, layers):
    """solve_single_layer_sweep / solve_stack_sweep (3 points in chunks of 2) against solve_global_smatrix + S_parameters per chunk."""
    import torcwa_amd
    from torcwa_amd.sweep import solve_single_layer_sweep, solve_stack_sweep
    eng = make_engine(backend)
    B = 3
    freq = torch.tensor([1 / 500., 1 / 530., 1 / 610.], dtype=torch.float64, device=eng.device)
    grids = torch.stack([_grid(shift=0.03 * i) for i in range(B)]).to(dtype).to(eng.device)
    grids2 = torch.stack([_grid(shift=-0.05 * i) for i in range(B)]).to(dtype).to(eng.device)
    orders = [tuple(o) for o in ORDERS_PROBE[:7]]
    for pol, dr, pt in (("xx", "forward", "transmission"), ("ps", "forward", "reflection"), ("yy", "backward", "transmission")):
        kw = dict(eps_in=1.46 ** 2, inc_ang=0.1, azi_ang=0.3, dtype=dtype, engine=eng, chunk=2, orders=orders, polarization=pol, direction=dr, port=pt)
        if layers == 1:
            got = solve_single_layer_sweep(freq, grids, 120., ORDER, L, **kw)
            lays = [(120., grids)]
        else:
            kw["eps_out"] = 2.1
            lays = [(120., grids), (80., grids2)]
            got = solve_stack_sweep(freq, lays, ORDER, L, **kw)
        parts = []
        for lo, hi in ((0, 2), (2, 3)):
            sim = torcwa_amd.BatchedRCWA(freq[lo:hi], ORDER, L, dtype=dtype, engine=eng, keep_coupling=False, fold_layers=True)
            sim.add_input_layer(eps=1.46 ** 2)
            if layers == 2:
                sim.add_output_layer(eps=2.1)
            sim.set_incident_angle(0.1, 0.3)
            for d, g in lays:
                sim.add_layer(d, g[lo:hi])
            sim.solve_global_smatrix()
            parts.append(sim.S_parameters([list(o) for o in orders], direction=dr, port=pt, polarization=pol))
        ref = torch.cat(parts, dim=0)
        assert got.shape == ref.shape == (B, len(orders)) and got.dtype == dtype
        assert _rel(got, ref) < TOL[dtype], (pol, dr, pt, _rel(got, ref))
