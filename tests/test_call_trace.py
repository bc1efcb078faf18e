"""The host layer asks the library for the same work: every stack below is solved through an engine whose library handle records the name and
the scalar arguments of each libtrx call, and the recorded trace must equal the one of tests/golden/call_trace.json, which
tests/golden/make_call_trace_golden.py wrote at the commit before BatchedRCWA was split into its modes.

The stacks are the smallest that reach every host branch -- two frequencies at order [2, 2] (n = 50) on 24 x 24 grids, between a glass input
half-space and an air output half-space, layers homogeneous / patterned / homogeneous / patterned -- one stack per host path.  Only call
names and scalar arguments are compared; every stack returns its results, which the test does not look at.
"""
import json
import os
from ctypes import c_double, c_int, c_long, c_size_t, c_uint

import pytest
import torch

from tests.backends import BACKENDS, get_backend
from tests.helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "call_trace.json")
_SCALARS = (c_int, c_long, c_size_t, c_uint, c_double)
_SILENT = ("strerror", "eig_last_fallback")


class RecordingLib:
    """Proxy of a TrxLib: records [name, scalar arguments ...] of every call (pointers left out; sizing queries and the two status
    read-outs are not recorded)."""

    def __init__(self, lib):
        self._lib, self.trace = lib, []

    def __getattr__(self, name):
        from torcwa_amd._lib import _SIGS
        fn = getattr(self._lib, name)
        if "trx_" + name not in _SIGS or "_ws_bytes" in name or name in _SILENT:
            return fn
        keep = [(i, float if t is c_double else int) for i, t in enumerate(_SIGS["trx_" + name][1]) if t in _SCALARS]

        def call(*args):
            self.trace.append([name] + [conv(args[i]) for i, conv in keep])
            return fn(*args)
        return call


def recording_engine(backend):
    import torcwa_amd
    lib = RecordingLib(get_backend(backend).lib)
    return torcwa_amd.Engine(lib=lib, device="cpu" if backend == "emu" else "cuda"), lib.trace


FREQ = [1 / 532., 1 / 600.]
ORDER, L, NG = [2, 2], [700., 660.], 24
EPS_GLASS, EPS_SI = 1.46 ** 2, 12.0116 + 0.5259j
DT = torch.complex128


def _masks(dev):
    """A centred rectangle and a centred disk on the NG x NG grid (samples at (i + 1/2) / NG: both mirrors about the same centre)."""
    x = (torch.arange(NG, dtype=torch.float64, device=dev) + 0.5) / NG - 0.5
    X, Y = torch.meshgrid(x, x, indexing="ij")
    return ((X.abs() < 0.3) & (Y.abs() < 0.2)).to(torch.float64), (X ** 2 + Y ** 2 < 0.35 ** 2).to(torch.float64)


def _layers(dev):
    rect, disk = (1. + (EPS_SI - 1.) * m for m in _masks(dev))
    return [(60., 2.1), (120., rect), (40., 1.9 + 0.05j), (90., disk)]


def _batched(eng, *, order=ORDER, lattice=L, layers=None, swept=None, **kw):
    import torcwa_amd
    sim = torcwa_amd.BatchedRCWA(torch.tensor(FREQ, dtype=torch.float64, device=eng.device), order, lattice, dtype=DT, engine=eng, **kw)
    sim.add_input_layer(eps=EPS_GLASS)
    sim.add_output_layer(eps=1.)
    sim.set_incident_angle(0., 0.)
    for i, (d, eps) in enumerate(_layers(eng.device) if layers is None else layers):
        if i == swept:
            sim.add_layer([100., 120., 140.], eps, swept=True)
        else:
            sim.add_layer(d, eps)
        # the per-layer lists stay in step in every mode (a solver from before the layer table has no _LAYER_FIELDS: nothing to check)
        assert all(len(getattr(sim, name)) == sim.layer_N for name in getattr(torcwa_amd.batched, "_LAYER_FIELDS", ()))
    return sim


def _two_readouts(sim):
    return [sim.solve_S_parameters([[0, 0], [1, 0]], polarization="xx"),
            sim.solve_S_parameters([[0, 0], [1, 0]], direction="b", port="r", polarization="pp")]


def stack_fold(eng):
    return _two_readouts(_batched(eng, keep_coupling=False, fold_layers=True))


def stack_coupling(eng):
    sim = _batched(eng, keep_coupling=True)
    sim.solve_global_smatrix()
    out = [sim.S_parameters([[0, 0], [1, 0]], polarization="xx")]
    sim.source_planewave(amplitude=[1., 0.], direction="forward")
    ab = sim.absorption()
    out += [ab["layers"], ab["R"], ab["T"], ab["A"]]
    out.append(sim.absorption_by_region(1, masks=torch.stack(_masks(eng.device))))
    return out


def stack_sector(eng):
    return _two_readouts(_batched(eng, keep_coupling=False, symmetry="xy", symmetry_sector=True))


def stack_swept(eng):
    return [_batched(eng, keep_coupling=False, fold_layers=True, swept=1, symmetry=sym).solve_S_parameters([[0, 0], [1, 0]], polarization="xx")
            for sym in (None, "xy")]


def stack_pinv(eng):
    out = []
    for keep in (True, False):
        sim = _batched(eng, keep_coupling=keep, avoid_Pinv_instability=True, max_Pinv_instability=0)       # every point takes the Q branch
        out += _two_readouts(sim) + sim.Pinv_instability + sim.Qinv_instability
    return out


def stack_rules(eng):
    return [t for rule in ("li", "normal") for t in _two_readouts(_batched(eng, keep_coupling=False, fold_layers=True, fourier_rule=rule))]


def stack_oblique(eng):
    from torcwa_amd.lattice import rect_orders
    sim = _batched(eng, order=rect_orders(*ORDER).tolist(), lattice=[[700., 0.], [330., 640.]], keep_coupling=False, fold_layers=True)
    return _two_readouts(sim)


def stack_grad(eng):
    """The drop-in rcwa with eps grids that require grad, plain and with the folded eigenproblem; one solver per frequency."""
    import torcwa_amd
    out = []
    for kw in ({}, dict(symmetry="xy", symmetry_grad=True)):
        for f in FREQ:
            lays = _layers(eng.device)
            grids = [lays[1][1].clone().requires_grad_(), lays[3][1].clone().requires_grad_()]
            sim = torcwa_amd.rcwa(freq=f, order=ORDER, L=L, dtype=DT, engine=eng, **kw)
            sim.add_input_layer(eps=EPS_GLASS)
            sim.add_output_layer(eps=1.)
            sim.set_incident_angle(inc_ang=0., azi_ang=0.)
            for (d, eps), g in zip(lays, (None, grids[0], None, grids[1])):
                sim.add_layer(thickness=d, eps=eps if g is None else g)
            sim.solve_global_smatrix()
            t = sim.S_parameters(orders=[0, 0], polarization="xx")[0].abs() ** 2
            t.backward()
            out += [t.detach(), grids[0].grad, grids[1].grad]
    return out


STACKS = {"fold": stack_fold, "coupling": stack_coupling, "sector": stack_sector, "swept": stack_swept, "pinv": stack_pinv,
          "rules": stack_rules, "oblique": stack_oblique, "grad": stack_grad}


def record(backend, name):
    """(trace, results) of one stack."""
    eng, trace = recording_engine(backend)
    return trace, STACKS[name](eng)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(STACKS))
def test_call_trace_matches_the_fixture(backend, name):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got, _ = record(backend, name)
    got = json.loads(json.dumps(got))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {i} is {a}, the fixture has {b}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, the fixture has {len(want)}"
