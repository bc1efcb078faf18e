#!/usr/bin/env python3
"""Golden power-flux values from the reference's own field maps (run where the reference is installed, like make_golden.py).

    python tests/golden/make_flux_golden.py            # -> tests/golden/flux_<name>.npz (about 2 kB each)

For the inputs of the S-matrix fixtures example1_o3, asym_o32, example1_o5 and config3_o8_l500 (tests/helpers.load_case) and the three sources
of tests/test_fields.py::SRCS, the reference's field_xy is sampled on a uniform grid of n_axis >= 4 order + 1 points per axis (starting at 0,
no duplicate end point) on the planes z = 0, 0.37 d and d of every layer and on two planes of each half-space.  The grid mean of
Ex conj(Hy) - Ey conj(Hx) is then an exact quadrature of the truncated Fourier series (its harmonics reach 2 order); this is asserted by
doubling the grid.  Stored: the real part of the mean per plane and the incident flux of the source.  Only numbers travel.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import torcwa  # noqa: E402  (the reference, located and imported as make_golden.py does)

from torcwa_amd.batched import PI_REF  # noqa: E402  (the reference's value of pi, a documented part of its behaviour)
from tests.helpers import case_inputs, load_case  # noqa: E402
from tests.test_fields import SRCS  # noqa: E402

CASES = [("example1_o3", "c128"), ("asym_o32", "c128"), ("example1_o5", "c128"), ("config3_o8_l500", "c128f32")]
INTERIOR = 0.37


def planes_of(thicknesses):
    """[(layer_num, z_prop)]: both half-spaces (two planes each) and z = 0, INTERIOR d, d of every layer."""
    pl = [(-1, 0.0), (-1, -35.0)]
    for l, d in enumerate(thicknesses):
        pl += [(l, 0.0), (l, INTERIOR * d), (l, d)]
    return pl + [(len(thicknesses), 0.0), (len(thicknesses), 25.0)]


def grid_mean(sim, ln, zp, L, n_axis):
    # The reference's pi is off in the 10th digit (torcwa/rcwa.py:5), so its harmonics e^{i omega G x} repeat after L pi / pi_ref, not L:
    # the grid spans that period (over L itself the mean is an exact quadrature only to ~3e-12).
    stretch = np.pi / PI_REF
    x = torch.arange(n_axis[0], dtype=torch.float64) * (L[0] * stretch / n_axis[0])
    y = torch.arange(n_axis[1], dtype=torch.float64) * (L[1] * stretch / n_axis[1])
    E, H = sim.field_xy(int(ln), x, y, float(zp))
    ex, ey, hx, hy = E[0].numpy(), E[1].numpy(), H[0].numpy(), H[1].numpy()
    val = (ex * np.conj(hy) - ey * np.conj(hx)).mean()
    scale = (np.abs(ex * np.conj(hy)) + np.abs(ey * np.conj(hx))).mean()
    return val, scale


def flux_case(name, tag):
    g = load_case(name, tag)
    ci = case_inputs(g, "c128")
    sim = torcwa.rcwa(freq=ci["freq"], order=ci["order"], L=ci["L"], dtype=torch.complex128, device=torch.device("cpu"), stable_eig_grad=False)
    if "eps_in" in ci:
        sim.add_input_layer(eps=ci["eps_in"])
    if "eps_out" in ci:
        sim.add_output_layer(eps=ci["eps_out"])
    sim.set_incident_angle(inc_ang=ci["inc_ang"], azi_ang=ci["azi_ang"], angle_layer=ci["angle_layer"])
    for (d, eps, mu) in ci["layers"]:
        sim.add_layer(thickness=d, eps=eps, mu=mu)
    sim.solve_global_smatrix()
    planes = planes_of([d for d, _, _ in ci["layers"]])
    n_axis = [4 * o + 1 for o in ci["order"]]
    N = sim.order_N
    out = {"layer": np.array([p[0] for p in planes], dtype=np.int64), "z_prop": np.array([p[1] for p in planes], dtype=np.float64)}
    worst = 0.0
    for sname, (kind, kw) in SRCS.items():
        (sim.source_planewave if kind == "pw" else sim.source_fourier)(**kw)
        vals = []
        for ln, zp in planes:
            v1, s1 = grid_mean(sim, ln, zp, ci["L"], n_axis)
            v2, _ = grid_mean(sim, ln, zp, ci["L"], [2 * a for a in n_axis])
            # the exact-quadrature claim, relative to the size of the averaged terms
            worst = max(worst, abs(v1 - v2) / s1)
            assert abs(v1 - v2) <= 1e-12 * s1, (name, sname, ln, zp, v1, v2)
            vals.append(v1.real)
        fwd = kw["direction"] in ("f", "forward")
        Vh = (sim.Vi if hasattr(sim, "Vi") else sim.Vf) if fwd else (sim.Vo if hasattr(sim, "Vo") else sim.Vf)
        Ei = sim.E_i.reshape(-1).numpy()
        Hi = (1.0 if fwd else -1.0) * (Vh.numpy() @ Ei)
        out[f"{sname}_flux"] = np.array(vals, dtype=np.float64)
        out[f"{sname}_incident"] = np.float64(np.real(Ei[:N] * np.conj(Hi[N:]) - Ei[N:] * np.conj(Hi[:N])).sum())
    path = os.path.join(HERE, f"flux_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"flux_{name}: {os.path.getsize(path)} bytes, {len(planes)} planes, grid doubling changes the mean by at most {worst:.1e} (relative)")


if __name__ == "__main__":
    for name, tag in CASES:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        flux_case(name, tag)
