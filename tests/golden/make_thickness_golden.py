#!/usr/bin/env python3
"""Golden S-parameters of thickness scans from the reference itself, one full solve per thickness (run where the reference is installed,
like make_golden.py).

    python tests/golden/make_thickness_golden.py            # -> tests/golden/thickness_<name>.npz (a few kB each)

(a) thickness_example1_o3: the stack and grid of example1_o3 (tests/helpers.load_case) at order [3, 3] and normal incidence, two wavelengths,
    the patterned layer at 1, 50, 300 and 2000 nm (the last: strongly evanescent phases).
(b) thickness_asym_o32: the grids of asym_o32 -- patterned eps AND mu, oblique incidence, order [3, 2] -- as the MIDDLE layer of three, between
    two layers that carry the third grid of that case, so that both sides of the scanned layer are dense S-matrices; the same thicknesses.
Stored: the scan's own inputs (frequencies, thicknesses, the outer layers' thicknesses) and sparams[freq, thickness, (direction, port), pol,
order] for ORDERS x POLS x all four (direction, port) pairs, computed in complex128 on the CPU.  The grids are those of the existing fixtures and
are not stored again: the float32-representable ones (*_c128f32), so that a complex64 run sees the identical problem.  Only numbers travel.
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

from tests.helpers import DIRPORT, case_inputs, load_case  # noqa: E402

THICKNESSES = [1.0, 50.0, 300.0, 2000.0]
ORDERS = [[0, 0], [1, 0]]
POLS = ["xx", "yy", "xy"]


def scan(name, freqs, order, L, layers_of, eps_in, eps_out, inc_ang, azi_ang, extra):
    out = np.zeros((len(freqs), len(THICKNESSES), len(DIRPORT), len(POLS), len(ORDERS)), dtype=np.complex128)
    for fi, freq in enumerate(freqs):
        for ti, d in enumerate(THICKNESSES):
            sim = torcwa.rcwa(freq=freq, order=order, L=L, dtype=torch.complex128, device=torch.device("cpu"), stable_eig_grad=False)
            if eps_in is not None:
                sim.add_input_layer(eps=eps_in)
            if eps_out is not None:
                sim.add_output_layer(eps=eps_out)
            sim.set_incident_angle(inc_ang=inc_ang, azi_ang=azi_ang)
            for (th, eps, mu) in layers_of(d):
                sim.add_layer(thickness=th, eps=eps, mu=mu)
            sim.solve_global_smatrix()
            for a, (dr, pt) in enumerate(DIRPORT):
                for b, pol in enumerate(POLS):
                    out[fi, ti, a, b] = sim.S_parameters(orders=ORDERS, direction=dr, port=pt, polarization=pol).numpy()
    path = os.path.join(HERE, f"thickness_{name}.npz")
    np.savez_compressed(path, freqs=np.array(freqs, dtype=np.float64), thicknesses=np.array(THICKNESSES), orders=np.array(ORDERS), sparams=out,
                        **extra)
    print(f"thickness_{name}: {os.path.getsize(path)} bytes, max |S| per (direction, port) = {np.abs(out).max(axis=(0, 1, 3, 4))}")


def main():
    ci = case_inputs(load_case("example1_o3", "c128f32"), "c128")
    (_, eps, mu), = ci["layers"]
    scan("example1_o3", [1 / 532., 1 / 610.], ci["order"], ci["L"], lambda d: [(d, eps, mu)], ci.get("eps_in"), ci.get("eps_out"), 0.0, 0.0, {})

    ci = case_inputs(load_case("asym_o32", "c128f32"), "c128")
    (_, eps0, mu0), _, (_, eps2, mu2) = ci["layers"]
    outer = [70.0, 110.0]
    scan("asym_o32", [ci["freq"]], ci["order"], ci["L"], lambda d: [(outer[0], eps2, mu2), (d, eps0, mu0), (outer[1], eps2, mu2)],
         ci.get("eps_in"), ci.get("eps_out"), ci["inc_ang"], ci["azi_ang"], {"outer_thicknesses": np.array(outer)})


if __name__ == "__main__":
    main()
