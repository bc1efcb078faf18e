#!/usr/bin/env python3
"""Golden S-parameters of a mirror-symmetric three-layer stack from the reference itself (run where the reference is installed, like
make_golden.py).

    python tests/golden/make_sector_golden.py            # -> tests/golden/sector_stack_o3.npz

The stack, at order [3, 2] and normal incidence between a substrate and a superstrate: a centred rectangle, a homogeneous spacer and a centred
circle, both patterns drawn by the reference's `geometry` on ONE 60 x 56 grid (samples at (i + 1/2) h: the mirrors sit at the half-cell centre
along x and y, the same for both layers).  Stored: the inputs (the two eps grids in complex128, thicknesses, scalars) and
sparams[variant, ref, (direction, port), pol, order] for ORDERS x POLS x all four (direction, port) pairs; variant 0 runs on the grids as stored,
variant 1 on their float32 / complex64 roundings (what a complex64 user hands over); ref 0 is ref_order [0, 0] (one mirror sector per column
under "xy"), ref 1 is ref_order [1, 0] (four).  Computed in complex128 on the CPU.  Only numbers travel.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import _via_f32, ref_geometry, torcwa  # noqa: E402  (the reference, located and imported as make_golden.py does)

from tests.helpers import DIRPORT, ORDERS_PROBE  # noqa: E402

POLS = ["xx", "yy", "yx", "xy"]
REFS = [[0, 0], [1, 0]]
FREQ, ORDER, L = 1 / 532., [3, 2], [700., 660.]          # order (1, 0) propagates in both half-spaces
NX, NY = 60, 56
EPS_IN, EPS_OUT, EPS_SPACER = 1.46 ** 2, 1.21, 2.1
THICKNESSES = [120., 60., 90.]
EPS_SI = 12.0116 + 0.5259j


def main():
    g = ref_geometry(NX, NY, L[0], L[1], torch.float64)
    rect = g.rectangle(Wx=400., Wy=240., Cx=L[0] / 2, Cy=L[1] / 2)
    circ = g.circle(R=200., Cx=L[0] / 2, Cy=L[1] / 2)
    grids = [d * EPS_SI + (1. - d) for d in (rect, circ)]
    out = np.zeros((2, len(REFS), len(DIRPORT), len(POLS), len(ORDERS_PROBE)), dtype=np.complex128)
    for vi in range(2):
        e0, e2 = grids if vi == 0 else [_via_f32(e) for e in grids]
        sim = torcwa.rcwa(freq=FREQ, order=ORDER, L=L, dtype=torch.complex128, device=torch.device("cpu"), stable_eig_grad=False)
        sim.add_input_layer(eps=EPS_IN)
        sim.add_output_layer(eps=EPS_OUT)
        sim.set_incident_angle(inc_ang=0., azi_ang=0.)
        sim.add_layer(thickness=THICKNESSES[0], eps=e0)
        sim.add_layer(thickness=THICKNESSES[1], eps=EPS_SPACER)
        sim.add_layer(thickness=THICKNESSES[2], eps=e2)
        sim.solve_global_smatrix()
        for ri, ref in enumerate(REFS):
            for a, (dr, pt) in enumerate(DIRPORT):
                for b, pol in enumerate(POLS):
                    out[vi, ri, a, b] = sim.S_parameters(orders=ORDERS_PROBE, direction=dr, port=pt, polarization=pol, ref_order=ref).numpy()
    path = os.path.join(HERE, "sector_stack_o3.npz")
    np.savez_compressed(path, freq=FREQ, order=np.array(ORDER), L=np.array(L), eps_in=EPS_IN, eps_out=EPS_OUT, eps_spacer=EPS_SPACER,
                        thicknesses=np.array(THICKNESSES), eps_rect=grids[0].numpy(), eps_circ=grids[1].numpy(), refs=np.array(REFS),
                        orders=np.array(ORDERS_PROBE), sparams=out)
    print(f"sector_stack_o3: {os.path.getsize(path)} bytes, max |S| per (ref, direction, port) = {np.abs(out).max(axis=(0, 3, 4))}")


if __name__ == "__main__":
    main()
