#!/usr/bin/env python3
"""How much of d|t00|^2 / dp the dependence of the normal field on the geometry carries: the gradient with shape_nv_grad=True (the derivative
of the forward) against the frozen-field gradient (shape_nv_grad=False), on the stack of tests/test_shape_nv_grad.py -- a rotated ellipse
150 x 90 with a nested core plus a 4-gon on the oblique cell [[700, 0], [150, 640]], glass below, air above, normal incidence, 1 / 600 --
at orders [2,2], [5,5] and [7,7] with shape_nv_grid=256, complex128, stable_eig_grad=False.  Runs through the library on the GPU.

    python profiles/shape_nv_grad_study.py [--out profiles/shape_nv_grad_study.txt]

At convergence the S-matrix does not depend on the field, so the term falls with the order; at any finite order it is part of the gradient of
the function the forward evaluates.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402
from torcwa_amd.lattice import rect_orders  # noqa: E402

LATTICE = [[700., 0.], [150., 640.]]
GRID = 256
PICK = {"R": (), "Cx": (), "theta": (), "vertex (2, x)": (2, 0)}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def gradients(eng, order, grad):
    t = lambda v: torch.tensor(v, dtype=torch.float64, device=eng.device, requires_grad=True)
    p = {"R": t(150.), "Cx": t(260.), "theta": t(0.3), "vertex (2, x)": t([[520., 120.], [680., 180.], [640., 330.], [560., 260.]])}
    ell = S.ellipse(p["R"], 90., p["Cx"], 250., 12.0116 + 0.5259j, theta=p["theta"])
    layer = S.ShapeLayer(1.0, [ell, S.circle(40., 260., 250., 2.0, host=ell), S.polygon(p["vertex (2, x)"], 3.0)])
    sim = torcwa_amd.BatchedRCWA(torch.full((1,), 1 / 600., dtype=torch.float64, device=eng.device), rect_orders(*order).tolist(), LATTICE,
                                 dtype=torch.complex128, engine=eng, fourier_rule="normal", stable_eig_grad=False, shape_nv_grid=GRID,
                                 shape_nv_grad=grad)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.add_output_layer(eps=1.)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(120., eps=layer)
    sim.solve_global_smatrix()
    T = (sim.S_parameters(orders=[[0, 0]], direction="forward", port="transmission", polarization="xx").abs() ** 2).sum()
    T.backward()
    return float(T.detach()), {k: float(p[k].grad[PICK[k]]) for k in p}


def main():
    eng = torcwa_amd.Engine(device=torch.device("cuda"))
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("S-level size of the field term of the gradient (profiles/shape_nv_grad_study.py, %s)" % torch.cuda.get_device_name(0))
    p("d|t00|^2 / dp with shape_nv_grad=True (full) and False (frozen field); shape_nv_grid=%d, complex128" % GRID)
    p("%-8s %-14s %16s %16s %24s" % ("order", "parameter", "g_full", "g_frozen", "|g_full - g_frozen| / |g_full|"))
    for order in ([2, 2], [5, 5], [7, 7]):
        T, full = gradients(eng, order, True)
        _, frozen = gradients(eng, order, False)
        for k in full:
            p("%-8s %-14s %16.8e %16.8e %24.3f" % (order, k, full[k], frozen[k], abs(full[k] - frozen[k]) / abs(full[k])))
        p("%-8s |t00|^2 = %.8f" % (order, T))
    with open(arg("--out", os.path.join(ROOT, "profiles", "shape_nv_grad_study.txt")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
