#!/usr/bin/env python3
"""Convergence study of the normal-vector rule on vector shapes (fourier_rule="normal" with a ShapeLayer) against closed-form Laurent, and
of the grid the field products are sampled on (shape_nv_grid).  Runs through the library on the GPU.

    python profiles/shape_nv_study.py [--out profiles/shape_nv_study.txt]

Set-up of profiles/normal_vector.txt: cell 0.5 x 0.5, lambda 1, depth 0.3, air over eps_out 2.25, inc 0.3, azi 0.4, eps 12.
Metric: worst | |S|^2 - |S_ref|^2 | over the 8 zeroth-order port / polarisation pairs; reference: the same method at [13,13] with a 512 grid.
"""
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402

ORDERS = [[5, 5], [7, 7], [9, 9]]
REF_ORDER = [13, 13]
GRIDS = [128, 256, 512]


def structures():
    c, s = math.cos(math.pi / 6), math.sin(math.pi / 6)
    L = [(0.10, 0.10), (0.40, 0.10), (0.40, 0.22), (0.22, 0.22), (0.22, 0.40), (0.10, 0.40)]
    return {
        "disk r 0.18": [S.circle(0.18, 0.25, 0.25, 12.0)],
        "ellipse 0.2 x 0.1, 0.3 rad": [S.ellipse(0.2, 0.1, 0.25, 0.25, 12.0, theta=0.3)],
        "rotated square, side 0.25, 30 deg": [S.square(0.25, 0.25, 0.25, 12.0, theta=math.pi / 6)],
        "two touching disks r 0.125": [S.circle(0.125, 0.125, 0.25, 12.0), S.circle(0.125, 0.375, 0.25, 12.0)],
        "L-shape (arms 0.12 wide, 0.3 long)": [S.polygon(L, 12.0)],
    }


def solve(shapes, order, rule, grid=256):
    dev = torch.device("cuda")
    sim = torcwa_amd.BatchedRCWA(torch.ones(1, dtype=torch.float64, device=dev), order, [0.5, 0.5], dtype=torch.complex128,
                                 fourier_rule=rule, keep_coupling=False, shape_nv_grid=grid)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(0.3, 0.4)
    sim.add_layer(0.3, eps=S.ShapeLayer(1.0, shapes))
    return torch.stack([sim.solve_S_parameters([[0, 0]], polarization=pol, port=port)[0, 0].abs() ** 2
                        for port in ("transmission", "reflection") for pol in ("xx", "xy", "yx", "yy")]).cpu()


def main():
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("Normal-vector rule on vector shapes: closed-form [eps], [1/eps], the blended field of the shape list sampled on a grid")
    p("(profiles/shape_nv_study.py, %s)" % torch.cuda.get_device_name(0))
    p("cell 0.5 x 0.5, lambda 1, depth 0.3, air over eps_out 2.25, inc 0.3, azi 0.4, eps 12")
    p("metric: worst | |S|^2 - |S_ref|^2 | over the 8 zeroth-order port / polarisation pairs; reference: NV at %s, field grid 512" % REF_ORDER)
    p("'ref 256 vs 512': how far the reference itself moves between field grids of 256 and 512")
    p("")
    t0 = time.time()
    for name, shapes in structures().items():
        ref = solve(shapes, REF_ORDER, "normal", 512)
        ref256 = solve(shapes, REF_ORDER, "normal", 256)
        p("%s   ref 256 vs 512: %.1e" % (name, float((ref - ref256).abs().max())))
        p("  %-22s %s" % ("rule", "  ".join("%9s" % str(o) for o in ORDERS)))
        p("  %-22s %s" % ("closed-form Laurent", "  ".join("%9.1e" % float((solve(shapes, o, "laurent") - ref).abs().max()) for o in ORDERS)))
        at = {}
        for g in GRIDS:
            at[g] = [solve(shapes, o, "normal", g) for o in ORDERS]
            p("  %-22s %s" % ("closed-form NV, %d" % g, "  ".join("%9.1e" % float((v - ref).abs().max()) for v in at[g])))
        p("  %-22s %s" % ("|NV 256 - NV 512|", "  ".join("%9.1e" % float((a - b).abs().max()) for a, b in zip(at[256], at[512]))))
        p("")
    p("wall time %.0f s" % (time.time() - t0))
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "shape_nv_study.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
