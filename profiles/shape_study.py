"""What the pixel grid costs: |S - S_shapes| of a disk layer at order [5, 5] for rasters of 64 ... 1024 points a side, hard-edged
(ShapeLayer.rasterise) and with the sigmoid edge of `geometry` (edge_sharpness = 1000), and the same for d|t00|^2 / dR -- autograd through the
sigmoid raster, and for the hard raster (piecewise constant in R) a central difference over one pixel.  The shapes' own derivative is the
reference (ShapeConvFn).  `geometry` samples at (i + 1/2) L / n while the DFT indexes from 0, so its disk is asked for at (Cx + L / 2n,
Cy + L / 2n) to sit where the shape does.

    python profiles/shape_study.py [--backend gpu|emu] [--order 5] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402

L, R0, C, D, FREQ, EPS = 300., 97., (141., 163.), 600., 1 / 473., 2.0709 ** 2
PROBE = [[0, 0], [1, 0], [0, 1], [-1, -1]]


def solve(eng, order, eps):
    sim = torcwa_amd.BatchedRCWA(torch.tensor([FREQ], dtype=torch.float64, device=eng.device), [order, order], [L, L], dtype=torch.complex128,
                                 engine=eng)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(D, eps=eps)
    sim.solve_global_smatrix()
    # t00 on its own: an evanescent probe order is zeroed through a where() whose masked branch would put NaN into a gradient
    return torch.cat([sim.S_parameters(PROBE, polarization=p)[0] for p in ("xx", "yy")]).detach(), sim.S_parameters([[0, 0]], polarization="xx")[0, 0]


def with_grad(eng, order, make):
    R = torch.tensor(R0, dtype=torch.float64, device=eng.device, requires_grad=True)
    s, t00 = solve(eng, order, make(R))
    (t00.abs() ** 2).backward()
    return s, float(R.grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="gpu", choices=["gpu", "emu"])
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.backend == "emu":
        from tests.emu import emu_lib
        eng = torcwa_amd.Engine(lib=emu_lib(), device="cpu")
    else:
        eng = torcwa_amd.engine.default_engine()
    dev, o = eng.device, a.order
    shape = lambda R: S.ShapeLayer(1.0, [S.circle(R, C[0], C[1], EPS)])
    s_ref, g_ref = with_grad(eng, o, shape)
    lines = ["disk R = %g at (%g, %g) in a %g x %g cell, eps %.4f, thickness %g, order [%d, %d], complex128, %s; d|t00,xx|^2/dR of the shapes: %.6e"
             % (R0, C[0], C[1], L, L, EPS, D, o, o, a.backend, g_ref),
             "%6s  %14s %14s   %16s %16s" % ("n", "|dS| hard", "|dS| sigmoid", "|d grad| hard*", "|d grad| sigmoid")]
    for n in (64, 128, 256, 512, 1024):
        hard = lambda R: shape(R).rasterise([L, 0.], [0., L], n, n, device=dev)[0].real
        geo = torcwa_amd.geometry(Lx=L, Ly=L, nx=n, ny=n, edge_sharpness=1000., dtype=torch.float64, device=dev)
        soft = lambda R: 1. + (EPS - 1.) * geo.circle(R=R, Cx=C[0] + L / (2 * n), Cy=C[1] + L / (2 * n))
        with torch.no_grad():
            s_hard = solve(eng, o, hard(R0))[0]
            h = L / n
            fd = (float(solve(eng, o, hard(R0 + h / 2))[1].abs() ** 2) - float(solve(eng, o, hard(R0 - h / 2))[1].abs() ** 2)) / h
        s_soft, g_soft = with_grad(eng, o, soft)
        lines.append("%6d  %14.3e %14.3e   %16.3e %16.3e" % (n, float((s_hard - s_ref).abs().max()), float((s_soft - s_ref).abs().max()),
                                                             abs(fd - g_ref), abs(g_soft - g_ref)))
    lines.append("* central difference over one pixel (R +- L / 2n): a hard raster is piecewise constant in R and has no derivative of its own")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
