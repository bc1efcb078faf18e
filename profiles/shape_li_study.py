#!/usr/bin/env python3
"""Convergence study of the eps = 16 pillar of tests/test_li_factorisation.py (0.25 x 0.2 of a 0.5 x 0.5 cell, lambda = 1, depth 0.4, air over
eps 2.25, incidence 0.3 / 0.3 rad) per order [4,4] .. [12,12]: the closed-form Laurent matrix, closed-form Li (trx_convmat_li_shapes), and the
grid rule trx_convmat_li on rasters of 120^2 and 480^2 -- each raster once with the rectangle's edges halfway between samples (aligned) and once
with the edges on samples (half a pixel off).  A raster's rectangle is the pillar translated by less than a pixel, which leaves |S|^2
unchanged at any truncation.  Figure: max over the four zero-order ports and polarisations of | |S|^2 - |S_ref|^2 |, S_ref closed-form Li at
[14,14].

    python profiles/shape_li_study.py [--out profiles/shape_li_study.txt]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402

LC = 0.5
WX, WY = 0.25, 0.2
PORTS = [(p, pol) for p in ("transmission", "reflection") for pol in ("xx", "xy", "yx", "yy")]


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def pillar(cx, cy):
    return S.ShapeLayer(1.0, [S.rectangle(WX, WY, cx, cy, 16.0)])


def solve(eng, order, rule, eps):
    sim = torcwa_amd.rcwa(freq=1.0, order=order, L=[LC, LC], dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=0.3, azi_ang=0.3)
    sim.add_layer(thickness=0.4, eps=eps)
    sim.solve_global_smatrix()
    return torch.stack([sim.S_parameters(orders=[[0, 0]], port=p, polarization=pol)[0].abs() ** 2 for p, pol in PORTS]).cpu()


def raster(n, aligned, dev):
    """The pillar on an n x n raster; its edges lie at multiples of the pixel when centred at 0.25 (both widths are even numbers of pixels of
    120 and 480): half a pixel further they lie halfway between samples."""
    h = LC / n
    c = 0.25 + (h / 2 if aligned else 0.0)
    return pillar(c, c).rasterise((LC, 0.), (0., LC), n, n, device=dev)[0].real.contiguous()


def main():
    dev = torch.device("cuda")
    eng = torcwa_amd.Engine(device=dev)
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    shape = pillar(0.25, 0.25)
    ref = solve(eng, [14, 14], "li", shape)
    err = lambda v: float((v - ref).abs().max())
    p("eps = 16 pillar, max | |S|^2 - |S_ref|^2 | over the zero-order ports (profiles/shape_li_study.py, %s); S_ref: closed-form Li at [14,14]"
      % torch.cuda.get_device_name(0))
    p("%-8s %12s %12s %14s %14s %14s %14s" % ("order", "Laurent (cf)", "Li (cf)", "Li 120^2 algn", "Li 120^2 off", "Li 480^2 algn", "Li 480^2 off"))
    grids = [raster(n, a, dev) for n in (120, 480) for a in (True, False)]
    for o in (4, 6, 8, 10, 12):
        row = [err(solve(eng, [o, o], "laurent", shape)), err(solve(eng, [o, o], "li", shape))] + [err(solve(eng, [o, o], "li", g)) for g in grids]
        p("%-8s %12.2e %12.2e %14.2e %14.2e %14.2e %14.2e" % ("[%d,%d]" % (o, o), *row))
    with open(arg("--out", os.path.join(ROOT, "profiles", "shape_li_study.txt")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
