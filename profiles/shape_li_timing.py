#!/usr/bin/env python3
"""MI355X timing of Li's rule on rectangle layers at the bench shape (order [15,15], 128 points): trx_convmat_li_shapes for S = 1, 4, 16
rectangles per point, with and without the kept inverses, next to the grid rule's trx_convmat_li on a 300 x 300 raster in the same process; and
the backward of ShapeLiFn (composition + trx_convmat_li_shapes_backward) next to ConvMatLiFn's.  Peak HBM of each call.

    python profiles/shape_li_timing.py [--out profiles/shape_li_timing.txt] [--points 128] [--grid 300]

Each figure is the median of 7 calls after 2 warm-up calls, HIP events on the current stream.
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402
from torcwa_amd import autograd_ops as ag  # noqa: E402

ORDER = [15, 15]
LX = LY = 300.
L = [[LX, 0.], [0., LY]]


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, dev, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), (torch.cuda.max_memory_allocated(dev) - base) / 1e9


def layer_of(count, B):
    """count rectangles on a sqrt(count) x sqrt(count) raster of the cell, the widths swept over the points."""
    k = int(round(count ** 0.5))
    w = torch.linspace(0.35, 0.6, B, dtype=torch.float64) * LX / k
    return S.ShapeLayer(1.0, [S.rectangle(w, 0.8 * w, (i + 0.5) * LX / k, (j + 0.5) * LY / k, 12.0 + 0.5j) for i in range(k) for j in range(k)])


def main():
    dev = torch.device("cuda")
    eng = torcwa_amd.Engine(device=dev)
    B, n = arg("--points", 128), arg("--grid", 300)
    cdt = torch.complex128
    N = (2 * ORDER[0] + 1) * (2 * ORDER[1] + 1)
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("Li's rule on rectangle layers (profiles/shape_li_timing.py, %s)" % torch.cuda.get_device_name(0))
    p("order %s (N = %d), %d points; median [min, max] of 7 calls in ms, peak HBM of the call in GB" % (ORDER, N, B))
    gE = torch.randn((2, B, N, N), dtype=cdt, device=dev)
    grid = layer_of(1, B).rasterise(L[0], L[1], n, n, device=dev)
    rows = [("grid rule (trx_convmat_li, %d^2 raster)" % n, lambda: eng.convmat_li(grid, ORDER[0], ORDER[1], cdt)),
            ("grid rule, inverses kept", lambda: eng.convmat_li(grid, ORDER[0], ORDER[1], cdt, keep_inverses=True))]
    g = grid.clone().requires_grad_(True)
    out = ag.ConvMatLiFn.apply(g, ORDER[0], ORDER[1], cdt, eng)
    rows.append(("grid rule, backward (ConvMatLiFn)", lambda: torch.autograd.grad(out, g, (gE[0], gE[1]), retain_graph=True)))
    for count in (1, 4, 16):
        layer = layer_of(count, B)
        pk, rval = layer.pack(L, B, dev), layer.reciprocal_values(B, dev)
        rows.append(("S = %2d: trx_convmat_li_shapes" % count, lambda pk=pk, rval=rval: eng.convmat_li_shapes(pk, rval, LX, LY, *ORDER, cdt)))
        rows.append(("S = %2d: inverses and strip record kept" % count,
                     lambda pk=pk, rval=rval: eng.convmat_li_shapes(pk, rval, LX, LY, *ORDER, cdt, keep=True)))
        par, rv = pk.par.clone().requires_grad_(True), rval.clone().requires_grad_(True)
        o = ag.ShapeLiFn.apply(par, rv, pk, LX, LY, ORDER[0], ORDER[1], cdt, eng)
        rows.append(("S = %2d: backward (ShapeLiFn)" % count,
                     lambda o=o, par=par, rv=rv: torch.autograd.grad(o, (par, rv), (gE[0], gE[1]), retain_graph=True)))
    for label, fn in rows:
        med, lo, hi, peak = timed(fn, dev)
        p("  %-52s %8.2f [%8.2f, %8.2f]   %6.2f GB" % (label, med, lo, hi, peak))
    with open(arg("--out", os.path.join(ROOT, "profiles", "shape_li_timing.txt")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
