#!/usr/bin/env python3
"""MI355X timing of the normal-vector assembly of a vector-shape layer at the bench shape (order [15,15], 128 points): the field kernel
(trx_shape_normal_field on 256 x 256), the two coefficient passes (trx_convmat_shapes with the values and with the reciprocal values), and the
whole trx_convmat_nv_shapes, next to the grid rule's trx_convmat_nv on a 256 x 256 raster in the same process; peak HBM of both.

    python profiles/shape_nv_timing.py [--out profiles/shape_nv_timing.txt] [--points 128] [--grid 256]

Each figure is the median of 7 calls after 2 warm-up calls, HIP events on the current stream.
"""
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402
from torcwa_amd.lattice import rect_orders  # noqa: E402

ORDER = [15, 15]
L = [[300., 0.], [0., 300.]]


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


def main():
    dev = torch.device("cuda")
    eng = torcwa_amd.Engine(device=dev)
    B, n = arg("--points", 128), arg("--grid", 256)
    R = torch.linspace(80., 110., B, dtype=torch.float64)
    t = 2 * math.pi * torch.arange(16, dtype=torch.float64) / 16
    gon = torch.stack([150. + R[:, None] * torch.cos(t), 150. + R[:, None] * torch.sin(t)], dim=-1)           # [B, 16, 2]
    layers = {"disk": S.ShapeLayer(1.0, [S.circle(R, 150., 150., 12.0 + 0.5j)]), "16-gon": S.ShapeLayer(1.0, [S.polygon(gon, 12.0 + 0.5j)])}
    mn = torch.as_tensor(rect_orders(*ORDER), dtype=torch.int32, device=dev)
    cdt = torch.complex128
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("Normal-vector assembly of a vector-shape layer (profiles/shape_nv_timing.py, %s)" % torch.cuda.get_device_name(0))
    p("order %s (N = %d), %d points, field grid %d x %d; median [min, max] of 7 calls in ms, peak HBM of the call in GB" % (ORDER, len(mn), B, n, n))
    for name, layer in layers.items():
        pk = layer.pack(L, B, dev)
        rval = layer.reciprocal_values(B, dev)
        rows = [("field kernel (trx_shape_normal_field)", lambda: eng.shape_normal_field(pk, L, n, n)),
                ("coefficients + gather, val", lambda: eng.convmat_shapes(pk, mn, cdt, *ORDER)),
                ("coefficients + gather, rval", lambda: eng.convmat_shapes(pk._replace(val=rval), mn, cdt, *ORDER)),
                ("whole assembly (trx_convmat_nv_shapes)", lambda: eng.convmat_nv_shapes(pk, rval, L, mn, cdt, n, n, mmax=ORDER[0], nmax=ORDER[1]))]
        grid = layer.rasterise(L[0], L[1], n, n, device=dev)
        rows.append(("grid rule (trx_convmat_nv, sigma 6, %d^2 raster)" % n, lambda: eng.convmat_nv(grid, ORDER[0], ORDER[1], cdt, sigma=6.0, hx=300. / n, hy=300. / n)))
        p(name)
        for label, fn in rows:
            med, lo, hi, peak = timed(fn, dev)
            p("  %-52s %8.2f [%8.2f, %8.2f]   %6.2f GB" % (label, med, lo, hi, peak))
    out = arg("--out", os.path.join(ROOT, "profiles", "shape_nv_timing.txt"))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
