"""MI355X timing of the factorisation of config 4's layer at order [15, 15]: a ShapeLayer of one rectangle (trx_convmat_shapes) against
trx_convmat of its 300 x 300 grid, at 128 sweep points -- forward, and forward + backward (ShapeConvFn: trx_toeplitz_sums +
trx_convmat_shapes_backward; ConvMatFn: index_add_ + the conjugate pruned DFT in torch).  Report only: the factorisation is a small share of a
layer-solve (the eigendecomposition dominates) and gets no gate.

    python profiles/shape_timing.py [--points 128] [--order 15] [--grid 300] [--reps 20] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402
from torcwa_amd import autograd_ops as ag  # noqa: E402
from torcwa_amd.lattice import rect_orders  # noqa: E402


def timed(fn, reps, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--order", type=int, default=15)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = torcwa_amd.engine.default_engine()
    B, o, cdt = a.points, a.order, torch.complex128
    # config 4: Wx, Wy in linspace(50, 250, 16), eps of a-Si:H; 128 of its points
    iw, jw = np.unravel_index(np.arange(B) % 256, (16, 16))
    wv = np.linspace(50., 250., 16)
    Wx = torch.tensor(wv[iw], dtype=torch.float64, device=dev)
    Wy = torch.tensor(wv[jw], dtype=torch.float64, device=dev)
    eps_si = torch.full((B,), 17.0 + 0.4j, dtype=cdt, device=dev)
    geo = torcwa_amd.geometry(Lx=300., Ly=300., nx=a.grid, ny=a.grid, edge_sharpness=1000., dtype=torch.float64, device=dev)
    mn = torch.as_tensor(rect_orders(o, o), dtype=torch.int32, device=dev)
    lattice = np.diag([300., 300.])
    gE = torch.randn((B, (2 * o + 1) ** 2, (2 * o + 1) ** 2), dtype=cdt, device=dev)

    def grid_of(wx, wy):
        dens = geo.rectangle(Wx=wx[:, None, None], Wy=wy[:, None, None], Cx=150., Cy=150.)
        return dens * eps_si[:, None, None] + (1. - dens)

    def packed_of(wx, wy):
        return S.ShapeLayer(1.0, [S.rectangle(wx, wy, 150., 150., eps_si)]).pack(lattice, B, dev)

    grid, packed = grid_of(Wx, Wy).contiguous(), packed_of(Wx, Wy)

    def shape_fb():
        wx, wy = Wx.clone().requires_grad_(), Wy.clone().requires_grad_()
        p = packed_of(wx, wy)
        ag.ShapeConvFn.apply(p.par, p.val, p, mn, o, o, cdt, eng).backward(gE)

    def grid_fb(raster):
        wx, wy = Wx.clone().requires_grad_(), Wy.clone().requires_grad_()
        g = grid_of(wx, wy) if raster else grid.clone().requires_grad_()
        ag.ConvMatFn.apply(g, o, o, cdt, eng).backward(gE)

    rows = [("trx_convmat_shapes, forward", timed(lambda: eng.convmat_shapes(packed, mn, cdt, o, o), a.reps, dev)),
            ("trx_convmat of the grid, forward", timed(lambda: eng.convmat(grid, o, o, cdt), a.reps, dev)),
            ("rasterising the grid (geometry.rectangle)", timed(lambda: grid_of(Wx, Wy), a.reps, dev)),
            ("ShapeConvFn forward + backward (to Wx, Wy)", timed(shape_fb, a.reps, dev)),
            ("ConvMatFn forward + backward (to the grid)", timed(lambda: grid_fb(False), a.reps, dev)),
            ("ConvMatFn forward + backward (through the raster to Wx, Wy)", timed(lambda: grid_fb(True), a.reps, dev))]
    N = (2 * o + 1) ** 2
    lines = ["factorisation of config 4's layer: %d points, order [%d, %d] (N = %d, box %d x %d), grid %d x %d, complex128; E is %.0f MB per call"
             % (B, o, o, N, 4 * o + 1, 4 * o + 1, a.grid, a.grid, B * N * N * 16 / 1e6)]
    lines += ["  %-62s %9.3f ms" % r for r in rows]
    lines.append("  the gather writes E once in both forwards; the closed forms add %d sincos-class evaluations per point, the grid path a %d-point pruned DFT"
                 % ((4 * o + 1) ** 2, a.grid * a.grid))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
