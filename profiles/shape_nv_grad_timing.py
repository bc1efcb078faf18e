#!/usr/bin/env python3
"""MI355X timing of the differentiable normal field of a vector-shape layer (shape_nv_grad=True): the adjoint entry
trx_shape_normal_field_backward next to the forward trx_shape_normal_field on 256 x 256, for a disk and a 16-edge layer at B = 1 and B = 16,
and one forward + backward step of a solve at order [15,15] with and without the keyword (the two alternate in one process).

    python profiles/shape_nv_grad_timing.py [--out profiles/shape_nv_grad_timing.txt] [--grid 256]

Kernel rows: the median [min, max] of 20 calls after 3 warm-up calls, HIP events on the current stream.  Step rows: the median of 5 steps
after 1 warm-up step, host clock around a step that ends in a device synchronise.  There is no gate: the work model (include/trx.h) is the
forward again plus one derivative pass over the same 9 (ellipses + edges) evaluations per sample.
"""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
import torcwa_amd.shapes as S  # noqa: E402

ORDER = [15, 15]
L = [[300., 0.], [0., 300.]]


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, dev, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def layers(B, dev, grad=False):
    R = torch.linspace(80., 110., B, dtype=torch.float64, device=dev).requires_grad_(grad)
    t = 2 * math.pi * torch.arange(16, dtype=torch.float64, device=dev) / 16
    gon = torch.stack([150. + R[:, None] * torch.cos(t), 150. + R[:, None] * torch.sin(t)], dim=-1)           # [B, 16, 2]
    return R, {"disk": S.ShapeLayer(1.0, [S.circle(R, 150., 150., 12.0 + 0.5j)]), "16-gon": S.ShapeLayer(1.0, [S.polygon(gon, 12.0 + 0.5j)])}


def step(eng, dev, name, n, grad_kw):
    R, lay = layers(1, dev, grad=True)
    sim = torcwa_amd.BatchedRCWA(torch.full((1,), 1 / 600., dtype=torch.float64, device=dev), ORDER, L, dtype=torch.complex128, engine=eng,
                                 fourier_rule="normal", shape_nv_grid=n, **grad_kw)
    sim.add_input_layer(eps=2.1316)
    sim.add_output_layer(eps=1.)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(120., eps=lay[name])
    sim.solve_global_smatrix()
    (sim.S_parameters(orders=[[0, 0]], direction="forward", port="transmission", polarization="xx").abs() ** 2).sum().backward()
    torch.cuda.synchronize(dev)
    return float(R.grad[0])


def main():
    dev = torch.device("cuda")
    eng = torcwa_amd.Engine(device=dev)
    n = arg("--grid", 256)
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("Differentiable normal field of a vector-shape layer (profiles/shape_nv_grad_timing.py, %s)" % torch.cuda.get_device_name(0))
    p("field grid %d x %d; kernel rows: median [min, max] of 20 calls in ms (HIP events)" % (n, n))
    for B in (1, 16):
        _, lay = layers(B, dev)
        for name, layer in lay.items():
            pk = layer.pack(L, B, dev)
            g = torch.randn((B, 3, n, n), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(3))
            for label, fn in (("forward  (trx_shape_normal_field)", lambda: eng.shape_normal_field(pk, L, n, n)),
                              ("backward (trx_shape_normal_field_backward)", lambda: eng.shape_normal_field_backward(pk, L, g))):
                p("  B = %2d  %-7s %-44s %8.3f [%8.3f, %8.3f]" % ((B, name, label) + timed(fn, dev)))
    p("forward + backward step of one solve, order %s (N = %d), B = 1, complex128; median [min, max] of 5 steps in ms (host clock, synchronised)"
      % (ORDER, (2 * ORDER[0] + 1) * (2 * ORDER[1] + 1)))
    for name in ("disk", "16-gon"):
        ms = {False: [], True: []}
        for kw in (False, True):
            step(eng, dev, name, n, dict(shape_nv_grad=kw))                                # warm-up of both variants
        for _ in range(5):
            for kw in (False, True):                                                       # alternating
                t0 = time.perf_counter()
                step(eng, dev, name, n, dict(shape_nv_grad=kw))
                ms[kw].append(1e3 * (time.perf_counter() - t0))
        for kw in (False, True):
            p("  %-7s shape_nv_grad=%-5s %9.1f [%9.1f, %9.1f]" % (name, kw, statistics.median(ms[kw]), min(ms[kw]), max(ms[kw])))
    with open(arg("--out", os.path.join(ROOT, "profiles", "shape_nv_grad_timing.txt")), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
