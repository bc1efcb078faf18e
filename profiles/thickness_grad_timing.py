#!/usr/bin/env python3
"""Forward + backward of a thickness scan on config 5's stack (bench.py: n = 1.46 substrate, one patterned silicon layer from the blurred random
density, 532 nm, complex128) at order [15,15] (n = 1922), one point:

  loop  : T plain differentiable BatchedRCWA solves, one per thickness -- T eigenproblems, T eigen-adjoints, T cascades: the only way to these
          gradients on a tree without swept_grad
  swept : one BatchedRCWA(swept_grad=True) solve with add_layer(d [T], swept=True) -- one eigenproblem and one eigen-adjoint, one GEMM + one LU
          per thickness forward and again backward (trx_thickness_columns / trx_thickness_columns_backward)

The figure of merit is sum_t w_t (|t_(1,0),xx|^2 + |t_(1,0),yy|^2) (two read-outs per solve in both modes), differentiated with respect to the
density and every thickness.

    python profiles/thickness_grad_timing.py [--T 4,16] [--steps 3] [--warmup 1] [--order 15] [--out profiles/thickness_grad_timing.txt]

Per mode and T: wall time of forward + backward (mean, min and max of the steps after a warm-up at the same T), the Engine's phase brackets
and the library's thickness_* prof tags; then both wall times and their ratio, and the largest difference between the two modes' gradients.
Results: profiles/thickness_grad_timing.txt.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--T", default="4,16")
    ap.add_argument("--order", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thickness_grad_timing.txt"))
    args = ap.parse_args()
    import bench
    import torcwa_amd
    eng = torcwa_amd.Engine()
    dev = eng.device
    rho0 = bench.make_inputs_topopt(dev)
    order = [args.order, args.order]
    n = 2 * (2 * args.order + 1) ** 2
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def solver(**kw):
        sim = torcwa_amd.BatchedRCWA(1 / 532., order, [700., 300.], batch=1, dtype=torch.complex128, engine=eng, keep_coupling=False, **kw)
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0., 0.)
        return sim

    def fom_of(sim):
        return sum(torch.abs(sim.solve_S_parameters([[1, 0]], direction="forward", port="transmission", polarization=p)) ** 2 for p in ("xx", "yy"))

    def run(mode, thick, w):
        rho = rho0.clone().requires_grad_(True)
        d = thick.clone().requires_grad_(True)
        eps = rho * bench.TOPOPT_EPS + (1. - rho)
        if mode == "swept":
            sim = solver(swept_grad=True)
            sim.add_layer(d, eps, swept=True)
            fom = (fom_of(sim).reshape(-1) * w).sum()                                   # [1, T, 1] -> weighted sum over T
        else:
            fom = 0
            for t in range(d.shape[0]):
                sim = solver()
                sim.add_layer(d[t], eps)
                fom = fom + w[t] * fom_of(sim).sum()
        fom.backward()
        return float(fom.detach()), rho.grad.detach(), d.grad.detach()

    say(f"thickness_grad_timing: config 5's stack, order {order} (n = {n}), complex128, 1 point, {torch.cuda.get_device_name(dev)}")
    for T in (int(t) for t in args.T.split(",")):
        thick = torch.linspace(250., 350., T, dtype=torch.float64, device=dev)
        w = torch.linspace(1.0, 0.4, T, dtype=torch.float64, device=dev)
        wall, grads = {}, {}
        for mode in ("loop", "swept"):
            for _ in range(args.warmup):                                                # the shapes of the timed steps: T decides the LU / GEMM batches
                run(mode, thick, w)
            torch.cuda.synchronize()
            eng.lib.prof_reset()
            eng.lib.prof_enable(1)
            eng.profile_phases = True
            eng.phase_report()
            each = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                grads[mode] = run(mode, thick, w)
                torch.cuda.synchronize()
                each.append(time.perf_counter() - t0)
            wall[mode] = sum(each) / args.steps
            phases = eng.phase_report()
            eng.profile_phases = False
            eng.lib.prof_enable(0)
            say(f"{mode}, T = {T}: {1e3 * wall[mode]:.1f} ms forward + backward, mean of {args.steps} steps (min {1e3 * min(each):.1f}, max {1e3 * max(each):.1f}; "
                f"{1e3 * wall[mode] / T:.1f} ms per thickness)")
            for name, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
                say(f"    {ms / args.steps:9.1f} ms  {name}")
            for tag in range(64):
                name = eng.lib.prof_tag_name(tag).decode()
                if name == "?":
                    break
                if name.startswith("thickness_"):
                    buf = (ctypes.c_double * 7)()
                    eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                    if buf[1] > 0:
                        ms = buf[4] / buf[1] * buf[0] / args.steps
                        say(f"    {ms:9.1f} ms  library tag {name}: {buf[0] / args.steps:.0f} calls, {buf[5] / args.steps / 8.0 / n ** 3:.2f} n^3 complex MACs "
                            f"-> {buf[5] / args.steps / (ms / 1e3) / 1e12:.1f} TFLOP/s (real flops, 8 per complex MAC)")
        (f0, r0, d0), (f1, r1, d1) = grads["loop"], grads["swept"]
        say(f"T = {T}: loop {1e3 * wall['loop']:.1f} ms, swept {1e3 * wall['swept']:.1f} ms, loop / swept = {wall['loop'] / wall['swept']:.2f}; "
            f"FoM {abs(f1 - f0) / abs(f0):.1e}, d/d density {float((r1 - r0).abs().max() / r0.abs().max()):.1e}, "
            f"d/d thickness {float((d1 - d0).abs().max() / d0.abs().max()):.1e} (swept against loop, relative)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
