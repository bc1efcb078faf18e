#!/usr/bin/env python3
"""Timing of a thickness scan on config 2's workload (centred 180 x 100 rectangle, order [15,15], 128 wavelengths as one chunk, complex64 I/O):

  loop  : one solve_single_layer_sweep per thickness (what a tree without swept=True offers: assembly and trx_eig repeated per thickness)
  swept : one solve_thickness_sweep over the same thicknesses (modes once, one GEMM and one LU per thickness)

    python profiles/thickness_sweep_timing.py [--modes loop,swept] [--T 8,4] [--steps 2] [--warmup 1] [--points 128] [--dump DIR]

Per mode and T: wall time per scan, the Engine's phase brackets, the library's thickness_* prof tags (swept) and, with --dump, the txx values
as DIR/<mode>_T<T>.npy.  On a tree without the driver (the parent commit) only `--modes loop` runs.  Results: profiles/thickness_sweep_timing.txt.
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
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="loop,swept")
    ap.add_argument("--T", default="8,4")
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    import bench
    import torcwa_amd
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = torcwa_amd.Engine()
    B = args.points
    freq, grids, lam, eps_si = bench.make_inputs(2, np.arange(B), 300, eng.device)
    kw = dict(eps_in=1.46 ** 2, dtype=torch.complex64, precision="high", engine=eng, chunk=B, streams=1, check_info=False, eig_route="auto")
    n = 1922
    for mode in args.modes.split(","):
        for T in (int(t) for t in args.T.split(",")):
            thick = np.linspace(100.0, 450.0, 8)[:T].tolist()

            def scan():
                if mode == "loop":
                    return torch.stack([solve_single_layer_sweep(freq, grids, d, [15, 15], [300., 300.], **kw) for d in thick], dim=1)
                from torcwa_amd.sweep import solve_thickness_sweep
                return solve_thickness_sweep(freq, [(None, grids)], [15, 15], [300., 300.], thicknesses=thick, **kw)
            for _ in range(args.warmup):
                out = scan()
            torch.cuda.synchronize()
            eng.lib.prof_reset()
            eng.lib.prof_enable(1)
            eng.profile_phases = True
            eng.phase_report()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = scan()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            phases = eng.phase_report()
            eng.profile_phases = False
            eng.lib.prof_enable(0)
            print(f"[{args.label}] {mode}, T = {T}, {B} points: {1e3 * dt:.1f} ms per scan ({1e3 * dt / T:.1f} ms per thickness)")
            for name, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
                print(f"    {ms / args.steps:9.1f} ms  {name}")
            for tag in range(64):
                name = eng.lib.prof_tag_name(tag).decode()
                if name == "?":
                    break
                if name.startswith("thickness_"):
                    buf = (ctypes.c_double * 7)()
                    eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                    if buf[1] > 0:
                        ms = buf[4] / buf[1] * buf[0] / args.steps
                        macs = buf[5] / args.steps / 8.0
                        print(f"    {ms:9.1f} ms  library tag {name}: {buf[0] / args.steps:.0f} calls per scan, {macs / (B * n ** 3):.2f} n^3 complex MACs per point "
                              f"-> {buf[5] / args.steps / (ms / 1e3) / 1e12:.1f} TFLOP/s (real flops, 8 per complex MAC)")
            o = out.cpu().numpy()
            print(f"    txx[0, :, 0] = {np.array2string(o[0, :, 0], precision=6)}")
            if args.dump:
                os.makedirs(args.dump, exist_ok=True)
                np.save(os.path.join(args.dump, f"{mode}_T{T}.npy"), o)


if __name__ == "__main__":
    main()
