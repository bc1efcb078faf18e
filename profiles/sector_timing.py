#!/usr/bin/env python3
"""Timing of symmetry_sector=True on config 2's shape (centred 180 x 100 rectangle, order [15,15], n = 1922, complex64 I/O, precision="high",
polarisation "xx"): solve_single_layer_sweep(symmetry="xy") against the same call with symmetry_sector=True, one chunk of 16 and of 128 points.
Per run: warm steps, the median of `--steps` (at least 5) timed ones, the Engine's phase brackets, the library's trx_prof tags of the fold
kernels and of the phases of trx_eig, and the largest difference between the two results.

    python profiles/sector_timing.py [--steps 5] [--warmup 2] [--modes xy,sector] [--points 16,128] [--label "this commit"]

On a tree without the keyword (the parent commit) only `--modes xy` runs: that run is the yardstick.  Results: profiles/sector_timing.txt.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="xy,sector")
    ap.add_argument("--points", default="16,128")
    ap.add_argument("--label", default="this commit")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be at least 5 (the figure is a median)")
    import bench
    import torcwa_amd
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = torcwa_amd.Engine()
    for B in (int(v) for v in args.points.split(",")):
        freq, grids, lam, eps_si = bench.make_inputs(2, np.arange(B), 300, eng.device)
        print(f"[{args.label}] {B} points, order [15,15], n = 1922, polarisation xx")
        ref, med = None, {}
        for mode in args.modes.split(","):
            kw = dict(symmetry="xy")
            if mode == "sector":
                kw["symmetry_sector"] = True

            def step():
                return solve_single_layer_sweep(freq, grids, 300., [15, 15], [300., 300.], eps_in=1.46 ** 2, dtype=torch.complex64, precision="high",
                                                engine=eng, chunk=B, streams=1, check_info=False, eig_route="auto", polarization="xx", **kw)
            for _ in range(args.warmup):
                out = step()
            torch.cuda.synchronize()
            eng.lib.prof_reset()
            eng.lib.prof_enable(1)
            eng.profile_phases = True
            eng.phase_report()
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                out = step()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            phases = eng.phase_report()
            eng.profile_phases = False
            eng.lib.prof_enable(0)
            med[mode] = statistics.median(times)
            print(f"[{args.label}] B = {B} {mode}: median {1e3 * med[mode]:.1f} ms per step of {args.steps} (min {1e3 * min(times):.1f}, max "
                  f"{1e3 * max(times):.1f}; {B / med[mode]:.1f} layer-solves/s)")
            for name, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
                print(f"    {ms / args.steps:9.1f} ms  {name}")
            for tag in range(64):
                name = eng.lib.prof_tag_name(tag).decode()
                if name == "?":
                    break
                if name.startswith("sym_") or name.startswith("phase:"):
                    buf = (ctypes.c_double * 7)()
                    eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                    if buf[1] > 0:
                        ms = buf[4] / buf[1] * buf[0] / args.steps
                        traffic = f", model traffic {buf[6] / args.steps / 1e9:.2f} GB" if name.startswith("sym_") else ""
                        print(f"    {ms:9.1f} ms  library tag {name}: {buf[0] / args.steps:.0f} launches per step{traffic}")
            o = out.cpu().numpy()
            if ref is None:
                ref = o
            else:
                print(f"    max |t - t(first mode)| / max |t| = {np.abs(o - ref).max() / np.abs(ref).max():.2e}")
        if "xy" in med and "sector" in med:
            print(f"[{args.label}] B = {B}: sector / xy = {med['sector'] / med['xy']:.3f} ({med['xy'] / med['sector']:.2f} x faster)")


if __name__ == "__main__":
    main()
