#!/usr/bin/env python3
"""Timing of symmetry= on config 2's workload (centred 180 x 100 rectangle, order [15,15], 128 wavelengths, one chunk of 128 points through
solve_single_layer_sweep, exactly bench.py's call): per-step time, the Engine's phase brackets (eig / fold / unfold / ...), the library's
sym_fold / sym_unfold tags and the number of matrices the mixed-precision eigensolver redid in fp64, for symmetry = None, "x", "xy".

    python profiles/symmetry_timing.py [--steps 2] [--warmup 1] [--modes none,x,xy] [--points 128]

On a tree without the keyword (the parent commit) only `--modes none` runs.  Results: profiles/symmetry_timing.txt.
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


def grid_asymmetry(g):
    g = g if g.dim() == 3 else g[None]
    a = float(torch.abs(g).max())
    return max(float(torch.abs(g - torch.flip(g, dims=(1,))).max()), float(torch.abs(g - torch.flip(g, dims=(2,))).max())) / a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="none,x,xy")
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--label", default="this commit")
    args = ap.parse_args()
    import bench
    import torcwa_amd
    from torcwa_amd.sweep import solve_single_layer_sweep
    eng = torcwa_amd.Engine()
    B = args.points
    freq, grids, lam, eps_si = bench.make_inputs(2, np.arange(B), 300, eng.device)
    delta = grid_asymmetry(grids)
    print(f"[{args.label}] {B} points, order [15,15], n = 1922; grid asymmetry max |g - mirror(g)| / max |g| = {delta:.3e}")
    if "x" in args.modes:
        from tests.helpers import load_case
        for name in ("example1_o3", "example1_o5", "config2_o15_l532"):
            g = load_case(name, "c128" if name.startswith("example") else "c128f32")
            print(f"  fixture {name}: grid asymmetry {grid_asymmetry(torch.from_numpy(g['L0_eps_grid'])):.3e}")
    tol = max(1e-6, 4 * delta)
    # count the fp64 redos of every eig call of a step
    redo = [0, 0]
    plain_eig = eng.eig

    def counting_eig(*a, **kw):
        out = plain_eig(*a, **kw)
        redo[0] += eng.eig_fallback_of_last_call()
        redo[1] += a[0].shape[0]
        return out
    eng.eig = counting_eig
    ref = None
    for mode in args.modes.split(","):
        kw = {} if mode == "none" else dict(symmetry=mode, symmetry_tol=tol)

        def step():
            return solve_single_layer_sweep(freq, grids, 300., [15, 15], [300., 300.], eps_in=1.46 ** 2, dtype=torch.complex64, precision="high",
                                            engine=eng, chunk=B, streams=1, check_info=False, eig_route="auto", **kw)
        for _ in range(args.warmup):
            out = step()
        torch.cuda.synchronize()
        eng.lib.prof_reset()
        eng.lib.prof_enable(1)
        eng.profile_phases = True
        eng.phase_report()
        redo[0] = redo[1] = 0
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        phases = eng.phase_report()
        eng.profile_phases = False
        eng.lib.prof_enable(0)
        print(f"[{args.label}] symmetry={mode}: {1e3 * dt:.1f} ms per step ({B / dt:.1f} layer-solves/s); fp64 redos {redo[0] // args.steps} of {redo[1] // args.steps} "
              f"matrices per step" + (f"; symmetry_tol = {tol:.1e}" if kw else ""))
        for name, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
            print(f"    {ms / args.steps:9.1f} ms  {name}")
        for tag in range(64):
            name = eng.lib.prof_tag_name(tag).decode()
            if name == "?":
                break
            if name.startswith("sym_"):
                buf = (ctypes.c_double * 7)()
                eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                if buf[1] > 0:
                    ms = buf[4] / buf[1] * buf[0] / args.steps
                    print(f"    {ms:9.1f} ms  library tag {name}: {buf[0] / args.steps:.0f} launches per step, model traffic {buf[6] / args.steps / 1e9:.1f} GB "
                          f"-> {buf[6] / args.steps / 1e9 / (ms / 1e3) / 1e3:.2f} TB/s")
        o = out.cpu().numpy()
        if ref is None:
            ref = o
        else:
            print(f"    max |t - t(symmetry=none)| / max |t| = {np.abs(o - ref).max() / np.abs(ref).max():.2e}")


if __name__ == "__main__":
    main()
