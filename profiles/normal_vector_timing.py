"""Step time of fourier_rule="normal" against Laurent's rule at the bench shape (GPU; numbers in profiles/normal_vector.txt and DESIGN.md).

Workload: solve_single_layer_sweep, order [15,15], a 300 x 300 complex64 disk grid (a-Si:H disk of radius 90 nm in a 300 nm cell),
128 wavelengths in one chunk, complex64 I/O, precision="high"; the rules' steps interleaved in one process.

    python profiles/normal_vector_timing.py [--steps 3] [--rules laurent,normal]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torcwa_amd  # noqa: E402
from torcwa_amd.geometry import geometry  # noqa: E402
from torcwa_amd.sweep import asih_eps_table, solve_single_layer_sweep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rules", default="laurent,normal")
    args = ap.parse_args()
    rules = args.rules.split(",")
    dev = torch.device("cuda")
    lam, eps_si = asih_eps_table()
    geo = geometry(Lx=300., Ly=300., nx=300, ny=300, edge_sharpness=1000., dtype=torch.float32, device=dev)
    dens = geo.circle(R=90., Cx=150., Cy=150.)[None]
    eps_c = torch.as_tensor(eps_si, dtype=torch.complex64, device=dev)
    grids = (dens * eps_c[:, None, None] + (1. - dens)).contiguous()
    freq = torch.as_tensor(1.0 / lam, dtype=torch.float64, device=dev)
    eng = torcwa_amd.Engine(device=dev)

    def step(rule):
        return solve_single_layer_sweep(freq, grids, 300., [15, 15], [300., 300.], eps_in=1.46 ** 2, dtype=torch.complex64, engine=eng,
                                        chunk=128, check_info=False, fourier_rule=rule)

    for r in rules:                                   # warm-up
        out = step(r)
    torch.cuda.synchronize()
    times = {r: [] for r in rules}
    phases = {r: {} for r in rules}
    peaks = {}
    for _ in range(args.steps):
        for r in rules:
            torch.cuda.reset_peak_memory_stats()
            eng.profile_phases = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = step(r)
            torch.cuda.synchronize()
            times[r].append(time.perf_counter() - t0)
            eng.profile_phases = False
            for k, v in eng.phase_report().items():
                phases[r][k] = phases[r].get(k, 0.0) + v / args.steps
            peaks[r] = (torch.cuda.max_memory_allocated() / 1e9, torch.cuda.max_memory_reserved() / 1e9)
            print(r, "txx[0] =", complex(out[0, 0]), flush=True)
    med = {r: sorted(t)[len(t) // 2] for r, t in times.items()}
    for r in rules:
        print("step time [s] %-8s %s (median %.4f)" % (r, ", ".join("%.4f" % t for t in times[r]), med[r]))
        print("phases [ms]   %-8s %s" % (r, ", ".join("%s %.1f" % kv for kv in phases[r].items())))
        print("HBM peak      %-8s allocated %.2f GB, reserved %.2f GB" % (r, *peaks[r]))
    if "laurent" in med and "normal" in med:
        print("normal / laurent %.4f" % (med["normal"] / med["laurent"]))
    print("failures", eng.failures())


if __name__ == "__main__":
    main()
