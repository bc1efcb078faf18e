"""MI355X timing of a hexagonal photonic crystal solved natively (oblique lattice, circular truncation) against its rectangular a x sqrt(3) a
supercell (rectangular truncation): a 128-wavelength sweep of one slab of eps = 12 disks (r = 0.3 a, t = 0.5 a, normal incidence) through
torcwa_amd.sweep.solve_single_layer_sweep.  Reports layer-solves per second, peak HBM and the zeroth-order transmission of both.

The two order sets are chosen from profiles/lattice.txt (--harmonics for the native circular set, --box for the supercell's [ox, oy]).
Without --box the supercell takes the smallest box that contains the native set's disk |G| <= |G|max: the two then share every harmonic
inside |G|max, but the box also holds harmonics beyond it in its corners, so they are not the same truncation.

--gather: instead, time trx_convmat_orders alone (128 grids, the native set) for a kernel trace (rocprofv3 --kernel-trace --stats).

    python profiles/lattice_timing.py [--harmonics 301] [--box OX OY] [--points 128] [--out FILE] [--gather]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
from torcwa_amd.lattice import circular_orders, reciprocal, rect_orders  # noqa: E402
from torcwa_amd.sweep import solve_single_layer_sweep  # noqa: E402

S3 = math.sqrt(3.0)
HEX = [[1.0, 0.0], [0.5, S3 / 2]]
SC = [[1.0, 0.0], [0.0, S3]]


def grids(M, dev):
    geo = torcwa_amd.lattice_geometry(HEX[0], HEX[1], 2 * M, M, 200.0, dtype=torch.float64, device=torch.device("cpu"))
    gh = (1.0 + 11.0 * geo.circle(0.3, 0.0, 0.0)).numpy()
    i, j = np.meshgrid(np.arange(2 * M), np.arange(2 * M), indexing="ij")
    gs = gh[(i - j) % (2 * M), j % M]                    # the supercell on the same samples
    return torch.as_tensor(gh).to(dev), torch.as_tensor(gs).to(dev)


def run(label, L, order, grid, lam, dev, reps):
    B = lam.shape[0]
    g = grid[None].expand(B, -1, -1).contiguous()
    kw = dict(eps_in=1.0, eps_out=1.0, inc_ang=0.0, azi_ang=0.0, dtype=torch.complex128, orders=((0, 0),), chunk=B)
    solve_single_layer_sweep((1 / lam).to(dev), g, 0.5, order, L, **kw)       # warm-up (allocator, code objects)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        t = solve_single_layer_sweep((1 / lam).to(dev), g, 0.5, order, L, **kw)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    peak = torch.cuda.max_memory_allocated(dev) / 1e9
    N = len(order) if np.ndim(order) == 2 else (2 * order[0] + 1) * (2 * order[1] + 1)
    T = (t.abs() ** 2).cpu().numpy()[:, 0]
    return {"case": label, "N": int(N), "n": 2 * int(N), "seconds_per_sweep": dt, "layer_solves_per_s": B / dt, "peak_hbm_gb": peak, "T00": T}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--harmonics", type=int, default=301)
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--box", type=int, nargs=2, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gather", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mh = circular_orders(HEX, n_harmonics=a.harmonics)
    gmax = float(np.hypot(*(mh @ reciprocal(HEX)).T).max())
    ox, oy = int(math.floor(gmax * 1.0 * (1 + 1e-9))), int(math.floor(gmax * S3 * (1 + 1e-9)))
    if a.box:
        ox, oy = a.box
    nmax = max(int(np.abs(mh).max()), oy)
    M = max(64, nmax + 1)
    gh, gs = grids(M, dev)
    if a.gather:
        eng = torcwa_amd.engine.default_engine()
        g = gh[None].expand(a.points, -1, -1).contiguous()
        for _ in range(20):
            eng.convmat_orders(g, mh, torch.complex128)
        torch.cuda.synchronize(dev)
        N = len(mh)
        print("trx_convmat_orders: %d grids %s, N = %d: output %.1f MB per call" % (a.points, list(gh.shape), N, a.points * N * N * 16 / 1e6))
        return
    lam = torch.linspace(1.2, 2.0, a.points, dtype=torch.float64)
    res = [run("hexagonal, circular", HEX, mh, gh, lam, dev, a.reps),
           run("supercell, rectangular [%d,%d]" % (ox, oy), SC, [ox, oy], gs, lam, dev, a.reps)]
    lines = ["hexagonal eps = 12 disk slab (r 0.3 a, t 0.5 a, normal incidence), %d wavelengths in [1.2, 2.0] a, native |G|max = %.4f / a, "
             "grids %s / %s, complex128" % (a.points, gmax, [2 * M, M], [2 * M, 2 * M])]
    for r in res:
        lines.append("  %-34s N %5d  n %5d  %.3f s / sweep  %.1f layer-solves/s  peak HBM %.2f GB"
                     % (r["case"], r["N"], r["n"], r["seconds_per_sweep"], r["layer_solves_per_s"], r["peak_hbm_gb"]))
    h, s = res
    lines.append("  native / supercell: %.2fx layer-solves/s, %.2fx peak HBM; max |T00 difference| over the sweep %.2e"
                 % (h["layer_solves_per_s"] / s["layer_solves_per_s"], h["peak_hbm_gb"] / s["peak_hbm_gb"], float(np.abs(h["T00"] - s["T00"]).max())))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
            f.write(json.dumps([{k: v for k, v in r.items() if k != "T00"} for r in res]) + "\n")


if __name__ == "__main__":
    main()
