"""MI355X timing of absorption by region: one patterned lossy layer (a disk in a lossy film) on glass, batch 16, complex128, orders [11,11]
(n = 1058) and [15,15] (n = 1922), the coupling matrices kept.

  (a) absorption_by_region(0, masks, z_range) with 2 masks x 16 depth bins   (2 convolution matrices, 4 x 2 trx_gemm pairs, 4 trx_modal_overlap)
  (b) absorption()                                                           (trx_matvec + trx_layer_flux)
  (c) the layer solve that produced W, V and C                               (add_layer + solve_global_smatrix)
  (d) trx_modal_overlap alone at nr = 1 and nr = 16

Events around warmed-up repeats; the median of --reps repeats is reported.

    python profiles/volume_integral_timing.py [--batch 16] [--reps 5] [--out profiles/volume_integral_timing.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torcwa_amd  # noqa: E402
from profiles.flux_timing import timed  # noqa: E402


def disk(nx, ny, r):
    x = (torch.arange(nx, dtype=torch.float64) + 0.5) / nx - 0.5
    y = (torch.arange(ny, dtype=torch.float64) + 0.5) / ny - 0.5
    return ((x[:, None] ** 2 + y[None, :] ** 2) < r * r).to(torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = torcwa_amd.engine.default_engine()
    B = a.batch
    lines, blob = [], {}
    for o in (11, 15):
        n = 2 * (2 * o + 1) ** 2
        m = disk(256, 256, 0.3).to(dev)
        eps = (m * (12.0 + 0.8j) + (1.0 - m) * (2.1 + 0.05j)).to(torch.complex128)
        masks = torch.stack((m, 1.0 - m))
        freq = torch.linspace(1 / 620., 1 / 500., B, dtype=torch.float64, device=dev)
        holder = {}

        def solve():
            sim = torcwa_amd.BatchedRCWA(freq, [o, o], [300., 300.], dtype=torch.complex128, engine=eng)
            sim.add_input_layer(eps=1.46 ** 2)
            sim.set_incident_angle(0.1, 0.2)
            sim.add_layer(200., eps)
            sim.solve_global_smatrix()
            holder["sim"] = sim

        tc = timed(solve, max(2, a.reps // 2), dev)
        sim = holder["sim"]
        sim.source_planewave(amplitude=[1.0, 0.0])
        edges = torch.linspace(0.0, 200.0, 17, dtype=torch.float64)
        bins = torch.stack((edges[:-1], edges[1:]), dim=1)
        ta = timed(lambda: sim.absorption_by_region(0, masks, bins), a.reps, dev)
        tb = timed(lambda: sim.absorption(), a.reps, dev)
        gap = float((sim.absorption_by_region(0, masks, bins).sum(dim=(1, 2)) - sim.absorption()["layers"][:, 0]).abs().max())
        c = sim._mv(sim.C[0][0], sim._E_i)
        M = eng.gemm(sim.E_eigvec[0], sim.E_eigvec[0], opA=2)
        zr = bins.to(dev)[None].expand(B, -1, -1)
        td = {nr: timed(lambda: eng.modal_overlap(M, c[:, :n], c[:, n:], sim.kz_norm[0], sim.omega, sim.thickness[0], zr[:, :nr], 1), a.reps, dev)
              for nr in (1, 16)}
        blob[str(o)] = {"n": n, "B": B, "region_ms": ta, "absorption_ms": tb, "solve_ms": tc, "overlap_ms": td, "sum_minus_layer": gap}
        lines.append("order [%d,%d] (n = %d), batch %d, complex128" % (o, o, n, B))
        lines.append("  (a) absorption_by_region, 2 masks x 16 bins   %.1f ms (%.1f - %.1f)   |sum - absorption()| %.1e" % (*ta, gap))
        lines.append("  (b) absorption()                              %.2f ms (%.2f - %.2f)" % tb)
        lines.append("  (c) layer solve + global S-matrix             %.1f ms (%.1f - %.1f)" % tc)
        for nr, t in td.items():
            lines.append("  (d) trx_modal_overlap nr = %2d                  %.2f ms (%.2f - %.2f)" % (nr, *t))
        del sim, holder, M
        torch.cuda.empty_cache()
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(blob) + "\n")


if __name__ == "__main__":
    main()
