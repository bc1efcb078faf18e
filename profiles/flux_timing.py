"""MI355X timing of per-layer absorption: the flagship sweep's geometry (one patterned a-Si:H layer on glass, order [15,15], n = 1922, complex64
I/O with precision="high") with the coupling matrices kept.

  (a) BatchedRCWA.absorption()                                   (trx_matvec + trx_layer_flux + O(n) half-space work)
  (b) the same numbers the way they could be had before: Engine.gemm with an [n, 2] right-hand side plus torch reductions
  (c) the sweep with absorption=True (keep_coupling=True, no streaming cascade) against the plain sweep, with peak HBM per point
  (d) trx_layer_flux alone at nz = 2 and nz = 64: achieved bytes/s over the 2 n^2 elem B bytes of W and V

Events around warmed-up repeats; the median of --reps repeats is reported.  --kernel-only runs (d) alone, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python profiles/flux_timing.py --kernel-only).

    python profiles/flux_timing.py [--points 128] [--order 15] [--reps 5] [--out profiles/flux_timing.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torcwa_amd  # noqa: E402
from torcwa_amd.sweep import auto_chunk, solve_single_layer_sweep  # noqa: E402


def timed(fn, reps, dev):
    fn()                                             # warm-up: code objects, allocator
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def absorption_by_gemm(sim):
    """The per-layer drops with the GEMM and torch ops only: C E_i, then W (a + b), V (a - b) on an [n, 2] right-hand side."""
    eng, n, N = sim.engine, sim.n, sim.order_N
    E = sim._E_i[:, :, None].contiguous()
    inc = sim.incident_flux()
    out = []
    for l in range(sim.layer_N):
        c = eng.gemm(sim.C[0][l], E)[:, :, 0]
        cp, cm, kz, d = c[:, :n], c[:, n:], sim.kz_norm[l], sim.thickness[l]
        z = torch.stack((torch.zeros_like(d), d), dim=1)
        w = sim.omega[:, None, None]
        a = cp[:, :, None] * torch.exp(1j * w * kz[:, :, None] * z[:, None, :])
        b = cm[:, :, None] * torch.exp(1j * w * kz[:, :, None] * (d[:, None, None] - z[:, None, :]))
        e, h = eng.gemm(sim.E_eigvec[l], (a + b).contiguous()), eng.gemm(sim.H_eigvec[l], (a - b).contiguous())
        phi = torch.real(e[:, :N] * torch.conj(h[:, N:]) - e[:, N:] * torch.conj(h[:, :N])).sum(dim=1) / inc[:, None]
        out.append(phi[:, 0] - phi[:, 1])
    return torch.stack(out, dim=1)


def kernel_only(eng, n, B, reps, dev, dtype=torch.complex128):
    gen = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    W = torch.complex(rnd(B, n, n), rnd(B, n, n)).to(dtype).to(dev)
    V = torch.complex(rnd(B, n, n), rnd(B, n, n)).to(dtype).to(dev)
    cp, cm = (torch.complex(rnd(B, n), rnd(B, n)).to(dtype).to(dev) for _ in range(2))
    kz = torch.complex(rnd(B, n), rnd(B, n).abs() + 0.01).to(dtype).to(dev)
    om = torch.full((B,), 0.0118, dtype=torch.float64, device=dev)
    d = torch.full((B,), 300.0, dtype=torch.float64, device=dev)
    rows = []
    for nz in (2, 16, 64):
        z = (torch.linspace(0, 1, nz, dtype=torch.float64)[None, :] * d[:, None].cpu()).to(dev)
        med, lo, hi = timed(lambda: eng.layer_flux(W, V, cp, cm, kz, om, d, z), reps, dev)
        byts = 2.0 * n * n * W.element_size() * B
        rows.append({"dtype": str(dtype).replace("torch.", ""), "n": n, "B": B, "nz": nz, "ms": med, "ms_min": lo, "ms_max": hi,
                     "GBps_over_one_read_of_W_and_V": byts / med / 1e6, "passes_over_W_and_V": -(-nz // 16)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--order", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = torcwa_amd.engine.default_engine()
    order = [a.order, a.order]
    n = 2 * (2 * a.order + 1) ** 2
    lines, blob = [], {}
    if a.kernel_only:
        for r in kernel_only(eng, n, 32, a.reps, dev):
            print(json.dumps(r))
        return
    freq, grids, lam, eps_si = bench.make_inputs(2, np.arange(a.points), 300, dev)
    kw = dict(eps_in=1.46 ** 2, dtype=torch.complex64, precision="high", engine=eng, orders=[(0, 0)], polarization="xx")

    # (c) the sweep with and without absorption, and the HBM a point takes
    res = {}
    for label, extra in (("plain", {}), ("absorption", {"absorption": True})):
        chunk = auto_chunk(a.points, order, 1, "high", dev, dtype=torch.complex64, **extra)
        fn = lambda: solve_single_layer_sweep(freq, grids, 300., order, [300., 300.], chunk=chunk, **kw, **extra)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        med, lo, hi = timed(fn, max(2, a.reps // 2), dev)
        mat = n * n * 16.0
        res[label] = {"chunk": chunk, "ms": med, "ms_min": lo, "ms_max": hi, "peak_allocated_gb": torch.cuda.max_memory_allocated(dev) / 1e9,
                      "peak_reserved_gb": torch.cuda.max_memory_reserved(dev) / 1e9,
                      "matrices_per_point_allocated": torch.cuda.max_memory_allocated(dev) / mat / chunk,
                      "matrices_per_point_reserved": torch.cuda.max_memory_reserved(dev) / mat / chunk}
    blob["sweep"] = res
    lines.append("%d points, order [%d,%d] (n = %d), one patterned layer, complex64 I/O, precision high" % (a.points, a.order, a.order, n))
    for k, r in res.items():
        lines.append("  (c) sweep %-10s chunk %3d  %.1f ms (%.1f - %.1f)  peak %.1f GB allocated / %.1f GB reserved = %.1f / %.1f matrices per point"
                     % (k, r["chunk"], r["ms"], r["ms_min"], r["ms_max"], r["peak_allocated_gb"], r["peak_reserved_gb"],
                        r["matrices_per_point_allocated"], r["matrices_per_point_reserved"]))
    torch.cuda.empty_cache()

    # (a), (b) on one resident chunk
    B = res["absorption"]["chunk"]
    sim = torcwa_amd.BatchedRCWA(freq[:B], order, [300., 300.], dtype=torch.complex64, precision="high", engine=eng)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(300., grids[:B])
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1.0, 0.0])
    ta = timed(lambda: sim.absorption(), a.reps, dev)
    tb = timed(lambda: absorption_by_gemm(sim), a.reps, dev)
    diff = float((sim.absorption()["layers"] - absorption_by_gemm(sim)).abs().max())
    blob["absorption_ms"], blob["gemm_way_ms"], blob["max_difference"], blob["resident_points"] = ta, tb, diff, B
    lines.append("  (a) absorption() on %d resident points          %.2f ms (%.2f - %.2f)" % (B, *ta))
    lines.append("  (b) the same by Engine.gemm + torch reductions   %.2f ms (%.2f - %.2f)   max |difference| %.1e" % (*tb, diff))
    del sim
    torch.cuda.empty_cache()

    # (d) the kernel alone
    rows = kernel_only(eng, n, 32, a.reps, dev) + kernel_only(eng, n, 32, a.reps, dev, torch.complex64)
    blob["kernel"] = rows
    for r in rows:
        lines.append("  (d) trx_layer_flux %-10s B %d nz %2d: %.2f ms (%.2f - %.2f) = %.0f GB/s over one read of W and V (%d passes)"
                     % (r["dtype"], r["B"], r["nz"], r["ms"], r["ms_min"], r["ms_max"], r["GBps_over_one_read_of_W_and_V"], r["passes_over_W_and_V"]))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(blob) + "\n")


if __name__ == "__main__":
    main()
