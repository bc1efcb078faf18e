"""MI355X timing of the batched field maps: config 2's stack (one patterned a-Si:H layer of 300 nm on glass) at order [15,15] (n = 1922), B = 16
wavelengths spread over 400-700 nm, complex64 I/O with precision="high" (complex128 inside).  The solves are excluded: they are the same
for every way of reading the fields.

  (a) BatchedRCWA.field_xy on 256 x 256 in the patterned layer       against a loop of 16 rcwa.field_xy calls on 16 solved rcwa stacks
  (b) BatchedRCWA.field_xz on 256 x 200 through the whole stack      against a loop of 16 rcwa.field_xz calls
  (c) trx_layer_field alone at nz = 1, 16, 64, 200: achieved bytes/s over one read of W and V per pass of 16 depths (roofline: 6.29 TB/s
      measured stream rate, MI355X), and the alternative that forms the [n, nz] right-hand sides in torch and calls trx_gemm twice
  (d) trx_field_synth alone: the 256 x 256 map (28 real fp64 multiply-adds per point and harmonic for six components) and the 256 x 200 cut
      (24), against the vector fp64 peak (78.6 TFLOP/s: 256 CUs x 4 SIMDs x 16 lanes x 2 flops x 2.4 GHz) and against the output stream

Events around warmed-up repeats; the median (min - max) of --reps repeats is reported.

    python profiles/field_timing.py [--points 16] [--order 15] [--reps 5] [--out profiles/field_timing.txt]
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

FP64_VECTOR_PEAK = 256 * 4 * 16 * 2 * 2.4e9        # flop/s
STREAM_RATE = 6.29e12                              # bytes/s, measured float4 copy


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


def coeffs_by_gemm(sim, l, z):
    """ex, ey, hx, hy of layer l at z [B, nz] with the right-hand sides formed in torch and two trx_gemm calls (what fields.py does at B = 1)."""
    eng, n = sim.engine, sim.n
    c = eng.matvec(sim.C[0][l], sim._E_i[:, :, None])[:, :, 0]
    cp, cm, kz, d = c[:, :n], c[:, n:], sim.kz_norm[l], sim.thickness[l]
    w = sim.omega[:, None, None]
    a = cp[:, :, None] * torch.exp(1j * w * kz[:, :, None] * z[:, None, :])
    b = cm[:, :, None] * torch.exp(1j * w * kz[:, :, None] * (d[:, None, None] - z[:, None, :]))
    return eng.gemm(sim.E_eigvec[l], (a + b).contiguous()), eng.gemm(sim.H_eigvec[l], (a - b).contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=16)
    ap.add_argument("--order", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nxy", type=int, default=256)
    ap.add_argument("--nz", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = torcwa_amd.engine.default_engine()
    order, B, nxy, nzc = [a.order, a.order], a.points, a.nxy, a.nz
    N = (2 * a.order + 1) ** 2
    n = 2 * N
    idx = np.linspace(0, 127, B).round().astype(int)
    freq, grids, lam, _ = bench.make_inputs(2, idx, 300, dev)
    kw = dict(dtype=torch.complex64, precision="high", engine=eng)

    sim = torcwa_amd.BatchedRCWA(freq, order, [300., 300.], **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0.0, 0.0)
    sim.add_layer(300., grids)
    sim.solve_global_smatrix()
    sim.source_planewave(amplitude=[1.0, 0.0])
    singles = []
    for b in range(B):
        s = torcwa_amd.rcwa(float(freq[b]), order, [300., 300.], **kw)
        s.add_input_layer(eps=1.46 ** 2)
        s.set_incident_angle(0.0, 0.0)
        s.add_layer(300., grids[b])
        s.solve_global_smatrix()
        s.source_planewave(amplitude=[1.0, 0.0])
        singles.append(s)

    x = torch.linspace(0., 300., nxy, dtype=torch.float64, device=dev)
    y = torch.linspace(0., 300., nxy, dtype=torch.float64, device=dev)
    z = torch.linspace(-100., 400., nzc, dtype=torch.float64, device=dev)
    lines, blob = [], {}
    lines.append("%d wavelengths, order [%d,%d] (n = %d), one patterned layer of 300 nm on glass, complex64 I/O, precision high; solves excluded"
                 % (B, a.order, a.order, n))

    stack = lambda EH: torch.stack(list(EH[0]) + list(EH[1]))
    # (a) field_xy
    ta = timed(lambda: sim.field_xy(0, x, y, 150.0), a.reps, dev)
    tl = timed(lambda: [s.field_xy(0, x, y, 150.0) for s in singles], a.reps, dev)
    got = stack(sim.field_xy(0, x, y, 150.0))
    ref = torch.stack([stack(s.field_xy(0, x, y, 150.0)) for s in singles], dim=1)
    dxy = float((got - ref).abs().max() / ref.abs().max())
    blob["field_xy"] = {"batched_ms": ta, "rcwa_loop_ms": tl, "max_rel_difference": dxy}
    lines.append("  (a) field_xy %d x %d, patterned layer: batched %.2f ms (%.2f - %.2f);  loop of %d rcwa.field_xy %.2f ms (%.2f - %.2f);  x%.1f;  "
                 "max difference / max |field| %.1e" % (nxy, nxy, *ta, B, *tl, tl[0] / ta[0], dxy))
    # (b) field_xz
    tb = timed(lambda: sim.field_xz(x, z, 150.0), a.reps, dev)
    tl = timed(lambda: [s.field_xz(x, z, 150.0) for s in singles], a.reps, dev)
    got = stack(sim.field_xz(x, z, 150.0))
    ref = torch.stack([stack(s.field_xz(x, z, 150.0)) for s in singles], dim=1)
    dxz = float((got - ref).abs().max() / ref.abs().max())
    nin = int(((z >= 0) & (z <= 300.)).sum())
    blob["field_xz"] = {"batched_ms": tb, "rcwa_loop_ms": tl, "max_rel_difference": dxz, "samples_in_layer": nin}
    lines.append("  (b) field_xz %d x %d (%d depths in the layer): batched %.2f ms (%.2f - %.2f);  loop of %d rcwa.field_xz %.2f ms (%.2f - %.2f);  x%.1f;  "
                 "max difference / max |field| %.1e" % (nxy, nzc, nin, *tb, B, *tl, tl[0] / tb[0], dxz))
    del singles, ref, got
    torch.cuda.empty_cache()

    # (c) trx_layer_field alone, and the right-hand sides in torch + trx_gemm
    W, V, kz, d = sim.E_eigvec[0], sim.H_eigvec[0], sim.kz_norm[0], sim.thickness[0]
    c = eng.matvec(sim.C[0][0], sim._E_i[:, :, None])[:, :, 0]
    cp, cm = c[:, :n].contiguous(), c[:, n:].contiguous()
    kx, ky = sim._field_k()
    rows = []
    for nz in (1, 16, 64, nzc):
        zz = torch.linspace(0., 300., nz, dtype=torch.float64, device=dev)[None, :].expand(B, -1).contiguous()
        tk = timed(lambda: eng.layer_field(W, V, cp, cm, kz, sim.omega, d, zz, kx, ky), a.reps, dev)
        tg = timed(lambda: coeffs_by_gemm(sim, 0, zz), a.reps, dev)
        passes = -(-nz // 16)
        byts = 2.0 * n * n * W.element_size() * B * passes
        rows.append({"nz": nz, "layer_field_ms": tk, "gemm_way_ms": tg, "passes": passes, "GBps": byts / tk[0] / 1e6,
                     "fraction_of_stream_rate": byts / (tk[0] * 1e-3) / STREAM_RATE})
        lines.append("  (c) trx_layer_field nz %3d: %.2f ms (%.2f - %.2f) = %.0f GB/s over %d pass(es) of W and V = %.0f %% of 6.29 TB/s;  "
                     "right-hand sides in torch + 2 trx_gemm: %.2f ms (%.2f - %.2f)"
                     % (nz, *tk, rows[-1]["GBps"], passes, 100 * rows[-1]["fraction_of_stream_rate"], *tg))
    blob["layer_field"] = rows

    # (d) trx_field_synth alone
    cdt = torch.complex128
    gen = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.complex(torch.randn(*s, generator=gen, dtype=torch.float64), torch.randn(*s, generator=gen, dtype=torch.float64)).to(cdt).to(dev)
    coef_map, coef_cut = rnd(B, 6, N, 1), rnd(B, 6, N, nzc)
    one = torch.tensor([150.0], dtype=torch.float64, device=dev)
    tm = timed(lambda: eng.field_synth(coef_map, kx, ky, sim.omega, x, y), a.reps, dev)
    tc = timed(lambda: eng.field_synth(coef_cut, kx, ky, sim.omega, x, one), a.reps, dev)
    fm, fc = 2.0 * 28 * N * nxy * nxy * B, 2.0 * 24 * N * nxy * nzc * B
    om, oc = 6.0 * nxy * nxy * 16 * B, 6.0 * nxy * nzc * 16 * B
    blob["field_synth"] = {"map_ms": tm, "cut_ms": tc, "map_TFLOPs": fm / tm[0] / 1e9, "cut_TFLOPs": fc / tc[0] / 1e9,
                           "map_out_GBps": om / tm[0] / 1e6, "cut_out_GBps": oc / tc[0] / 1e6}
    lines.append("  (d) trx_field_synth map %d x %d, 6 components: %.2f ms (%.2f - %.2f) = %.1f TFLOP/s fp64 = %.0f %% of the 78.6 vector peak;  "
                 "output stream %.0f GB/s" % (nxy, nxy, *tm, fm / tm[0] / 1e9, 100 * fm / (tm[0] * 1e-3) / FP64_VECTOR_PEAK, om / tm[0] / 1e6))
    lines.append("  (d) trx_field_synth cut %d x %d, 6 components: %.2f ms (%.2f - %.2f) = %.1f TFLOP/s fp64 = %.0f %% of the 78.6 vector peak;  "
                 "output stream %.0f GB/s" % (nxy, nzc, *tc, fc / tc[0] / 1e9, 100 * fc / (tc[0] * 1e-3) / FP64_VECTOR_PEAK, oc / tc[0] / 1e6))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(blob) + "\n")


if __name__ == "__main__":
    main()
