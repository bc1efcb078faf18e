#!/usr/bin/env python3
"""Forward + adjoint step of one patterned mirror-symmetric layer with and without the folded eigenproblem (symmetry="xy", symmetry_grad=True).

The workload is config 5's optimiser step (bench.py: 700 x 300 nm cell, smooth random density, silicon at 532 nm, FoM = power into the +1
order, complex128, stable eigen-gradient) with the density symmetrised under both mirrors.  Per order: every mode is warmed up once, then the
two modes alternate for --reps timed steps each (host clock around a step that ends in a device synchronise, profiling off); a last step per
mode runs with the library's event tags and the Engine's phase brackets on and reports trx_eig, trx_eig_backward (event pairs around the
Engine calls) and the four sym_* tags.  The two paths are compared on the FoM and on the mirror average of the density gradient.

    python profiles/symmetry_grad_timing.py [--orders 15,25] [--reps 3]

Results: profiles/symmetry_grad_timing.txt.
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

EPS_SI = 12.011610263133004 + 0.525912014756j


def density(device, nx=700, ny=300):
    rho = torch.rand(nx, ny, generator=torch.Generator().manual_seed(333), dtype=torch.float64)
    kx, ky = torch.fft.fftfreq(nx, d=1.0)[:, None], torch.fft.fftfreq(ny, d=1.0)[None, :]
    blur = torch.exp(-2 * (np.pi * 20.0) ** 2 * (kx ** 2 + ky ** 2) / 4)
    rho = torch.real(torch.fft.ifft2(torch.fft.fft2(rho) * blur)).clamp(0, 1)
    return mirror_average(rho).to(device)


def mirror_average(g):
    return (g + torch.flip(g, dims=[0]) + torch.flip(g, dims=[1]) + torch.flip(g, dims=[0, 1])) / 4


def step(eng, rho0, order, kw):
    import torcwa_amd
    rho = rho0.clone().requires_grad_(True)
    sim = torcwa_amd.rcwa(freq=1 / 532., order=[order, order], L=[700., 300.], dtype=torch.complex128, device=rho0.device, stable_eig_grad=True,
                          engine=eng, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(inc_ang=0., azi_ang=0.)
    sim.add_layer(thickness=300., eps=rho * EPS_SI + (1. - rho))
    sim.solve_global_smatrix()
    t = [sim.S_parameters(orders=[1, 0], direction="forward", port="transmission", polarization=p, ref_order=[0, 0]) for p in ("xx", "yx", "xy", "yy")]
    fom = sum(torch.abs(v) ** 2 for v in t).sum()
    fom.backward()
    res = sim.symmetry_residual[0]
    return float(fom.detach()), rho.grad.detach(), (None if res is None else float(res))


def bracket(eng, name, acc):
    """Event pairs around an Engine method (summed per step into acc[name])."""
    plain = getattr(eng, name)

    def wrapped(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            return plain(*a, **k)
        finally:
            e1.record()
            acc.setdefault(name, []).append((e0, e1))
    setattr(eng, name, wrapped)
    return plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default="15,25")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torcwa_amd
    eng = torcwa_amd.Engine()                      # no GPU: TrxError, nothing is measured
    rho0 = density(eng.device)
    modes = [("symmetry=None", {}), ('symmetry="xy", symmetry_grad=True', dict(symmetry="xy", symmetry_grad=True))]
    for order in [int(v) for v in args.orders.split(",")]:
        n = 2 * (2 * order + 1) ** 2
        print(f"order [{order},{order}], n = {n}, complex128, one patterned layer, forward + backward", flush=True)
        out = {}
        for name, kw in modes:
            out[name] = step(eng, rho0, order, kw)                   # warm-up of every shape the timed window uses
        torch.cuda.synchronize()
        times = {name: [] for name, _ in modes}
        for _ in range(args.reps):
            for name, kw in modes:                                    # alternating: both modes see the same neighbours
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(eng, rho0, order, kw)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        for name, kw in modes:
            ts = sorted(times[name])
            print(f"  {name}: median {1e3 * ts[len(ts) // 2]:.1f} ms per step (steps: {', '.join(f'{1e3 * t:.1f}' for t in times[name])} ms)", flush=True)
            acc = {}
            plain = [(m, bracket(eng, m, acc)) for m in ("eig", "eig_backward")]
            eng.lib.prof_reset()
            eng.lib.prof_enable(1)
            eng.profile_phases = True
            eng.phase_report()
            step(eng, rho0, order, kw)
            phases = eng.phase_report()
            eng.profile_phases = False
            eng.lib.prof_enable(0)
            for m, fn in plain:
                setattr(eng, m, fn)
            for m, evs in acc.items():
                print(f"    {sum(e0.elapsed_time(e1) for e0, e1 in evs):9.1f} ms  Engine.{m}: {len(evs)} calls")
            for tag in range(64):
                tname = eng.lib.prof_tag_name(tag).decode()
                if tname == "?":
                    break
                if tname.startswith("sym_"):
                    buf = (ctypes.c_double * 7)()
                    eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                    if buf[1] > 0:
                        ms = buf[4] / buf[1] * buf[0]
                        print(f"    {ms:9.2f} ms  library tag {tname}: {buf[0]:.0f} launches, model traffic {buf[6] / 1e9:.2f} GB -> {buf[6] / 1e9 / ms:.2f} TB/s")
            for pname, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
                print(f"    {ms:9.1f} ms  phase {pname}")
        (f0, g0, _), (f1, g1, res) = out[modes[0][0]], out[modes[1][0]]
        a0, a1 = mirror_average(g0), mirror_average(g1)
        med = [sorted(times[name])[len(times[name]) // 2] for name, _ in modes]
        print(f"  step time folded / unfolded = {med[1] / med[0]:.3f}; |FoM difference| / FoM = {abs(f1 - f0) / abs(f0):.2e}; mirror-averaged gradient: "
              f"max difference / max = {float((a1 - a0).abs().max() / a0.abs().max()):.2e}; raw gradient: {float((g1 - g0).abs().max() / g0.abs().max()):.2e}; "
              f"symmetry_residual {res:.2e}", flush=True)


if __name__ == "__main__":
    main()
