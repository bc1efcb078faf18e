#!/usr/bin/env python3
"""Forward + adjoint step of one patterned mirror-symmetric layer three ways: the unfolded differentiable path, the folded eigenproblem
(symmetry="xy", symmetry_grad=True) and the differentiable sector solve (symmetry_sector=True, sector_grad=True).

The workload and the shapes are those of profiles/symmetry_grad_timing.py: config 5's optimiser step (bench.py: 700 x 300 nm cell, smooth random
density symmetrised under both mirrors, silicon at 532 nm, complex128, stable eigen-gradient), with two objectives: the power into the +1 order
summed over the four polarisation pairs (x and y sources: two sectors) and its xx term alone (one sector).  Per order and objective every mode
is warmed up once, then the modes alternate for --reps timed steps each (a HIP event pair around a step, profiling off; the median is
reported); a last step per mode runs with the library's event tags and the Engine's phase brackets on and reports the sym_* tags -- for the
sector mode the kernel time and the achieved bandwidth of trx_sym_fold_pairs_backward and trx_sym_fold_pair_bd_backward against their traffic
models.  The sector path's raw density gradient is compared with the mirror average of the unfolded path's.

    python profiles/sector_grad_timing.py [--orders 15,25] [--reps 3]

Results: profiles/sector_grad_timing.txt.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.symmetry_grad_timing import EPS_SI, density, mirror_average  # noqa: E402

POLS = {"four polarisation pairs": ("xx", "yx", "xy", "yy"), "xx alone": ("xx",)}


def step(eng, rho0, order, kw, pols):
    import torcwa_amd
    rho = rho0.clone().requires_grad_(True)
    sim = torcwa_amd.BatchedRCWA(1 / 532., [order, order], [700., 300.], dtype=torch.complex128, engine=eng, stable_eig_grad=True, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(300., rho * EPS_SI + (1. - rho))
    t = [sim.solve_S_parameters([[1, 0]], direction="forward", port="transmission", polarization=p, ref_order=[0, 0]) for p in pols]
    fom = sum(torch.abs(v) ** 2 for v in t).sum()
    fom.backward()
    return float(fom.detach()), rho.grad.detach()


def bd_backward(eng, order, reps=20):
    """trx_sym_fold_pair_bd_backward on its own: this workload's half-spaces and Vf^-1 carry no gradient, so a step never launches it.  One
    warm-up, then `reps` launches of each pair (k, k) and (k, k') of the order's plan under the library's tag."""
    from torcwa_amd import lattice, symmetry
    plan = symmetry.build_plan(lattice.rect_orders(order, order), "xy", 699, 700, 299, 300)
    pairs = [(k, k) for k in range(4)] + [(k, symmetry.opposite_block(4, k)) for k in range(4)]
    G = {p: torch.randn(1, plan.sizes[p[0]], plan.sizes[p[1]], dtype=torch.complex128, device=eng.device) for p in pairs}
    for p in pairs:
        eng.sym_fold_pair_bd_backward(G[p], plan, *p)
    eng.lib.prof_reset()
    eng.lib.prof_enable(1)
    for _ in range(reps):
        for p in pairs:
            eng.sym_fold_pair_bd_backward(G[p], plan, *p)
    torch.cuda.synchronize()
    eng.lib.prof_enable(0)
    for tag in range(64):
        tname = eng.lib.prof_tag_name(tag).decode()
        if tname == "?":
            break
        if tname == "sym_fold_pair_bd_backward":
            buf = (ctypes.c_double * 7)()
            eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
            ms = buf[4] / buf[1]
            print(f"order [{order},{order}]: library tag {tname} alone, complex128, batch 1, N = {plan.n // 2}:{buf[0]:.0f} launches, {1e3 * ms:.1f} us per launch, model traffic "
                  f"{buf[6] / buf[0] / 1e6:.3f} MB per launch -> {buf[6] / buf[0] / 1e9 / ms:.3f} TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default="15,25")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torcwa_amd
    eng = torcwa_amd.Engine()                      # no GPU: TrxError, nothing is measured
    rho0 = density(eng.device)
    modes = [("symmetry=None", {}), ('symmetry="xy", symmetry_grad=True', dict(symmetry="xy", symmetry_grad=True)),
             ('symmetry="xy", symmetry_sector=True, sector_grad=True', dict(symmetry="xy", keep_coupling=False, symmetry_sector=True, sector_grad=True))]
    for order in [int(v) for v in args.orders.split(",")]:
        n = 2 * (2 * order + 1) ** 2
        bd_backward(eng, order)
        for what, pols in POLS.items():
            print(f"order [{order},{order}], n = {n}, complex128, one patterned layer, forward + backward, objective: {what}", flush=True)
            out = {name: step(eng, rho0, order, kw, pols) for name, kw in modes}          # warm-up of every shape the timed window uses
            torch.cuda.synchronize()
            times = {name: [] for name, _ in modes}
            for _ in range(args.reps):
                for name, kw in modes:                                                  # alternating: the modes see the same neighbours
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    step(eng, rho0, order, kw, pols)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            med = {}
            for name, kw in modes:
                ts = sorted(times[name])
                med[name] = ts[len(ts) // 2]
                print(f"  {name}: median {med[name]:.1f} ms per step (steps: {', '.join(f'{t:.1f}' for t in times[name])} ms)", flush=True)
                eng.lib.prof_reset()
                eng.lib.prof_enable(1)
                eng.profile_phases = True
                eng.phase_report()
                step(eng, rho0, order, kw, pols)
                phases = eng.phase_report()
                eng.profile_phases = False
                eng.lib.prof_enable(0)
                for tag in range(64):
                    tname = eng.lib.prof_tag_name(tag).decode()
                    if tname == "?":
                        break
                    if tname.startswith("sym_"):
                        buf = (ctypes.c_double * 7)()
                        eng.lib.check(eng.lib.prof_get(tag, ctypes.addressof(buf)))
                        if buf[1] > 0:
                            ms = buf[4] / buf[1] * buf[0]
                            print(f"    {ms:9.3f} ms  library tag {tname}: {buf[0]:.0f} launches, model traffic {buf[6] / 1e9:.3f} GB -> "
                                  f"{buf[6] / 1e9 / ms:.2f} TB/s")
                for pname, ms in sorted(phases.items(), key=lambda kv: -kv[1]):
                    print(f"    {ms:9.1f} ms  phase {pname}")
            (f0, g0), (f1, g1), (f2, g2) = (out[name] for name, _ in modes)
            a0 = mirror_average(g0)
            u, s, c = (med[name] for name, _ in modes)
            print(f"  step time: sector / unfolded = {c / u:.3f}, sector / symmetry_grad = {c / s:.3f}, symmetry_grad / unfolded = {s / u:.3f}; "
                  f"sector |FoM difference| / FoM = {abs(f2 - f0) / abs(f0):.2e}; RAW sector gradient against the mirror-averaged unfolded one: "
                  f"max difference / max = {float((g2 - a0).abs().max() / a0.abs().max()):.2e}; its asymmetry "
                  f"{float((g2 - mirror_average(g2)).abs().max() / g2.abs().max()):.2e}", flush=True)


if __name__ == "__main__":
    main()
