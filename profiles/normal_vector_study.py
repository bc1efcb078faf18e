"""CPU study behind the defaults of fourier_rule="normal" (blur width sigma and the fallback where the structure tensor is unresolvable).

Runs on the CPU oracle (oracle/rcwa_oracle.py) with the normal-vector tensor swapped into Q, exactly as tests/test_normal_vector.py does;
no GPU is needed.  Output: profiles/normal_vector.txt.

    python profiles/normal_vector_study.py
"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rcwa_oracle as orc  # noqa: E402

_conv = orc.conv_matrix

SYMMETRIC = "--plain" not in sys.argv     # {D, C} = (D C + C D)/2 (the library's form); --plain: the product D C
TAU = 1e-3          # coherence floor (lambda1 - lambda2) / (lambda1 + lambda2) below which the direction counts as unresolvable


def nv_products(g, sigma, hx=1.0, hy=1.0, fallback="zero"):
    """(Nx^2, Nx Ny, Ny^2) of the smoothed principal direction of the structure tensor of grid g (numpy restatement of the kernel)."""
    g = np.asarray(g, dtype=np.complex128)
    gx = (np.roll(g, -1, 0) - np.roll(g, 1, 0)) / (2 * hx)
    gy = (np.roll(g, -1, 1) - np.roll(g, 1, 1)) / (2 * hy)
    J = [np.abs(gx) ** 2, np.real(gx * np.conj(gy)), np.abs(gy) ** 2]
    if sigma > 0:
        R = int(math.ceil(3 * sigma))
        k = np.arange(-R, R + 1)
        w = np.exp(-k * k / (2.0 * sigma * sigma))
        w /= w.sum()
        for ax in (1, 0):
            J = [sum(w[i] * np.roll(c, -k[i], ax) for i in range(len(k))) for c in J]
    d, o = J[0] - J[2], 2 * J[1]
    r = np.hypot(d, o)
    ok = r > TAU * (J[0] + J[2])
    rs = np.where(ok, r, 1.0)
    fb = (0.0, 0.0, 0.0) if fallback == "zero" else (1.0, 0.0, 0.0)
    return [np.where(ok, v, f) for v, f in zip((0.5 * (1 + d / rs), 0.5 * o / rs, 0.5 * (1 - d / rs)), fb)]


def radial_products(nx, ny, cx, cy):
    x = (np.arange(nx) + 0.5) / nx - cx
    y = (np.arange(ny) + 0.5) / ny - cy
    X, Y = np.meshgrid(x, y, indexing="ij")
    r2 = X * X + Y * Y
    r2 = np.where(r2 > 0, r2, 1.0)
    return [X * X / r2, X * Y / r2, Y * Y / r2]


def nv_tensor(grid, order, prods):
    E = _conv(grid, order)
    R = _conv(1 / grid, order)
    D = E - torch.linalg.inv(R)
    C = [_conv(torch.as_tensor(p, dtype=torch.float64), order) for p in prods]
    if SYMMETRIC:
        S = [(D @ c + c @ D) / 2 for c in C]
        return E - S[0], -S[1], E - S[2]
    return E - D @ C[0], -(D @ C[1]), E - D @ C[2]


def solve(grid, order, prods):
    conv0, pq0 = orc.conv_matrix, orc.pq_patterned

    def conv(gr, o):
        E = conv0(gr, o)
        if prods is not None and gr is grid:
            E._nv = nv_tensor(grid, o, prods)
        return E

    def pq(E, M, kx, ky):
        P, Q = pq0(E, M, kx, ky)
        if hasattr(E, "_nv"):
            Exx, Exy, Eyy = E._nv
            N = E.shape[0]
            Q = Q.clone()
            Q[:N, :N] -= Exy
            Q[:N, N:] += E - Eyy
            Q[N:, :N] += Exx - E
            Q[N:, N:] += Exy
        return P, Q

    orc.conv_matrix, orc.pq_patterned = conv, pq
    try:
        s, _, S, _ = orc.solve_stack(1.0, order, [0.5, 0.5], [(0.3, grid)], eps_in=1.0, eps_out=2.25, inc_ang=0.3, azi_ang=0.4)
    finally:
        orc.conv_matrix, orc.pq_patterned = conv0, pq0
    return np.array([float(orc.s_parameters(s, S, [[0, 0]], port=p, polarization=q).abs()[0] ** 2)
                     for p in ("transmission", "reflection") for q in ("xx", "xy", "yx", "yy")])


def shapes(n=256):
    x = (np.arange(n) + 0.5) / n * 0.5
    X, Y = np.meshgrid(x, x, indexing="ij")
    metal = (0.22 + 6.71j) ** 2
    out = {}
    out["dielectric disk (eps 12, r 0.18)"] = (np.where((X - .25) ** 2 + (Y - .25) ** 2 < .18 ** 2, 12.0, 1.0), 12.0)
    out["metal disk (eps (0.22+6.71i)^2, r 0.18)"] = (np.where((X - .25) ** 2 + (Y - .25) ** 2 < .18 ** 2, metal, 1.0), metal)
    c, s_ = math.cos(0.3), math.sin(0.3)
    u, v = (X - .25) * c + (Y - .25) * s_, -(X - .25) * s_ + (Y - .25) * c
    out["ellipse (eps 12, 0.2 x 0.1, 0.3 rad)"] = (np.where((u / .2) ** 2 + (v / .1) ** 2 < 1, 12.0, 1.0), 12.0)
    c, s_ = math.cos(math.pi / 6), math.sin(math.pi / 6)
    u, v = (X - .25) * c + (Y - .25) * s_, -(X - .25) * s_ + (Y - .25) * c
    out["rotated square (eps 12, side 0.25, 30 deg)"] = (np.where((np.abs(u) < .125) & (np.abs(v) < .125), 12.0, 1.0), 12.0)
    two = ((X - .125) ** 2 + (Y - .25) ** 2 < .125 ** 2) | ((X - .375) ** 2 + (Y - .25) ** 2 < .125 ** 2)
    out["two touching disks (eps 12, r 0.125)"] = (np.where(two, 12.0, 1.0), 12.0)
    return out


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    n = 256
    sigmas = [3.0, 6.0, 12.0]
    orders = [[5, 5], [7, 7], [9, 9]]
    ref_order = [13, 13]
    lines = []
    p = lambda s: (print(s, flush=True), lines.append(s))
    p("Normal-vector factorisation: CPU study of the field construction (profiles/normal_vector_study.py, CPU oracle with the NV tensor in Q)")
    p("cell 0.5 x 0.5, lambda 1, depth 0.3, air over eps_out 2.25, inc 0.3, azi 0.4, %d x %d binary grid" % (n, n))
    p("metric: worst | |S|^2 - |S_ref|^2 | over the 8 zeroth-order port / polarisation pairs")
    p("reference: NV (grid field, sigma 6, fallback zero) at order %s; 'ref spread' = the same with sigma 12 (reference uncertainty)" % ref_order)
    p("fallback 'zero': N N^T = 0 where the coherence (l1-l2)/(l1+l2) of the blurred tensor is <= %g (local Laurent); '(1,0)': N = x^" % TAU)
    p("")
    t0 = time.time()
    for name, (g, _) in shapes(n).items():
        grid = torch.as_tensor(g)
        ref = solve(grid, ref_order, nv_products(g, 6.0))
        ref2 = solve(grid, ref_order, nv_products(g, 12.0))
        p("%s   ref spread %.1e" % (name, np.abs(ref - ref2).max()))
        p("  %-28s %s" % ("variant", "  ".join("%9s" % str(o) for o in orders)))
        rows = [("laurent", None)]
        if "disk" in name and "two" not in name:
            rows.append(("radial (analytic)", radial_products(n, n, 0.5, 0.5)))
        for sg in sigmas:
            rows.append(("sigma %g, zero" % sg, nv_products(g, sg)))
        rows.append(("sigma 6, (1,0)", nv_products(g, 6.0, fallback="x")))
        for label, prods in rows:
            errs = [np.abs(solve(grid, o, prods) - ref).max() for o in orders]
            p("  %-28s %s" % (label, "  ".join("%9.1e" % e for e in errs)))
        p("")
    p("wall time %.0f s" % (time.time() - t0))
    with open(os.path.join(ROOT, "profiles", "normal_vector.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
