"""CPU study: accuracy per harmonic of circular against rectangular truncation, and of a hexagonal lattice solved natively against its
rectangular supercell, under Laurent's rule and the normal-vector rule.

Runs on the CPU oracle (oracle/rcwa_oracle.py): its pq_patterned, modes_patterned, layer_smatrix and redheffer, fed with the kx, ky of
an arbitrary lattice and order list and with a restated gather of the convolution matrix (out[i, j] = c[m_i - m_j, n_i - n_j] of the full
FFT); the normal-vector tensor goes into Q as in profiles/normal_vector_study.py.  No GPU is needed.  Output: profiles/lattice.txt.

  1. the Example-1 a-Si:H rectangle (300 x 300 nm cell, 180 x 100 nm block, 300 nm thick, glass input, lambda 532 nm, normal incidence):
     rectangular [o, o] against circular truncation; the normal rule with the field derived from the grid (sigma = 6 cells);
  2. a hexagonal array of eps = 12 disks (r = 0.3 a, t = 0.5 a, air on both sides, lambda = 1.6 a, normal incidence): the native lattice
     with circular truncation against the a x sqrt(3) a supercell with rectangular truncation [o, round(sqrt(3) o)] (the box that grows
     like a disk); the normal rule with the analytic radial field.

Errors are those of T00 (power into the zeroth transmitted order) and R_total (power into all propagating reflected orders), x-polarised
incidence, against the normal rule at the largest native circular set of each case.

    python profiles/lattice_study.py [--quick]
"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from oracle import rcwa_oracle as orc  # noqa: E402
from normal_vector_study import nv_products  # noqa: E402
from torcwa_amd.lattice import circular_orders, reciprocal, rect_orders  # noqa: E402

QUICK = "--quick" in sys.argv
TOLS = (2e-2, 1e-2, 3e-3, 1e-3, 1e-4)
S3 = math.sqrt(3.0)
CDT = torch.complex128


def gather(coef, mn):
    """Convolution matrix of an order list from the full-FFT coefficients coef = fft2(g) / (n1 n2)."""
    n1, n2 = coef.shape
    m, n = torch.as_tensor(mn[:, 0]), torch.as_tensor(mn[:, 1])
    return coef[(m[:, None] - m[None, :]) % n1, (n[:, None] - n[None, :]) % n2]


def coefs(g):
    g = torch.as_tensor(g, dtype=CDT)
    return torch.fft.fft2(g) / (g.shape[0] * g.shape[1])


def solve(L, mn, grid, lam, d, eps_in, eps_out, prods=None):
    """(T00, R_total) of one patterned layer between two half spaces, x-polarised normal incidence."""
    b = reciprocal(L)
    f = 1.0 / lam
    G = torch.as_tensor(mn @ b, dtype=torch.float64) / f
    kx, ky = G[:, 0].to(CDT), G[:, 1].to(CDT)
    N = len(mn)
    E = gather(coefs(grid), mn)
    M = torch.eye(N, dtype=CDT)
    P, Q = orc.pq_patterned(E, M, kx, ky)
    if prods is not None:                      # normal-vector tensor in Q (D = [eps] - [1/eps]^-1, symmetrised products)
        D = E - torch.linalg.inv(gather(coefs(1 / torch.as_tensor(grid, dtype=CDT)), mn))
        C = [gather(coefs(p), mn) for p in prods]
        S = [(D @ c + c @ D) / 2 for c in C]
        Exx, Exy, Eyy = E - S[0], -S[1], E - S[2]
        Kx, Ky = torch.diag(kx), torch.diag(ky)
        Q = torch.cat((torch.cat((-Kx @ Ky - Exy, Kx @ Kx - Eyy), 1), torch.cat((Exx - Ky @ Ky, Ky @ Kx + Exy), 1)), 0)
    kz, W = orc.modes_patterned(P, Q)
    Vf = orc._halfspace_V(kx, ky, 1.0)
    lay = orc.layer_smatrix(orc.Layer(thickness=d, E=E, M=M, P=P, Q=Q, kz=kz, W=W), Vf, 2 * orc.PI_REF * f)

    def half(epsv, side):
        V = orc._halfspace_V(kx, ky, torch.tensor(epsv, dtype=CDT))
        T = torch.linalg.inv(Vf + V)
        Dd = Vf - V
        return [2 * (T @ V), -(T @ Dd), T @ Dd, 2 * (T @ Vf)] if side == "in" else [2 * (T @ Vf), T @ Dd, -(T @ Dd), 2 * (T @ V)]

    S, _ = orc.redheffer(half(eps_in, "in"), lay.S, [[], []], [[], []])
    S, _ = orc.redheffer(S, half(eps_out, "out"), [[], []], [[], []])
    i0 = int(np.flatnonzero((mn[:, 0] == 0) & (mn[:, 1] == 0))[0])
    e = torch.zeros(2 * N, dtype=CDT)
    e[i0] = 1.0

    def power(v, epsv):
        """z-flux of every harmonic (kz |E|^2 of a plane wave, E_z from div D = 0), per unit incident flux; 0 when evanescent."""
        kz = torch.sqrt(epsv - kx ** 2 - ky ** 2)
        ex, ey = v[:N], v[N:]
        ez = -(kx * ex + ky * ey) / kz
        prop = torch.abs(torch.imag(kz)) < 1e-12
        p = torch.real(kz) * (ex.abs() ** 2 + ey.abs() ** 2 + ez.abs() ** 2)
        return torch.where(prop, p, torch.zeros_like(p)) / math.sqrt(eps_in)

    t, r = power(S[0] @ e, eps_out), power(S[1] @ e, eps_in)
    return float(t[i0]), float(r.sum())


def first_n(rows, tol):
    """Smallest n from which both errors stay at or below tol for every larger n of the sweep."""
    best = None
    for n, eT, eR in sorted(rows, reverse=True):
        if max(eT, eR) > tol:
            break
        best = n
    return best


def report(out, title, series, ref):
    out.append(title)
    out.append("  converged (normal rule, largest native circular set): T00 = %.8f, R_total = %.8f" % ref)
    table = {}
    for name, pts in series.items():
        out.append("  %s" % name)
        out.append("      N      n   err T00    err R_total")
        rows = []
        for N, (T, R) in pts:
            eT, eR = abs(T - ref[0]), abs(R - ref[1])
            rows.append((2 * N, eT, eR))
            out.append("  %5d  %5d   %.2e   %.2e" % (N, 2 * N, eT, eR))
        table[name] = [first_n(rows, tol) for tol in TOLS]
    out.append("  n needed (both errors <= tol from there on; '-' = not reached in the sweep):")
    out.append("    %-50s %s" % ("", "".join("%8s" % ("%.0e" % t) for t in TOLS)))
    for name, ns in table.items():
        out.append("    %-50s %s" % (name, "".join("%8s" % (v or "-") for v in ns)))
    out.append("")
    sys.stdout.write("\n".join(out[-3 - len(series):]) + "\n")
    sys.stdout.flush()
    return table


def case1(out):
    L = [300.0, 300.0]
    n = 256
    dens = orc.rectangle_density(n, n, 300., 300., 180., 100., 150., 150.)
    grid = (dens * (12.0116 + 0.5259j) + (1. - dens)).to(CDT)
    prods = nv_products(grid.numpy(), 6.0, 300. / n, 300. / n)
    args = (grid, 532.0, 300.0, 1.46 ** 2, 1.0)
    ref = solve(L, circular_orders(L, n_harmonics=450 if QUICK else 900), *args, prods=prods)
    series = {}
    rect = range(2, 9 if QUICK else 13)
    circ = [13, 29, 49, 81, 113, 149, 197, 253, 317, 377, 441, 529][: (7 if QUICK else 12)]
    for rule, pr in (("laurent", None), ("normal", prods)):
        series["rectangular [o,o], %s" % rule] = [(len(rect_orders(o, o)), solve(L, rect_orders(o, o), *args, prods=pr)) for o in rect]
        series["circular, %s" % rule] = [(len(mn), solve(L, mn, *args, prods=pr)) for mn in (circular_orders(L, n_harmonics=k) for k in circ)]
    return report(out, "1. Example-1 a-Si:H rectangle, rectangular lattice 300 x 300 nm, grid 256 x 256", series, ref)


def case2(out):
    from torcwa_amd import lattice_geometry
    HEX = [[1.0, 0.0], [0.5, S3 / 2]]
    SC = [[1.0, 0.0], [0.0, S3]]
    M = 64
    geo = lattice_geometry(HEX[0], HEX[1], 2 * M, M, 200.0, dtype=torch.float64, device=torch.device("cpu"))
    gh = (1.0 + 11.0 * geo.circle(0.3, 0.0, 0.0)).numpy()
    u, v = geo._disp(0.0, 0.0)
    r2 = u * u + v * v
    ph = [(u * u / r2).numpy(), (u * v / r2).numpy(), (v * v / r2).numpy()]
    i, j = np.meshgrid(np.arange(2 * M), np.arange(2 * M), indexing="ij")
    pick = ((i - j) % (2 * M), j % M)                     # the supercell on the same samples
    gs = gh[pick]
    ps = [p[pick] for p in ph]
    args = (1.6, 0.5, 1.0, 1.0)
    ref = solve(HEX, circular_orders(HEX, n_harmonics=420 if QUICK else 800), gh, *args, prods=ph)
    series = {}
    circ = [19, 37, 61, 91, 127, 169, 217, 271, 331, 397, 469][: (7 if QUICK else 11)]
    boxes = range(1, 6 if QUICK else 9)
    for rule, (qh, qs) in (("laurent", (None, None)), ("normal", (ph, ps))):
        series["hexagonal, circular, %s" % rule] = [(len(mn), solve(HEX, mn, gh, *args, prods=qh))
                                                    for mn in (circular_orders(HEX, n_harmonics=k) for k in circ)]
        series["supercell, rectangular [o, round(sqrt3 o)], %s" % rule] = [
            (len(rect_orders(o, round(S3 * o))), solve(SC, rect_orders(o, round(S3 * o)), gs, *args, prods=qs)) for o in boxes]
    return report(out, "2. hexagonal array of eps = 12 disks (r 0.3 a, t 0.5 a, lambda 1.6 a), hexagonal grid 128 x 64 / supercell 128 x 128",
                  series, ref)


def main():
    t0 = time.time()
    out = ["Accuracy per harmonic on the CPU oracle (complex128)%s" % (" -- QUICK" if QUICK else ""), ""]
    case1(out)
    case2(out)
    out.append("wall time %.0f s" % (time.time() - t0))
    txt = "\n".join(out)
    print(txt)
    if not QUICK:
        with open(os.path.join(ROOT, "profiles", "lattice.txt"), "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
