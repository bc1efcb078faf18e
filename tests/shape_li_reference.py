"""Reference for Li's rule on axis-aligned rectangles (include/trx.h: trx_convmat_li_shapes), in np.clongdouble and with algebra unlike the
kernel's:

  - the strips come from the sorted UNIQUE breakpoints, and a strip's state from an explicit point-in-rectangle test of its midpoint over the
    images -1, 0, +1 (the kernel ranks events and derives the states from the ranks);
  - a rectangle's coefficients and a strip's weight are differences of the antiderivative, (e^{-i g t1} - e^{-i g t0}) / (-i g L) (the kernel
    uses sinc times a midpoint phase);
  - the Toeplitz blocks are solved by helpers.solve_hp (LAPACK plus refinement in extended precision; the kernel runs Gauss-Jordan in LDS).

rects: a list of (Wx, Wy, Cx, Cy[, theta]); rval: S + 1 complex values, rval[0] = 1/eps of the background and rval[s+1] = 1/eps_s - 1/eps_host,
so that 1/eps = rval[0] + sum_s rval[s+1] chi_s.  `dtype=np.complex128` gives the plain restatement (the same algebra in double, np.linalg.inv)
whose error against the long-double result is the e_plain of the block tests.  Derivatives are Richardson-extrapolated differences of this
reference (richardson); li_torch is the float64 restatement that autograd differentiates, the e_plain of the adjoint.
"""
import numpy as np

from tests.helpers import solve_hp

LD, CLD = np.longdouble, np.clongdouble
PI_LD = 4 * np.arctan(LD(1))


def _real(dtype):
    return LD if np.dtype(dtype) == np.dtype(CLD) else np.float64


def _segment(t0, t1, o, L, dtype):
    """c[p + 2o] = (1/L) int_t0^t1 e^{-2 pi i p t / L} dt for |p| <= 2o."""
    R = _real(dtype)
    pi = PI_LD if R is LD else np.pi
    p = np.arange(-2 * o, 2 * o + 1)
    g = 2 * pi * p.astype(R) / R(L)
    out = np.empty(len(p), dtype=dtype)
    nz = p != 0
    e = lambda t: np.exp(-1j * g[nz].astype(dtype) * R(t))
    out[nz] = (e(t1) - e(t0)) / (-1j * g[nz].astype(dtype) * R(L))
    out[~nz] = (R(t1) - R(t0)) / R(L)
    return out


def strips(rects, axis, L, dtype=CLD):
    """(breakpoints [K+1] sorted and unique, from 0 to L; inside [K, S] bool) of the strips across `axis` (0: x-edges, 1: y-edges)."""
    R = _real(dtype)
    pts = [R(0), R(L)]
    for r in rects:
        W, C = R(r[axis]), R(r[2 + axis])
        for edge in (C - W / 2, C + W / 2):
            pts.append(edge - np.floor(edge / R(L)) * R(L))
    t = np.unique(np.array(pts, dtype=R))
    t = t[(t >= 0) & (t <= R(L))]
    mid = (t[:-1] + t[1:]) / 2
    inside = np.zeros((len(mid), len(rects)), dtype=bool)
    for s, r in enumerate(rects):
        W, C = R(r[axis]), R(r[2 + axis])
        for i in (-1, 0, 1):
            inside[:, s] |= np.abs(mid - (C + i * R(L))) < W / 2
    return t, inside


def _toeplitz_index(o):
    a = np.arange(2 * o + 1)
    return a[:, None] - a[None, :] + 2 * o


def _inverse(T, dtype):
    if np.dtype(dtype) == np.dtype(CLD):
        return solve_hp(T, np.eye(T.shape[0]))
    return np.linalg.inv(T)


def direction(rects, rval, axis, Ls, Lc, os, oc, dtype=CLD):
    """One direction: the strips across `axis` (period Ls, order os), coefficients along the other axis (period Lc, order oc).
    Returns (H [wc, wc, 4 os + 1] = sum_k U_k w_k, the Toeplitz blocks T [K, wc, wc], their inverses U)."""
    rval = np.asarray(rval, dtype=dtype)
    t, inside = strips(rects, axis, Ls, dtype)
    wc = 2 * oc + 1
    H = np.zeros((wc, wc, 4 * os + 1), dtype=dtype)
    Ts, Us = [], []
    for k in range(len(t) - 1):
        a = np.zeros(4 * oc + 1, dtype=dtype)
        a[2 * oc] = rval[0]
        for s, r in enumerate(rects):
            if inside[k, s]:
                W, C = r[1 - axis], r[3 - axis]
                R = _real(dtype)
                a = a + rval[s + 1] * _segment(R(C) - R(W) / 2, R(C) + R(W) / 2, oc, Lc, dtype)
        T = a[_toeplitz_index(oc)]
        U = _inverse(T, dtype)
        H = H + U[:, :, None] * _segment(t[k], t[k + 1], os, Ls, dtype)[None, None, :]
        Ts.append(T)
        Us.append(U)
    return H, np.array(Ts), np.array(Us)


def li(rects, rval, Lx, Ly, ox, oy, dtype=CLD, want_blocks=False):
    """(Ex, Ey) [N, N] in `dtype`, index (m + ox)(2oy + 1) + (n + oy) as trx_convmat_li; want_blocks: also the Toeplitz blocks of the two
    directions (for the guards of the block tests)."""
    wx, wy = 2 * ox + 1, 2 * oy + 1
    N = wx * wy
    F, Tx, _ = direction(rects, rval, 1, Ly, Lx, oy, ox, dtype)          # horizontal strips: inverse rule across x
    G, Ty, _ = direction(rects, rval, 0, Lx, Ly, ox, oy, dtype)
    Ex = F[:, :, _toeplitz_index(oy)].transpose(0, 2, 1, 3).reshape(N, N)               # [m, m', n, n'] -> [m, n, m', n']
    Ey = G[:, :, _toeplitz_index(ox)].transpose(2, 0, 3, 1).reshape(N, N)               # [n, n', m, m'] -> [m, n, m', n']
    return (Ex, Ey, Tx, Ty) if want_blocks else (Ex, Ey)


def rasterise(rects, eps, eps_bg, hosts, Lx, Ly, nx, ny):
    """[nx, ny] complex grid sampled at (i / nx) Lx, (j / ny) Ly (the DFT's positions), images -1, 0, +1; hosts before what they hold."""
    x = (np.arange(nx) / nx * Lx)[:, None]
    y = (np.arange(ny) / ny * Ly)[None, :]
    g = np.full((nx, ny), eps_bg, dtype=np.complex128)
    depth = lambda s: 0 if hosts[s] is None else 1 + depth(hosts[s])
    for s in sorted(range(len(rects)), key=depth):
        Wx, Wy, Cx, Cy = rects[s][:4]
        inx = np.zeros_like(x, dtype=bool)
        iny = np.zeros_like(y, dtype=bool)
        for i in (-1, 0, 1):
            inx |= np.abs(x - Cx - i * Lx) < Wx / 2
            iny |= np.abs(y - Cy - i * Ly) < Wy / 2
        g[inx & iny] = eps[s]
    return g


def rvals(eps, eps_bg, hosts):
    """rval of a list: 1/eps_bg, then 1/eps_s - 1/eps_host."""
    return np.array([1 / eps_bg] + [1 / eps[s] - 1 / (eps_bg if h is None else eps[h]) for s, h in enumerate(hosts)], dtype=np.complex128)


def self_check(ns=(64, 128, 256)):
    """The reference against the grid definition of Li's rule (li_ref of tests/test_li_factorisation.py): max |F_grid - F_strips| / max |F| per
    raster size for a wrapped eps = 12 + 0.3i rectangle with a nested eps = 4 core on a 1.0 x 1.3 cell at order (3, 2), every edge halfway
    between two samples of the raster.  Second order in 1 / n."""
    import torch
    from tests.helpers import relmax
    from tests.test_li_factorisation import li_ref
    Lx, Ly, ox, oy = 1.0, 1.3, 3, 2
    eps, hosts = [12 + 0.3j, 4.0], [None, 0]
    errs = []
    for n in ns:
        edge = lambda e, L: (np.floor(e * n / L) + 0.5) * L / n              # the nearest position halfway between two samples
        boxes = [(edge(0.63, Lx), edge(0.63, Lx) + 32 * Lx / 64, edge(0.95, Ly), edge(0.95, Ly) + 36 * Ly / 64),     # crosses both cell boundaries
                 (edge(0.78, Lx), edge(0.78, Lx) + 12 * Lx / 64, edge(1.05, Ly), edge(1.05, Ly) + 10 * Ly / 64)]
        rects = [(x1 - x0, y1 - y0, (x0 + x1) / 2, (y0 + y1) / 2) for x0, x1, y0, y1 in boxes]
        Ex, Ey = li(rects, rvals(eps, 1.0, hosts), Lx, Ly, ox, oy)
        gx, gy = li_ref(torch.from_numpy(rasterise(rects, eps, 1.0, hosts, Lx, Ly, n, n)), ox, oy)
        errs.append(max(relmax(gx.numpy(), Ex), relmax(gy.numpy(), Ey)))
    return errs


# ---- derivatives: Richardson-extrapolated differences of a scalar function of this reference ---------------------------------------------------
def richardson(f, h, side=0, levels=4):
    """(d, err): the derivative at 0 of the scalar function f of one long-double offset, from differences with steps h, h/2, ... and `levels`
    Richardson eliminations; err = |last two diagonal entries' difference|, the truncation error of the less accurate of the two.
    side 0: central differences (even error terms); +1 / -1: one-sided differences towards positive / negative offsets (every order)."""
    h = LD(h)
    col = []
    for i in range(levels + 1):
        s = h / LD(2) ** i
        col.append((f(s) - f(-s)) / (2 * s) if side == 0 else (f(side * s) - f(LD(0))) / (side * s))
    diag = [col[0]]
    for j in range(1, levels + 1):
        r = LD(4) ** j if side == 0 else LD(2) ** j
        col = [(r * col[i + 1] - col[i]) / (r - 1) for i in range(len(col) - 1)]
        diag.append(col[0])
    return diag[-1], abs(diag[-1] - diag[-2])


# ---- float64 restatement with automatic differentiation (the e_plain of the adjoint) -----------------------------------------------------------
def li_torch(par, rval, Lx, Ly, ox, oy):
    """(Ex, Ey) of par [S, 5] float64 and rval [S+1] complex128 torch tensors, differentiable by autograd: sinc forms, torch.linalg.inv.
    Strips from a stable sort of (origin, lower edge and upper edge per rectangle); states from the midpoints (strict inequalities)."""
    import torch

    def tix(o):
        a = torch.arange(2 * o + 1)
        return a[:, None] - a[None, :] + 2 * o

    def one(axis, Ls, Lc, os, oc):
        W, C, Wc, Cc = par[:, axis], par[:, 2 + axis], par[:, 1 - axis], par[:, 3 - axis]
        lo = C - W / 2
        lo = lo - torch.floor(lo.detach() / Ls) * Ls
        hi = lo + W
        close = torch.where(hi > Ls, hi - Ls, hi)
        t = torch.sort(torch.cat((lo.new_zeros(1), torch.stack((lo, close), dim=1).reshape(-1))), stable=True)[0]
        t = torch.cat((t, t.new_full((1,), Ls)))
        h, mid = t[1:] - t[:-1], (t[1:] + t[:-1]) / 2
        inside = torch.zeros((len(mid), len(W)), dtype=torch.bool)
        for i in (-1, 0, 1):
            inside |= (mid.detach()[:, None] - (C.detach()[None, :] + i * Ls)).abs() < W.detach()[None, :] / 2
        p = torch.arange(-2 * oc, 2 * oc + 1, dtype=torch.float64)
        q = torch.arange(-2 * os, 2 * os + 1, dtype=torch.float64)
        term = (Wc / Lc)[:, None] * torch.sinc(p[None, :] * (Wc / Lc)[:, None]) * torch.exp(-2j * np.pi * p[None, :] * Cc[:, None] / Lc)
        a = inside.to(torch.complex128) @ (rval[1:, None] * term) + rval[0] * (p == 0).to(torch.complex128)[None, :]
        U = torch.linalg.inv(a[:, tix(oc)])
        w = (h / Ls)[:, None] * torch.sinc(q[None, :] * (h / Ls)[:, None]) * torch.exp(-2j * np.pi * q[None, :] * mid[:, None] / Ls)
        return torch.einsum("kab,kq->abq", U, w)

    wx, wy = 2 * ox + 1, 2 * oy + 1
    N = wx * wy
    F = one(1, Ly, Lx, oy, ox)
    G = one(0, Lx, Ly, ox, oy)
    Ex = F[:, :, tix(oy)].permute(0, 2, 1, 3).reshape(N, N)
    Ey = G[:, :, tix(ox)].permute(2, 0, 3, 1).reshape(N, N)
    return Ex, Ey
