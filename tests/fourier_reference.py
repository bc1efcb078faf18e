"""References beyond complex128 for the Fourier-factorisation entries of include/trx.h (trx_convmat*, trx_convmat_li, trx_normal_field*,
trx_convmat_nv*), next to helpers.solve_hp and eig_reference.eig_hp.  Everything is np.longdouble / np.clongdouble (x87 extended, eps 1.1e-19;
tests/test_fourier_blocks.py asserts that and validates dft_hp against 40-digit mpmath), and none of it follows the kernels' algebra:

  dft_hp       the pruned DFT as a matrix product Fx @ g @ Fy (the kernels: separable thread-serial sums with a running twiddle index);
               the phase p*x is reduced exactly in integers and sin / cos are taken of a residual angle of at most pi/8;
  li_hp        Toeplitz blocks from dft_hp of 1/g, inverted by solve_hp(T, I) (the kernel: in-LDS Gauss-Jordan with row interchanges), the
               second transform a long-double matrix product;
  tensor_hp    the normal-vector tensor from its definition: convolution matrices from dft_hp, [1/eps]^-1 from solve_hp, long-double products;
  field_hp     the Gaussian periodised FIRST (wp[j] = sum of w[k] over k = j mod n), the blur as two circulant matrix products, and the
               principal direction from np.linalg.eigh of the 2 x 2 blurred tensor as v v^T (the kernel: wrapped tap loops and a closed form).
The `*_plain` functions are the same operations through the library (np.fft, torch.linalg.inv) in complex128: their error against the
references above is the e_plain of the block-test policy ("Block tests").
"""
import math

import numpy as np
import torch

from tests.helpers import solve_hp

LD = np.longdouble
CLD = np.clongdouble
PI_LD = LD("3.14159265358979323846264338327950288")
TAU = 1e-3                       # NV_TAU of csrc/convmat_nv.hip: the coherence floor of a resolvable direction


# ---- the pruned DFT -------------------------------------------------------------------------------------------------------------------
def twiddle_hp(n, P):
    """[len(P), n] clongdouble: exp(-2 pi i p x / n).  k = (p x) mod n exactly (int64); the angle 2 pi k / n is split into the nearest
    multiple of pi/4 (exact table but for sqrt(1/2)) and a residual pi r / (4 n), |r| <= n/2, whose sin and cos carry an absolute error of
    a fraction of eps(long double)."""
    p = np.asarray(P, dtype=np.int64).reshape(-1, 1)
    k = (p * np.arange(n, dtype=np.int64)[None, :]) % n
    j = (8 * k + n // 2) // n
    r = 8 * k - j * n
    a = PI_LD * r.astype(LD) / LD(4 * n)
    c, s = np.cos(a), np.sin(a)
    h = np.sqrt(LD(0.5))
    zero, one = LD(0), LD(1)
    oc = np.array([one, h, zero, -h, -one, -h, zero, h], dtype=LD)[j % 8]
    os_ = np.array([zero, h, one, h, zero, -h, -one, -h], dtype=LD)[j % 8]
    out = np.empty(k.shape, dtype=CLD)
    out.real = oc * c - os_ * s
    out.imag = -(os_ * c + oc * s)
    return out


def dft_hp(g, P, Q):
    """c[i, j] = (1 / (nx ny)) sum_xy g[x, y] exp(-2 pi i (P[i] x / nx + Q[j] y / ny)) as Fx @ g @ Fy in clongdouble.  P or Q = None leaves
    that axis untransformed (the 1-D transforms of Li's rule), its 1/n included."""
    out = np.asarray(g, dtype=CLD)
    nx, ny = out.shape
    if P is not None:
        out = (twiddle_hp(nx, P) @ out) / LD(nx)
    if Q is not None:
        out = (out @ twiddle_hp(ny, Q).T) / LD(ny)
    return out


def rect_orders(ox, oy):
    """[N, 2] harmonics of trx_convmat's index map, i = (m + ox)(2 oy + 1) + (n + oy)."""
    mm, nn = np.meshgrid(np.arange(-ox, ox + 1), np.arange(-oy, oy + 1), indexing="ij")
    return np.stack([mm.reshape(-1), nn.reshape(-1)], 1)


def _gather(c, mn, mmax, nmax):
    dm = mn[:, None, 0] - mn[None, :, 0]
    dn = mn[:, None, 1] - mn[None, :, 1]
    return c[dm + 2 * mmax, dn + 2 * nmax]


def convmat_hp(g, mn, mmax, nmax):
    """out[i, j] = c[m_i - m_j, n_i - n_j] from dft_hp over the box |p| <= 2 mmax, |q| <= 2 nmax."""
    return _gather(dft_hp(g, np.arange(-2 * mmax, 2 * mmax + 1), np.arange(-2 * nmax, 2 * nmax + 1)), np.asarray(mn), mmax, nmax)


def convmat_plain(g, mn):
    """np.fft.fft2 in complex128 and the gather with negative differences wrapped."""
    g = np.asarray(g, dtype=np.complex128)
    mn = np.asarray(mn)
    c = np.fft.fft2(g) / (g.shape[0] * g.shape[1])
    return c[(mn[:, None, 0] - mn[None, :, 0]) % g.shape[0], (mn[:, None, 1] - mn[None, :, 1]) % g.shape[1]]


# ---- Li's inverse rule ----------------------------------------------------------------------------------------------------------------
def _toeplitz_rows(a, o):
    """a [rows, 4o+1] (index d + 2o) -> [rows, w, w], T[m, m'] = a[m - m']."""
    w = 2 * o + 1
    d = np.arange(w)[:, None] - np.arange(w)[None, :] + 2 * o
    return a[:, d]


def li_hp(g, ox, oy):
    """dict(Ex, Ey [N, N]; Ux [nx, wy, wy], Uy [ny, wx, wx]; Tx, Ty the Toeplitz blocks that were inverted) in clongdouble.  1/g is formed in
    long double from g as given (the caller passes the grid as rounded to the kernel's input type)."""
    rg = LD(1) / np.asarray(g, dtype=CLD)
    nx, ny = rg.shape
    wx, wy = 2 * ox + 1, 2 * oy + 1
    P, Q = np.arange(-2 * ox, 2 * ox + 1), np.arange(-2 * oy, 2 * oy + 1)
    Ty = _toeplitz_rows(dft_hp(rg, P, None).T, ox)                  # per grid row y: the x-Toeplitz block
    Tx = _toeplitz_rows(dft_hp(rg, None, Q), oy)                    # per grid row x: the y-Toeplitz block
    Uy = np.stack([solve_hp(T, np.eye(wx)) for T in Ty])
    Ux = np.stack([solve_hp(T, np.eye(wy)) for T in Tx])
    F = (twiddle_hp(ny, Q) @ Uy.reshape(ny, wx * wx)) / LD(ny)      # [4oy+1, wx wx]
    G = (twiddle_hp(nx, P) @ Ux.reshape(nx, wy * wy)) / LD(nx)      # [4ox+1, wy wy]
    mn = rect_orders(ox, oy)
    m, n = mn[:, 0] + ox, mn[:, 1] + oy
    Ex = F[(n[:, None] - n[None, :]) + 2 * oy, m[:, None] * wx + m[None, :]]
    Ey = G[(m[:, None] - m[None, :]) + 2 * ox, n[:, None] * wy + n[None, :]]
    return dict(Ex=Ex, Ey=Ey, Ux=Ux, Uy=Uy, Tx=Tx, Ty=Ty)


def li_plain(g, ox, oy):
    """The same through np.fft and torch.linalg.inv in complex128: (Ex, Ey, Ux, Uy)."""
    rg = 1.0 / np.asarray(g, dtype=np.complex128)
    nx, ny = rg.shape
    wx, wy = 2 * ox + 1, 2 * oy + 1
    ay = (np.fft.fft(rg, axis=0) / nx).T                            # [ny, nx], index p mod nx
    ax = np.fft.fft(rg, axis=1) / ny                                # [nx, ny], index q mod ny
    dx = (np.arange(wx)[:, None] - np.arange(wx)[None, :]) % nx
    dy = (np.arange(wy)[:, None] - np.arange(wy)[None, :]) % ny
    Uy = torch.linalg.inv(torch.from_numpy(np.ascontiguousarray(ay[:, dx]))).numpy()
    Ux = torch.linalg.inv(torch.from_numpy(np.ascontiguousarray(ax[:, dy]))).numpy()
    F = np.fft.fft(Uy, axis=0) / ny                                 # [q mod ny, wx, wx]
    G = np.fft.fft(Ux, axis=0) / nx
    mn = rect_orders(ox, oy)
    m, n = mn[:, 0] + ox, mn[:, 1] + oy
    Ex = F[(n[:, None] - n[None, :]) % ny, m[:, None], m[None, :]]
    Ey = G[(m[:, None] - m[None, :]) % nx, n[:, None], n[None, :]]
    return Ex, Ey, Ux, Uy


# ---- the normal-vector tensor ---------------------------------------------------------------------------------------------------------
def tensor_hp(g, mn, mmax, nmax, nn):
    """(Exx, Exy, Eyy, R): D = [eps] - [1/eps]^-1, {D, C} = (D C + C D) / 2, Exx = [eps] - {D, [Nx Nx]}, Exy = -{D, [Nx Ny]},
    Eyy = [eps] - {D, [Ny Ny]}, all in clongdouble; R = [1/eps] for the condition guard.  nn [3, nx, ny] float64 products of the field."""
    gl = np.asarray(g, dtype=CLD)
    E = convmat_hp(gl, mn, mmax, nmax)
    R = convmat_hp(LD(1) / gl, mn, mmax, nmax)
    D = E - solve_hp(R, np.eye(len(mn)))
    half = LD(0.5)
    S = []
    for c in range(3):
        C = convmat_hp(np.asarray(nn[c], dtype=LD), mn, mmax, nmax)
        S.append((D @ C + C @ D) * half)
    return E - S[0], -S[1], E - S[2], R


def tensor_plain(g, mn, nn):
    g = np.asarray(g, dtype=np.complex128)
    E = convmat_plain(g, mn)
    D = E - torch.linalg.inv(torch.from_numpy(np.ascontiguousarray(convmat_plain(1.0 / g, mn)))).numpy()
    S = []
    for c in range(3):
        C = convmat_plain(nn[c], mn)
        S.append((D @ C + C @ D) / 2)
    return E - S[0], -S[1], E - S[2]


# ---- the normal field -----------------------------------------------------------------------------------------------------------------
def _circulant_blur(n, sigma):
    """C [n, n] long double with (C f)[i] = sum_k w[k] f[(i + k) mod n], w the truncated normalised Gaussian: periodised first."""
    R = int(math.ceil(3.0 * sigma)) if sigma > 0 else 0
    k = np.arange(-R, R + 1)
    w = np.exp(-(k.astype(LD) ** 2) / (LD(2) * LD(sigma) * LD(sigma))) if R > 0 else np.ones(1, dtype=LD)
    w = w / w.sum()
    wp = np.zeros(n, dtype=LD)
    np.add.at(wp, k % n, w)
    i = np.arange(n)
    return wp[(i[None, :] - i[:, None]) % n]


def field_hp(g, sigma, hinv):
    """dict(dir [3, nx, ny] = v v^T of the principal eigenvector of the blurred structure tensor wherever its trace is > 0 (else 0);
    coh [nx, ny] = (l1 - l2) / (l1 + l2), 0 where the trace is 0).  hinv: the 2 x 2 inverse cell matrix (diag(1/hx, 1/hy) for a rectangle).
    The output the kernel should produce is dir where coh > TAU, 0 elsewhere."""
    gl = np.asarray(g, dtype=CLD)
    nx, ny = gl.shape
    hi = np.asarray(hinv, dtype=LD)
    half = LD(0.5)
    du = (np.roll(gl, -1, 0) - np.roll(gl, 1, 0)) * half
    dv = (np.roll(gl, -1, 1) - np.roll(gl, 1, 1)) * half
    gx, gy = hi[0, 0] * du + hi[0, 1] * dv, hi[1, 0] * du + hi[1, 1] * dv
    J = [gx.real ** 2 + gx.imag ** 2, gx.real * gy.real + gx.imag * gy.imag, gy.real ** 2 + gy.imag ** 2]
    Cx, Cy = _circulant_blur(nx, sigma), _circulant_blur(ny, sigma)
    J = [Cx @ c @ Cy.T for c in J]
    tr = J[0] + J[2]
    on = tr > 0
    scale = np.where(on, tr, LD(1))
    M = np.empty((nx, ny, 2, 2))
    M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1] = (J[0] / scale), (J[1] / scale), (J[1] / scale), (J[2] / scale)
    lam, V = np.linalg.eigh(M)                                      # ascending: column 1 is the principal direction
    v = V[..., :, 1]
    dirs = np.stack([v[..., 0] ** 2, v[..., 0] * v[..., 1], v[..., 1] ** 2]) * on
    coh = np.where(on, lam[..., 1] - lam[..., 0], 0.0)              # trace scaled to 1
    return dict(dir=dirs, coh=coh)
