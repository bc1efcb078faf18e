"""References for the normal-vector rule on vector shapes (include/trx.h: trx_shape_normal_field, trx_convmat_nv_shapes).

  field        the definition of the blended normal field restated in numpy over whole grids, in np.longdouble (the reference) or float64
               (`dtype=np.float64`: the e_plain of the block-test policy, DESIGN.md "Block tests").  It shares none of the kernel's code: whole
               arrays per primitive and image, np.where in place of branches.
  tensor_hp    the tensor from its definition in clongdouble: [eps] and [1/eps] from the 40-digit mpmath boxes of shape_reference.coef_box, the
               products' matrices from fourier_reference.convmat_hp, [1/eps]^-1 from helpers.solve_hp.
  tensor_plain the same through shape_reference.plain_box, np.fft and torch.linalg.inv in complex128.
"""
import numpy as np
import torch

from tests import fourier_reference as fr
from tests import shape_reference as sr
from tests.helpers import solve_hp

LD = np.longdouble
TAU = 1e-3
ELLIPSE, RECTANGLE, POLYGON = sr.ELLIPSE, sr.RECTANGLE, sr.POLYGON


def primitives(shapes, T=LD):
    """[("ellipse", Rx, Ry, cx, cy, theta) | ("edge", ax, ay, bx, by)] of a list of (kind, par), in the order of the sum; a rectangle is the
    4-gon C + R(theta)(-+Wx/2, -+Wy/2), counter-clockwise from (-, -)."""
    out = []
    for kind, par in shapes:
        p = [T(v) for v in par]
        if kind == ELLIPSE:
            out.append(("ellipse",) + tuple(p))
            continue
        if kind == RECTANGLE:
            c, s = np.cos(p[4]), np.sin(p[4])
            hx, hy = p[0] / 2, p[1] / 2
            v = [(p[2] + c * u - s * w, p[3] + s * u + c * w) for u, w in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]
        else:
            v = [(p[2 * k], p[2 * k + 1]) for k in range(len(p) // 2)]
        out += [("edge",) + v[k] + v[(k + 1) % len(v)] for k in range(len(v))]
    return out


def points(shapes):
    """Ellipse centres and polygon / rectangle vertices (float64): where the field has no direction."""
    pts = []
    for pr in primitives(shapes, np.float64):
        pts.append((pr[3], pr[4]) if pr[0] == "ellipse" else (pr[1], pr[2]))
    return np.array(pts)


def samples(a1, a2, n1, n2, T=LD):
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    fu, fv = i.astype(T) / T(n1), j.astype(T) / T(n2)
    return fu * T(a1[0]) + fv * T(a2[0]), fu * T(a1[1]) + fv * T(a2[1])


def structure_tensor(shapes, a1, a2, n1, n2, dtype=LD):
    T = dtype
    X0, Y0 = samples(a1, a2, n1, n2, T)
    a1, a2 = [T(v) for v in a1], [T(v) for v in a2]
    eta2 = T(1e-12) * abs(a1[0] * a2[1] - a1[1] * a2[0])
    J = [np.zeros((n1, n2), dtype=T) for _ in range(3)]
    one = T(1)

    def add(nx, ny, delta, on):
        w = np.where(on, one / (delta * delta + eta2) ** 2, T(0))
        J[0] += w * nx * nx
        J[1] += w * nx * ny
        J[2] += w * ny * ny

    with np.errstate(divide="ignore", invalid="ignore"):
        for kind, par in shapes:                                           # shapes ascending, images p outer and q inner, edges ascending
            prims = primitives([(kind, par)], T)
            for p in (-1, 0, 1):
                for q in (-1, 0, 1):
                    X, Y = X0 - p * a1[0] - q * a2[0], Y0 - p * a1[1] - q * a2[1]
                    for pr in prims:
                        if pr[0] == "ellipse":
                            Rx, Ry, cx, cy, th = pr[1:]
                            c, s = np.cos(th), np.sin(th)
                            dx, dy = X - cx, Y - cy
                            u, w = c * dx + s * dy, -s * dx + c * dy
                            delta = np.abs(np.hypot(u / Rx, w / Ry) - one) * min(Rx, Ry)
                            gu, gw = u / (Rx * Rx), w / (Ry * Ry)
                            gx, gy = c * gu - s * gw, s * gu + c * gw
                            g = np.hypot(gx, gy)
                            on = g > 0
                            gs = np.where(on, g, one)
                            add(gx / gs, gy / gs, delta, on)
                        else:
                            ax, ay, bx, by = pr[1:]
                            ex, ey = bx - ax, by - ay
                            l2 = ex * ex + ey * ey
                            dx, dy = X - ax, Y - ay
                            tau = (dx * ex + dy * ey) / l2
                            inner = (tau > 0) & (tau < 1)
                            l = np.sqrt(l2)
                            nx, ny = ey / l, -ex / l
                            vx = np.where(tau <= 0, X - ax, X - bx)
                            vy = np.where(tau <= 0, Y - ay, Y - by)
                            dv = np.hypot(vx, vy)
                            on = inner | (dv > 0)
                            ds = np.where(dv > 0, dv, one)
                            add(np.where(inner, nx, vx / ds), np.where(inner, ny, vy / ds), np.where(inner, np.abs(dx * nx + dy * ny), dv), on)
    return J


def field(shapes, a1, a2, n1, n2, dtype=LD):
    """dict(nn [3, n1, n2] the products where the coherence exceeds TAU (else 0), coh [n1, n2] the coherence r / (Jxx + Jyy), 0 where the trace
    is 0) in `dtype`."""
    T = dtype
    Jxx, Jxy, Jyy = structure_tensor(shapes, a1, a2, n1, n2, T)
    d, o, tr = Jxx - Jyy, 2 * Jxy, Jxx + Jyy
    r = np.hypot(d, o)
    on = r > T(TAU) * tr
    rs = np.where(on, r, T(1))
    half = T(0.5)
    nn = np.stack([half * (1 + d / rs), half * (o / rs), half * (1 - d / rs)]) * on
    with np.errstate(divide="ignore", invalid="ignore"):
        coh = np.where(tr > 0, r / np.where(tr > 0, tr, T(1)), T(0))
    return dict(nn=nn, coh=coh)


def excluded(shapes, a1, a2, n1, n2, coh):
    """[n1, n2] bool: the samples the bound may leave out -- |coherence - TAU| < 1e-6, or within 1e-6 sqrt(area) of an ellipse centre or a
    polygon vertex of any image."""
    X, Y = samples(a1, a2, n1, n2, np.float64)
    area = abs(a1[0] * a2[1] - a1[1] * a2[0])
    out = np.abs(np.asarray(coh, dtype=np.float64) - TAU) < 1e-6
    for px, py in points(shapes):
        for p in (-1, 0, 1):
            for q in (-1, 0, 1):
                out |= np.hypot(X - p * a1[0] - q * a2[0] - px, Y - p * a1[1] - q * a2[1] - py) < 1e-6 * np.sqrt(area)
    return out


def tensor_hp(shapes, val, rval, recip, area, mn, mmax, nmax, nn):
    """(Exx, Exy, Eyy, R) in clongdouble; R = [1/eps] for the condition guard.  nn [3, n1, n2] float64 products."""
    mn = np.asarray(mn)
    E = sr.gather(sr.coef_box(shapes, val, recip, area, mmax, nmax), mn, mmax, nmax)
    R = sr.gather(sr.coef_box(shapes, rval, recip, area, mmax, nmax), mn, mmax, nmax)
    D = E - solve_hp(R, np.eye(len(mn)))
    S = []
    for c in range(3):
        C = fr.convmat_hp(np.asarray(nn[c], dtype=LD), mn, mmax, nmax)
        S.append((D @ C + C @ D) * LD(0.5))
    return E - S[0], -S[1], E - S[2], R


def tensor_plain(shapes, val, rval, recip, area, mn, mmax, nmax, nn):
    mn = np.asarray(mn)
    E = sr.gather(sr.plain_box(shapes, np.asarray(val), recip, area, mmax, nmax), mn, mmax, nmax)
    R = sr.gather(sr.plain_box(shapes, np.asarray(rval), recip, area, mmax, nmax), mn, mmax, nmax)
    D = E - torch.linalg.inv(torch.from_numpy(np.ascontiguousarray(R))).numpy()
    S = []
    for c in range(3):
        C = fr.convmat_plain(nn[c], mn)
        S.append((D @ C + C @ D) / 2)
    return E - S[0], -S[1], E - S[2]
