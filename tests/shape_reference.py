"""References for the vector-shape entries of include/trx.h (trx_convmat_shapes, trx_convmat_shapes_backward), evaluated with mpmath at DPS
digits and following none of the kernels' algebra:

  ellipse    pi Rx Ry 2 J1(rho) / rho from mpmath.besselj;
  rectangle  the product of two exact 1-D exponential integrals over [-W/2, W/2] in the rotated frame;
  polygon    a signed fan of triangles (v0, vk, vk+1), each mapped onto the unit triangle and integrated by mpmath.quad -- not the edge sum.
             The outer variable is integrated by mpmath.quad and the inner one, an exponential over [0, 1 - s], exactly: the nested 2-D
             mpmath.quad costs about a second per (triangle, G) at this precision, which no test could afford over a whole box.  The two
             agree to 1e-30 (asserted below on one triangle);
  derivatives  mpmath.diff of those, parameter by parameter.

Self-checks, asserted at import: the polygon reference of a rotated rectangle equals the rectangle reference, and the polygon reference of an
axis-aligned L equals a 1-D slab integration (x by mpmath.quad, y exact), both to 1e-30.

`plain_*` are the float64 numpy / scipy restatements of the closed forms of include/trx.h: their error against the references is the e_plain
of the block-test policy ("Block tests"), and they supply E for the end-to-end tests.
"""
import functools

import mpmath as mp
import numpy as np
import scipy.special

DPS = 40
ELLIPSE, RECTANGLE, POLYGON = 0, 1, 2


def recip_of(a1, a2):
    """float64 (b1x, b1y, b2x, b2y) with b_i . a_j = 2 pi delta_ij, and the cell area."""
    A = np.array([a1, a2], dtype=np.float64)
    return tuple((2 * np.pi * np.linalg.inv(A).T).ravel()), abs(float(np.linalg.det(A)))


# ---- mpmath ------------------------------------------------------------------------------------------------------------------------------
def _rot(par, Gx, Gy):
    c, s = mp.cos(par[4]), mp.sin(par[4])
    return c * Gx + s * Gy, -s * Gx + c * Gy


def _seg(g, W):
    """int_{-W/2}^{W/2} e^{-i g u} du"""
    if g == 0:
        return W
    return (mp.expj(-g * W / 2) - mp.expj(g * W / 2)) / (-1j * g)


def _triangle(v0, v1, v2, Gx, Gy, nested=False):
    e1, e2 = (v1[0] - v0[0], v1[1] - v0[1]), (v2[0] - v0[0], v2[1] - v0[1])
    det = e1[0] * e2[1] - e1[1] * e2[0]
    a, b = Gx * e1[0] + Gy * e1[1], Gx * e2[0] + Gy * e2[1]
    if nested:
        val = mp.quad(lambda s: mp.quad(lambda t: mp.expj(-(a * s + b * t)), [0, 1 - s], method="gauss-legendre"), [0, 1], method="gauss-legendre")
    else:
        inner = (lambda s: 1 - s) if b == 0 else (lambda s: (mp.expj(-b * (1 - s)) - 1) / (-1j * b))
        val = mp.quad(lambda s: mp.expj(-a * s) * inner(s), [0, 1], method="gauss-legendre")
    return det * mp.expj(-(Gx * v0[0] + Gy * v0[1])) * val


def chi_mp(kind, par, Gx, Gy):
    """int_shape e^{-iG.r} d2r (NOT divided by the cell area), mpmath."""
    par = [mp.mpf(v) for v in par]
    Gx, Gy = mp.mpf(Gx), mp.mpf(Gy)
    if kind == POLYGON:
        v = [(par[2 * k], par[2 * k + 1]) for k in range(len(par) // 2)]
        return mp.fsum(_triangle(v[0], v[k], v[k + 1], Gx, Gy) for k in range(1, len(v) - 1))
    gx, gy = _rot(par, Gx, Gy)
    ph = mp.expj(-(Gx * par[2] + Gy * par[3]))
    if kind == ELLIPSE:
        rho = mp.sqrt((par[0] * gx) ** 2 + (par[1] * gy) ** 2)
        return mp.pi * par[0] * par[1] * (1 if rho == 0 else 2 * mp.besselj(1, rho) / rho) * ph
    return _seg(gx, par[0]) * _seg(gy, par[1]) * ph


def dchi_mp(kind, par, j, Gx, Gy):
    """d/dpar[j] of chi_mp by mpmath.diff: a central difference with h = 2^-60 at 13 more bits than the DPS digits (mpmath's default doubles the
    precision, which the quadratures of a polygon cannot afford); truncation h^2 ~ 1e-36, cancellation leaves about 26 digits."""
    par = [mp.mpf(v) for v in par]
    return mp.diff(lambda x: chi_mp(kind, par[:j] + [x] + par[j + 1:], Gx, Gy), par[j], h=mp.ldexp(1, -60), addprec=-30)


def _ld(z):
    return np.clongdouble(np.longdouble(mp.nstr(mp.re(z), 25)) + 1j * np.longdouble(mp.nstr(mp.im(z), 25)))


def _box_G(recip, mmax, nmax):
    P, Q = np.meshgrid(np.arange(-2 * mmax, 2 * mmax + 1), np.arange(-2 * nmax, 2 * nmax + 1), indexing="ij")
    return P, Q, P * recip[0] + Q * recip[2], P * recip[1] + Q * recip[3]


@functools.lru_cache(maxsize=None)
def _chi_one_cached(kind, par, recip, area, mmax, nmax):
    with mp.workdps(DPS):
        P, Q, Gx, Gy = _box_G(recip, mmax, nmax)
        b = [mp.mpf(v) for v in recip]
        out = np.zeros(P.shape, dtype=np.clongdouble)
        for i in range(P.shape[0]):
            for j in range(P.shape[1]):
                p, q = int(P[i, j]), int(Q[i, j])
                if (p, q) > (0, 0):                                       # a real region: chi(-G) = conj(chi(G)), from the integral itself
                    continue
                out[i, j] = _ld(chi_mp(kind, par, p * b[0] + q * b[2], p * b[1] + q * b[3]) / mp.mpf(area))
                out[-1 - i, -1 - j] = np.conj(out[i, j])
        return out


def chi_box(shapes, recip, area, mmax, nmax):
    """[S, 4mmax+1, 4nmax+1] clongdouble: chi_s(G) / area of every shape (kind, par) over the coefficient box; each shape is computed once per
    (parameters, lattice, box) and shared by every test that asks for it."""
    return np.stack([_chi_one_cached(int(k), tuple(float(v) for v in par), tuple(float(v) for v in recip), float(area), int(mmax), int(nmax))
                     for k, par in shapes])


def coef_box(shapes, val, recip, area, mmax, nmax):
    """The reference box c = val[0] delta_G0 + sum_s val[s+1] chi_s, clongdouble."""
    chi = chi_box(shapes, recip, area, mmax, nmax)
    c = np.tensordot(np.asarray(val[1:], dtype=np.clongdouble), chi, axes=(0, 0))
    c[2 * mmax, 2 * nmax] += np.clongdouble(val[0])
    return c


@functools.lru_cache(maxsize=None)
def _dchi_box_cached(kind, par, recip, area, mmax, nmax):
    with mp.workdps(DPS):
        P, Q, Gx, Gy = _box_G(recip, mmax, nmax)
        b = [mp.mpf(v) for v in recip]
        out = np.zeros((len(par),) + P.shape, dtype=np.clongdouble)
        for k in range(len(par)):
            for i in range(P.shape[0]):
                for j in range(P.shape[1]):
                    p, q = int(P[i, j]), int(Q[i, j])
                    if (p, q) > (0, 0):
                        continue
                    out[k, i, j] = _ld(dchi_mp(kind, list(par), k, p * b[0] + q * b[2], p * b[1] + q * b[3]) / mp.mpf(area))
                    out[k, -1 - i, -1 - j] = np.conj(out[k, i, j])
        return out


def dchi_box(kind, par, recip, area, mmax, nmax):
    """[len(par), 4mmax+1, 4nmax+1] clongdouble: d(chi / area) / dpar[k] over the box."""
    return _dchi_box_cached(int(kind), tuple(float(v) for v in par), tuple(float(v) for v in recip), float(area), int(mmax), int(nmax))


# ---- float64 restatement of the closed forms (e_plain; E of the end-to-end tests) -----------------------------------------------------------
def _sinc(t):
    return np.sinc(t / np.pi)


def plain_chi(kind, par, Gx, Gy, area):
    par = np.asarray(par, dtype=np.float64)
    if kind == POLYGON:
        v = par.reshape(-1, 2)
        w = np.roll(v, -1, axis=0)
        e, m = w - v, (w + v) / 2
        G2 = Gx ** 2 + Gy ** 2
        zero = G2 == 0
        tot = np.zeros(np.shape(Gx), dtype=np.complex128)
        for k in range(len(v)):
            tot = tot + (Gx * e[k, 1] - Gy * e[k, 0]) * np.exp(-1j * (Gx * m[k, 0] + Gy * m[k, 1])) * _sinc((Gx * e[k, 0] + Gy * e[k, 1]) / 2)
        shoelace = 0.5 * np.sum(v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1])
        return np.where(zero, shoelace / area, 1j * tot / (area * np.where(zero, 1.0, G2)))
    c, s = np.cos(par[4]), np.sin(par[4])
    gx, gy = c * Gx + s * Gy, -s * Gx + c * Gy
    ph = np.exp(-1j * (Gx * par[2] + Gy * par[3]))
    if kind == ELLIPSE:
        rho = np.hypot(par[0] * gx, par[1] * gy)
        jinc = np.where(rho == 0, 1.0, 2 * scipy.special.j1(rho) / np.where(rho == 0, 1.0, rho))
        return np.pi * par[0] * par[1] / area * jinc * ph
    return par[0] * par[1] / area * _sinc(gx * par[0] / 2) * _sinc(gy * par[1] / 2) * ph


def plain_box(shapes, val, recip, area, mmax, nmax):
    P, Q, Gx, Gy = _box_G(recip, mmax, nmax)
    c = np.zeros(P.shape, dtype=np.complex128)
    for (kind, par), dv in zip(shapes, val[1:]):
        c = c + dv * plain_chi(kind, par, Gx, Gy, area)
    c[2 * mmax, 2 * nmax] += val[0]
    return c


def gather(box, mn, mmax, nmax):
    """out[i, j] = box[m_i - m_j + 2mmax, n_i - n_j + 2nmax]"""
    mn = np.asarray(mn)
    dm = mn[:, None, 0] - mn[None, :, 0] + 2 * mmax
    dn = mn[:, None, 1] - mn[None, :, 1] + 2 * nmax
    return box[..., dm, dn]


# ---- self-checks ----------------------------------------------------------------------------------------------------------------------------
def _rect_vertices(Wx, Wy, Cx, Cy, th):
    c, s = mp.cos(th), mp.sin(th)
    return [v for u, w in ((-Wx / 2, -Wy / 2), (Wx / 2, -Wy / 2), (Wx / 2, Wy / 2), (-Wx / 2, Wy / 2)) for v in (Cx + c * u - s * w, Cy + s * u + c * w)]


def _self_check():
    with mp.workdps(DPS):
        tol = mp.mpf(10) ** -30
        rect = [mp.mpf("0.37"), mp.mpf("0.21"), mp.mpf("0.45"), mp.mpf("0.55"), mp.mpf("0.4")]
        poly = _rect_vertices(*rect)
        for Gx, Gy in ((0, 0), (mp.mpf("6.3"), 0), (mp.mpf("-12.6"), mp.mpf("7.1"))):
            assert abs(chi_mp(POLYGON, poly, Gx, Gy) - chi_mp(RECTANGLE, rect, Gx, Gy)) < tol
        # an axis-aligned L: [0.1, 0.7] x [0.2, 0.4] joined to [0.1, 0.3] x [0.4, 0.8], against slabs in x (y integrated exactly)
        L = [mp.mpf(v) for v in ("0.1", "0.2", "0.7", "0.2", "0.7", "0.4", "0.3", "0.4", "0.3", "0.8", "0.1", "0.8")]
        for Gx, Gy in ((0, 0), (mp.mpf("6.3"), mp.mpf("-6.3")), (0, mp.mpf("12.6"))):
            Gx, Gy = mp.mpf(Gx), mp.mpf(Gy)
            col = lambda y0, y1: (y1 - y0) if Gy == 0 else (mp.expj(-Gy * y1) - mp.expj(-Gy * y0)) / (-1j * Gy)
            top = lambda x: mp.mpf("0.8") if x < mp.mpf("0.3") else mp.mpf("0.4")
            slab = mp.quad(lambda x: mp.expj(-Gx * x) * col(mp.mpf("0.2"), top(x)), [mp.mpf("0.1"), mp.mpf("0.3"), mp.mpf("0.7")])
            assert abs(chi_mp(POLYGON, L, Gx, Gy) - slab) < tol
        v = [(mp.mpf("0.1"), mp.mpf("0.2")), (mp.mpf("0.8"), mp.mpf("0.3")), (mp.mpf("0.4"), mp.mpf("0.9"))]
        assert abs(_triangle(*v, mp.mpf("6.3"), mp.mpf("-3.1")) - _triangle(*v, mp.mpf("6.3"), mp.mpf("-3.1"), nested=True)) < tol


_self_check()
