"""Reference for the adjoint of the blended normal field (include/trx.h: trx_shape_normal_field_backward).

  tangents     the derivative of the field products with respect to ONE parameter of the packed row, in forward mode: every intermediate of
               tests/shape_nv_reference.structure_tensor carries its tangent (dual numbers written out by hand) over whole numpy arrays, np.where
               in place of branches, in np.longdouble (the reference) or float64 (`dtype=np.float64`: the e_plain of the block-test policy).  It
               shares no code with the kernel, which works in reverse mode from (n^T G n, t^T G n); only the primitives that depend on the
               parameter are differentiated (an ellipse, the four edges of a rectangle, the two edges at a polygon vertex), against the
               structure tensor of the whole list.
  gpar         gpar_k = sum gnn * d nn / d par_k, and the policy's denominator sum |gnn * d nn / d par_k|, for every parameter of the row.

The branch conventions are the kernel's contract: sign(0) = 0, d min(Rx, Ry) goes to Rx when Rx <= Ry, a vertex branch differentiates the
selected vertex, a sample on a branch line tau = 0 / 1 (to within 16 eps of fp64 in the numerator, in both dtypes) takes the mean of the two
pieces' derivatives, zero products have a zero derivative.

Self-check (tests/test_shape_nv_grad_blocks.py::test_reference_matches_central_differences): against central differences of
shape_nv_reference.field(..., dtype=np.longdouble) with h = 1e-8, every parameter of a rotated rectangle + an ellipse with a nested ellipse + a
triangle on the oblique cell at (33, 17): max |tangent - FD| / max |tangent| = 5.8e-11 or less per parameter, and it falls as h^2 from h = 1e-5
down to there (the truncation of the difference; the x87 long double rounds at 1e-19 / h = 1e-11).
"""
import numpy as np

from tests import shape_nv_reference as nvr

LD = np.longdouble
TIE = 16 * float(np.finfo(np.float64).eps)      # on a branch line of an edge: within 16 eps (of fp64, in either dtype) of the numerator's size
ELLIPSE, RECTANGLE, POLYGON = nvr.ELLIPSE, nvr.RECTANGLE, nvr.POLYGON


def _sign(v, T):
    return np.where(v > 0, T(1), np.where(v < 0, T(-1), T(0)))


def _ellipse(p, dp, X, Y, T):
    """The pieces (nx, ny, delta, dnx, dny, ddelta, share) of one ellipse image for the parameter tangent dp of (Rx, Ry, cx, cy, theta): the
    term, its tangents, and the share of the piece in the derivative (1 where the term exists, else 0)."""
    Rx, Ry, cx, cy, th = p
    dRx, dRy, dcx, dcy, dth = dp
    one = T(1)
    c, s = np.cos(th), np.sin(th)
    dc, ds = -s * dth, c * dth
    dx, dy = X - cx, Y - cy
    u, w = c * dx + s * dy, -s * dx + c * dy
    du = dc * dx - c * dcx + ds * dy - s * dcy
    dw = -ds * dx + s * dcx + dc * dy - c * dcy
    U, W = u / Rx, w / Ry
    dU, dW = du / Rx - u * dRx / (Rx * Rx), dw / Ry - w * dRy / (Ry * Ry)
    f = np.hypot(U, W)
    fs = np.where(f > 0, f, one)
    df = (U * dU + W * dW) / fs
    m, dm = (Rx, dRx) if Rx <= Ry else (Ry, dRy)
    delta = np.abs(f - one) * m
    ddelta = _sign(f - one, T) * df * m + np.abs(f - one) * dm
    gu, gw = u / (Rx * Rx), w / (Ry * Ry)
    dgu = du / (Rx * Rx) - 2 * u * dRx / (Rx * Rx * Rx)
    dgw = dw / (Ry * Ry) - 2 * w * dRy / (Ry * Ry * Ry)
    gx, gy = c * gu - s * gw, s * gu + c * gw
    dgx = dc * gu + c * dgu - ds * gw - s * dgw
    dgy = ds * gu + s * dgu + dc * gw + c * dgw
    g = np.hypot(gx, gy)
    on = g > 0
    gs = np.where(on, g, one)
    dg = (gx * dgx + gy * dgy) / gs
    yield gx / gs, gy / gs, delta, dgx / gs - gx * dg / (gs * gs), dgy / gs - gy * dg / (gs * gs), ddelta, np.where(on, one, 0 * one)


def _edge(p, dp, X, Y, T):
    """The two pieces of one edge image, interior and vertex, each with its share: 1 on its own branch, 0 on the other and on a vertex hit, and
    1/2 each for a sample on a branch line (tau = 0 or 1 to within TIE of the numerator's size), whose derivative is the mean of the two
    pieces'."""
    ax, ay, bx, by = p
    dax, day, dbx, dby = dp
    one = T(1)
    ex, ey, dex, dey = bx - ax, by - ay, dbx - dax, dby - day
    l2 = ex * ex + ey * ey
    dl2 = 2 * (ex * dex + ey * dey)
    dx, dy = X - ax, Y - ay
    tau = (dx * ex + dy * ey) / l2
    inner = (tau > 0) & (tau < 1)
    l = np.sqrt(l2)
    dl = dl2 / (2 * l)
    nx, ny = ey / l, -ex / l
    dnx, dny = dey / l - ey * dl / l2, -dex / l + ex * dl / l2
    sd = dx * nx + dy * ny
    dsd = -dax * nx + dx * dnx - day * ny + dy * dny
    num, mag = dx * ex + dy * ey, np.abs(dx * ex) + np.abs(dy * ey)
    tie0, tie1 = np.abs(num) <= T(TIE) * mag, np.abs(num - l2) <= T(TIE) * (mag + l2)
    tie = tie0 | tie1
    inner = inner & ~tie
    first = np.where(tie, tie0, tau <= 0)
    vx, vy = np.where(first, X - ax, X - bx), np.where(first, Y - ay, Y - by)
    dvx, dvy = np.where(first, -dax, -dbx), np.where(first, -day, -dby)
    dv = np.hypot(vx, vy)
    ds = np.where(dv > 0, dv, one)
    ddv = (vx * dvx + vy * dvy) / ds
    hit = ~inner & ~(dv > 0)               # a vertex hit: no term
    half = T(0.5)
    yield (nx + 0 * X, ny + 0 * X, np.abs(sd), dnx + 0 * X, dny + 0 * X, _sign(sd, T) * dsd, np.where(inner, one, np.where(tie & ~hit, half, 0 * one)))
    yield (vx / ds, vy / ds, dv, dvx / ds - vx * ddv / (ds * ds), dvy / ds - vy * ddv / (ds * ds), ddv,
           np.where(inner | hit, 0 * one, np.where(tie, half, one)))


def _dependent(kind, par, j, T):
    """The primitives of one shape that depend on its parameter j, with the tangent of their own parameters: [(fn, p, dp)]."""
    p = [T(v) for v in par]
    dp = [T(1) if i == j else T(0) for i in range(len(p))]
    if kind == ELLIPSE:
        return [(_ellipse, p, dp)]
    if kind == RECTANGLE:
        c, s = np.cos(p[4]), np.sin(p[4])
        dc, ds = -s * dp[4], c * dp[4]
        v, dv = [], []
        for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            u, w, du, dw = sx * p[0] / 2, sy * p[1] / 2, sx * dp[0] / 2, sy * dp[1] / 2
            v.append((p[2] + c * u - s * w, p[3] + s * u + c * w))
            dv.append((dp[2] + dc * u + c * du - ds * w - s * dw, dp[3] + ds * u + s * du + dc * w + c * dw))
    else:
        K = len(p) // 2
        v, dv = [(p[2 * k], p[2 * k + 1]) for k in range(K)], [(dp[2 * k], dp[2 * k + 1]) for k in range(K)]
    out = []
    for k in range(len(v)):
        k1 = (k + 1) % len(v)
        if any(t != 0 for t in dv[k] + dv[k1]):
            out.append((_edge, v[k] + v[k1], dv[k] + dv[k1]))
    return out


def tangents(shapes, a1, a2, n1, n2, dtype=LD):
    """Generator of d nn / d par_k [3, n1, n2] over the parameters k of the packed row (shapes in order, each shape's parameters in order)."""
    T = dtype
    X0, Y0 = nvr.samples(a1, a2, n1, n2, T)
    b1, b2 = [T(v) for v in a1], [T(v) for v in a2]
    eta2 = T(1e-12) * abs(b1[0] * b2[1] - b1[1] * b2[0])
    Jxx, Jxy, Jyy = nvr.structure_tensor(shapes, a1, a2, n1, n2, T)
    d, o, tr = Jxx - Jyy, 2 * Jxy, Jxx + Jyy
    r = np.hypot(d, o)
    on = r > T(nvr.TAU) * tr
    rs = np.where(on, r, T(1))
    half = T(0.5)
    for kind, par in shapes:
        for j in range(len(par)):
            dJ = [np.zeros((n1, n2), dtype=T) for _ in range(3)]
            with np.errstate(divide="ignore", invalid="ignore"):
                for fn, p, dp in _dependent(kind, par, j, T):
                    for pi in (-1, 0, 1):
                        for qi in (-1, 0, 1):
                            X, Y = X0 - pi * b1[0] - qi * b2[0], Y0 - pi * b1[1] - qi * b2[1]
                            for nx, ny, delta, dnx, dny, ddelta, share in fn(p, dp, X, Y, T):
                                live = share > 0
                                t = delta * delta + eta2
                                w = np.where(live, share / (t * t), T(0))
                                dw = np.where(live, -4 * share * delta * ddelta / (t * t * t), T(0))
                                dnx, dny = np.where(live, dnx, T(0)), np.where(live, dny, T(0))
                                dJ[0] += dw * nx * nx + 2 * w * nx * dnx
                                dJ[1] += dw * nx * ny + w * (dnx * ny + nx * dny)
                                dJ[2] += dw * ny * ny + 2 * w * ny * dny
            dd, do = dJ[0] - dJ[2], 2 * dJ[1]
            dr = (d * dd + o * do) / rs
            dc, dsn = dd / rs - d * dr / (rs * rs), do / rs - o * dr / (rs * rs)
            yield np.stack([half * dc, half * dsn, -half * dc]) * on


def gpar(shapes, a1, a2, n1, n2, gnn, dtype=LD):
    """(gpar [npar], scale [npar]) in `dtype`: sum gnn * d nn / d par_k and sum |gnn * d nn / d par_k| over the components and samples."""
    g = np.asarray(gnn).astype(dtype)
    terms = [g * t for t in tangents(shapes, a1, a2, n1, n2, dtype)]
    return np.array([t.sum() for t in terms], dtype=dtype), np.array([np.abs(t).sum() for t in terms], dtype=dtype)
