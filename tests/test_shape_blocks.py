"""Block tests of the vector-shape entries of include/trx.h -- trx_convmat_shapes, trx_toeplitz_sums, trx_convmat_shapes_backward -- through the
C ABI with caller-owned buffers, guard bytes around every output and around the exactly sized workspace, on both backends of
tests/backends.py.

Policy ("Block tests"): err = max |c - c_ref| / max |c_ref| <= 16 * max(e_plain, T * eps), c_ref the 40-digit mpmath reference of
tests/shape_reference.py (Bessel function, exact 1-D integrals, triangle fans -- none of the kernels' algebra), e_plain the error of the float64
numpy / scipy restatement of the closed forms against the same reference, T the number of summed terms (shapes + edges; for a gradient also
the coefficients of the box; gradient boxes (1,1), (4,4) = 289 and (7,5) = 609 coefficients, so that a thread sums several), eps that of fp64.  `out` is held to more: bit-equal to the numpy gather of the returned box cast to the dtype.
No tuned number anywhere.  Every case prints its ratio err / max(e_plain, T eps) with `-s`.

Worst ratios (bound 16), rounded up: WORST_EMU / WORST_MI355X at the end of the file.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import shape_reference as sr
from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import relmax

EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
GUARD = 64
E, R, P = sr.ELLIPSE, sr.RECTANGLE, sr.POLYGON
CELLS = {"square": ((1.0, 0.0), (0.0, 1.0)), "oblique": ((1.0, 0.0), (0.5, math.sqrt(3) / 2))}
RATIOS = {}


def note(entry, backend, what, err, floor):
    ratio = err / floor
    RATIOS[(entry, backend)] = max(RATIOS.get((entry, backend), 0.0), ratio)
    print(f"{entry}[{backend}] {what}: {ratio:.2f} | worst so far {RATIOS[(entry, backend)]:.2f}  (err / max(e_plain, T eps); bound {MARGIN:g})")
    assert err <= MARGIN * floor, f"{what}: err {err:.3e}  floor {floor:.3e}  bound {MARGIN * floor:.3e}"


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------------------
def gbuf(be, nbytes):
    h = be.dev(np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8))
    return h, be.ptr(h) + GUARD


def gread(be, h, dtype, shape):
    a = be.host(h)
    assert (a[:GUARD] == 0xA5).all() and (a[len(a) - GUARD:] == 0xA5).all(), "a kernel wrote outside its buffer"
    return a[GUARD:len(a) - GUARD].view(dtype).reshape(shape).copy()


def rect_mn(mmax, nmax):
    return np.array([(m, n) for m in range(-mmax, mmax + 1) for n in range(-nmax, nmax + 1)], dtype=np.int32)


def circ_mn(cell, mmax, nmax, count):
    from torcwa_amd.lattice import circular_orders
    mn = circular_orders(np.array(CELLS[cell]), n_harmonics=count)
    return np.ascontiguousarray(mn[(np.abs(mn[:, 0]) <= mmax) & (np.abs(mn[:, 1]) <= nmax)].astype(np.int32))


def pack(points):
    """points: per batch entry a list of (kind, par); every entry has the same kinds and lengths."""
    kind = np.array([k for k, _ in points[0]], dtype=np.int32)
    voff = np.concatenate(([0], np.cumsum([len(p) for _, p in points[0]]))).astype(np.int32)
    par = np.array([[v for _, p in pt for v in p] for pt in points], dtype=np.float64)
    return kind, voff, par


def call_shapes(be, dtype, points, vals, cell, mn, mmax, nmax, want_coef=True):
    """(rc, out, box) of trx_convmat_shapes with guarded out / coef / workspace."""
    lib = be.lib
    kind, voff, par = pack(points)
    vals = np.ascontiguousarray(vals, dtype=np.complex128)
    recip, area = sr.recip_of(*CELLS[cell])
    B, N = len(points), len(mn)
    nbox = (4 * mmax + 1) * (4 * nmax + 1)
    isz = np.dtype(dtype).itemsize
    ho, po = gbuf(be, B * N * N * isz)
    hc, pc = gbuf(be, B * nbox * 16)
    nws = lib.convmat_shapes_ws_bytes(dtcode(dtype), B, N, mmax, nmax)
    hw, pw = gbuf(be, nws)
    dk, dv, dp, dl, dm = be.dev(kind), be.dev(voff), be.dev(par), be.dev(vals), be.dev(mn)
    rv = (ctypes.c_double * 4)(*recip)
    rc = lib.convmat_shapes(dtcode(dtype), be.ptr(dk), be.ptr(dv), len(kind), be.ptr(dp), par.shape[1], be.ptr(dl),
                            ctypes.addressof(rv), area, B, be.ptr(dm), N, mmax, nmax, po, pc if want_coef else None,
                            pw, nws, be.stream)
    be.sync()
    gread(be, hw, np.uint8, (nws,))
    return rc, gread(be, ho, dtype, (B, N, N)), gread(be, hc, np.complex128, (B, 4 * mmax + 1, 4 * nmax + 1))


def terms(shapes):
    return sum(len(p) // 2 if k == P else 1 for k, p in shapes)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def regular(K, cx, cy, r, lobes=0.0, phase=0.1):
    t = phase + 2 * np.pi * np.arange(K) / K
    rr = r * (1 + lobes * np.cos(3 * t))
    return [v for x, y in zip(cx + rr * np.cos(t), cy + rr * np.sin(t)) for v in (x, y)]


def rect_poly(Wx, Wy, Cx, Cy, th):
    c, s = math.cos(th), math.sin(th)
    return [v for u, w in ((-Wx / 2, -Wy / 2), (Wx / 2, -Wy / 2), (Wx / 2, Wy / 2), (-Wx / 2, Wy / 2)) for v in (Cx + c * u - s * w, Cy + s * u + c * w)]


L_SHAPE = [0.55, 0.1, 0.95, 0.1, 0.95, 0.25, 0.7, 0.25, 0.7, 0.5, 0.55, 0.5]        # axis-aligned, non-convex: exact zeros of G.e
TRIANGLE = [0.1, 0.55, 0.4, 0.6, 0.2, 0.8]


def case(name):
    """(cell, (mmax, nmax), mn, points [B][S](kind, par), vals [B, S+1])"""
    if name == "ellipse_11":
        return "square", (1, 1), rect_mn(1, 1), [[(E, [0.30, 0.17, 0.5, 0.45, 0.4])]], [[1.0, 11.0 + 0.5j]]
    if name == "gon130_03":               # 260 parameters: two staging passes
        return "oblique", (0, 3), rect_mn(0, 3), [[(P, regular(130, 0.7, 0.42, 0.3, lobes=0.15))]], [[2.1, 9.0 - 0.3j]]
    if name == "mixed_32":                # S = 5, mixed kinds, per-point parameters, a core nested in the ellipse (contrast against its host)
        pts, vals = [], []
        for b in range(3):
            pts.append([(E, [0.17 + 0.01 * b, 0.11, 0.32, 0.27, 0.3]), (R, [0.2 + 0.02 * b, 0.1, 0.95, 0.62, -0.5]), (P, TRIANGLE), (P, L_SHAPE),
                        (E, [0.05 + 0.005 * b, 0.05 + 0.005 * b, 0.32, 0.27, 0.0])])
            e_ell, e_core = 6.0 + 0.2j * b, 2.0 - 0.1j
            vals.append([1.5 + 0.01j, e_ell - (1.5 + 0.01j), 3.0 - (1.5 + 0.01j), 4.0 + 1j - (1.5 + 0.01j), 12.0 - (1.5 + 0.01j), e_core - e_ell])
        return "oblique", (3, 2), circ_mn("oblique", 3, 2, 21), pts, vals
    if name == "rectpoly_44":             # 17 x 17 = 289 coefficients: more than one 256-thread workgroup per entry
        return ("square", (4, 4), rect_mn(4, 4), [[(R, [0.3, 0.2, 0.3, 0.3, 0.35]), (P, rect_poly(0.25, 0.15, 0.7, 0.7, 0.6))]],
                [[1.0, 3.0 + 0.1j, 5.0 - 0.2j]])
    if name == "big_75":
        return ("square", (7, 5), circ_mn("square", 7, 5, 61), [[(E, [0.2, 0.3, 0.4, 0.5, 1.1]), (R, [0.15, 0.6, 0.85, 0.5, 0.2])]],
                [[2.0 + 0.3j, 7.0 - 1j, -0.5 + 0.2j]])
    if name == "gon17_11":
        return "square", (1, 1), rect_mn(1, 1), [[(P, regular(17, 0.45, 0.5, 0.33, lobes=0.1))]], [[1.0, 4.0]]
    if name == "gon17_batch":             # batch 3 on one staging pass, circular list
        return ("oblique", (1, 1), circ_mn("oblique", 1, 1, 7), [[(P, regular(17, 0.6 + 0.02 * (b % 2), 0.4, 0.25, lobes=0.1))] for b in range(3)],
                [[1.0 + 0.1j * b, 4.0] for b in range(3)])
    if name == "edges_11":                # for G = b1 = (2 pi, 0): G.e = 1e-9 on one edge, 2e-3 on another (either side of a series threshold)
        t1 = [0.2, 0.2, 0.6, 0.3, 0.6 + 1e-9 / (2 * np.pi), 0.8]
        t2 = [0.7, 0.1, 0.9, 0.2, 0.9 + 2e-3 / (2 * np.pi), 0.6]
        return "square", (1, 1), rect_mn(1, 1), [[(P, t1), (P, t2)]], [[1.0, 2.0 + 1j, 3.0]]
    raise KeyError(name)


CASES = ["ellipse_11", "gon130_03", "mixed_32", "rectpoly_44", "big_75", "gon17_11", "gon17_batch", "edges_11"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_convmat_shapes(backend, name):
    be = get_backend(backend)
    cell, (mmax, nmax), mn, points, vals = case(name)
    recip, area = sr.recip_of(*CELLS[cell])
    rc, out, box = call_shapes(be, np.complex128, points, vals, cell, mn, mmax, nmax)
    assert rc == 0
    for b, (shapes, val) in enumerate(zip(points, vals)):
        ref = sr.coef_box(shapes, val, recip, area, mmax, nmax)
        plain = sr.plain_box(shapes, np.asarray(val), recip, area, mmax, nmax)
        floor = max(relmax(plain, ref), terms(shapes) * EPS)
        note("convmat_shapes", backend, f"{name}[{b}]", relmax(box[b], ref), floor)
        assert np.array_equal(out[b], sr.gather(box[b], mn, mmax, nmax)), "out is not the gather of the box"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["mixed_32", "rectpoly_44"])
def test_convmat_shapes_complex64_is_the_box_rounded_once(backend, name):
    be = get_backend(backend)
    cell, (mmax, nmax), mn, points, vals = case(name)
    _, out128, box128 = call_shapes(be, np.complex128, points, vals, cell, mn, mmax, nmax)
    rc, out, box = call_shapes(be, np.complex64, points, vals, cell, mn, mmax, nmax)
    assert rc == 0 and np.array_equal(box, box128)                        # all arithmetic is fp64 for both dtypes
    assert np.array_equal(out, sr.gather(box, mn, mmax, nmax).astype(np.complex64))
    rc, out_ws, _ = call_shapes(be, np.complex64, points, vals, cell, mn, mmax, nmax, want_coef=False)      # the box stays in the workspace
    assert rc == 0 and np.array_equal(out_ws, out)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rotated_rectangle_as_polygon_equals_the_rectangle_kind(backend):
    be = get_backend(backend)
    rect = [0.37, 0.21, 0.45, 0.55, 0.4]
    recip, area = sr.recip_of(*CELLS["oblique"])
    mn = rect_mn(1, 1)
    boxes = [call_shapes(be, np.complex128, [[shape]], [[0.0, 1.0]], "oblique", mn, 1, 1)[2][0] for shape in ((R, rect), (P, rect_poly(*rect)))]
    ref = sr.coef_box([(R, rect)], [0.0, 1.0], recip, area, 1, 1)
    for box, shape, T in zip(boxes, ((R, rect), (P, rect_poly(*rect))), (1, 4)):          # both kinds against the one rectangle reference
        e_plain = relmax(sr.plain_box([shape], np.array([0.0, 1.0]), recip, area, 1, 1), ref)
        note("convmat_shapes", backend, "rectangle as kind %d" % shape[0], relmax(box, ref), max(e_plain, T * EPS))


@pytest.mark.parametrize("backend", BACKENDS)
def test_full_cell_rectangle_is_homogeneous(backend):
    be = get_backend(backend)
    eps_s, bg = 7.0 - 0.4j, 2.0
    mn = rect_mn(3, 2)
    rc, out, box = call_shapes(be, np.complex128, [[(R, [1.0, 1.0, 0.5, 0.5, 0.0])]], [[bg, eps_s - bg]], "square", mn, 3, 2)
    assert rc == 0
    ref = np.zeros((13, 9), dtype=np.complex128)
    ref[6, 4] = eps_s
    plain = sr.plain_box([(R, [1.0, 1.0, 0.5, 0.5, 0.0])], np.array([bg, eps_s - bg]), sr.recip_of(*CELLS["square"])[0], 1.0, 3, 2)
    note("convmat_shapes", backend, "full cell", relmax(box[0], ref), max(relmax(plain, ref), EPS))


@pytest.mark.parametrize("backend", BACKENDS)
def test_pixel_aligned_rectangle_against_the_grid_kernel(backend):
    """A rectangle whose edges lie on pixel boundaries of an n1 x n2 raster: the raster is the rectangle convolved with one pixel, so the shapes box
    equals trx_convmat_orders' coefficient times sinc(pi p / n1) sinc(pi q / n2) e^{-i pi (p / n1 + q / n2)}, the transform of the pixel."""
    be = get_backend(backend)
    lib = be.lib
    n1, n2, mmax, nmax = 24, 20, 2, 2
    x0, x1, y0, y1 = 5, 17, 3, 12                                         # pixels [x0, x1) x [y0, y1)
    bg, eps_s = 1.0, 12.0 + 0.5j
    grid = np.full((1, n1, n2), bg, dtype=np.complex128)
    grid[0, x0:x1, y0:y1] = eps_s
    mn = rect_mn(mmax, nmax)
    N = len(mn)
    nws = lib.convmat_orders_ws_bytes(1, 1, n1, n2, N, mmax, nmax)
    hg, hm, ho, hw = be.dev(grid), be.dev(mn), be.empty((1, N, N), np.complex128), be.empty((nws,), np.uint8)
    assert lib.convmat_orders(1, 1, be.ptr(hg), 1, n1, n2, be.ptr(hm), N, mmax, nmax, be.ptr(ho), be.ptr(hw), nws, be.stream) == 0
    Eg = be.host(ho)[0]
    P_, Q_ = np.meshgrid(np.arange(-2 * mmax, 2 * mmax + 1), np.arange(-2 * nmax, 2 * nmax + 1), indexing="ij")
    pixel = np.sinc(P_ / n1) * np.sinc(Q_ / n2) * np.exp(-1j * np.pi * (P_ / n1 + Q_ / n2))

    def unbox(M):                                                         # coefficient (p, q) from any pair with that difference
        box = np.zeros(P_.shape, dtype=np.complex128)
        box[mn[:, None, 0] - mn[None, :, 0] + 2 * mmax, mn[:, None, 1] - mn[None, :, 1] + 2 * nmax] = M
        return box
    rect = (R, [(x1 - x0) / n1, (y1 - y0) / n2, (x0 + x1) / (2 * n1), (y0 + y1) / (2 * n2), 0.0])
    rc, _, box = call_shapes(be, np.complex128, [[rect]], [[bg, eps_s - bg]], "square", mn, mmax, nmax)
    assert rc == 0
    plain = sr.plain_box([rect], np.array([bg, eps_s - bg]), sr.recip_of(*CELLS["square"])[0], 1.0, mmax, nmax)
    plain_grid = np.fft.fft2(grid[0])[P_ % n1, Q_ % n2] / (n1 * n2)
    note("convmat_shapes", backend, "pixel identity", relmax(box[0], unbox(Eg) * pixel), max(relmax(plain, plain_grid * pixel), (n1 + n2) * EPS))


# ---- trx_toeplitz_sums ----------------------------------------------------------------------------------------------------------------------
def call_sums(be, dtype, gE, mn, mmax, nmax):
    lib = be.lib
    B, N = gE.shape[0], len(mn)
    hb, pb = gbuf(be, B * (4 * mmax + 1) * (4 * nmax + 1) * 16)
    nws = lib.toeplitz_sums_ws_bytes(dtcode(dtype), B, N, mmax, nmax)
    hw, pw = gbuf(be, nws)
    dg, dm = be.dev(gE.astype(dtype)), be.dev(mn)
    rc = lib.toeplitz_sums(dtcode(dtype), be.ptr(dg), B, be.ptr(dm), N, mmax, nmax, pb, pw, nws, be.stream)
    be.sync()
    gread(be, hw, np.uint8, (nws,))
    return rc, gread(be, hb, np.complex128, (B, 4 * mmax + 1, 4 * nmax + 1))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["rect25", "rect81", "circular"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_toeplitz_sums(backend, name, dtype):
    be = get_backend(backend)
    mmax, nmax = (4, 4) if name == "rect81" else (2, 2)
    mn = circ_mn("oblique", 2, 2, 13) if name == "circular" else rect_mn(mmax, nmax)
    rng = np.random.default_rng([7, len(mn), np.dtype(dtype).itemsize])
    gE = (rng.standard_normal((2, len(mn), len(mn))) + 1j * rng.standard_normal((2, len(mn), len(mn)))).astype(dtype)
    rc, got = call_sums(be, dtype, gE, mn, mmax, nmax)
    assert rc == 0
    want = np.zeros(got.shape, dtype=np.clongdouble)
    dm, dn = mn[:, None, 0] - mn[None, :, 0] + 2 * mmax, mn[:, None, 1] - mn[None, :, 1] + 2 * nmax
    for b in range(2):
        np.add.at(want[b], (dm, dn), gE[b].astype(np.clongdouble))
    if name == "circular":
        hit = np.zeros(got.shape[1:], dtype=bool)
        hit[dm, dn] = True
        assert not hit.all() and (got[:, ~hit] == 0).all()                 # differences no pair of the list has
    note("toeplitz_sums", backend, f"{name} {np.dtype(dtype).name}", relmax(got, want), len(mn) * EPS)
    assert np.array_equal(call_sums(be, dtype, gE, mn, mmax, nmax)[1], got), "not bit-identical on repetition"


# ---- trx_convmat_shapes_backward --------------------------------------------------------------------------------------------------------------
def plain_dchi(kind, par, j, Gx, Gy, area):
    """float64 restatement of the derivative formulas of include/trx.h (d(chi)/dpar[j] over the box)."""
    import scipy.special
    par = np.asarray(par, dtype=np.float64)
    if kind == P:
        v = par.reshape(-1, 2)
        k, comp, K = j // 2, j % 2, len(par) // 2

        def hat(beta):
            small = np.abs(beta) < 1.0
            bs = np.where(small, beta, 0.0)
            ser = sum((-1j * bs) ** n / (math.factorial(n) * (n + 2)) for n in range(24))
            bl = np.where(small, 1.0, beta)
            return np.where(small, ser, (np.exp(-1j * bl) * (1 + 1j * bl) - 1) / bl ** 2)
        tot = 0
        for a, e in ((v[k - 1], v[k] - v[k - 1]), (v[(k + 1) % K], v[(k + 1) % K] - v[k])):
            nl = e[1] if comp == 0 else -e[0]
            tot = tot + nl * np.exp(-1j * (Gx * a[0] + Gy * a[1])) * hat(Gx * (v[k][0] - a[0]) + Gy * (v[k][1] - a[1]))
        return tot / area
    c, s = np.cos(par[4]), np.sin(par[4])
    gx, gy = c * Gx + s * Gy, -s * Gx + c * Gy
    ph = np.exp(-1j * (Gx * par[2] + Gy * par[3]))
    if j in (2, 3):
        return -1j * (Gx if j == 2 else Gy) * sr.plain_chi(kind, par, Gx, Gy, area)
    if kind == E:
        rho = np.hypot(par[0] * gx, par[1] * gy)
        r1 = np.where(rho == 0, 1.0, rho)
        jinc = np.where(rho == 0, 1.0, 2 * scipy.special.j1(r1) / r1)
        j2 = np.where(rho == 0, 0.25, 2 * scipy.special.jv(2, r1) / r1 ** 2)
        amp = np.pi * par[0] * par[1] / area
        if j == 0:
            return (np.pi * par[1] / area * jinc - amp * j2 * par[0] * gx ** 2) * ph
        if j == 1:
            return (np.pi * par[0] / area * jinc - amp * j2 * par[1] * gy ** 2) * ph
        return -amp * j2 * (par[0] ** 2 - par[1] ** 2) * gx * gy * ph
    tx, ty = gx * par[0] / 2, gy * par[1] / 2
    sinc = lambda t: np.sinc(t / np.pi)

    def dsinc(t):
        small = np.abs(t) < 1.0
        ts = np.where(small, t, 0.0)
        ser = sum((-1) ** n * 2 * n * ts ** (2 * n - 1) / math.factorial(2 * n + 1) for n in range(1, 13))
        tl = np.where(small, 1.0, t)
        return np.where(small, ser, (np.cos(tl) - np.sin(tl) / tl) / tl)
    if j == 0:
        return par[1] / area * np.cos(tx) * sinc(ty) * ph
    if j == 1:
        return par[0] / area * sinc(tx) * np.cos(ty) * ph
    return par[0] * par[1] / area * (dsinc(tx) * par[0] / 2 * gy * sinc(ty) - sinc(tx) * dsinc(ty) * par[1] / 2 * gx) * ph


def call_backward(be, points, vals, cell, mmax, nmax, gbox):
    lib = be.lib
    kind, voff, par = pack(points)
    vals = np.ascontiguousarray(vals, dtype=np.complex128)
    recip, area = sr.recip_of(*CELLS[cell])
    B, S, npar = len(points), len(kind), par.shape[1]
    hp, pp = gbuf(be, B * npar * 8)
    hv, pv = gbuf(be, B * (S + 1) * 16)
    dk, dv, dp, dl, dg = be.dev(kind), be.dev(voff), be.dev(par), be.dev(vals), be.dev(gbox)
    rv = (ctypes.c_double * 4)(*recip)
    rc = lib.convmat_shapes_backward(be.ptr(dk), be.ptr(dv), S, be.ptr(dp), npar, be.ptr(dl), ctypes.addressof(rv), area,
                                     B, mmax, nmax, be.ptr(dg), pp, pv, be.stream)
    be.sync()
    return rc, gread(be, hp, np.float64, (B, npar)), gread(be, hv, np.complex128, (B, S + 1))


SQUARE_POLY = [0.2, 0.2, 0.6, 0.2, 0.6, 0.7, 0.2, 0.7]                     # axis-aligned: G.(v - a) = 0 in the hat integral for whole rows
GRAD_CASES = {
    "ellipse": ("oblique", [[(E, [0.30, 0.17, 0.5, 0.45, 0.4])]], [[1.0, 11.0 + 0.5j]]),
    "circle": ("square", [[(E, [0.25, 0.25, 0.5, 0.5, 0.0])]], [[1.0, 3.0]]),
    "rectangle": ("oblique", [[(R, [0.37, 0.21, 0.45, 0.55, 0.4])]], [[2.0, 5.0 - 1j]]),
    "square": ("square", [[(R, [0.5, 0.5, 0.5, 0.5, 0.0])]], [[2.0, 5.0 - 1j]]),              # G'x W / 2 = 0: the series of sinc'
    "triangle": ("oblique", [[(P, TRIANGLE)]], [[1.0, 4.0 + 1j]]),
    "polygon4": ("square", [[(P, SQUARE_POLY)]], [[1.0, 4.0 + 1j]]),
    "mixed": ("square", [[(E, [0.1 + 0.01 * b, 0.15, 0.25, 0.3, 0.2]), (R, [0.2, 0.3, 0.7, 0.6, 0.1 * b]), (P, TRIANGLE)] for b in range(2)],
              [[1.0 + 0.1j, 2.0, 3.0 - 1j * b, 4.0] for b in range(2)]),
    # boxes larger than one 256-thread workgroup: every thread sums several coefficients before the tree (289 = 256 + 33, 609 = 2 * 256 + 97)
    "box44": ("oblique", [[(E, [0.30 - 0.02 * b, 0.17, 0.5, 0.45, 0.4]), (R, [0.2, 0.3 + 0.05 * b, 0.7, 0.6, -0.3])] for b in range(2)],
              [[1.0, 11.0 + 0.5j, 3.0 - 1j * b] for b in range(2)]),
    "box75": ("square", [[(E, [0.2, 0.3, 0.4, 0.5, 1.1]), (R, [0.5, 0.25, 0.5, 0.375, 0.0])]], [[2.0 + 0.3j, 7.0 - 1j, -0.5 + 0.2j]]),
}
GRAD_BOXES = {"box44": (4, 4), "box75": (7, 5)}                             # every other case: (1, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(GRAD_CASES))
def test_convmat_shapes_backward(backend, name):
    be = get_backend(backend)
    cell, points, vals = GRAD_CASES[name]
    mmax, nmax = GRAD_BOXES.get(name, (1, 1))
    recip, area = sr.recip_of(*CELLS[cell])
    P_, Q_, Gx, Gy = sr._box_G(recip, mmax, nmax)
    rng = np.random.default_rng([11, len(name)])
    gbox = rng.standard_normal((len(points),) + P_.shape) + 1j * rng.standard_normal((len(points),) + P_.shape)
    rc, gpar, gval = call_backward(be, points, vals, cell, mmax, nmax, gbox)
    assert rc == 0
    for b, (shapes, val) in enumerate(zip(points, vals)):
        want, plain, nterm = [], [], 0
        for s, (kind, par) in enumerate(shapes):
            d = sr.dchi_box(kind, par, recip, area, mmax, nmax)
            g = gbox[b].astype(np.clongdouble)
            want += [np.real(np.sum(np.conj(g) * np.clongdouble(val[s + 1]) * d[j])) for j in range(len(par))]
            plain += [np.real(np.sum(np.conj(gbox[b]) * val[s + 1] * plain_dchi(kind, par, j, Gx, Gy, area))) for j in range(len(par))]
            nterm = max(nterm, 2 if kind == P else 1)
        want, plain = np.array(want), np.array(plain, dtype=np.float64)
        floor = max(relmax(plain, want), nterm * P_.size * EPS)
        note("convmat_shapes_backward", backend, f"{name}[{b}] gpar", relmax(gpar[b], want), floor)
        chi = sr.chi_box(shapes, recip, area, mmax, nmax)
        wv = np.array([gbox[b][2 * mmax, 2 * nmax]] + [np.sum(np.conj(chi[s]) * gbox[b].astype(np.clongdouble)) for s in range(len(shapes))])
        pv = np.array([gbox[b][2 * mmax, 2 * nmax]] + [np.sum(np.conj(sr.plain_chi(k, p, Gx, Gy, area)) * gbox[b]) for k, p in shapes])
        note("convmat_shapes_backward", backend, f"{name}[{b}] gval", relmax(gval[b], wv), max(relmax(pv, wv), terms(shapes) * P_.size * EPS))
    again = call_backward(be, points, vals, cell, mmax, nmax, gbox)
    assert np.array_equal(again[1], gpar) and np.array_equal(again[2], gval), "not bit-identical on repetition"


# ---- error paths ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_error_codes(backend):
    be = get_backend(backend)
    lib = be.lib
    ARG, WS, DT = -2, -3, -1
    mn = rect_mn(1, 1)
    ok = [[(E, [0.3, 0.2, 0.5, 0.5, 0.0])]]
    assert call_shapes(be, np.complex128, ok, [[1.0, 2.0]], "square", mn, 1, 1)[0] == 0

    def raw(kind, voff, npar=5, S=1, area=1.0, dtype=1, N=9, mn_=mn, ws_short=0, mmax=1):
        par, val = np.full((1, max(npar, 1)), 0.25), np.ones((1, S + 1), dtype=np.complex128)
        out, coef = be.empty((1, 9, 9), np.complex128), be.empty((1, 4 * mmax + 1, 5), np.complex128)
        nws = lib.convmat_shapes_ws_bytes(1, 1, 9, mmax, 1)
        ws = be.empty((nws,), np.uint8)
        hs = [be.dev(np.array(kind, dtype=np.int32)), be.dev(np.array(voff, dtype=np.int32)), be.dev(par), be.dev(val), be.dev(mn_)]
        rv = (ctypes.c_double * 4)(2 * np.pi, 0, 0, 2 * np.pi)
        rc = lib.convmat_shapes(dtype, be.ptr(hs[0]), be.ptr(hs[1]), S, be.ptr(hs[2]), npar, be.ptr(hs[3]),
                                ctypes.addressof(rv), area, 1, be.ptr(hs[4]), N, mmax, 1, be.ptr(out),
                                None if ws_short else be.ptr(coef), be.ptr(ws), nws - ws_short, be.stream)
        be.sync()
        return rc
    assert raw([0], [0, 5]) == 0
    assert raw([3], [0, 5]) == ARG                                         # unknown kind
    assert raw([0], [0, 4]) == ARG and raw([1], [0, 6], npar=6) == ARG     # an ellipse / rectangle has five parameters
    assert raw([2], [0, 4]) == ARG and raw([2], [0, 5]) == ARG             # K < 3; an odd number of coordinates
    assert raw([0], [0, 5], npar=4) == ARG                                 # offsets past the row
    assert raw([0, 0], [5, 10, 5], npar=10, S=2) == ARG                    # decreasing offsets
    assert raw([0], [0, 5], area=0.0) == ARG and raw([0], [0, 5], area=-1.0) == ARG
    assert raw([0], [0, 5], dtype=7) == DT
    assert raw([0], [0, 5], ws_short=16) == WS
    assert raw([0], [0, 5], mn_=np.array([[2, 0]] * 9, dtype=np.int32)) == ARG          # a harmonic outside the box
    # backward: the same checks of kind / voff / area
    gbox = np.ones((1, 5, 5), dtype=np.complex128)
    assert call_backward(be, ok, [[1.0, 2.0]], "square", 1, 1, gbox)[0] == 0
    assert call_backward(be, [[(5, [0.3, 0.2, 0.5, 0.5, 0.0])]], [[1.0, 2.0]], "square", 1, 1, gbox)[0] == ARG
    assert call_backward(be, [[(P, [0.1, 0.1, 0.5, 0.1])]], [[1.0, 2.0]], "square", 1, 1, gbox)[0] == ARG
    # toeplitz sums: dtype, workspace, a harmonic outside the box, a repeated harmonic
    gE = np.ones((1, 9, 9), dtype=np.complex128)
    assert call_sums(be, np.complex128, gE, mn, 1, 1)[0] == 0
    dup = mn.copy()
    dup[3] = dup[2]
    assert call_sums(be, np.complex128, gE, dup, 1, 1)[0] == ARG
    assert call_sums(be, np.complex128, gE, mn * 2, 1, 1)[0] == ARG
    hb, hw, dg, dm = be.empty((1, 5, 5), np.complex128), be.empty((64,), np.uint8), be.dev(gE), be.dev(mn)
    assert lib.toeplitz_sums(1, be.ptr(dg), 1, be.ptr(dm), 9, 1, 1, be.ptr(hb), be.ptr(hw), 8, be.stream) == WS
    assert lib.toeplitz_sums(5, be.ptr(dg), 1, be.ptr(dm), 9, 1, 1, be.ptr(hb), be.ptr(hw), 64, be.stream) == DT


# Worst err / max(e_plain, T eps) per entry over all the cases a backend runs, rounded up (the bound is 16).
WORST_EMU = {"convmat_shapes": 1.0, "toeplitz_sums": 0.1, "convmat_shapes_backward": 0.3}
WORST_MI355X = {"convmat_shapes": 0.9, "toeplitz_sums": 0.1, "convmat_shapes_backward": 0.2}
