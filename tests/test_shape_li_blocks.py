"""Block tests of Li's rule on axis-aligned rectangles -- trx_convmat_li_shapes, trx_convmat_li_shapes_backward -- through the C ABI with
caller-owned buffers, guard bytes around every output and around the exactly sized workspace, on both backends of tests/backends.py.

Policy (tests/test_fourier_blocks.py): err = relmax(kernel, reference) <= 16 * max(e_plain, T * eps) against tests/shape_li_reference.li
(np.clongdouble: unique breakpoints, midpoint states, antiderivative differences, solve_hp), e_plain the error of the same algebra in float64,
eps that of fp64, T = sum over the strips of (1 + the rectangles active in the strip) + w the number of summed terms: every entry of F sums the
strips, a strip's coefficients sum the background and its active rectangles (counted from the reference's own point-in-rectangle states, the
direction with more terms), and the inverse takes dot products of the block size w = 2 max(ox, oy) + 1.

Guards, asserted on the reference's Toeplitz blocks of every case: cond <= 1e4; and plain partial pivoting interchanges rows at >= half of
the steps of a direction's blocks taken together.  The reading chosen for "a direction's blocks": the strips that hold a rectangle -- the
block of a strip of bare background is rval[0] I, which no data makes pivot (nor the diagonal block of a rectangle as wide as the cell).  rval is complex of random phase, (0.5 + u) e^{2 pi i v} like the
"phase" grids of that file, with the contrast of a rectangle divided by the larger of its fills Wx / Lx, Wy / Ly so that the diagonal a[0] = rval_0 +
sum rval_s f_s is a sum of terms of one size; the seed of a case is the smallest one that passes the guards (SEEDS, searched on the CPU).

Backward: trx_convmat_li_shapes_backward fed with the adjoints of the tables that the composition of torcwa_amd.autograd_ops.ShapeLiFn forms (here
in numpy, from the kernel's own Ux / Uy and breakpoints) for random gEx, gEy, against Richardson-extrapolated differences of
l = Re <gEx, Ex> + Re <gEy, Ey> of the reference; same policy with the difference's own truncation estimate in the floor, e_plain from the
float64 autograd restatement shape_li_reference.li_torch, errors relative to the largest component of the case's gradient.  At a tie the
adjoint is the one-sided derivative towards the side on which the tied strip opens (include/trx.h), and the difference is taken on that side.

Every case prints its ratio err / floor with `-s`.  Worst ratios (bound 16), rounded up: WORST_EMU / WORST_MI355X at the end of the file.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import shape_li_reference as lr
from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import crandn, lu_interchanges, relmax
from tests import shape_reference as sr
from tests.test_shape_blocks import gbuf, gread, pack, rect_mn

EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
R = 1
ARG, WS, DT, UNSUPPORTED = -2, -3, -1, -5
C128, C64 = np.complex128, np.complex64
RATIOS = {}
LX, LY = 1.0, 1.25                    # dyadic periods: edges placed on dyadic numbers tie, wrap and meet the boundary exactly


def note(entry, backend, what, err, floor):
    ratio = err / floor
    RATIOS[(entry, backend)] = max(RATIOS.get((entry, backend), 0.0), ratio)
    print(f"{entry}[{backend}] {what}: {ratio:.2f} | worst so far {RATIOS[(entry, backend)]:.2f}  (err / floor; bound {MARGIN:g})")
    assert err <= MARGIN * floor, f"{what}: err {err:.3e}  floor {floor:.3e}  bound {MARGIN * floor:.3e}"


def call_li(be, dtype, points, rvals, ox, oy, keep=True, Lx=LX, Ly=LY, ws_short=0, **over):
    """(rc, dict(Ex, Ey, info[, Ux, Uy, brk, rec])) of trx_convmat_li_shapes with guarded outputs, info and workspace."""
    kind, voff, par = pack(points)
    kind = np.asarray(over.pop("kinds", kind), dtype=np.int32)
    rvals = np.ascontiguousarray(rvals, dtype=C128)
    B, S = len(points), len(kind)
    K, wx, wy = 2 * S + 1, 2 * ox + 1, 2 * oy + 1
    N = wx * wy
    isz = np.dtype(dtype).itemsize
    bufs = dict(Ex=gbuf(be, B * N * N * isz), Ey=gbuf(be, B * N * N * isz), info=gbuf(be, B * 4))
    if keep:
        bufs.update(Ux=gbuf(be, B * K * wy * wy * 16), Uy=gbuf(be, B * K * wx * wx * 16), brk=gbuf(be, B * 2 * (K + 1) * 8),
                    rec=gbuf(be, B * 2 * 3 * S * 4))
    opt = lambda k: bufs[k][1] if keep else None
    a = dict(code=dtcode(dtype), S=S, npar=par.shape[1], batch=B, ox=over.pop("ox_arg", ox), oy=oy)
    a.update(over)
    nws = be.lib.convmat_li_shapes_ws_bytes(dtcode(dtype), B, S, ox, oy)
    hw, pw = gbuf(be, nws)
    dk, dv, dp, dr = be.dev(kind), be.dev(voff), be.dev(par), be.dev(rvals)
    rc = be.lib.convmat_li_shapes(a["code"], be.ptr(dk), be.ptr(dv), a["S"], be.ptr(dp), a["npar"], be.ptr(dr), Lx, Ly, a["batch"], a["ox"],
                                  a["oy"], bufs["Ex"][1], bufs["Ey"][1], opt("Ux"), opt("Uy"), opt("brk"), opt("rec"), bufs["info"][1], pw,
                                  nws - ws_short, be.stream)
    be.sync()
    gread(be, hw, np.uint8, (nws,))
    out = dict(Ex=gread(be, bufs["Ex"][0], dtype, (B, N, N)), Ey=gread(be, bufs["Ey"][0], dtype, (B, N, N)),
               info=gread(be, bufs["info"][0], np.int32, (B,)))
    if keep:
        out.update(Ux=gread(be, bufs["Ux"][0], C128, (B, K, wy, wy)), Uy=gread(be, bufs["Uy"][0], C128, (B, K, wx, wx)),
                   brk=gread(be, bufs["brk"][0], np.float64, (B, 2, K + 1)), rec=gread(be, bufs["rec"][0], np.int32, (B, 2, S, 3)))
    return rc, out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
GENERIC = [(0.45, 0.5, 0.4, 0.6)]
TIE = [(0.3, 0.25, 0.3, 0.5), (0.25, 0.25, 0.7, 0.75)]           # the upper y-edge of the first is the lower y-edge of the second: 0.625
NESTED = [(0.5, 0.6, 0.9, 1.1), (0.2, 0.25, 0.95, 1.15)]         # a host that wraps in both directions, and a core inside it


def many(S):
    """S small rectangles at jittered sites of a 12 x 11 raster of the cell: disjoint, every edge coordinate distinct."""
    rng = np.random.default_rng([7, S])
    sites = rng.permutation(12 * 11)[:S]
    return [(LX / 12 * (0.3 + 0.4 * rng.random()), LY / 11 * (0.3 + 0.4 * rng.random()), LX / 12 * (s % 12 + 0.45 + 0.1 * rng.random()),
             LY / 11 * (s // 12 + 0.45 + 0.1 * rng.random())) for s in sites]


# name -> (ox, oy, per-point rectangle lists)
CASES = {
    "s1_o11": (1, 1, [GENERIC]), "s1_o21": (2, 1, [GENERIC]), "s1_o13": (1, 3, [GENERIC]), "s1_o02": (0, 2, [GENERIC]),
    "s1_o30": (3, 0, [GENERIC]),
    "wrap_x": (2, 1, [[(0.5, 0.4, 0.9, 0.6)]]), "wrap_y": (2, 1, [[(0.5, 0.6, 0.5, 1.2)]]), "wrap_xy": (2, 1, [[(0.5, 0.6, 0.9, 1.2)]]),
    "boundary": (2, 1, [[(0.5, 0.5, 0.25, 1.0)]]),               # Cy + Wy/2 = Ly and Cx - Wx/2 = 0, exactly
    "lamellar": (2, 2, [[(0.5, LY, 0.4, 0.7)]]),                 # Wy = Ly
    "nested": (2, 1, [NESTED]), "tie": (1, 2, [TIE]),
    "batch3": (1, 1, [[(0.3, 0.4, 0.3, 0.5), (0.25, 0.3, 0.7, 0.75)], [(0.3, 0.4, 0.35, 0.9), (0.25, 0.3, 0.8, 0.45)],
                      [(0.3, 0.4, 0.9, 1.1), (0.25, 0.3, 0.45, 0.3)]]),      # the breakpoints of the three points sort in three orders
    "s32": (1, 1, [many(32)]), "s127": (1, 0, [many(127)]),
    "w65": (32, 0, [[(0.45, 0.5, 0.4, 0.6)]]),
}
# the smallest seed at which a case passes the guards (0 where not listed)
SEEDS = {("s1_o11", 0): 1, ("s1_o13", 0): 12, ("s1_o02", 0): 1, ("wrap_x", 0): 9, ("wrap_y", 0): 10, ("wrap_xy", 0): 31, ("boundary", 0): 4,
         ("lamellar", 0): 4, ("nested", 0): 5, ("tie", 0): 49, ("batch3", 0): 1, ("batch3", 1): 11, ("batch3", 2): 8, ("s32", 0): 6, ("w65", 0): 21}


def rval_of(name, rects, b):
    rng = np.random.default_rng([11, sum(map(ord, name)), b, SEEDS.get((name, b), 0)])
    S = len(rects)
    v = (0.5 + rng.random(S + 1)) * np.exp(2j * np.pi * rng.random(S + 1))
    fill = np.array([1.0] + [max(r[0] / LX, r[1] / LY) for r in rects])
    return v / fill


def guards(Tblocks, rects, axis, Ls):
    """(worst cond, interchange fraction over the blocks of the strips that hold a rectangle) of one direction."""
    T = Tblocks.astype(C128)
    _, inside = lr.strips(rects, axis, Ls)
    worst = max(float(np.linalg.cond(t)) for t in T)
    w = T.shape[1]
    Lc = LX if axis == 1 else LY
    spans = np.array([r[1 - axis] == Lc for r in rects])              # a rectangle as wide as the cell adds to a[0] alone: a diagonal block
    held = [t for t, ins in zip(T, inside) if (ins & ~spans).any()]
    steps = len(held) * (w - 1)
    frac = sum(lu_interchanges(t) for t in held) / steps if steps else None
    return worst, frac


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per point (rects, rval, Ex, Ey, Ex_plain, Ey_plain, summed terms), computed once and shared by the tests and both backends; the guards are
    asserted here."""
    ox, oy, points = CASES[name]
    out = []
    for b, rects in enumerate(points):
        rv = rval_of(name, rects, b)
        Ex, Ey, Tx, Ty = lr.li(rects, rv, LX, LY, ox, oy, want_blocks=True)
        Exp, Eyp = lr.li(rects, rv, LX, LY, ox, oy, dtype=C128)
        summed = 0
        for T, axis, Ls in ((Tx, 1, LY), (Ty, 0, LX)):
            cond, frac = guards(T, rects, axis, Ls)
            assert cond <= 1e4, (name, b, cond)
            assert frac is None or frac >= 0.5, (name, b, axis, frac)
            summed = max(summed, int((1 + lr.strips(rects, axis, Ls)[1].sum(axis=1)).sum()))      # sum over the strips of 1 + active rectangles
        out.append((rects, rv, Ex, Ey, Exp, Eyp, summed))
    return out


def points_of(name):
    return [[(R, list(r) + [0.0]) for r in rects] for rects in CASES[name][2]]


def terms(name, summed):
    """T of the floor: the terms summed into an entry -- over the strips of the direction that has more of them, the background and the
    rectangles ACTIVE in the strip (the seventh entry of reference()) -- and the block size w of the inverse's dot products."""
    ox, oy, _ = CASES[name]
    return summed + 2 * max(ox, oy) + 1


def check_case(backend, name, keep):
    be = get_backend(backend)
    ox, oy, _ = CASES[name]
    ref = reference(name)
    rc, o = call_li(be, C128, points_of(name), [r[1] for r in ref], ox, oy, keep)
    assert rc == 0 and not o["info"].any()
    for b, (rects, rv, Ex, Ey, Exp, Eyp, strips) in enumerate(ref):
        for k, got, hp, plain in (("Ex", o["Ex"][b], Ex, Exp), ("Ey", o["Ey"][b], Ey, Eyp)):
            e_plain = relmax(plain, hp)
            note("convmat_li_shapes", backend, f"{name} keep={keep} {k} b{b} e_plain {e_plain:.1e}", relmax(got, hp),
                 max(e_plain, terms(name, strips) * EPS))
    rc, o64 = call_li(be, C64, points_of(name), [r[1] for r in ref], ox, oy, keep)
    assert rc == 0 and not o64["info"].any()
    assert np.array_equal(o64["Ex"], o["Ex"].astype(C64)) and np.array_equal(o64["Ey"], o["Ey"].astype(C64)), "complex64 is not complex128 rounded once"
    return o


def test_reference_self_check_against_the_grid_definition():
    """The REFERENCE's own test (it runs no code of the library and passes with or without the feature): shape_li_reference.self_check
    compares the reference with the definition of trx_convmat_li (li_ref of tests/test_li_factorisation.py) on rasters whose samples lie half
    a pixel from every edge.  The raster error is second order: it must fall to <= 1/3 per doubling from n = 64 to 256 (1/4 predicted; a
    first-order error would give 1/2)."""
    errs = lr.self_check()
    print(f"max |F_grid - F_strips| / max |F| at n = 64, 128, 256: {errs}; ratios {errs[1] / errs[0]:.3f}, {errs[2] / errs[1]:.3f}")
    assert errs[0] > 1e-6 and errs[1] <= errs[0] / 3 and errs[2] <= errs[1] / 3, errs


SMALL = [n for n in CASES if n not in ("s127", "w65")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_convmat_li_shapes(backend, name, keep):
    """Orders (1,1), (2,1), (1,3), (0,2), (3,0) on a 1 x 1.25 cell; a rectangle that wraps in x, in y, in both; edges exactly on the cell
    boundary; the lamellar case; a nested core; two rectangles that share an edge coordinate; a batch of three whose breakpoints sort in
    three orders; S = 32 (K = 65: the rank sort leaves one wave, and without Ux / Uy the inverses run in 17 chunks of strips).  keep: Ux, Uy
    and the strip record are outputs."""
    o = check_case(backend, name, keep)
    if keep:
        ox, oy, points = CASES[name]
        for b, rects in enumerate(points):
            S = len(rects)
            for d, L in ((0, LY), (1, LX)):
                t = o["brk"][b, d]
                assert t[0] == 0.0 and t[-1] == L and (np.diff(t) >= 0).all()
                ranks = np.sort(o["rec"][b, d, :, :2].ravel())
                assert ranks.tolist() == list(range(1, 2 * S + 1))                      # a permutation: the origin keeps rank 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_repetition_is_bit_identical_and_kept_inverses_match(backend):
    """Two calls give the same bits; without ties the kernel's strips are the reference's, and Ux / Uy are held to the policy as well."""
    be = get_backend(backend)
    name = "nested"
    ox, oy, points = CASES[name]
    rects, rv = reference(name)[0][:2]
    rc, a = call_li(be, C128, points_of(name), [rv], ox, oy, True)
    rc2, b = call_li(be, C128, points_of(name), [rv], ox, oy, True)
    assert rc == 0 and rc2 == 0
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    c, d = call_li(be, C128, points_of(name), [rv], ox, oy, False), call_li(be, C128, points_of(name), [rv], ox, oy, False)
    assert c[0] == 0 and d[0] == 0 and all(c[1][k].tobytes() == d[1][k].tobytes() for k in c[1])     # the chunked path, too
    for key, axis, Ls, Lc, os_, oc in (("Uy", 1, LY, LX, oy, ox), ("Ux", 0, LX, LY, ox, oy)):
        _, _, U = lr.direction(rects, rv, axis, Ls, Lc, os_, oc)
        _, _, Up = lr.direction(rects, rv, axis, Ls, Lc, os_, oc, dtype=C128)
        assert U.shape == a[key][0].shape
        note("convmat_li_shapes", backend, f"{name} {key}", relmax(a[key][0], U), max(relmax(Up, U), (2 * oc + 1) * EPS))


@pytest.mark.parametrize("backend", BACKENDS)
def test_lamellar_is_laurent_in_y(backend):
    """Wy = Ly: nothing varies along y, so F = U delta_q0 (Ex couples no n != n') and Ey is Laurent's matrix of eps, the `out` of
    trx_convmat_shapes, to the bound of the case."""
    be = get_backend(backend)
    name = "lamellar"
    ox, oy, points = CASES[name]
    rects, rv, Ex, Ey, Exp, Eyp, strips = reference(name)[0]
    rc, o = call_li(be, C128, points_of(name), [rv], ox, oy, False)
    assert rc == 0 and not o["info"].any()
    floor = max(relmax(Eyp, Ey), relmax(Exp, Ex), terms(name, strips) * EPS)
    wx, wy = 2 * ox + 1, 2 * oy + 1
    off = o["Ex"][0].reshape(wx, wy, wx, wy) * (1 - np.eye(wy))[None, :, None, :]
    note("convmat_li_shapes", backend, "lamellar: Ex off n = n'", float(np.abs(off).max() / np.abs(o["Ex"][0]).max()), floor)
    # Laurent's E of the same structure on the same cell
    eps_bg, eps_in = 1 / rv[0], 1 / (rv[0] + rv[1])
    kind, voff, par = pack(points_of(name))
    mn = rect_mn(ox, oy)
    recip, area = sr.recip_of((LX, 0.0), (0.0, LY))
    N = len(mn)
    ho, po = gbuf(be, N * N * 16)
    nws = be.lib.convmat_shapes_ws_bytes(1, 1, N, ox, oy)
    hw, pw = gbuf(be, nws)
    hs = [be.dev(a) for a in (kind, voff, par, np.array([[eps_bg, eps_in - eps_bg]], dtype=C128), mn)]
    rcp = (ctypes.c_double * 4)(*recip)
    assert be.lib.convmat_shapes(1, be.ptr(hs[0]), be.ptr(hs[1]), 1, be.ptr(hs[2]), 5, be.ptr(hs[3]), ctypes.addressof(rcp), area, 1,
                                 be.ptr(hs[4]), N, ox, oy, po, None, pw, nws, be.stream) == 0
    be.sync()
    E = gread(be, ho, C128, (N, N))
    note("convmat_li_shapes", backend, "lamellar: Ey against Laurent's E", relmax(o["Ey"][0], E), floor)


@pytest.mark.parametrize("backend", BACKENDS)
def test_size_limits(backend):
    """S = 127 (K = 255 events, the most one workgroup sorts) is accepted and correct, S = 128 is TRX_ERR_UNSUPPORTED; a block of w = 65
    (ox = 32: the pivot-search stride and the 67 KB LDS opt-in of the Toeplitz inverse); order 50 (w = 101) is refused like trx_convmat_li.
    A refused call writes nothing."""
    be = get_backend(backend)
    check_case(backend, "s127", False)
    check_case(backend, "w65", True)
    pts = [[(R, list(r) + [0.0]) for r in many(128)]]
    rc, o = call_li(be, C128, pts, np.ones((1, 129)), 1, 0, True)
    assert rc == UNSUPPORTED and all((v.view(np.uint8) == 0xA5).all() for v in o.values())
    for ox, oy in ((50, 0), (0, 50)):
        rc, o = call_li(be, C128, points_of("s1_o11"), np.ones((1, 2)), ox, oy, False)
        assert rc == UNSUPPORTED and all((v.view(np.uint8) == 0xA5).all() for v in o.values())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("keep", [True, False])
def test_info(backend, keep):
    """info per point, each code provoked by its input, next to a point that stays correct: 1 an rval entry that is not finite, or a zero
    background; 2 a singular block (order 0: a[0] = 1 - 2 * 0.5 = 0 inside the rectangle); 3 a rotated rectangle, a width of 0, a width
    beyond the cell."""
    be = get_backend(backend)
    good = [(R, [0.5, 0.5, 0.4, 0.6, 0.0])]
    rv = np.array([1.0, -0.75])
    rc, want = call_li(be, C128, [good], [rv], 1, 1, keep)
    assert rc == 0 and want["info"].tolist() == [0]
    bad_rv = [np.array([1.0, np.nan]), np.array([np.inf, -0.75]), np.array([0.0, 1.0])]
    bad_geom = [[0.5, 0.5, 0.4, 0.6, 0.1], [0.0, 0.5, 0.4, 0.6, 0.0], [0.5, -0.1, 0.4, 0.6, 0.0], [1.5, 0.5, 0.4, 0.6, 0.0], [0.5, 1.3, 0.4, 0.6, 0.0]]
    trials = [([good, good], [rv, r], 1) for r in bad_rv] + [([good, [(R, g)]], [rv, rv], 3) for g in bad_geom]
    for pts, rvs, code in trials:
        rc, o = call_li(be, C128, pts, rvs, 1, 1, keep)
        assert rc == 0 and o["info"].tolist() == [0, code], (rvs, pts, o["info"])
        assert o["Ex"][0].tobytes() == want["Ex"][0].tobytes() and o["Ey"][0].tobytes() == want["Ey"][0].tobytes()
    rc, o = call_li(be, C128, [good, good], [rv, np.array([1.0, -2.0])], 0, 0, keep)
    assert rc == 0 and o["info"].tolist() == [0, 2]
    assert np.isfinite(o["Ex"][0]).all() and np.isfinite(o["Ey"][0]).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_error_codes(backend):
    be = get_backend(backend)
    pts, rv = points_of("s1_o11"), np.array([[1.0, -0.75]])
    untouched = lambda o: all((v.view(np.uint8) == 0xA5).all() for v in o.values())
    assert call_li(be, C128, pts, rv, 1, 1)[0] == 0
    for kinds in ([0], [2], [3]):                                # an ellipse, a polygon, an unknown kind: rectangles only
        rc, o = call_li(be, C128, pts, rv, 1, 1, kinds=kinds)
        assert rc == ARG and untouched(o)
    rc, o = call_li(be, C128, [[(R, [0.5, 0.5, 0.4, 0.6])]], rv, 1, 1)                   # a rectangle has five parameters
    assert rc == ARG and untouched(o)
    for kw in (dict(batch=0), dict(batch=65536), dict(S=0), dict(ox_arg=-1), dict(Lx=0.0), dict(Ly=-1.0), dict(Lx=float("inf"))):
        rc, o = call_li(be, C128, pts, rv, 1, 1, **kw)
        assert rc == ARG and untouched(o), kw
    assert call_li(be, C128, pts, rv, 1, 1, ws_short=16)[0] == WS
    assert call_li(be, C128, pts, rv, 1, 1, code=7)[0] == DT


# ---- the adjoint ----------------------------------------------------------------------------------------------------------------------------------
def tix(o):
    a = np.arange(2 * o + 1)
    return (a[:, None] - a[None, :] + 2 * o).ravel()


def table_adjoints(o, b, gEx, gEy, ox, oy):
    """(ga_x, gw_y, ga_y, gw_x) of point b: the composition of ShapeLiFn.backward in numpy, from the forward's Ux, Uy and breakpoints."""
    wx, wy = 2 * ox + 1, 2 * oy + 1

    def weights(t, os_, L):
        f, mid, q = (np.diff(t) / L)[:, None], ((t[1:] + t[:-1]) / 2)[:, None], np.arange(-2 * os_, 2 * os_ + 1)[None, :]
        return f * np.sinc(q * f) * np.exp(-2j * np.pi * q * mid / L)

    def one(g, U, wgt, o_other, o_own):
        K, w, _ = U.shape
        gF = np.zeros((w * w, 4 * o_other + 1), dtype=C128)
        np.add.at(gF, (slice(None), tix(o_other)), g)
        gU = (np.conj(wgt) @ gF.T).reshape(K, w, w)
        UH = np.conj(U.transpose(0, 2, 1))
        gT = -(UH @ gU @ UH)
        ga = np.zeros((K, 4 * o_own + 1), dtype=C128)
        np.add.at(ga, (slice(None), tix(o_own)), gT.reshape(K, w * w))
        return ga, np.conj(U.reshape(K, w * w)) @ gF

    ga_x, gw_y = one(gEx.reshape(wx, wy, wx, wy).transpose(0, 2, 1, 3).reshape(wx * wx, wy * wy), o["Uy"][b], weights(o["brk"][b, 0], oy, LY), oy, ox)
    ga_y, gw_x = one(gEy.reshape(wx, wy, wx, wy).transpose(1, 3, 0, 2).reshape(wy * wy, wx * wx), o["Ux"][b], weights(o["brk"][b, 1], ox, LX), ox, oy)
    return ga_x, gw_y, ga_y, gw_x


def call_backward(be, points, rvals, ox, oy, o, tabs, **over):
    """(rc, gpar [B, npar], grval [B, S+1]) of trx_convmat_li_shapes_backward with guarded outputs."""
    kind, voff, par = pack(points)
    kind = np.asarray(over.pop("kinds", kind), dtype=np.int32)
    B, S = len(points), len(kind)
    hp, pp = gbuf(be, B * par.shape[1] * 8)
    hv, pv = gbuf(be, B * (S + 1) * 16)
    hs = [be.dev(a) for a in (kind, voff, par, np.ascontiguousarray(rvals, dtype=C128), np.ascontiguousarray(o["brk"]),
                               np.ascontiguousarray(o["rec"]))] + [be.dev(np.ascontiguousarray(t, dtype=C128)) for t in tabs]
    a = dict(S=S, batch=B)
    a.update(over)
    rc = be.lib.convmat_li_shapes_backward(be.ptr(hs[0]), be.ptr(hs[1]), a["S"], be.ptr(hs[2]), par.shape[1], be.ptr(hs[3]), LX, LY, a["batch"],
                                           ox, oy, be.ptr(hs[4]), be.ptr(hs[5]), *[be.ptr(h) for h in hs[6:]], pp, pv, be.stream)
    be.sync()
    return rc, gread(be, hp, np.float64, (B, par.shape[1])), gread(be, hv, C128, (B, S + 1))


# (rectangle, parameter) -> the side of the one-sided difference at the tie of TIE: the side on which the strip between the two tied edges
# opens (rectangle 0 closes at 0.625 before rectangle 1 opens there: the strip holds neither)
TIE_SIDES = {(0, 1): -1, (0, 3): -1, (1, 1): -1, (1, 3): +1}


@functools.lru_cache(maxsize=None)
def gradient_reference(name):
    """Per point (gEx, gEy, gpar_ref [S, 4], grval_ref [S+1], truncation estimates of both, gpar_plain, grval_plain)."""
    import torch
    ox, oy, points = CASES[name]
    N = (2 * ox + 1) * (2 * oy + 1)
    out = []
    for b, (rects, rv, *_) in enumerate(reference(name)):
        rng = np.random.default_rng([13, sum(map(ord, name)), b])
        gEx, gEy = crandn(rng, (N, N)), crandn(rng, (N, N))
        gxl, gyl = np.conj(gEx).astype(lr.CLD), np.conj(gEy).astype(lr.CLD)

        def loss(rc, rvv):
            Ex, Ey = lr.li(rc, rvv, LX, LY, ox, oy)
            return ((gxl * Ex).sum() + (gyl * Ey).sum()).real

        S = len(rects)
        gp, tp = np.zeros((S, 4), dtype=lr.LD), np.zeros((S, 4), dtype=lr.LD)
        for s in range(S):
            for j in range(4):
                def f(off, s=s, j=j):
                    rc = [list(map(lr.LD, r)) for r in rects]
                    rc[s][j] = rc[s][j] + off
                    return loss(rc, rv.astype(lr.CLD))
                side = TIE_SIDES.get((s, j), 0) if name == "tie" else 0
                gp[s, j], tp[s, j] = lr.richardson(f, 2e-3, side, levels=9 if side else 5)
        gv, tv = np.zeros(S + 1, dtype=lr.CLD), np.zeros(S + 1, dtype=lr.LD)
        for v in range(S + 1):
            parts = []
            for unit in (1.0, 1j):
                def f(off, v=v, unit=unit):
                    rvv = rv.astype(lr.CLD)
                    rvv[v] = rvv[v] + lr.CLD(unit) * off
                    return loss(rects, rvv)
                parts.append(lr.richardson(f, 2e-3 * abs(rv[v]), 0, levels=5))
            gv[v], tv[v] = parts[0][0] + 1j * parts[1][0], parts[0][1] + parts[1][1]
        par = torch.tensor([list(r) + [0.0] for r in rects], dtype=torch.float64, requires_grad=True)
        rvt = torch.tensor(rv, dtype=torch.complex128, requires_grad=True)
        Ex, Ey = lr.li_torch(par, rvt, LX, LY, ox, oy)
        (torch.conj(torch.as_tensor(gEx)) * Ex + torch.conj(torch.as_tensor(gEy)) * Ey).sum().real.backward()
        out.append((gEx, gEy, gp, gv, tp, tv, par.grad.numpy()[:, :4].copy(), rvt.grad.numpy().copy()))
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["wrap_xy", "nested", "tie", "batch3"])
def test_convmat_li_shapes_backward(backend, name):
    """Every parameter and every value of the wrapped, the nested, the tie and the batch-3 case; theta receives exactly 0; two calls give the
    same bits."""
    be = get_backend(backend)
    ox, oy, points = CASES[name]
    ref = reference(name)
    rvs = [r[1] for r in ref]
    rc, o = call_li(be, C128, points_of(name), rvs, ox, oy, True)
    assert rc == 0 and not o["info"].any()
    grads = gradient_reference(name)
    tabs = [np.stack(t) for t in zip(*[table_adjoints(o, b, g[0], g[1], ox, oy) for b, g in enumerate(grads)])]
    rc, gpar, grval = call_backward(be, points_of(name), rvs, ox, oy, o, tabs)
    assert rc == 0
    rc2, gpar2, grval2 = call_backward(be, points_of(name), rvs, ox, oy, o, tabs)
    assert rc2 == 0 and gpar2.tobytes() == gpar.tobytes() and grval2.tobytes() == grval.tobytes()
    for b, (gEx, gEy, gp, gv, tp, tv, gp_plain, gv_plain) in enumerate(grads):
        S = len(points[b])
        got = gpar[b].reshape(S, 5)
        assert (got[:, 4] == 0).all()
        T = terms(name, ref[b][6])
        free = np.ones((S, 4), dtype=bool)
        if name == "tie":                                     # autograd of the restatement takes no side at a tie: left out of e_plain
            for k in TIE_SIDES:
                free[k] = False
        scale = float(np.abs(gp).max())
        e_plain = float(np.abs(gp_plain - gp)[free].max()) / scale
        note("convmat_li_shapes_backward", backend, f"{name} gpar b{b} e_plain {e_plain:.1e} trunc {float(tp.max()) / scale:.1e}",
             float(np.abs(got[:, :4] - gp).max()) / scale, max(e_plain, T * EPS, float(tp.max()) / scale))
        scale = float(np.abs(gv).max())
        e_plain = float(np.abs(gv_plain - gv).max()) / scale
        note("convmat_li_shapes_backward", backend, f"{name} grval b{b} e_plain {e_plain:.1e} trunc {float(tv.max()) / scale:.1e}",
             float(np.abs(grval[b] - gv).max()) / scale, max(e_plain, T * EPS, float(tv.max()) / scale))


@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_error_codes(backend):
    be = get_backend(backend)
    name = "s1_o11"
    ox, oy, _ = CASES[name]
    rv = [reference(name)[0][1]]
    rc, o = call_li(be, C128, points_of(name), rv, ox, oy, True)
    assert rc == 0
    tabs = [np.zeros((1, 3, 5), dtype=C128)] * 4
    untouched = lambda *a: all((v.view(np.uint8) == 0xA5).all() for v in a)
    rc, gp, gv = call_backward(be, points_of(name), rv, ox, oy, o, tabs)
    assert rc == 0 and not gp.any() and not gv.any()                                    # zero adjoints in, zero gradients out
    for kw in (dict(kinds=[0]), dict(batch=0), dict(S=0)):
        rc, gp, gv = call_backward(be, points_of(name), rv, ox, oy, o, tabs, **kw)
        assert rc == ARG and untouched(gp, gv), kw
    rc, gp, gv = call_backward(be, points_of(name), rv, ox, oy, o, tabs, S=128)
    assert rc == UNSUPPORTED and untouched(gp, gv)


# Worst err / floor per entry over all the cases a backend runs, rounded up (the bound is 16).
WORST_EMU = {"convmat_li_shapes": 1.2, "convmat_li_shapes_backward": 1.1}
WORST_MI355X = {"convmat_li_shapes": 0.9, "convmat_li_shapes_backward": 1.2}
