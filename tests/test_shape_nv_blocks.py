"""Block tests of the normal-vector entries for vector shapes -- trx_shape_normal_field, trx_convmat_nv_shapes -- through the C ABI with
caller-owned buffers, guard bytes around every output and around the exactly sized workspace, on both backends of tests/backends.py.

Field.  err = max |nn - nn_ref| over the samples kept, nn_ref the long-double numpy restatement of the definition
(tests/shape_nv_reference.field); bound err <= 16 * max(e_plain, T * eps), e_plain the error of the float64 restatement against the same
reference, T = 9 * (ellipses + edges) the number of summed terms, eps that of fp64.  A sample is left out only where |coherence - 1e-3| < 1e-6
(it may fall on either side of the threshold) or within 1e-6 sqrt(area) of an ellipse centre or a polygon vertex of any image (the field has no
direction there); at most 1 % of a case.  Five structures at generic positions x two cells x three grids, a batch of 3 with per-point
parameters, and a 150-gon (two staging passes).

Tensor.  The policy tests/test_fourier_blocks.py applies to trx_convmat_nv_orders: err = relmax(kernel, reference) <= 16 * max(e_plain, N * eps)
against shape_nv_reference.tensor_hp (mpmath boxes, long-double products and solve), e_plain from tensor_plain; cond([1/eps]) <= 1e4 asserted;
the complex64 call equals the complex128 call rounded once, bit for bit.

Every case prints its ratio err / floor with `-s`.  Worst ratios (bound 16), rounded up: WORST_EMU / WORST_MI355X at the end of the file.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import shape_nv_reference as nvr
from tests import shape_reference as sr
from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import relmax
from tests.test_shape_blocks import CELLS, L_SHAPE, TRIANGLE, call_shapes, circ_mn, gbuf, gread, pack, rect_mn, regular

EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
E, R, P = sr.ELLIPSE, sr.RECTANGLE, sr.POLYGON
ARG, WS, DT, UNSUPPORTED = -2, -3, -1, -5
RATIOS = {}


def note(entry, backend, what, err, floor):
    ratio = err / floor
    RATIOS[(entry, backend)] = max(RATIOS.get((entry, backend), 0.0), ratio)
    print(f"{entry}[{backend}] {what}: {ratio:.2f} | worst so far {RATIOS[(entry, backend)]:.2f}  (err / floor; bound {MARGIN:g})")
    assert err <= MARGIN * floor, f"{what}: err {err:.3e}  floor {floor:.3e}  bound {MARGIN * floor:.3e}"


def lattice_of(cell):
    return (ctypes.c_double * 4)(*[v for a in CELLS[cell] for v in a])


def call_field(be, points, cell, n1, n2, lattice=None, batch=None):
    """(rc, nn [B, 3, n1, n2]) of trx_shape_normal_field with a guarded output."""
    kind, voff, par = pack(points)
    B = len(points) if batch is None else batch
    hn, pn = gbuf(be, len(points) * 3 * n1 * n2 * 8)
    dk, dv, dp = be.dev(kind), be.dev(voff), be.dev(par)
    lat = lattice_of(cell) if lattice is None else (ctypes.c_double * 4)(*lattice)
    rc = be.lib.shape_normal_field(be.ptr(dk), be.ptr(dv), len(kind), be.ptr(dp), par.shape[1], lat, B, n1, n2, pn, be.stream)
    be.sync()
    return rc, gread(be, hn, np.float64, (len(points), 3, n1, n2))


def terms(shapes):
    return 9 * sum(len(p) // 2 if k == P else (4 if k == R else 1) for k, p in shapes)


STRUCTURES = {
    "disk": [(E, [0.18, 0.18, 0.47, 0.53, 0.0])],
    "ellipse_edge": [(E, [0.30, 0.12, 0.90, 0.20, 0.6])],                      # crosses the cell edge: the images matter
    "rectangle": [(R, [0.37, 0.21, 0.45, 0.55, 0.4])],
    "l_triangle": [(P, L_SHAPE), (P, TRIANGLE)],
    "core_shell": [(E, [0.30, 0.20, 0.52, 0.48, 0.3]), (E, [0.10, 0.10, 0.50, 0.50, 0.0])],
}
GRIDS = [(32, 32), (33, 17), (64, 48)]


def check_field(backend, what, got, shapes, cell, n1, n2):
    a1, a2 = CELLS[cell]
    ref = nvr.field(shapes, a1, a2, n1, n2)
    plain = nvr.field(shapes, a1, a2, n1, n2, dtype=np.float64)
    out = nvr.excluded(shapes, a1, a2, n1, n2, ref["coh"])
    assert out.mean() <= 0.01, f"{what}: {out.sum()} of {out.size} samples left out"
    keep = ~out
    err = float(np.abs(got - ref["nn"])[:, keep].max())
    e_plain = float(np.abs(plain["nn"] - ref["nn"])[:, keep].max())
    floor = max(e_plain, terms(shapes) * EPS)
    note("shape_normal_field", backend, f"{what} e_plain {e_plain:.1e} left out {int(out.sum())}", err, floor)
    return floor, keep, ref


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cell", ["square", "oblique"])
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_shape_normal_field(backend, name, cell):
    be = get_backend(backend)
    shapes = STRUCTURES[name]
    for n1, n2 in GRIDS:
        rc, nn = call_field(be, [shapes], cell, n1, n2)
        assert rc == 0
        assert (nn != 0).any() and np.isfinite(nn).all()
        check_field(backend, f"{name} {cell} ({n1},{n2})", nn[0], shapes, cell, n1, n2)
        if (n1, n2) == GRIDS[1]:
            assert np.array_equal(call_field(be, [shapes], cell, n1, n2)[1], nn), "not bit-identical on repetition"


@pytest.mark.parametrize("backend", BACKENDS)
def test_shape_normal_field_batch_with_per_point_parameters(backend):
    be = get_backend(backend)
    pts = [[(E, [0.17 + 0.02 * b, 0.11, 0.32, 0.27 + 0.01 * b, 0.3]), (R, [0.2 + 0.02 * b, 0.1, 0.95, 0.62, -0.5 + 0.1 * b]), (P, TRIANGLE)]
           for b in range(3)]
    rc, nn = call_field(be, pts, "oblique", 33, 17)
    assert rc == 0
    for b in range(3):
        check_field(backend, f"batch[{b}]", nn[b], pts[b], "oblique", 33, 17)
    assert not np.array_equal(nn[0], nn[1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_shape_normal_field_150_gon_takes_two_staging_passes(backend):
    be = get_backend(backend)
    shapes = [(P, regular(150, 0.52, 0.47, 0.3, lobes=0.15)), (E, [0.05, 0.08, 0.5, 0.5, 0.2])]      # a shape after the passes, too
    rc, nn = call_field(be, [shapes], "square", 16, 16)
    assert rc == 0
    check_field(backend, "gon150", nn[0], shapes, "square", 16, 16)


@pytest.mark.parametrize("backend", BACKENDS)
def test_centred_disk_has_the_mirror_symmetry_of_the_blend(backend):
    """A centred disk on the square cell: Nx Ny is odd under x -> -x.  The sample positions i / 32 mirror exactly, so the two values differ by
    the rounding of two sums taken in a different order of images: each is within the field bound of the reference, whose own asymmetry is
    added."""
    be = get_backend(backend)
    n = 32
    shapes = [(E, [0.3, 0.3, 0.5, 0.5, 0.0])]
    rc, nn = call_field(be, [shapes], "square", n, n)
    assert rc == 0
    floor, keep, ref = check_field(backend, "centred disk", nn[0], shapes, "square", n, n)
    mirror = (n - np.arange(1, n)) % n
    both = keep[1:] & keep[mirror]
    asym = np.abs(nn[0, 1, 1:] + nn[0, 1, mirror])[both].max()
    asym_ref = float(np.abs(ref["nn"][1, 1:] + ref["nn"][1, mirror])[both].max())
    assert (nn[0, 1] != 0).any()
    note("shape_normal_field", backend, "mirror asymmetry / 2", asym / 2, floor + asym_ref / 2)


# ---- the tensor --------------------------------------------------------------------------------------------------------------------------------
def recips(vals, hosts):
    """rval of trx_convmat_nv_shapes from val: hosts[s] = index of the shape that holds shape s, or None."""
    vals = np.asarray(vals, dtype=np.complex128)
    eps = [vals[:, 0]]
    for s, h in enumerate(hosts):
        eps.append(vals[:, s + 1] + eps[0 if h is None else h + 1])
    r = [1 / eps[0]] + [1 / eps[s + 1] - 1 / eps[0 if h is None else h + 1] for s, h in enumerate(hosts)]
    return np.stack(r, axis=1)


def call_tensor(be, dtype, points, vals, rvals, cell, mn, mmax, nmax, n1, n2, nn=None, ws_short=0, **over):
    """(rc, [Exx, Exy, Eyy], info) of trx_convmat_nv_shapes with guarded outputs, info and workspace."""
    lib = be.lib
    kind, voff, par = pack(points)
    vals, rvals = np.ascontiguousarray(vals, dtype=np.complex128), np.ascontiguousarray(rvals, dtype=np.complex128)
    recip, area = sr.recip_of(*CELLS[cell])
    B, N = len(points), len(mn)
    isz = np.dtype(dtype).itemsize
    outs = [gbuf(be, B * N * N * isz) for _ in range(3)]
    hi, pi = gbuf(be, B * 4)
    nws = lib.convmat_nv_shapes_ws_bytes(dtcode(dtype), B, n1, n2, N, mmax, nmax)
    hw, pw = gbuf(be, nws)
    dk, dv, dp, dl, dr, dm = be.dev(kind), be.dev(voff), be.dev(par), be.dev(vals), be.dev(rvals), be.dev(mn)
    dn = be.dev(np.ascontiguousarray(nn, dtype=np.float64)) if nn is not None else None
    rv = (ctypes.c_double * 4)(*recip)
    a = dict(code=dtcode(dtype), S=len(kind), npar=par.shape[1], area=area, lattice=lattice_of(cell), batch=B, n1=n1, n2=n2, N=N, mmax=mmax,
             nmax=nmax, kind=be.ptr(dk))
    a.update(over)
    rc = lib.convmat_nv_shapes(a["code"], a["kind"], be.ptr(dv), a["S"], be.ptr(dp), a["npar"], be.ptr(dl), be.ptr(dr), ctypes.addressof(rv),
                               a["area"], a["lattice"], a["batch"], a["n1"], a["n2"], be.ptr(dm), a["N"], a["mmax"], a["nmax"],
                               be.ptr(dn) if nn is not None else None, outs[0][1], outs[1][1], outs[2][1], pi, pw, nws - ws_short, be.stream)
    be.sync()
    gread(be, hw, np.uint8, (nws,))
    return rc, [gread(be, h, dtype, (B, N, N)) for h, _ in outs], gread(be, hi, np.int32, (B,))


def tensor_case(name):
    """(cell, (mmax, nmax), mn, (n1, n2), points, vals, hosts)"""
    if name == "rect_11":
        return "square", (1, 1), rect_mn(1, 1), (24, 20), [[(E, [0.30, 0.17, 0.5, 0.45, 0.4])]], [[1.0, 11.0 + 0.5j]], [None]
    if name == "rect_23":                 # per-point parameters and a core nested in the ellipse
        pts = [[(E, [0.30 - 0.02 * b, 0.2, 0.45, 0.5, 0.3]), (R, [0.15, 0.3, 0.85, 0.3, 0.2]), (E, [0.08, 0.08, 0.45, 0.5, 0.0])] for b in range(2)]
        vals = [[1.5 + 0.01j, 6.0 + 0.2j * b - (1.5 + 0.01j), 3.0 - (1.5 + 0.01j), 2.0 - 0.1j - (6.0 + 0.2j * b)] for b in range(2)]
        return "square", (2, 3), rect_mn(2, 3), (21, 30), pts, vals, [None, None, 0]
    if name == "circular_oblique":
        return ("oblique", (2, 2), circ_mn("oblique", 2, 2, 13), (20, 24), [[(E, [0.2, 0.3, 0.4, 0.5, 1.1]), (P, TRIANGLE)]],
                [[2.0 + 0.3j, 7.0 - 1j - (2.0 + 0.3j), 4.0 - (2.0 + 0.3j)]], [None, None])
    raise KeyError(name)


def check_tensor(backend, name, supplied):
    be = get_backend(backend)
    cell, (mmax, nmax), mn, (n1, n2), points, vals, hosts = tensor_case(name)
    rvals = recips(vals, hosts)
    recip, area = sr.recip_of(*CELLS[cell])
    B = len(points)
    if supplied:                          # a random field: the threshold stays out of it
        nn = np.random.default_rng([21, len(name)]).random((B, 3, n1, n2))
    else:
        rc, nn = call_field(be, points, cell, n1, n2)
        assert rc == 0 and (nn != 0).any()
    rc, o128, info = call_tensor(be, np.complex128, points, vals, rvals, cell, mn, mmax, nmax, n1, n2, nn=nn)
    assert rc == 0 and not info.any()
    for b in range(B):
        ref = nvr.tensor_hp(points[b], vals[b], rvals[b], recip, area, mn, mmax, nmax, nn[b])
        assert np.linalg.cond(ref[3].astype(np.complex128)) <= 1e4
        plain = nvr.tensor_plain(points[b], vals[b], rvals[b], recip, area, mn, mmax, nmax, nn[b])
        for c, comp in enumerate(("Exx", "Exy", "Eyy")):
            floor = max(relmax(plain[c], ref[c]), len(mn) * EPS)
            note("convmat_nv_shapes", backend, f"{name} {comp} b{b}", relmax(o128[c][b], ref[c]), floor)
    rc, o64, info = call_tensor(be, np.complex64, points, vals, rvals, cell, mn, mmax, nmax, n1, n2, nn=nn)
    assert rc == 0 and not info.any()
    assert all(np.array_equal(a, b.astype(np.complex64)) for a, b in zip(o64, o128)), "complex64 is not complex128 rounded once"
    if not supplied:                      # nn = NULL runs the field kernel into the workspace: the same bits as the field handed in
        for dtype, want in ((np.complex128, o128), (np.complex64, o64)):
            rc, got, info = call_tensor(be, dtype, points, vals, rvals, cell, mn, mmax, nmax, n1, n2, nn=None)
            assert rc == 0 and not info.any()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["rect_11", "rect_23", "circular_oblique"])
def test_convmat_nv_shapes_supplied_field(backend, name):
    check_tensor(backend, name, supplied=True)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["rect_11", "circular_oblique"])
def test_convmat_nv_shapes_null_field_is_the_field_kernel(backend, name):
    check_tensor(backend, name, supplied=False)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_zero_field_is_laurents_matrix_bit_for_bit(backend, dtype):
    be = get_backend(backend)
    cell, (mmax, nmax), mn, (n1, n2), points, vals, hosts = tensor_case("rect_23")
    rc, (exx, exy, eyy), info = call_tensor(be, dtype, points, vals, recips(vals, hosts), cell, mn, mmax, nmax, n1, n2,
                                            nn=np.zeros((len(points), 3, n1, n2)))
    assert rc == 0 and not info.any()
    rc, out, _ = call_shapes(be, dtype, points, vals, cell, mn, mmax, nmax)
    assert rc == 0
    assert np.array_equal(exx, out) and np.array_equal(eyy, out) and not exy.any()


@pytest.mark.parametrize("backend", BACKENDS)
def test_info(backend):
    be = get_backend(backend)
    mn0 = np.zeros((1, 2), dtype=np.int32)
    full = [[(R, [1.0, 1.0, 0.5, 0.5, 0.0])]]
    nn = np.zeros((1, 3, 8, 8))
    # [1/eps] = rval[0] + rval[1] chi(0) = 1 - 1 = 0 exactly: a singular 1 x 1 matrix
    rc, _, info = call_tensor(be, np.complex128, full, [[1.0, 1.0]], [[1.0, -1.0]], "square", mn0, 0, 0, 8, 8, nn=nn)
    assert rc == 0 and info.tolist() == [2]
    # a zero background entry: a medium without a finite eps, whatever the inverse then reports
    ok = [[(E, [0.3, 0.2, 0.5, 0.5, 0.0])], [(E, [0.3, 0.2, 0.5, 0.5, 0.0])]]
    rc, _, info = call_tensor(be, np.complex128, ok, [[1.0, 2.0], [1.0, 2.0]], [[1.0, -0.5], [0.0, 0.5]], "square", rect_mn(1, 1), 1, 1, 8, 8,
                              nn=np.zeros((2, 3, 8, 8)))
    assert rc == 0 and info.tolist() == [0, 1]


@pytest.mark.parametrize("backend", BACKENDS)
def test_error_codes(backend):
    be = get_backend(backend)
    ok = [[(E, [0.3, 0.2, 0.5, 0.5, 0.0])]]
    assert call_field(be, ok, "square", 8, 8)[0] == 0
    assert call_field(be, [[(3, [0.3, 0.2, 0.5, 0.5, 0.0])]], "square", 8, 8)[0] == ARG              # unknown kind
    assert call_field(be, [[(P, [0.1, 0.1, 0.5, 0.1])]], "square", 8, 8)[0] == ARG                   # K < 3
    assert call_field(be, [[(E, [0.3, 0.2, 0.5, 0.5])]], "square", 8, 8)[0] == ARG                   # an ellipse has five parameters
    assert call_field(be, ok, "square", 8, 8, lattice=(1.0, 0.0, 2.0, 0.0))[0] == ARG                # a cell without area
    assert call_field(be, ok, "square", 8, 8, lattice=(1.0, 0.0, 0.0, math.inf))[0] == ARG
    assert call_field(be, ok, "square", 0, 8)[0] == ARG
    # a zero-size batch and a grid line beyond 2048 are refused before anything is touched (the output stays as it was filled)
    for kw in (dict(batch=0), dict(batch=65536)):
        rc, nn = call_field(be, ok, "square", 8, 8, **kw)
        assert rc == ARG and (nn.view(np.uint8) == 0xA5).all()
    kind, voff, par = pack(ok)
    hs = [be.dev(kind), be.dev(voff), be.dev(par), be.empty((8,), np.float64)]
    assert be.lib.shape_normal_field(be.ptr(hs[0]), be.ptr(hs[1]), 1, be.ptr(hs[2]), 5, lattice_of("square"), 1, 2049, 1, be.ptr(hs[3]),
                                     be.stream) == UNSUPPORTED
    assert be.lib.shape_normal_field(be.ptr(hs[0]), be.ptr(hs[1]), 1, be.ptr(hs[2]), 5, None, 1, 8, 8, be.ptr(hs[3]), be.stream) == ARG
    # the tensor
    mn = rect_mn(1, 1)
    t = lambda **kw: call_tensor(be, np.complex128, ok, [[1.0, 2.0]], [[1.0, -2.0 / 3.0]], "square", mn, 1, 1, kw.pop("n1", 8), 8,
                                 nn=kw.pop("nn", None), **kw)
    rc, outs, info = t()
    assert rc == 0 and info.tolist() == [0]
    assert t(ws_short=16)[0] == WS
    assert t(code=7)[0] == DT
    assert t(n1=2)[0] == ARG                                                                        # n1 <= 2 mmax
    assert t(n1=2049)[0] == UNSUPPORTED
    assert t(area=0.0)[0] == ARG and t(kind=None)[0] == ARG and t(S=0)[0] == ARG
    assert t(lattice=None)[0] == ARG                                                                 # nn = NULL needs the cell
    assert t(lattice=None, nn=np.zeros((1, 3, 8, 8)))[0] == 0                                         # ... and a supplied field does not
    assert call_tensor(be, np.complex128, ok, [[1.0, 2.0]], [[1.0, -2.0 / 3.0]], "square", mn * 2, 1, 1, 8, 8)[0] == ARG   # outside the box
    for kw in (dict(batch=0), dict(batch=21846)):                                                    # 3 batch <= 65535
        rc, outs, info = t(**kw)
        assert rc == ARG and all((o.view(np.uint8) == 0xA5).all() for o in outs) and (info.view(np.uint8) == 0xA5).all()


# Worst err / floor per entry over all the cases a backend runs, rounded up (the bound is 16).
WORST_EMU = {"shape_normal_field": 1.2, "convmat_nv_shapes": 0.9}
WORST_MI355X = {"shape_normal_field": 2.2, "convmat_nv_shapes": 1.1}
