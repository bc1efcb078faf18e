"""The seven Fourier-factorisation entries in front of the eigensolver under the block-test policy ("Block tests"):
trx_convmat, trx_convmat_orders (csrc/convmat.hip), trx_convmat_li (csrc/convmat_li.hip), trx_normal_field, trx_normal_field_lattice,
trx_convmat_nv and trx_convmat_nv_orders (csrc/convmat_nv.hip), at the shapes where each kernel leaves its first tile, takes a second trip of
a thread-stride loop, changes workgroup size or LDS regime, or pivots.

References (tests/fourier_reference.py, all np.clongdouble, none restating the kernels' algebra): dft_hp, the pruned DFT as a matrix product
with exactly reduced phases (validated against 40-digit mpmath below); li_hp, Toeplitz blocks from dft_hp of 1/g inverted by
helpers.solve_hp; tensor_hp, the normal-vector tensor from its definition; field_hp, the Gaussian periodised first, two circulant products
and np.linalg.eigh per pixel.
Bound: err <= 16 * max(e_plain, n * eps), err = relmax(kernel, reference), e_plain = the same operation through np.fft / torch.linalg.inv
(or the existing field_ref / field_ref_h) in complex128 against the same reference, n = max(nx, ny) for the DFT entries,
max(nx, ny, 2o+1) for Li, N for the tensor.
complex64: every kernel of the three files computes in fp64 for both dtypes and rounds once on the final store, so the complex64 output of a
call must equal the complex128 output of the same call rounded to complex64 BIT FOR BIT (Ux, Uy of Li are complex128 in both).  Every grid
is therefore float32-representable: the complex128 call is held to the bound, the complex64 call to bit equality.
Field metric: N N^T depends on (d, o) / r, r = coherence * trace, so an error of the blurred tensor is amplified by 1 / coherence; the
metric is |nn - ref| * min(1, coherence_ref), maximised over pixels, bounded by 16 * max(e_plain under the same metric, taps * eps),
taps = 2 (2R + 1).  Pixels whose reference coherence lies in [TAU/2, 2 TAU] may fall on either side of NV_TAU: they are left out of the
metric, must be either the reference direction (same bound) or exactly 0, and are at most 1 % of a case (asserted; measured <= 0.011 % on
the grids here, see the record at the end of the file).  Below the band the output must be exactly 0.
Guards (asserted, never skipped): np.longdouble is the 80-bit type; every Toeplitz block of every Li case has cond <= 1e4, and plain
partial-pivot LU interchanges rows at >= half of the steps summed over the blocks of a direction, and every block with w >= 65 at >= half of
its own (_li_guards says why the small blocks are counted together; grids built to pivot: random-phase complex and signed real; the positive grids of tests/test_li_factorisation.py never interchange); cond([1/eps]) <= 1e4; every order list holds the
four corners of its box; every output, info, Ux / Uy, mn and the workspace (exactly *_ws_bytes) carry guard words; outputs start as NaN and
the workspace as 0xFF bytes (a NaN at every float, double or complex read), so a result that takes in anything the call has not written is
NaN: in particular the chunked Li accumulation must start from beta = 0 and not from its buffer (mutation 4 of MUTATIONS).
Every test draws from its own np.random.default_rng([...]) and prints its worst err / max(e_plain, n eps) with `-s`.

Worst ratios per entry (bound 16; the bit-for-bit checks have none), rounded up: WORST_EMU / WORST_MI355X at the end of the file.

That the file bites (emulator, scratch copies of the kernels, nothing committed): see MUTATIONS at the end of the file.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import fourier_reference as fr
from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import lu_interchanges, relmax, solve_hp
from tests.test_lattice import field_ref_h
from tests.test_normal_vector import _disk, field_ref
from tests.test_smatrix_blocks import GUARD, MARGIN, SENT, Guarded

EPS = float(np.finfo(np.float64).eps)
TAU = fr.TAU
UNSUPPORTED = -5
C128, C64 = np.complex128, np.complex64
S3 = 3 ** 0.5
CELLS = {"hex": [[1.0, 0.0], [0.5, S3 / 2]], "skew": [[1.0, 0.15], [-0.35, 0.8]]}


class GuardedReal(Guarded):
    """Guarded for a float64 buffer (Guarded knows complex, integer and byte elements): NaN body, Re(SENT) behind it."""

    def __init__(self, be, count, body=None):
        self.be, self.count, self.dtype, self.sent = be, int(count), np.dtype(np.float64), SENT.real
        flat = np.full(self.count + GUARD, self.sent)
        flat[:self.count] = np.nan if body is None else np.asarray(body, dtype=np.float64).reshape(-1)
        self.buf = be.dev(flat)


def _workspace(be, nbytes):
    """Exactly `nbytes` of 0xFF -- every aligned float, double or complex read of it is a NaN, every int32 is -1 -- and the guard bytes behind
    it.  (Guarded's own byte fill, 0xA5, reads as the double -2.5e-127: adding it to a result would change nothing measurable.)"""
    return Guarded(be, nbytes, np.uint8, body=np.full(int(nbytes), 0xFF, dtype=np.uint8))


RATIOS = {}                      # (entry, backend) -> worst err / max(e_plain, n eps) over the cases run so far


def _record(entry, backend, ratio, what):
    RATIOS[(entry, backend)] = max(RATIOS.get((entry, backend), 0.0), ratio)
    print(f"{entry}[{backend}] {what}: {ratio:.2f} | worst so far {RATIOS[(entry, backend)]:.2f}  (err / max(e_plain, n eps); bound {MARGIN:g})")


def _check(entry, backend, what, got, ref, plain, n):
    err, e_plain = relmax(got, ref), relmax(plain, ref)
    floor = max(e_plain, n * EPS)
    _record(entry, backend, err / floor, what)
    assert err <= MARGIN * floor, f"{what}: err {err:.3e}  e_plain {e_plain:.3e}  n*eps {n * EPS:.3e}  bound {MARGIN * floor:.3e}"


def _same_bits(a64, a128):
    """The complex64 output equals the complex128 output rounded to complex64, bit for bit."""
    a64 = np.ascontiguousarray(a64)
    want = np.ascontiguousarray(np.asarray(a128).astype(a64.dtype))
    return a64.shape == want.shape and a64.tobytes() == want.tobytes()


def _f32(g):
    """Round to what float32 / complex64 holds, kept in double: both dtypes of a call then see the same numbers."""
    g = np.asarray(g)
    return g.astype(C64).astype(C128) if np.iscomplexobj(g) else g.astype(np.float32).astype(np.float64)


def _dev_grid(be, g, dtype):
    rdt = np.float64 if dtype == C128 else np.float32
    return be.dev(g.astype(dtype if np.iscomplexobj(g) else rdt))


def _textured(rng, B, nx, ny, cplx):
    """Unrelated positive (or lossy) grids per batch member: a disk of its own radius and centre plus texture; no zero."""
    gs = []
    for _ in range(B):
        seed = int(rng.integers(1 << 30))
        gs.append(_disk(nx, ny, cplx, seed, eps=(1.5 + rng.random(), 6.0 + 4 * rng.random()), r=0.2 + 0.2 * rng.random(),
                        c=(0.3 + 0.4 * rng.random(), 0.3 + 0.4 * rng.random())))
    return _f32(np.stack(gs))


# ---- the reference of the references --------------------------------------------------------------------------------------------------
def test_dft_hp_against_mpmath():
    """fourier_reference.dft_hp against the DFT summed in 40-digit mpmath at (7, 12) and (13, 5), every coefficient of the full index range
    (negative and aliased indices included): at most 1e-18 of the largest coefficient.  Fails loudly where long double is not the 80-bit
    extended type: every complex128 case of this file would silently lose its reference."""
    import mpmath
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not extended precision here: no reference beyond complex128"
    mpmath.mp.dps = 40
    rng = np.random.default_rng([7, 12, 13, 5])
    for nx, ny in [(7, 12), (13, 5)]:
        g = 1.0 + rng.random((nx, ny)) + 1j * rng.standard_normal((nx, ny))
        P, Q = np.arange(-nx - 2, nx + 3), np.arange(-ny - 2, ny + 3)
        c = fr.dft_hp(g, P, Q)
        assert c.dtype == np.clongdouble
        gm = [[mpmath.mpc(complex(g[x, y])) for y in range(ny)] for x in range(nx)]
        ex = [mpmath.expjpi(mpmath.mpf(-2 * k) / nx) for k in range(nx)]
        ey = [mpmath.expjpi(mpmath.mpf(-2 * k) / ny) for k in range(ny)]
        worst, scale = mpmath.mpf(0), mpmath.mpf(0)
        for i, p in enumerate(P):
            for j, q in enumerate(Q):
                s = mpmath.fsum(gm[x][y] * ex[(int(p) * x) % nx] * ey[(int(q) * y) % ny] for x in range(nx) for y in range(ny)) / (nx * ny)
                z = c[i, j]
                zr, zi = z.real, z.imag          # a long double is the sum of two doubles: exact conversion
                zm = mpmath.mpc(mpmath.mpf(float(zr)) + mpmath.mpf(float(zr - np.longdouble(float(zr)))),
                                mpmath.mpf(float(zi)) + mpmath.mpf(float(zi - np.longdouble(float(zi)))))
                worst, scale = max(worst, abs(zm - s)), max(scale, abs(s))
        assert worst <= 1e-18 * scale, (nx, ny, float(worst / scale))
        # ... and the library transform in double is visibly worse, so the comparison has resolution
        assert relmax(np.fft.fft2(g)[P[:, None] % nx, Q[None, :] % ny] / (nx * ny), c) > 1e-17


# ---- 1. trx_convmat -------------------------------------------------------------------------------------------------------------------
def _call_convmat(be, dtype, g, ox, oy):
    B, nx, ny = g.shape
    N = (2 * ox + 1) * (2 * oy + 1)
    gin = _dev_grid(be, g, dtype)
    out = Guarded(be, B * N * N, dtype)
    nws = be.lib.convmat_ws_bytes(dtcode(dtype), B, nx, ny, ox, oy)
    ws = _workspace(be, nws)
    rc = be.lib.convmat(dtcode(dtype), int(np.iscomplexobj(g)), be.ptr(gin), B, nx, ny, ox, oy, out.ptr(), ws.ptr(), nws, be.stream)
    be.sync()
    ws.host()
    return rc, out.host((B, N, N))


CONVMAT_SHAPES = [(3, 131, 0, 32), (131, 3, 32, 0), (20, 18, 8, 8), (17, 17, 8, 8), (257, 130, 2, 3), (3, 2048, 1, 1), (2048, 2, 1, 0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cplx", [0, 1])
@pytest.mark.parametrize("nx,ny,ox,oy", CONVMAT_SHAPES)
def test_convmat_tile_edges(backend, nx, ny, ox, oy, cplx):
    """(3,131,0,32), (131,3,32,0): the stride loops over ny > 128 cells and over 4o+1 = 129 coefficients, each axis; (20,18,8,8),
    (17,17,8,8): N = 289, the second column block of toeplitz_kernel, and aliased differences (nx <= 4 ox); (257,130,2,3): mixed;
    (3,2048,1,1), (2048,2,1,0): a 2048-cell line, 64 KB of dynamic LDS."""
    be = get_backend(backend)
    rng = np.random.default_rng([1, nx, ny, ox, oy, cplx])
    B = 2
    g = rng.standard_normal((B, nx, ny)) + (1j * rng.standard_normal((B, nx, ny)) if cplx else 0)
    g = _f32(g + 0.5)
    mn = fr.rect_orders(ox, oy)
    rc, o128 = _call_convmat(be, C128, g, ox, oy)
    assert rc == 0
    for b in range(B):
        _check("trx_convmat", backend, f"({nx},{ny},{ox},{oy}) b{b}", o128[b], fr.convmat_hp(g[b], mn, ox, oy), fr.convmat_plain(g[b], mn),
               max(nx, ny))
    rc, o64 = _call_convmat(be, C64, g, ox, oy)
    assert rc == 0 and _same_bits(o64, o128)


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_refuses_2049_cell_line(backend):
    """One cell past the 64 KB LDS line: an argument check that returns before any launch; the output stays untouched."""
    be = get_backend(backend)
    for shape in [(1, 3, 2049), (1, 2049, 3)]:
        rc, out = _call_convmat(be, C128, np.ones(shape), 1, 1)
        assert rc == UNSUPPORTED and np.isnan(out).all()


def _harmonic(n1, n2, p, q):
    """e^{2 pi i (p x / n1 + q y / n2)} rounded to complex128 from the long-double twiddles."""
    return np.conj(fr.twiddle_hp(n1, [p])[0])[:, None] * np.conj(fr.twiddle_hp(n2, [q])[0])[None, :]


def _indicator(mn, n1, n2, p, q):
    dm, dn = mn[:, None, 0] - mn[None, :, 0], mn[:, None, 1] - mn[None, :, 1]
    return ((dm - p) % n1 == 0) & ((dn - q) % n2 == 0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_single_harmonic_aliased(backend):
    """test_convmat_index_map_is_exact past one column block (N = 289) and into the aliased regime: the matrix of a single harmonic (p, q)
    is the indicator of (m_i - m_j, n_i - n_j) = (p, q) modulo (nx, ny)."""
    be = get_backend(backend)
    nx, ny, ox, oy = 20, 18, 8, 8
    mn = fr.rect_orders(ox, oy)
    for (p, q) in [(1, 0), (0, -1), (-3, 2), (9, -7), (-16, 13)]:
        g = _harmonic(nx, ny, p, q).astype(C128)
        want = _indicator(mn, nx, ny, p, q)
        assert want.any()
        rc, out = _call_convmat(be, C128, g[None], ox, oy)
        assert rc == 0
        assert ((np.abs(out[0]) > 0.5) == want).all()
        _check("trx_convmat", backend, f"harmonic ({p},{q})", out[0], fr.convmat_hp(g, mn, ox, oy), fr.convmat_plain(g, mn), max(nx, ny))


# ---- 2. trx_convmat_orders ------------------------------------------------------------------------------------------------------------
def _order_list(rng, N, mmax, nmax, distinct=False):
    """N harmonics of the box |m| <= mmax, |n| <= nmax in no particular order, the four corners among them (the extreme coefficient
    indices are read).  Repeats are allowed unless `distinct` (a repeated harmonic makes [1/eps] of the tensor entries singular)."""
    corners = np.array([[mmax, nmax], [-mmax, nmax], [mmax, -nmax], [-mmax, -nmax]])
    if distinct:
        box = fr.rect_orders(mmax, nmax)
        box = box[(np.abs(box[:, 0]) != mmax) | (np.abs(box[:, 1]) != nmax)]
        rest = box[rng.permutation(len(box))[:N - 4]]
    else:
        rest = np.stack([rng.integers(-mmax, mmax + 1, N - 4), rng.integers(-nmax, nmax + 1, N - 4)], 1)
    mn = np.concatenate([corners, rest])[rng.permutation(N)]
    for c in corners:
        assert (mn == c).all(1).any()
    return mn


def _call_orders(be, dtype, g, mn, mmax, nmax):
    B, n1, n2 = g.shape
    N = len(mn)
    gin = _dev_grid(be, g, dtype)
    mnd = Guarded(be, 2 * N, np.int32, body=mn)
    out = Guarded(be, B * N * N, dtype)
    nws = be.lib.convmat_orders_ws_bytes(dtcode(dtype), B, n1, n2, N, mmax, nmax)
    ws = _workspace(be, nws)
    rc = be.lib.convmat_orders(dtcode(dtype), int(np.iscomplexobj(g)), be.ptr(gin), B, n1, n2, mnd.ptr(), N, mmax, nmax, out.ptr(), ws.ptr(),
                               nws, be.stream)
    be.sync()
    ws.host()
    assert (mnd.host((N, 2)) == mn).all()
    return rc, out.host((B, N, N))


ORDERS_SHAPES = ([(9, 11, 2, 3, N) for N in (31, 32, 33)] + [(30, 30, 7, 7, N) for N in (64, 65, 255, 256, 257)]
                 + [(53, 55, 26, 26, 33), (53, 55, 26, 26, 257), (51, 53, 25, 25, 33)])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cplx", [0, 1])
@pytest.mark.parametrize("n1,n2,mmax,nmax,N", ORDERS_SHAPES)
def test_convmat_orders_tile_edges(backend, n1, n2, mmax, nmax, N, cplx):
    """(9,11,2,3; 31..33): the ORD_ROWS = 32 row-block edge; (30,30,7,7; 64, 65, 255, 256, 257): the three workgroup sizes and more than
    one j trip; (53,55,26,26): the coefficient box of 105^2 x 16 B > 160 KB, read from global memory; (51,53,25,25): the largest LDS box."""
    be = get_backend(backend)
    rng = np.random.default_rng([2, n1, n2, mmax, nmax, N, cplx])
    B = 2
    g = _f32(0.5 + rng.standard_normal((B, n1, n2)) + (1j * rng.standard_normal((B, n1, n2)) if cplx else 0))
    mn = _order_list(rng, N, mmax, nmax)
    assert (16 * (4 * mmax + 1) * (4 * nmax + 1) > 160 * 1024) == (mmax == 26)
    rc, o128 = _call_orders(be, C128, g, mn, mmax, nmax)
    assert rc == 0
    for b in range(B):
        _check("trx_convmat_orders", backend, f"({n1},{n2},{mmax},{nmax};{N}) b{b}", o128[b], fr.convmat_hp(g[b], mn, mmax, nmax),
               fr.convmat_plain(g[b], mn), max(n1, n2))
    rc, o64 = _call_orders(be, C64, g, mn, mmax, nmax)
    assert rc == 0 and _same_bits(o64, o128)


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_orders_single_harmonic_global_box(backend):
    """The index map of the global-memory gather: a single harmonic gives the indicator matrix of its difference."""
    be = get_backend(backend)
    n1, n2, mmax, nmax, N = 53, 55, 26, 26, 257
    rng = np.random.default_rng([3, n1, n2, N])
    mn = _order_list(rng, N, mmax, nmax)
    for (p, q) in [(1, 0), (-52, 51), (17, -40)]:
        g = _harmonic(n1, n2, p, q).astype(C128)
        want = _indicator(mn, n1, n2, p, q)
        rc, out = _call_orders(be, C128, g[None], mn, mmax, nmax)
        assert rc == 0 and want.any()
        assert ((np.abs(out[0]) > 0.5) == want).all()
        _check("trx_convmat_orders", backend, f"harmonic ({p},{q})", out[0], fr.convmat_hp(g, mn, mmax, nmax), fr.convmat_plain(g, mn),
               max(n1, n2))


# ---- 3. trx_convmat_li ----------------------------------------------------------------------------------------------------------------
def _li_grid(cls, B, nx, ny, seed=0):
    """Grids whose Toeplitz blocks are NOT diagonally dominant, so that the Gauss-Jordan inverse pivots: "phase" (0.5 + u) e^{2 pi i v}
    (complex), "signed" +-(1 + 3u) (real)."""
    rng = np.random.default_rng([4, nx, ny, seed, int(cls == "phase")])
    if cls == "phase":
        return _f32((0.5 + rng.random((B, nx, ny))) * np.exp(2j * np.pi * rng.random((B, nx, ny))))
    return _f32(np.where(rng.random((B, nx, ny)) < 0.5, -1.0, 1.0) * (1 + 3 * rng.random((B, nx, ny))))


# (cls, nx, ny, ox, oy) -> seed where seed 0 misses a guard (searched on the CPU: the smallest seed that passes; a direction with few small
# blocks, 9 rows of 7 x 7 or 5 of 3 x 3, interchanges at less than half of its steps for about one seed in four)
LI_SEED = {("phase", 131, 9, 2, 3): 1, ("signed", 131, 9, 2, 3): 1, ("phase", 260, 5, 1, 1): 5}


@functools.lru_cache(maxsize=None)
def _li_case(cls, nx, ny, ox, oy):
    """(grid, per-member references and e_plain data), computed once and shared by the kept / chunked cases and both backends."""
    g = _li_grid(cls, 2, nx, ny, LI_SEED.get((cls, nx, ny, ox, oy), 0))
    refs = [fr.li_hp(g[b], ox, oy) for b in range(2)]
    plains = [fr.li_plain(g[b], ox, oy) for b in range(2)]
    for a in [g] + [v for r in refs for v in r.values()]:
        a.setflags(write=False)
    return g, refs, plains


def _li_guards(refs):
    """Every inverted block is well conditioned, and plain partial pivoting interchanges at >= half of its steps.  The reading chosen for
    "its steps": the steps of all the blocks of one direction of one batch member together, because a case holds up to 260 blocks of
    3 x 3 ... 7 x 7 and a random block that small takes its two to six steps without any interchange now and then (measured: 36 ... 77 of
    the 260 blocks of (260,5,1,1), up to 7 of the 131 of (9,131,3,2) / (131,9,2,3)); no seed makes every one of them pivot.  A block large
    enough for the count to mean something, w >= 65, is also held to the half on its own (measured: 56 ... 62 of 64 steps, 85 ... 97 of
    98)."""
    worst_cond, fracs = 0.0, []
    for r in refs:
        for T in (r["Tx"], r["Ty"]):
            T = T.astype(C128)
            worst_cond = max(worst_cond, max(float(np.linalg.cond(t)) for t in T))
            w = T.shape[1]
            steps = len(T) * (w - 1)
            if steps:
                counts = [lu_interchanges(t) for t in T]
                fracs.append(sum(counts) / steps)
                assert w < 65 or 2 * min(counts) >= w - 1, (w, counts)
    assert worst_cond <= 1e4, worst_cond
    assert fracs and min(fracs) >= 0.5, fracs
    return worst_cond, min(fracs)


def _call_li(be, dtype, g, ox, oy, keep):
    B, nx, ny = g.shape
    wx, wy = 2 * ox + 1, 2 * oy + 1
    N = wx * wy
    gin = _dev_grid(be, g, dtype)
    Ex, Ey = Guarded(be, B * N * N, dtype), Guarded(be, B * N * N, dtype)
    Ux = Guarded(be, B * nx * wy * wy, C128) if keep else None
    Uy = Guarded(be, B * ny * wx * wx, C128) if keep else None
    info = Guarded(be, B, np.int32)
    nws = be.lib.convmat_li_ws_bytes(dtcode(dtype), B, nx, ny, ox, oy)
    ws = _workspace(be, nws)
    rc = be.lib.convmat_li(dtcode(dtype), int(np.iscomplexobj(g)), be.ptr(gin), B, nx, ny, ox, oy, Ex.ptr(), Ey.ptr(),
                           Ux.ptr() if keep else None, Uy.ptr() if keep else None, info.ptr(), ws.ptr(), nws, be.stream)
    be.sync()
    ws.host()
    out = dict(Ex=Ex.host((B, N, N)), Ey=Ey.host((B, N, N)), info=info.host())
    if keep:
        out.update(Ux=Ux.host((B, nx, wy, wy)), Uy=Uy.host((B, ny, wx, wx)))
    return rc, out


LI_SHAPES = [(13, 9, 3, 1), (9, 131, 3, 2), (131, 9, 2, 3), (260, 5, 1, 1), (67, 3, 32, 0), (3, 67, 0, 32), (101, 2, 49, 0), (2, 101, 0, 49)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("cls", ["phase", "signed"])
@pytest.mark.parametrize("nx,ny,ox,oy", LI_SHAPES)
def test_convmat_li_pivoting(backend, nx, ny, ox, oy, cls, keep):
    """(13,9,3,1): baseline; (9,131,3,2), (131,9,2,3): y tiles 0..2 of recip_dft_x_kernel with a partial last wave, row chunks that do not
    divide the row count; (260,5,1,1): the nx > 256 twiddle stride; (67,3,32,0), (3,67,0,32): w = 65, the pivot-search stride and the
    67 KB LDS opt-in; (101,2,49,0), (2,101,0,49): w = 99, the documented maximum, 158 KB.  keep: Ux / Uy are outputs (one pass); else the
    inverses live in the workspace and E accumulates over row chunks."""
    be = get_backend(backend)
    g, refs, plains = _li_case(cls, nx, ny, ox, oy)
    _li_guards(refs)
    n = max(nx, ny, 2 * max(ox, oy) + 1)
    rc, o128 = _call_li(be, C128, g, ox, oy, keep)
    assert rc == 0 and not o128["info"].any()
    for b in range(2):
        for i, k in enumerate(("Ex", "Ey", "Ux", "Uy") if keep else ("Ex", "Ey")):
            _check("trx_convmat_li", backend, f"({nx},{ny},{ox},{oy}) {cls} keep={keep} {k} b{b}", o128[k][b], refs[b][k], plains[b][i], n)
    rc, o64 = _call_li(be, C64, g, ox, oy, keep)
    assert rc == 0 and not o64["info"].any()
    assert _same_bits(o64["Ex"], o128["Ex"]) and _same_bits(o64["Ey"], o128["Ey"])
    if keep:
        assert _same_bits(o64["Ux"], o128["Ux"]) and _same_bits(o64["Uy"], o128["Uy"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_li_refuses_order_50(backend):
    """w = 101 does not fit the LDS of one CU: an argument check that returns before any launch."""
    be = get_backend(backend)
    for nx, ny, ox, oy in [(101, 2, 50, 0), (2, 101, 0, 50)]:
        rc, out = _call_li(be, C128, np.ones((1, nx, ny)), ox, oy, False)
        assert rc == UNSUPPORTED and np.isnan(out["Ex"]).all() and np.isnan(out["Ey"]).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("keep", [True, False])
def test_convmat_li_info(backend, keep):
    """info per batch member: a zero grid value -> 1; an exactly singular first Toeplitz block (1/g = +-1 with zero mean along x, o = 0)
    -> 2, and the other member of that batch is untouched by it and correct."""
    be = get_backend(backend)
    nx, ny, ox, oy = 13, 9, 3, 1
    g, refs, plains = _li_case("phase", nx, ny, ox, oy)
    gz = g.copy()
    gz[1, 5, 4] = 0.0
    rc, out = _call_li(be, C128, gz, ox, oy, keep)
    assert rc == 0 and out["info"].tolist() == [0, 1]
    for i, k in enumerate(("Ex", "Ey")):
        _check("trx_convmat_li", backend, f"zero in the other member {k}", out[k][0], refs[0][k], plains[0][i], max(nx, ny, 7))
    # o = 0: every block is the 1 x 1 mean of 1/g along its line; member 1 has mean 0 along x in row y = 0
    rng = np.random.default_rng([5, 8, 6])
    gs = _f32(np.where(rng.random((2, 8, 6)) < 0.5, -1.0, 1.0) * (1 + 3 * rng.random((2, 8, 6))))
    gs[1, :, 0] = [1, -1, 1, -1, -1, 1, -1, 1]
    ref, plain = fr.li_hp(gs[0], 0, 0), fr.li_plain(gs[0], 0, 0)
    rc, out = _call_li(be, C128, gs, 0, 0, keep)
    assert rc == 0 and out["info"].tolist() == [0, 2]
    for i, k in enumerate(("Ex", "Ey", "Ux", "Uy") if keep else ("Ex", "Ey")):
        _check("trx_convmat_li", backend, f"singular block in the other member {k}", out[k][0], ref[k], plain[i], 8)


# ---- 4. trx_normal_field, trx_normal_field_lattice ------------------------------------------------------------------------------------
def _call_field(be, dtype, g, sigma, hx=1.0, hy=1.0, h=None):
    B, nx, ny = g.shape
    gin = _dev_grid(be, g, dtype)
    nn = GuardedReal(be, B * 3 * nx * ny)
    nws = be.lib.normal_field_ws_bytes(dtcode(dtype), B, nx, ny)
    ws = _workspace(be, nws)
    if h is None:
        rc = be.lib.normal_field(dtcode(dtype), int(np.iscomplexobj(g)), be.ptr(gin), B, nx, ny, sigma, hx, hy, nn.ptr(), ws.ptr(), nws, be.stream)
    else:
        hc = (ctypes.c_double * 4)(*np.asarray(h, dtype=np.float64).ravel().tolist())
        rc = be.lib.normal_field_lattice(dtcode(dtype), int(np.iscomplexobj(g)), be.ptr(gin), B, nx, ny, sigma, hc, nn.ptr(), ws.ptr(), nws,
                                         be.stream)
    be.sync()
    ws.host()
    return rc, nn.host((B, 3, nx, ny))


def _field_check(entry, backend, what, nn, ref, plain, sigma):
    """The per-pixel metric of the module docstring for one batch member; returns (share of the threshold band, mask of the pixels with a
    unit field, mask of the pixels that are exactly 0)."""
    coh, dirs = ref["coh"], ref["dir"]
    band = (coh >= TAU / 2) & (coh <= 2 * TAU)
    assert band.mean() <= 0.01, f"{what}: {band.mean():.4f} of the pixels lie in the threshold band"
    want = dirs * (coh > TAU)
    wgt = np.minimum(1.0, coh)
    taps = 2 * (2 * int(np.ceil(3 * sigma)) + 1)

    def metric(a, target, sel):
        return float((np.abs(a - target).max(0) * wgt)[sel].max()) if sel.any() else 0.0

    err, e_plain = metric(nn, want, ~band), metric(plain, want, ~band)
    floor = max(e_plain, taps * EPS)
    _record(entry, backend, err / floor, f"{what} (threshold band {100 * band.mean():.3f} % of the pixels)")
    assert np.isfinite(nn).all()
    assert err <= MARGIN * floor, f"{what}: err {err:.3e}  e_plain {e_plain:.3e}  taps*eps {taps * EPS:.3e}  bound {MARGIN * floor:.3e}"
    assert (nn[:, coh < TAU / 2] == 0.0).all(), f"{what}: a direction where none is resolvable"
    zero = (nn == 0.0).all(0)
    close = np.abs(nn - dirs).max(0) * wgt <= MARGIN * floor
    assert (zero | close)[band].all(), f"{what}: a band pixel is neither the reference direction nor 0"
    unit = np.abs(nn[0] + nn[2] - 1.0) < 1e-12
    return float(band.mean()), unit, zero


FIELD_SHAPES = [(70, 131, 1.5, 1.0, 1.0), (5, 300, 2.0, 1.0, 1.0), (130, 66, 43.0, 0.7, 1.1), (40, 70, 256.0, 1.0, 1.0), (6, 65, 0.0, 1.0, 2.0),
                (1, 70, 1.0, 1.0, 1.0), (2, 2, 1.0, 1.0, 1.0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cplx", [0, 1])
@pytest.mark.parametrize("nx,ny,sigma,hx,hy", FIELD_SHAPES)
def test_normal_field_tile_edges(backend, nx, ny, sigma, hx, hy, cplx):
    """(70,131,1.5): three y tiles of nv_field_x_kernel with a partial wave, nx no multiple of 4; (5,300,2): the ny > 256 stride of
    nv_tensor_y_kernel; (130,66,43): 2R+1 = 259 weights, R > ny so the blur wraps more than once; (40,70,256): sigma at its maximum,
    R = 768; (6,65,0): no blur; (1,70,1), (2,2,1): degenerate periodic differences, output exactly 0 or finite."""
    be = get_backend(backend)
    rng = np.random.default_rng([6, nx, ny, int(sigma * 10), cplx])
    B = 2
    g = _textured(rng, B, nx, ny, cplx)
    rc, n128 = _call_field(be, C128, g, sigma, hx, hy)
    assert rc == 0
    for b in range(B):
        ref = fr.field_hp(g[b], sigma, [[1 / np.longdouble(hx), 0], [0, 1 / np.longdouble(hy)]])
        _field_check("trx_normal_field", backend, f"({nx},{ny},{sigma}) b{b}", n128[b], ref, field_ref(g[b], sigma, hx, hy), sigma)
    if (nx, ny) == (2, 2):
        assert (n128 == 0.0).all()                                 # x+1 = x-1 (mod 2) on both axes: no gradient at all
    rc, n64 = _call_field(be, C64, g, sigma, hx, hy)
    assert rc == 0 and n64.tobytes() == n128.tobytes()             # nn is float64 in both dtypes: the same bits


@pytest.mark.parametrize("backend", BACKENDS)
def test_normal_field_refuses_sigma_257(backend):
    be = get_backend(backend)
    rc, nn = _call_field(be, C128, np.ones((1, 8, 8)), 257.0)
    assert rc == UNSUPPORTED and np.isnan(nn).all()


def _flat_disks():
    """Two flat disks (test_normal_field_fallback_and_radial_disk scaled past one tile): exact zero gradient away from the edge."""
    x, y = np.arange(96) + 0.5, np.arange(80) + 0.5
    X, Y = np.meshgrid(x, y, indexing="ij")
    return np.stack([np.where((X - 48) ** 2 + (Y - 40) ** 2 < 24 ** 2, 12.0, 1.0), np.where((X - 40) ** 2 + (Y - 44) ** 2 < 20 ** 2, 2.5, 7.0)])


@pytest.mark.parametrize("backend", BACKENDS)
def test_normal_field_both_branches(backend):
    """Flat disks at 96 x 80, sigma 3: at least 5 % of the pixels carry a unit field and at least 5 % exactly 0."""
    be = get_backend(backend)
    g = _flat_disks()
    rc, nn = _call_field(be, C128, g, 3.0)
    assert rc == 0
    for b in range(2):
        ref = fr.field_hp(g[b], 3.0, np.eye(2))
        _, unit, zero = _field_check("trx_normal_field", backend, f"flat disk b{b}", nn[b], ref, field_ref(g[b], 3.0), 3.0)
        assert 20 * unit.sum() >= unit.size and 20 * zero.sum() >= zero.size, (int(unit.sum()), int(zero.sum()), unit.size)
        assert (unit ^ zero).all()                                 # every pixel is one or the other


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cell", ["hex", "skew"])
@pytest.mark.parametrize("n1,n2,sigma", [(70, 131, 1.5), (5, 300, 2.0)])
def test_normal_field_lattice_tile_edges(backend, n1, n2, sigma, cell):
    be = get_backend(backend)
    rng = np.random.default_rng([7, n1, n2, int(cell == "hex")])
    h = np.array(CELLS[cell]) / np.array([[n1], [n2]])
    hinv = solve_hp(h, np.eye(2)).real
    for cplx in (0, 1):
        g = _textured(rng, 2, n1, n2, cplx)
        rc, n128 = _call_field(be, C128, g, sigma, h=h)
        assert rc == 0
        for b in range(2):
            _field_check("trx_normal_field_lattice", backend, f"{cell} ({n1},{n2},{sigma}) cplx={cplx} b{b}", n128[b],
                         fr.field_hp(g[b], sigma, hinv), field_ref_h(g[b], sigma, h), sigma)
        rc, n64 = _call_field(be, C64, g, sigma, h=h)
        assert rc == 0 and n64.tobytes() == n128.tobytes()


@pytest.mark.parametrize("backend", BACKENDS)
def test_normal_field_lattice_diagonal_is_rectangle(backend):
    """A diagonal positive cell matrix takes trx_normal_field's path: the same bits."""
    be = get_backend(backend)
    rng = np.random.default_rng([8])
    g = _textured(rng, 2, 70, 131, 1)
    rc0, a = _call_field(be, C128, g, 1.5, 0.03, 0.05)
    rc1, b = _call_field(be, C128, g, 1.5, h=[[0.03, 0.0], [0.0, 0.05]])
    assert rc0 == 0 and rc1 == 0 and a.tobytes() == b.tobytes()


# ---- 5. trx_convmat_nv, trx_convmat_nv_orders -----------------------------------------------------------------------------------------
def _call_nv(be, dtype, g, ox, oy, nn=None, sigma=1.5, hx=1.0, hy=1.0, mn=None, h=None):
    """mn = None: trx_convmat_nv on the rectangle (ox, oy); else trx_convmat_nv_orders with mmax = ox, nmax = oy and the cell matrix h."""
    B, nx, ny = g.shape
    N = (2 * ox + 1) * (2 * oy + 1) if mn is None else len(mn)
    code, cplx = dtcode(dtype), int(np.iscomplexobj(g))
    gin = _dev_grid(be, g, dtype)
    outs = [Guarded(be, B * N * N, dtype) for _ in range(3)]
    info = Guarded(be, B, np.int32)
    nnd = be.dev(np.ascontiguousarray(nn, dtype=np.float64)) if nn is not None else None
    nnp = be.ptr(nnd) if nn is not None else None
    if mn is None:
        nws = be.lib.convmat_nv_ws_bytes(code, B, nx, ny, ox, oy)
        ws = _workspace(be, nws)
        rc = be.lib.convmat_nv(code, cplx, be.ptr(gin), B, nx, ny, ox, oy, sigma, hx, hy, nnp, *[o.ptr() for o in outs], info.ptr(), ws.ptr(),
                               nws, be.stream)
    else:
        mnd = Guarded(be, 2 * N, np.int32, body=mn)
        hc = (ctypes.c_double * 4)(*np.asarray(h, dtype=np.float64).ravel().tolist())
        nws = be.lib.convmat_nv_orders_ws_bytes(code, B, nx, ny, N, ox, oy)
        ws = _workspace(be, nws)
        rc = be.lib.convmat_nv_orders(code, cplx, be.ptr(gin), B, nx, ny, mnd.ptr(), N, ox, oy, sigma, hc, nnp, *[o.ptr() for o in outs],
                                      info.ptr(), ws.ptr(), nws, be.stream)
        be.sync()
        mnd.host()
    be.sync()
    ws.host()
    return rc, [o.host((B, N, N)) for o in outs], info.host()


def _tensor_case(entry, backend, be, g, nn, ox, oy, mn_list=None, h=None):
    """Supplied random field (the threshold stays out of it): the complex128 call against tensor_hp, the complex64 call bit for bit."""
    B, nx, ny = g.shape
    mn = fr.rect_orders(ox, oy) if mn_list is None else mn_list
    rc, o128, info = _call_nv(be, C128, g, ox, oy, nn=nn, mn=mn_list, h=h)
    assert rc == 0 and not info.any()
    for b in range(B):
        ref = fr.tensor_hp(g[b], mn, ox, oy, nn[b])
        assert np.linalg.cond(ref[3].astype(C128)) <= 1e4
        plain = fr.tensor_plain(g[b], mn, nn[b])
        for c, name in enumerate(("Exx", "Exy", "Eyy")):
            _check(entry, backend, f"({nx},{ny},{ox},{oy};{len(mn)}) {name} b{b}", o128[c][b], ref[c], plain[c], len(mn))
    rc, o64, info = _call_nv(be, C64, g, ox, oy, nn=nn, mn=mn_list, h=h)
    assert rc == 0 and not info.any()
    assert all(_same_bits(a, b) for a, b in zip(o64, o128))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cplx", [0, 1])
@pytest.mark.parametrize("nx,ny,ox,oy", [(13, 11, 2, 1), (70, 131, 2, 3), (20, 18, 8, 8)])
def test_convmat_nv_tensor(backend, nx, ny, ox, oy, cplx):
    be = get_backend(backend)
    rng = np.random.default_rng([9, nx, ny, ox, oy, cplx])
    g = _textured(rng, 2, nx, ny, cplx)
    _tensor_case("trx_convmat_nv", backend, be, g, rng.random((2, 3, nx, ny)), ox, oy)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [C128, C64])
def test_convmat_nv_null_field_is_normal_field(backend, dtype):
    """nn = NULL equals, bit for bit, the call given trx_normal_field's output for the same grid and arguments: both run field_core on the
    same converted grid."""
    be = get_backend(backend)
    rng = np.random.default_rng([10])
    nx, ny, ox, oy, sigma, hx, hy = 70, 131, 2, 3, 1.5, 0.7, 1.1
    g = _textured(rng, 2, nx, ny, 1)
    rc, nn = _call_field(be, dtype, g, sigma, hx, hy)
    assert rc == 0 and (nn != 0).any()
    rc0, a, i0 = _call_nv(be, dtype, g, ox, oy, nn=None, sigma=sigma, hx=hx, hy=hy)
    rc1, b, i1 = _call_nv(be, dtype, g, ox, oy, nn=nn)
    assert rc0 == 0 and rc1 == 0 and not i0.any() and not i1.any()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


NV_ORDERS_SHAPES = [(30, 30, 7, 7, 65), (53, 55, 26, 26, 33)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n1,n2,mmax,nmax,N", NV_ORDERS_SHAPES)
def test_convmat_nv_orders_tensor(backend, n1, n2, mmax, nmax, N):
    be = get_backend(backend)
    rng = np.random.default_rng([11, n1, n2, N])
    h = np.array(CELLS["skew"]) / np.array([[n1], [n2]])
    mn = _order_list(rng, N, mmax, nmax, distinct=True)
    for cplx in (0, 1):
        g = _textured(rng, 2, n1, n2, cplx)
        _tensor_case("trx_convmat_nv_orders", backend, be, g, rng.random((2, 3, n1, n2)), mmax, nmax, mn_list=mn, h=h)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n1,n2,mmax,nmax,N", NV_ORDERS_SHAPES)
def test_convmat_nv_orders_null_field_is_lattice_field(backend, n1, n2, mmax, nmax, N):
    be = get_backend(backend)
    rng = np.random.default_rng([12, n1, n2, N])
    h = np.array(CELLS["skew"]) / np.array([[n1], [n2]])
    mn = _order_list(rng, N, mmax, nmax, distinct=True)
    g = _textured(rng, 2, n1, n2, 1)
    for dtype in (C128, C64):
        rc, nn = _call_field(be, dtype, g, 1.5, h=h)
        assert rc == 0 and (nn != 0).any()
        rc0, a, i0 = _call_nv(be, dtype, g, mmax, nmax, nn=None, sigma=1.5, mn=mn, h=h)
        rc1, b, i1 = _call_nv(be, dtype, g, mmax, nmax, nn=nn, mn=mn, h=h)
        assert rc0 == 0 and rc1 == 0 and not i0.any() and not i1.any()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# Worst err / max(e_plain, n eps) per entry over all the cases a backend runs, rounded up (the bound is 16; no entry needed a margin of its own).
# trx_normal_field: the sigma = 0 case, where err and the floor taps * eps = 2 eps are both one or two roundings of N N^T.
WORST_EMU = {
    "trx_convmat": 0.1, "trx_convmat_orders": 0.2, "trx_convmat_li": 5.2, "trx_normal_field": 1.0, "trx_normal_field_lattice": 0.1,
    "trx_convmat_nv": 1.3, "trx_convmat_nv_orders": 0.6,
}
WORST_MI355X = {
    "trx_convmat": 0.1, "trx_convmat_orders": 0.1, "trx_convmat_li": 2.6, "trx_normal_field": 1.0, "trx_normal_field_lattice": 0.1,
    "trx_convmat_nv": 1.6, "trx_convmat_nv_orders": 0.6,
}
# Largest share of pixels in the threshold band [TAU/2, 2 TAU] over all field cases: 0.011 % (one pixel of (70,131,1.5), real grid, member 0);
# 0 in every other case, the flat disks included (cap: 1 %).

MUTATIONS = """
Four one-line changes, each on a scratch copy of the kernels, run through the emulator (nothing of it is committed):
 1. toeplitz_inv_kernel without the column interchanges in reverse order at its end: all 32 cases of test_convmat_li_pivoting and both of
    test_convmat_li_info fail (errors of O(1)); every emulator test of tests/test_li_factorisation.py still passes -- its positive grids
    never interchange a row.
 2. dft_rows_kernel without `if (idx >= ny) idx -= ny`: test_convmat_tile_edges fails at every shape with oy > 0 (10 of 14 cases; with
    oy = 0 the step is 0), as do all 22 cases of test_convmat_orders_tile_edges, test_convmat_orders_single_harmonic_global_box and the tensor
    tests built on these coefficients.  The old tests of the kernel fail too (test_blocks.py::test_convmat, ::test_convmat_index_map_is_exact,
    test_lattice.py::test_convmat_orders_*, test_normal_vector.py::test_convmat_nv_*): this line was never a gap, a second trip of the
    stride loops around it was.
 3. nv_field_x_kernel with `blockIdx.x * 32` for its y tile: test_normal_field_tile_edges fails at (70,131,1.5) and (5,300,2) (4 cases: the
    columns past the last overlapping tile are never written and stay NaN), as do the 4 cases of test_normal_field_lattice_tile_edges and both
    of test_convmat_nv_null_field_is_normal_field; at ny = 66 the two overlapping tiles still cover every column with the right values, so
    (130,66,43) passes.  The old field tests (test_normal_vector.py::test_normal_field_*, test_lattice.py::test_normal_field_lattice,
    ny <= 26: one tile) all still pass.
 4. li_direction with beta = 1 for the first row chunk too (`r0 == 0 ? zero : one` -> `one`), so that E accumulates onto the unwritten F / G
    of the workspace: the 16 keep=False cases of test_convmat_li_pivoting and test_convmat_li_info[False] fail (NaN outputs; the 0xFF fill
    of _workspace is what makes them fail -- with a fill that reads as a tiny double they all passed); the keep=True cases take the
    one-pass branch and pass.  The kernel-level tests of tests/test_li_factorisation.py, whose workspaces are zero-filled, still pass; its
    end-to-end runs through the engine, whose workspace is whatever the allocator returns, fail.
"""

# Findings of this file, both in csrc/convmat_li.hip and both fixed with it ("Block tests"):
#  * the rows per chunk of the not-kept inverses depended on the dtype, so a complex64 call accumulated in another order than the complex128
#    call and was not its rounding ((13,9,3,1), (9,131,3,2) and (260,5,1,1) on the signed grids differed in the last complex64 bit);
#  * a zero grid value was reported as info 2, not 1: the NaN block of its row ends the Gauss-Jordan sweep as "singular", which overwrote the 1.
