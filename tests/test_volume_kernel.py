"""trx_modal_overlap through the C ABI (emulator + MI355X).

Reference: out = sum_kl M_kl T_kl summed in numpy clongdouble, T assembled from the four G matrices.  For n <= 7 every G is the closed form
(exp(a z1 + b) - exp(a z0 + b)) / a evaluated by mpmath at 50 digits; for larger n it is the end-point / phi rule of include/trx.h evaluated in
clongdouble, and that rule is itself held to the mpmath values at n <= 7 (test_rule_against_mpmath).  The reference of one (n, B, dtype) is
computed once for a pool of 17 ranges and shared by the nr, s and z_is_fraction cases, which call the kernel on consecutive slices of the pool.

Bound:  |out - ref| <= 16 max(e_plain, n^2 eps) sum_kl |M_kl| (|c+_k| + |c-_k|)(|c+_l| + |c-_l|) |z1 - z0|, e_plain the error of
the same rule in numpy complex128 relative to the same magnitude sum (the largest over the case's outputs), eps = 2^-53 for complex128 and the
fp32 eps for complex64 inputs.  Measured from the reference, not tuned to the kernel.

The n^2 reference in clongdouble costs 0.1 s per output at n = 242 and half a second at n = 1054, so at n = 242 the first and the last batch entry
are compared (all 17 ranges) and at n = 1054 four outputs per case (special ranges and the one past the 16-range tile, the last batch entry
included); every output is still checked for finiteness, reproducibility, the reversed and the split range.
"""
import functools

import numpy as np
import pytest

from tests.backends import dtcode, get_backend

LD = np.clongdouble
POOL = 17
BACKEND_N = ([pytest.param(b, n, marks=getattr(pytest.mark, b)) for b in ("emu", "gpu") for n in (1, 7, 98, 242)]
             + [pytest.param("gpu", 1054, marks=pytest.mark.gpu)])


def _eps(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else float(np.finfo(np.float32).eps)


def _phi(x):
    """(e^x - 1) / x in the dtype of x: the series where |x| < 1/2 (phi(0) = 1 exactly), the quotient elsewhere."""
    out = np.empty_like(x)
    small = np.abs(x) < 0.5
    xs = x[small]
    p = np.ones_like(xs)
    for j in range(26, 1, -1):
        p = 1 + xs * p / j
    out[small] = p
    xl = x[~small]
    with np.errstate(under="ignore"):
        out[~small] = (np.exp(xl) - 1) / xl
    return out


def g_rule(kz, om, d, z0, z1, ctype):
    """(G++, G+-, G-+, G--) [n, n] over [z0, z1] by the end-point / phi rule, in `ctype` arithmetic."""
    rt = np.real(np.zeros(1, ctype)).dtype
    kz = kz.astype(ctype)
    om, d, z0, z1 = (np.asarray(v, dtype=rt) for v in (om, d, z0, z1))
    lo, hi = (z1, z0) if z1 < z0 else (z0, z1)
    sg = -1 if z1 < z0 else 1
    D = hi - lo
    with np.errstate(under="ignore"):
        e = lambda z: np.exp(1j * om * kz * z)
        elo, ehi, flo, fhi = e(lo), e(hi), e(d - lo), e(d - hi)
        wr, wi = om * kz.real * D, om * kz.imag * D
        p1 = _phi((-(wi[:, None] + wi[None, :]) + 1j * (wr[None, :] - wr[:, None])).astype(ctype))
        re2 = wi[None, :] - wi[:, None]
        im2 = -(wr[:, None] + wr[None, :])
        first = re2 <= 0
        p2 = _phi(np.where(first, re2 + 1j * im2, -re2 - 1j * im2).astype(ctype))
        c = np.conj
        gpp = c(elo)[:, None] * elo[None, :] * p1
        gmm = c(fhi)[:, None] * fhi[None, :] * p1
        gpm = np.where(first, c(elo)[:, None] * flo[None, :], c(ehi)[:, None] * fhi[None, :]) * p2
        gmp = np.where(first, c(fhi)[:, None] * ehi[None, :], c(flo)[:, None] * elo[None, :]) * p2
    return [g * (sg * D) for g in (gpp, gpm, gmp, gmm)]


def g_mpmath(kz, om, d, z0, z1):
    """The same four matrices from the closed form at 50 digits, rounded to clongdouble."""
    import mpmath as mp
    mp.mp.dps = 50
    n = len(kz)
    q = [mp.mpc(float(v.real), float(v.imag)) for v in kz]
    om, d, z0, z1 = (mp.mpf(float(v)) for v in (om, d, z0, z1))
    j = mp.mpc(0, 1)

    def integ(a, b):
        if a == 0:
            return mp.exp(b) * (z1 - z0)
        return (mp.exp(a * z1 + b) - mp.exp(a * z0 + b)) / a

    out = [np.zeros((n, n), dtype=LD) for _ in range(4)]
    for k in range(n):
        for l in range(n):
            ck = mp.conj(q[k])
            vals = (integ(j * om * (q[l] - ck), 0), integ(-j * om * (ck + q[l]), j * om * q[l] * d),
                    integ(j * om * (ck + q[l]), -j * om * ck * d), integ(-j * om * (q[l] - ck), j * om * (q[l] - ck) * d))
            for g, v in zip(out, vals):
                g[k, l] = np.longdouble(mp.nstr(v.real, 30)) + 1j * np.longdouble(mp.nstr(v.imag, 30))
    return out


def _parts(M, cp, cm, G):
    """(P1, P2) with out = P1 + s P2, in the dtype of G."""
    c = np.conj
    gpp, gpm, gmp, gmm = G
    p1 = (M * (c(cp)[:, None] * cp[None, :] * gpp + c(cm)[:, None] * cm[None, :] * gmm)).sum()
    p2 = (M * (c(cp)[:, None] * cm[None, :] * gpm + c(cm)[:, None] * cp[None, :] * gmp)).sum()
    return p1, p2


def _inputs(n, B, dtype):
    rng = np.random.default_rng(1000 * n + 10 * B + (np.dtype(dtype) == np.complex64))
    r = lambda shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    M, cp, cm = r((B, n, n)), r((B, n)), r((B, n))
    omega = rng.uniform(0.008, 0.015, B)
    d = rng.uniform(50.0, 150.0, B)
    # three families in one vector: exactly real | Im kz in [1e-9, 1e-6] | evanescent with omega Im kz d up to 800
    n1 = (n + 1) // 2
    n2 = (n - n1 + 1) // 2
    kr = rng.uniform(-2.0, 2.0, (B, n))
    ki = np.zeros((B, n))
    ki[:, n1:n1 + n2] = 10.0 ** rng.uniform(-9.0, -6.0, (B, n2))
    n3 = n - n1 - n2
    if n3:
        ki[:, n1 + n2:] = rng.uniform(0.0, 1.0, (B, n3)) * 800.0 / (omega * d)[:, None]
        ki[:, n - 1] = 800.0 / (omega * d)
    kz = (kr + 1j * ki).astype(dtype)
    if n1 >= 4:                       # two pairs of equal real modes: the off-diagonal alpha of G++ and G-- is exactly 0 too
        kz[:, 1], kz[:, 3] = kz[:, 0], kz[:, 2]
    if n3 >= 3:                       # and a pair of equal evanescent ones: Re x2 = 0
        kz[:, n1 + n2 + 1] = kz[:, n1 + n2]
    # the pool of ranges as fractions of d: [0,d], [0,0], an inner range and its reverse, the split [0,z*], [z*,d], then random ones
    fr = rng.uniform(0.0, 1.0, (B, POOL, 2))
    za, zb, zs = 0.21, 0.68, 0.37
    fr[:, :6] = np.array([[0.0, 1.0], [0.0, 0.0], [za, zb], [zb, za], [0.0, zs], [zs, 1.0]])
    return M, cp, cm, kz, omega, d, fr


def _checked(n, B):
    """(b, pool index) pairs that are compared with the reference."""
    if n <= 98:
        return [(b, i) for b in range(B) for i in range(POOL)]
    if n <= 242:
        return [(b, i) for b in sorted({0, B - 1}) for i in range(POOL)]
    return [(0, 0), (B - 1, 3), (B - 1, 5), (B - 1, 16)]


@functools.lru_cache(maxsize=None)
def _reference(n, B, dtname):
    """{(b, i): (P1, P2, P1_plain, P2_plain, mag)} for the checked outputs; P in clongdouble, the plain ones in complex128."""
    dtype = np.dtype(dtname)
    M, cp, cm, kz, omega, d, fr = _inputs(n, B, dtype)
    ref = {}
    for b, i in _checked(n, B):
        z0, z1 = fr[b, i, 0] * d[b], fr[b, i, 1] * d[b]
        k128 = kz[b].astype(np.complex128)
        G = g_mpmath(k128, omega[b], d[b], z0, z1) if n <= 7 else g_rule(k128, omega[b], d[b], z0, z1, LD)
        Ml, cpl, cml = M[b].astype(LD), cp[b].astype(LD), cm[b].astype(LD)
        p1, p2 = _parts(Ml, cpl, cml, G)
        Gp = g_rule(k128, omega[b], d[b], z0, z1, np.complex128)
        q1, q2 = _parts(M[b].astype(np.complex128), cp[b].astype(np.complex128), cm[b].astype(np.complex128), Gp)
        a = np.abs(cp[b].astype(np.complex128)) + np.abs(cm[b].astype(np.complex128))
        mag = float((np.abs(M[b].astype(np.complex128)) * a[:, None] * a[None, :]).sum() * abs(z1 - z0))
        ref[(b, i)] = (p1, p2, q1, q2, mag)
    return ref


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 7])
def test_rule_against_mpmath(n, B):
    """The end-point / phi rule in clongdouble against the closed form at 50 digits: 64 clongdouble eps of |z1 - z0| per element."""
    M, cp, cm, kz, omega, d, fr = _inputs(n, B, np.complex128)
    eps_ld = float(np.finfo(np.longdouble).eps)
    for b in range(B):
        for i in range(POOL):
            z0, z1 = fr[b, i, 0] * d[b], fr[b, i, 1] * d[b]
            for gr, gm in zip(g_rule(kz[b], omega[b], d[b], z0, z1, LD), g_mpmath(kz[b], omega[b], d[b], z0, z1)):
                assert np.isfinite(gr).all()
                assert (np.abs(gr - gm) <= 64 * eps_ld * abs(z1 - z0)).all(), (b, i, np.abs(gr - gm).max())


@pytest.mark.parametrize("s", [-1, 1])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nr", [1, 2, 17])
@pytest.mark.parametrize("backend,n", BACKEND_N)
def test_modal_overlap(backend, n, nr, B, dtype, s):
    be = get_backend(backend)
    M, cp, cm, kz, omega, d, fr = _inputs(n, B, dtype)
    ref = _reference(n, B, np.dtype(dtype).name)
    dev = [be.dev(a) for a in (M, cp, cm, kz, omega, d)]
    nws = be.lib.modal_overlap_ws_bytes(dtcode(dtype), n, nr, B)
    assert nws == 16 * -(-n // 16) * nr * B
    guard = complex(-7.25, 3.5)
    nsl = 1 if nr == POOL else -(-6 // nr)               # slices of the pool that cover the six special ranges
    res = {}
    for z_is_fraction in (0, 1):
        got = np.zeros((B, nsl * nr), dtype=np.complex128)
        for sl in range(nsl):
            f = fr[:, sl * nr:(sl + 1) * nr]
            dz = be.dev(f if z_is_fraction else f * d[:, None, None])
            runs = []
            for _ in range(2 if sl == 0 else 1):
                out = be.dev(np.full(B * nr + 4, guard, dtype=np.complex128))
                ws = be.dev(np.full(nws + 64, 0xA5, dtype=np.uint8))
                rc = be.lib.modal_overlap(dtcode(dtype), *[be.ptr(a) for a in dev], be.ptr(dz), z_is_fraction, s, n, nr, B, be.ptr(out), be.ptr(ws),
                                          nws, be.stream)
                assert rc == 0
                o, w = be.host(out), be.host(ws)
                assert (o[B * nr:] == guard).all() and (w[nws:] == 0xA5).all()        # nothing past out or the exactly sized workspace
                runs.append(o[:B * nr].reshape(B, nr))
            if len(runs) == 2:
                assert np.array_equal(runs[0], runs[1])                             # deterministic
            got[:, sl * nr:(sl + 1) * nr] = runs[0]
        assert np.isfinite(got).all()
        res[z_is_fraction] = got
        e_plain = max(abs((q1 + s * q2) - complex(p1 + s * p2)) / mag for (p1, p2, q1, q2, mag) in ref.values() if mag > 0)
        factor = 16 * max(e_plain, n * n * _eps(dtype))
        worst = 0.0
        for (b, i), (p1, p2, _, _, mag) in ref.items():
            if i >= got.shape[1]:
                continue
            err = abs(got[b, i] - complex(p1 + s * p2))
            worst = max(worst, err / mag if mag > 0 else err)
            assert err <= factor * mag, (b, i, err, factor * mag)
        print(f"n={n} nr={nr} B={B} {np.dtype(dtype).name} s={s} frac={z_is_fraction}: max err / mag = {worst:.2e}, e_plain = {e_plain:.2e}, "
              f"bound factor = {factor:.2e}")
        # the pool's special ranges: [0,0] is exactly 0; the reverse is the negation bit for bit; [0,z*] + [z*,d] = [0,d]
        assert (got[:, 1] == 0).all()
        assert np.array_equal(got[:, 3], -got[:, 2])
        a = np.abs(cp.astype(np.complex128)) + np.abs(cm.astype(np.complex128))
        magd = (np.abs(M.astype(np.complex128)) * a[:, :, None] * a[:, None, :]).sum(axis=(1, 2)) * d
        assert (np.abs(got[:, 4] + got[:, 5] - got[:, 0]) <= 3 * factor * magd).all()
    # z given as a fraction and as an offset: the kernel forms the same z = fraction * d
    assert np.array_equal(res[0], res[1])
    # argument checks
    args = [be.ptr(a) for a in dev] + [be.ptr(dz), 0]
    tail = [be.ptr(out), be.ptr(ws), nws, be.stream]
    assert be.lib.modal_overlap(dtcode(dtype), *args, 0, n, nr, B, *tail) == -2                   # s not in {-1, +1}
    assert be.lib.modal_overlap(dtcode(dtype), *args, 2, n, nr, B, *tail) == -2
    assert be.lib.modal_overlap(dtcode(dtype), *args, s, n, -1, B, *tail) == -2                  # nr < 0
    assert be.lib.modal_overlap(dtcode(dtype), *args, s, n, nr, B, be.ptr(out), be.ptr(ws), nws - 16, be.stream) == -3
    assert be.lib.modal_overlap(7, *args, s, n, nr, B, *tail) == -1
    assert be.lib.modal_overlap(dtcode(dtype), None, None, None, None, None, None, None, 0, s, n, 0, B, None, None, 0, be.stream) == 0   # nr = 0
    assert be.lib.modal_overlap(dtcode(dtype), None, None, None, None, None, None, None, 0, s, n, nr, 0, None, None, 0, be.stream) == 0  # batch = 0
