"""trx_layer_field and trx_field_synth through the C ABI (emulator + MI355X), caller-owned buffers with guard words around `out`.

trx_layer_field against numpy in complex128, bounds derived as in test_flux_kernel.py (the forward error of an n-term sum accumulated in fp64,
eps = that of the input dtype for complex64 and 2^-53 for complex128):
    rows 0-3   4 n eps sum|terms|
    rows 4, 5  (4 n + 4) eps (|ky| M_hx + |kx| M_hy)  resp.  (|kx| M_ey + |ky| M_ex),   M = sum|terms| of the row
trx_field_synth against the full, non-separable phase theta = w (kx u + ky v) in longdouble, summed in clongdouble:
    4 (N + theta_max + 2) eps sum_m |coef|     (N terms; a phase formed in fp64 from three roundings of theta carries ~ theta eps)
Derived, not tuned.  Two identical calls must give bit-identical output (every element is owned by one thread; no atomics).
"""
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend

BACKEND_N = ([pytest.param(b, n, marks=getattr(pytest.mark, b)) for b in ("emu", "gpu") for n in (98, 242)]
             + [pytest.param("gpu", n, marks=pytest.mark.gpu) for n in (1054, 1922)])
BACKEND_NH = ([pytest.param(b, N, marks=getattr(pytest.mark, b)) for b in ("emu", "gpu") for N in (1, 49, 121)]
              + [pytest.param("gpu", 481, marks=pytest.mark.gpu)])

GUARD = 5                      # elements on either side of `out`: the output pointer is then only element-aligned
SENTINEL = -7.25 + 3.5j


def _eps(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else float(np.finfo(np.float32).eps)


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _guarded(be, count, dtype):
    buf = be.dev(np.full(count + 2 * GUARD, SENTINEL, dtype=dtype))
    return buf, be.ptr(buf) + GUARD * np.dtype(dtype).itemsize


def _unguard(be, buf, shape):
    h = be.host(buf)
    assert (h[:GUARD] == h.dtype.type(SENTINEL)).all() and (h[-GUARD:] == h.dtype.type(SENTINEL)).all(), "guard words overwritten"
    return h[GUARD:len(h) - GUARD].reshape(shape).copy()


# ---- trx_layer_field -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _layer_operands(n, B):
    """complex128 operands of one (n, B), shared by the nz / dtype cases (read-only)."""
    rng = np.random.default_rng(n * 100 + B)
    N = n // 2
    ops = dict(W=_rand(rng, (B, n, n)), V=_rand(rng, (B, n, n)), cp=_rand(rng, (B, n)), cm=_rand(rng, (B, n)),
               kz=rng.uniform(-2, 2, (B, n)) + 1j * rng.uniform(0.01, 1.0, (B, n)),                 # positive imaginary parts
               omega=rng.uniform(0.008, 0.015, B), d=rng.uniform(50.0, 150.0, B),
               kx=rng.uniform(-8, 8, (B, N)), ky=rng.uniform(-8, 8, (B, N)), frac=rng.uniform(0.0, 1.0, (B, 17)))
    for a in ops.values():
        a.setflags(write=False)
    return ops


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("nz", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("backend,n", BACKEND_N)
def test_layer_field(backend, n, B, nz, dtype):
    be = get_backend(backend)
    N = n // 2
    o = _layer_operands(n, B)
    W, V, cp, cm, kz = (o[k].astype(dtype) for k in ("W", "V", "cp", "cm", "kz"))
    omega, d, kx, ky = (o[k].copy() for k in ("omega", "d", "kx", "ky"))
    frac = o["frac"][:, :nz].copy()
    frac[:, 0] = 0.0
    if nz > 1:
        frac[:, 1] = 1.0
    dev = [be.dev(a) for a in (W, V, cp, cm, kz, omega, d)]
    dk = [be.dev(kx), be.dev(ky)]
    W128, V128 = W.astype(np.complex128), V.astype(np.complex128)
    zz = frac * d[:, None]
    k128 = kz.astype(np.complex128)
    a = cp.astype(np.complex128)[:, :, None] * np.exp(1j * omega[:, None, None] * k128[:, :, None] * zz[:, None, :])
    b = cm.astype(np.complex128)[:, :, None] * np.exp(1j * omega[:, None, None] * k128[:, :, None] * (d[:, None, None] - zz[:, None, :]))
    e = np.einsum("bik,bkt->bit", W128, a + b)
    h = np.einsum("bik,bkt->bit", V128, a - b)
    me = np.einsum("bik,bkt->bit", np.abs(W128), np.abs(a) + np.abs(b))
    mh = np.einsum("bik,bkt->bit", np.abs(V128), np.abs(a) + np.abs(b))
    ex, ey, hx, hy = e[:, :N], e[:, N:], h[:, :N], h[:, N:]
    kxc, kyc = kx[:, :, None], ky[:, :, None]
    ref = np.stack((ex, ey, hx, hy, kyc * hx - kxc * hy, kxc * ey - kyc * ex), axis=1)
    eps = _eps(dtype)
    bound = np.stack((4 * n * eps * me[:, :N], 4 * n * eps * me[:, N:], 4 * n * eps * mh[:, :N], 4 * n * eps * mh[:, N:],
                      (4 * n + 4) * eps * (np.abs(kyc) * mh[:, :N] + np.abs(kxc) * mh[:, N:]),
                      (4 * n + 4) * eps * (np.abs(kxc) * me[:, N:] + np.abs(kyc) * me[:, :N])), axis=1)
    for z_is_fraction in (0, 1):
        dz = be.dev(frac if z_is_fraction else zz)
        outs = []
        for _ in range(2):
            buf, optr = _guarded(be, B * 6 * N * nz, dtype)
            rc = be.lib.layer_field(dtcode(dtype), *[be.ptr(t) for t in dev], be.ptr(dz), z_is_fraction, be.ptr(dk[0]), be.ptr(dk[1]), N, nz, B,
                                    optr, be.stream)
            assert rc == 0
            outs.append(_unguard(be, buf, (B, 6, N, nz)))
        assert np.array_equal(outs[0], outs[1])                                                       # deterministic
        err = np.abs(outs[0] - ref)
        worst = (err / bound).reshape(B, 6, -1).max(axis=(0, 2))
        print(f"n={n} B={B} nz={nz} {np.dtype(dtype).name} frac={z_is_fraction}: max err / bound per row = {np.array2string(worst, precision=3)}")
        assert (err <= bound).all(), worst


# ---- trx_field_synth -------------------------------------------------------------------------------------------------------------------
# (nu, nv, T): horizontal maps (T = 1; one sample, two tiles along u / partial lanes, and the transposed shape), then vertical cuts (nv = 1)
SYNTH_SHAPES = [(1, 1, 1), (17, 33, 1), (33, 17, 1), (1, 1, 2), (1, 1, 17), (33, 1, 2), (33, 1, 17)]


def _synth_reference(coef, ku, kv, omega, u, v):
    """out[b,c,iu,iv,t] and sum_m |coef| [b,c,1,1,t] and theta_max, the phase in longdouble and the sum in clongdouble."""
    L = np.longdouble
    th = omega.astype(L)[:, None, None, None] * (ku.astype(L)[:, None, None, :] * u.astype(L)[None, :, None, None]
                                                 + kv.astype(L)[:, None, None, :] * v.astype(L)[None, None, :, None])     # [B, nu, nv, N]
    ph = np.cos(th) + 1j * np.sin(th)
    ref = np.einsum("buvm,bcmt->bcuvt", ph, coef.astype(np.clongdouble))
    mag = np.abs(coef.astype(np.clongdouble)).sum(axis=2)[:, :, None, None, :]
    return ref, mag, float(np.abs(th).max())


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("ncomp", [1, 6])
@pytest.mark.parametrize("nu,nv,T", SYNTH_SHAPES)
@pytest.mark.parametrize("backend,N", BACKEND_NH)
def test_field_synth(backend, N, nu, nv, T, ncomp, B, dtype):
    be = get_backend(backend)
    rng = np.random.default_rng(N * 1000 + nu * 100 + nv * 10 + T + ncomp + B)
    coef = _rand(rng, (B, ncomp, N, T)).astype(dtype)
    kx, ky = rng.uniform(-8, 8, (B, N)), rng.uniform(-8, 8, (B, N))
    omega = rng.uniform(0.008, 0.015, B)
    u, v = rng.uniform(0.0, 300.0, nu), rng.uniform(0.0, 300.0, nv)
    dcoef, dkx, dky, dom, du, dv = (be.dev(a) for a in (coef, kx, ky, omega, u, v))
    calls = [((dkx, dky), (kx, ky))]
    if nv == 1:
        calls.append(((dky, dkx), (ky, kx)))      # a yz cut: the caller swaps the roles; the reference exchanges x and y
    for (dku, dkv), (ku, kv) in calls:
        outs = []
        for _ in range(2):
            buf, optr = _guarded(be, B * ncomp * nu * nv * T, dtype)
            rc = be.lib.field_synth(dtcode(dtype), be.ptr(dcoef), be.ptr(dku), be.ptr(dkv), be.ptr(dom), be.ptr(du), be.ptr(dv), ncomp, N, T, nu, nv,
                                    B, optr, be.stream)
            assert rc == 0
            outs.append(_unguard(be, buf, (B, ncomp, nu, nv, T)))
        assert np.array_equal(outs[0], outs[1])                                                       # deterministic
        ref, mag, thmax = _synth_reference(coef, ku, kv, omega, u, v)
        bound = 4 * (N + thmax + 2) * _eps(dtype) * mag
        err = np.abs(outs[0] - ref)
        print(f"N={N} ({nu},{nv},{T}) ncomp={ncomp} B={B} {np.dtype(dtype).name}: max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), float((err / bound).max())


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_field_kernel_argument_checks(backend):
    be = get_backend(backend)
    rng = np.random.default_rng(3)
    dtype, n, N, B, nz = np.complex128, 6, 3, 2, 2
    ops = [be.dev(_rand(rng, s)) for s in ((B, n, n), (B, n, n), (B, n), (B, n), (B, n))] + [be.dev(rng.uniform(0.01, 0.02, B)),
                                                                                            be.dev(rng.uniform(50, 60, B))]
    z, kx, ky = be.dev(rng.uniform(0, 1, (B, nz))), be.dev(rng.uniform(-1, 1, (B, N))), be.dev(rng.uniform(-1, 1, (B, N)))
    p = [be.ptr(t) for t in ops]

    def layer(code, nz_, B_):
        buf, optr = _guarded(be, B * 6 * N * nz, dtype)
        rc = be.lib.layer_field(code, *p, be.ptr(z), 1, be.ptr(kx), be.ptr(ky), N, nz_, B_, optr, be.stream)
        return rc, _unguard(be, buf, (B, 6, N, nz))

    assert layer(7, nz, B)[0] == -1                                          # TRX_ERR_DTYPE
    for nz_, B_ in ((0, B), (nz, 0)):                                        # nothing to compute: TRX_OK, `out` and its guard words untouched
        rc, out = layer(1, nz_, B_)
        assert rc == 0 and (out == SENTINEL).all()
    assert layer(1, -1, B)[0] == -2 and layer(1, nz, 65536)[0] == -2
    rc, out = layer(1, nz, B)
    assert rc == 0 and not (out == SENTINEL).any()

    nu, nv = 3, 4
    coef, om, u, v = be.dev(_rand(rng, (B, 6, N, 2))), be.dev(rng.uniform(0.01, 0.02, B)), be.dev(rng.uniform(0, 300, nu)), be.dev(rng.uniform(0, 300, nv))

    def synth(code, ncomp, T, nu_, nv_, B_):
        buf, optr = _guarded(be, B * 6 * nu * nv * 2, dtype)
        rc = be.lib.field_synth(code, be.ptr(coef), be.ptr(kx), be.ptr(ky), be.ptr(om), be.ptr(u), be.ptr(v), ncomp, N, T, nu_, nv_, B_, optr, be.stream)
        return rc, _unguard(be, buf, (-1,))

    assert synth(7, 6, 1, nu, nv, B)[0] == -1                                # TRX_ERR_DTYPE
    assert synth(1, 7, 1, nu, nv, B)[0] == -2 and synth(1, 0, 1, nu, nv, B)[0] == -2      # 1 <= ncomp <= 6
    assert synth(1, 6, 2, nu, nv, B)[0] == -2                                # nv > 1 with T > 1
    for nu_, nv_, B_ in ((0, nv, B), (nu, 0, B), (nu, nv, 0)):
        rc, out = synth(1, 6, 1, nu_, nv_, B_)
        assert rc == 0 and (out == SENTINEL).all()
    assert synth(1, 6, 1, nu, nv, B)[0] == 0 and synth(1, 6, 2, nu, 1, B)[0] == 0
