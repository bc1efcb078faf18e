"""trx_matvec and trx_layer_flux through the C ABI (emulator + MI355X) against numpy in complex128.

Bound: 4 n eps sum|terms| -- the forward error of an n-term sum accumulated in fp64, eps = that of the input dtype for complex64 inputs
(the result, or the operands' own rounding, is then in fp32) and 2^-53 for complex128.  Derived, not tuned.  Two identical calls must give
bit-identical output (partials are combined in a fixed order; no floating-point atomics).
"""
import numpy as np
import pytest

from tests.backends import dtcode, get_backend

# n = 2N: no multiple of a tile size; 1054 and 1922 (orders [11,11] and [15,15]) on the GPU only
BACKEND_N = ([pytest.param(b, n, marks=getattr(pytest.mark, b)) for b in ("emu", "gpu") for n in (98, 242)]
             + [pytest.param("gpu", n, marks=pytest.mark.gpu) for n in (1054, 1922)])


def _eps(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.complex128 else float(np.finfo(np.float32).eps)


def _rand(rng, shape, dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("c", [1, 3, 16])
@pytest.mark.parametrize("backend,n", BACKEND_N)
def test_matvec(backend, n, c, B, dtype):
    be = get_backend(backend)
    rng = np.random.default_rng(n * 100 + c * 10 + B)
    m = 2 * n if c == 1 else n                       # C_layer E_i has m = 2n rows
    A = _rand(rng, (B, m, n), dtype)
    for shared in (False, True):
        X = _rand(rng, (n, c) if shared else (B, n, c), dtype)
        dA, dX = be.dev(A), be.dev(X)
        out = []
        for _ in range(2):
            Y = be.empty((B, m, c), dtype)
            rc = be.lib.matvec(dtcode(dtype), be.ptr(dA), be.ptr(dX), 0 if shared else n * c, be.ptr(Y), m, n, c, B, be.stream)
            assert rc == 0
            out.append(be.host(Y))
        assert np.array_equal(out[0], out[1])
        A128, X128 = A.astype(np.complex128), X.astype(np.complex128)
        ref = np.einsum("bmk,kc->bmc", A128, X128) if shared else np.einsum("bmk,bkc->bmc", A128, X128)
        mag = np.einsum("bmk,kc->bmc", np.abs(A128), np.abs(X128)) if shared else np.einsum("bmk,bkc->bmc", np.abs(A128), np.abs(X128))
        assert (np.abs(out[0] - ref) <= 4 * n * _eps(dtype) * mag).all()
    assert be.lib.matvec(dtcode(dtype), be.ptr(dA), be.ptr(dX), 0, be.ptr(Y), m, n, 17, B, be.stream) == -2      # c > 16: TRX_ERR_ARG


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nz", [1, 2, 17])
@pytest.mark.parametrize("backend,n", BACKEND_N)
def test_layer_flux(backend, n, nz, B, dtype):
    be = get_backend(backend)
    rng = np.random.default_rng(n * 100 + nz * 10 + B)
    N = n // 2
    W, V = _rand(rng, (B, n, n), dtype), _rand(rng, (B, n, n), dtype)
    cp, cm = _rand(rng, (B, n), dtype), _rand(rng, (B, n), dtype)
    kz = (rng.uniform(-2, 2, (B, n)) + 1j * rng.uniform(0.01, 1.0, (B, n))).astype(dtype)           # positive imaginary parts
    omega = rng.uniform(0.008, 0.015, B)
    d = rng.uniform(50.0, 150.0, B)
    frac = rng.uniform(0.0, 1.0, (B, nz))
    frac[:, 0] = 0.0
    if nz > 1:
        frac[:, 1] = 1.0
    dev = [be.dev(a) for a in (W, V, cp, cm, kz, omega, d)]
    for z_is_fraction in (0, 1):
        z = frac if z_is_fraction else frac * d[:, None]
        dz = be.dev(z)
        nws = be.lib.layer_flux_ws_bytes(dtcode(dtype), N, nz, B)
        assert nws == 8 * -(-N // 32) * nz * B
        out = []
        for _ in range(2):
            ws = be.empty((max(nws, 16),), np.uint8)
            flux = be.empty((B, nz), np.float64)
            rc = be.lib.layer_flux(dtcode(dtype), *[be.ptr(a) for a in dev], be.ptr(dz), z_is_fraction, N, nz, B, be.ptr(flux), be.ptr(ws), nws,
                                   be.stream)
            assert rc == 0
            out.append(be.host(flux))
        assert np.array_equal(out[0], out[1])                                                         # deterministic
        zz = frac * d[:, None]
        k128 = kz.astype(np.complex128)
        a = cp.astype(np.complex128)[:, :, None] * np.exp(1j * omega[:, None, None] * k128[:, :, None] * zz[:, None, :])
        b = cm.astype(np.complex128)[:, :, None] * np.exp(1j * omega[:, None, None] * k128[:, :, None] * (d[:, None, None] - zz[:, None, :]))
        W128, V128 = W.astype(np.complex128), V.astype(np.complex128)
        e = np.einsum("bik,bkt->bit", W128, a + b)
        h = np.einsum("bik,bkt->bit", V128, a - b)
        ref = np.real(e[:, :N] * np.conj(h[:, N:]) - e[:, N:] * np.conj(h[:, :N])).sum(axis=1)
        me = np.einsum("bik,bkt->bit", np.abs(W128), np.abs(a) + np.abs(b))
        mh = np.einsum("bik,bkt->bit", np.abs(V128), np.abs(a) + np.abs(b))
        mag = (me[:, :N] * mh[:, N:] + me[:, N:] * mh[:, :N]).sum(axis=1)                              # sum |terms|
        assert out[0].shape == (B, nz)
        assert (np.abs(out[0] - ref) <= 4 * n * _eps(dtype) * mag).all(), (np.abs(out[0] - ref) / mag).max()
    # argument checks: a workspace that is too small, a bad dtype
    assert be.lib.layer_flux(dtcode(dtype), *[be.ptr(a) for a in dev], be.ptr(dz), 0, N, nz, B, be.ptr(flux), be.ptr(ws), nws - 8, be.stream) == -3
    assert be.lib.layer_flux(7, *[be.ptr(a) for a in dev], be.ptr(dz), 0, N, nz, B, be.ptr(flux), be.ptr(ws), nws, be.stream) == -1
