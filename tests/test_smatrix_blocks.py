"""The middle of the pipeline at block level: trx_layer_smatrix (with the right solves of lu.hip behind it), trx_redheffer and the XY
coupling factors, trx_eig_backward and the six trx_build_pq* / trx_build_a* entries, each against an independent numpy restatement of the
same operation.

Policy ("Block tests"):
  * independent algebra: the layer reference inverts the 2n x 2n matrix of torcwa/rcwa.py:1268-1274 (the kernel: two n x n solves), the star
    product reference forms both inverses (the kernel: one LU and the push-through identity);
  * reference precision: complex128 for a complex64 kernel; for a complex128 kernel every solve is refined with clongdouble residuals
    (helpers.solve_hp, validated against mpmath below) and every product is formed in clongdouble;
  * the tolerance comes from the reference, not from the library: e_plain = the error of the SAME formulas evaluated by LAPACK in the
    kernel's own dtype against that reference, and the kernel must satisfy  err <= 16 * max(e_plain, n * eps(dtype))  (another summation
    order than LAPACK's costs a small factor; a wrong block, sign, permutation or a dropped K tail is O(1) off);
  * guards on the reference data (asserted, never skipped): every inverted matrix has condition number <= 1e4, and a plain partial-pivot
    LU of it interchanges rows at >= half of its steps, so a wrong permutation cannot pass;
  * every output and the workspace carry a tail of guard words behind the size include/trx.h states; the workspace has exactly *_ws_bytes.
Every test draws from its own np.random.default_rng(seed).  Bodies run on the emulator (`-m emu`) and on the MI355X (`-m gpu`).
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import crandn, lu_interchanges, relmax, solve_hp, star_full

GUARD = 64                       # guard elements behind every buffer
SENT = 7.25 - 3.5j
MARGIN = 16.0
LD = np.clongdouble


def _eps(dtype):
    return float(np.finfo(dtype).eps)


def _solve_plain(A, B):
    """LAPACK in the dtype of A (numpy.linalg computes complex64 problems in double; torch calls cgesv)."""
    return torch.linalg.solve(torch.from_numpy(np.ascontiguousarray(A)), torch.from_numpy(np.ascontiguousarray(B))).numpy()


def _arith(dtype, hp):
    """(working dtype, solve) of a reference evaluation: hp -> the high-precision reference of a kernel of `dtype`, else LAPACK in `dtype`."""
    if not hp:
        return dtype, _solve_plain
    return (LD, solve_hp) if dtype == np.complex128 else (np.complex128, _solve_plain)


def _bound(e_plain, n, dtype):
    return MARGIN * max(e_plain, n * _eps(dtype))


def _check(what, got, ref, e_plain, n, dtype, ratios):
    err = relmax(got, ref)
    ratios.append(err / max(e_plain, n * _eps(dtype)))
    assert err <= _bound(e_plain, n, dtype), (f"{what}: err {err:.3e}  e_plain {e_plain:.3e}  err/e_plain {err / max(e_plain, 1e-300):.2f}  "
                                              f"n*eps {n * _eps(dtype):.3e}  bound {_bound(e_plain, n, dtype):.3e}")


class Guarded:
    """A device buffer of `count` elements followed by GUARD sentinel elements."""

    def __init__(self, be, count, dtype, body=None):
        dtype = np.dtype(dtype)
        self.be, self.count, self.dtype = be, int(count), dtype
        self.sent = {"c": SENT, "i": -77, "u": 0xA5}[dtype.kind]
        flat = np.empty(self.count + GUARD, dtype=dtype)
        flat[:self.count] = (np.nan if dtype.kind == "c" else self.sent) if body is None else np.asarray(body, dtype=dtype).reshape(-1)
        flat[self.count:] = self.sent
        self.buf = be.dev(flat)

    def ptr(self, offset=0):
        return self.be.ptr(self.buf) + offset * self.dtype.itemsize

    def host(self, shape=None):
        h = self.be.host(self.buf)
        assert (h[self.count:] == self.dtype.type(self.sent)).all(), "guard words behind the buffer were overwritten"
        return h[:self.count].reshape(shape if shape is not None else (-1,))


# ---- the high-precision solve ---------------------------------------------------------------------------------------------------------

def test_solve_hp_against_mpmath():
    """helpers.solve_hp (LAPACK + two refinement steps with clongdouble residuals) against a 50-digit mpmath solve, n <= 24.  Fails loudly
    where long double is not the 80-bit extended type: the complex128 cases of this file would silently lose their reference."""
    import mpmath
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not extended precision here: no reference beyond complex128"
    mpmath.mp.dps = 50
    rng = np.random.default_rng(31)

    def to_mp(z):          # exact: a long double is the sum of two doubles
        def r(x):
            hi = float(x)
            return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))
        return mpmath.mpc(r(z.real), r(z.imag))

    for n, nrhs in [(5, 2), (16, 3), (24, 4)]:
        A = crandn(rng, (n, n)) / np.sqrt(n)
        A[:, 0] *= 1e-3                                      # cond ~ 1e3 - 1e4: plain LAPACK loses 3 - 4 of its 16 digits
        B = crandn(rng, (n, nrhs))
        X = solve_hp(A, B)
        assert X.dtype == LD
        Am = mpmath.matrix(A.tolist())
        cols = [mpmath.lu_solve(Am, mpmath.matrix(B[:, j].tolist())) for j in range(nrhs)]          # mpmath solves one column at a time
        Xm = {(i, j): cols[j][i] for i in range(n) for j in range(nrhs)}
        scale = max(abs(Xm[i, j]) for i in range(n) for j in range(nrhs))
        err_hp = max(abs(to_mp(X[i, j]) - Xm[i, j]) for i in range(n) for j in range(nrhs)) / scale
        Xd = np.linalg.solve(A, B)
        err_plain = max(abs(mpmath.mpc(complex(Xd[i, j])) - Xm[i, j]) for i in range(n) for j in range(nrhs)) / scale
        cond = np.linalg.cond(A)
        assert err_hp < 4 * cond * 1.1e-19, (n, float(err_hp), cond)          # the limiting accuracy of refinement: cond * eps(residual)
        assert err_hp < 1e-3 * err_plain, (n, float(err_hp), float(err_plain))


# ---- 1. trx_layer_smatrix -------------------------------------------------------------------------------------------------------------

def _layer_formulas(inp, use_q, wd, solve):
    """torcwa/rcwa.py:1244-1281 restated: F = Vf^-1 V, C = [[W+F, (W-F)X],[(W-F)X, W+F]], [c+; c-] = C^-1 [2I; 0] with the 2n x 2n inverse,
    S11 = W X c+ + W c-, S21 = W c+ + W X c- - I.  Evaluated in the working dtype `wd` with `solve`."""
    P, Q, W, Vin, kzfac, vf, x = [np.asarray(inp[k], dtype=wd) for k in ("P", "Q", "W", "Vin", "kzfac", "vf", "x")]
    n = W.shape[0]
    N = n // 2
    I = np.eye(n, dtype=wd)
    if use_q == 0:
        V = solve(P, W * kzfac[None, :])
    elif use_q == 1:
        V = Q @ (W * kzfac[None, :])
    else:
        V = Vin
    F = np.concatenate([vf[0][:, None] * V[:N] + vf[1][:, None] * V[N:], vf[2][:, None] * V[:N] + vf[3][:, None] * V[N:]])
    A, Bm = W + F, (W - F) * x[None, :]
    C = np.block([[A, Bm], [Bm, A]])
    c = solve(C, np.concatenate([2 * I, np.zeros((n, n), dtype=wd)]))
    cp, cm = c[:n], c[n:]
    WX = W * x[None, :]
    out = {"V": V, "S11": WX @ cp + W @ cm, "S21": W @ cp + WX @ cm - I, "Cplus": cp, "Cminus": cm}
    return out, (A + Bm, A - Bm, C)


def _layer_inputs(N, b, use_q, dtype, zero_col=None):
    """Inputs of one point, drawn from a generator of its own and rounded to the kernel's dtype."""
    n = 2 * N
    rng = np.random.default_rng([20261, N, b, use_q])
    inp = {k: crandn(rng, (n, n)) / np.sqrt(n) for k in ("P", "Q", "W", "Vin")}
    # P: a random unitary with column scales 0.5 ... 2 (cond 4; its LU still pivots), so that V = P^-1 W diag(kz) has the size of the other
    # branches' V: with a Gaussian P the spread of its singular values goes into Tp and Tm (cond 2e4 ... 3e6 at these sizes)
    inp["P"] = np.linalg.qr(inp["P"])[0] * (0.5 + 1.5 * rng.random(n))[None, :]
    inp["kzfac"] = crandn(rng, (n,))
    inp["vf"] = 0.5 * crandn(rng, (4, N))
    # evanescent modes: magnitudes spread evenly (in the exponent) over 1e-40 ... 1, in random order; most of them underflow in complex64.
    # Stratified, not sampled: the range is covered up to |x| = 1 at every n (see the note on S11 in test_layer_smatrix)
    mag = 10.0 ** (-40.0 * rng.permutation(n) / (n - 1.0))
    mag[rng.choice(n, size=4, replace=False)] = 0.0
    inp["x"] = mag * np.exp(2j * np.pi * rng.random(n))
    if zero_col is not None:                                 # a mode without field: column zero_col of Tp and of Tm is exactly zero
        inp["W"][:, zero_col] = 0.0
        inp["Vin"][:, zero_col] = 0.0
    with np.errstate(under="ignore"):
        return {k: v.astype(dtype) for k, v in inp.items()}


@functools.lru_cache(maxsize=3)
def _layer_point(N, b, use_q, dtname):
    """Inputs, high-precision reference, e_plain and the two guards of one point (cached: the three output modes and both batch sizes share it)."""
    dtype = np.dtype(dtname).type
    n = 2 * N
    inp = _layer_inputs(N, b, use_q, dtype)
    ref, (Tp, Tm, C) = _layer_formulas(inp, use_q, *_arith(dtype, True))
    ref = {k: v.astype(np.complex128) for k, v in ref.items()}
    plain, _ = _layer_formulas(inp, use_q, *_arith(dtype, False))
    e_plain = {k: relmax(plain[k], ref[k]) for k in ref}
    inverted = {"Tp": Tp, "Tm": Tm, "C": C}
    if use_q == 0:
        inverted["P"] = inp["P"]
    conds = {k: float(np.linalg.cond(np.asarray(v, dtype=np.complex128))) for k, v in inverted.items()}
    swaps = lu_interchanges(Tp)
    return inp, ref, e_plain, conds, swaps


def _layer_cases():
    out = []
    for dtype, N, use_q, batch, mode in itertools.product((np.complex128, np.complex64), (35, 41, 150, 265), (0, 1, 2), (3, 1),
                                                          ("coupling", "lean", "split")):
        out.append(pytest.param(dtype, N, use_q, batch, mode, id=f"{np.dtype(dtype).name}-N{N}-q{use_q}-b{batch}-{mode}"))
    return out


def _call_layer_smatrix(be, dtype, inps, use_q, N, mode, ws_lean=None):
    """One call through the C ABI with caller-owned, guarded buffers.  mode: coupling (Cplus / Cminus requested, full workspace), lean (no
    coupling, S11 | S21 one [2B,n,n] block, lean workspace), split (no coupling, S11 and S21 separate allocations, full workspace)."""
    B, n = len(inps), 2 * N
    nn = n * n
    st = {k: np.stack([p[k] for p in inps]) for k in ("P", "Q", "W", "Vin", "kzfac", "x")}
    vf = np.stack([p["vf"] for p in inps], axis=1)                              # [4, B, N]
    dP, dQ, dW, dkz, dvf, dx = [be.dev(a) for a in (st["P"], st["Q"], st["W"], st["kzfac"], vf, st["x"])]
    if mode == "lean":
        S = Guarded(be, 2 * B * nn, dtype)
        p11, p21 = S.ptr(), S.ptr(B * nn)
    else:
        S11, S21 = Guarded(be, B * nn, dtype), Guarded(be, B * nn, dtype)
        p11, p21 = S11.ptr(), S21.ptr()
        assert p21 != p11 + B * nn * np.dtype(dtype).itemsize
    V = Guarded(be, B * nn, dtype, body=st["Vin"] if use_q == 2 else None)
    Cp = Cm = None
    if mode == "coupling":
        Cp, Cm = Guarded(be, B * nn, dtype), Guarded(be, B * nn, dtype)
    piv = Guarded(be, 3 * B * n, np.int32)
    info = Guarded(be, 3 * B, np.int32, body=np.full(3 * B, -7))
    nws = (be.lib.layer_smatrix_ws_bytes_lean if mode == "lean" else be.lib.layer_smatrix_ws_bytes)(dtcode(dtype), N, B)
    assert nws == np.dtype(dtype).itemsize * (4 if mode == "lean" else 6) * B * nn          # include/trx.h: 4 / 6 matrices per point
    ws = Guarded(be, nws, np.uint8)
    rc = be.lib.layer_smatrix(dtcode(dtype), be.ptr(dP) if use_q == 0 else None, be.ptr(dQ) if use_q == 1 else None, be.ptr(dW), be.ptr(dkz),
                              be.ptr(dvf), be.ptr(dx), use_q, N, B, p11, p21, V.ptr(), Cp.ptr() if Cp else None, Cm.ptr() if Cm else None,
                              piv.ptr(), info.ptr(), ws.ptr(), nws, be.stream)
    assert rc == 0
    ws.host()
    piv.host()
    out = {"V": V.host((B, n, n)), "info": info.host()}
    if mode == "lean":
        h = S.host((2, B, n, n))
        out["S11"], out["S21"] = h[0], h[1]
    else:
        out["S11"], out["S21"] = S11.host((B, n, n)), S21.host((B, n, n))
    if Cp:
        out["Cplus"], out["Cminus"] = Cp.host((B, n, n)), Cm.host((B, n, n))
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,use_q,batch,mode", _layer_cases())
def test_layer_smatrix(backend, dtype, N, use_q, batch, mode):
    """trx_layer_smatrix against the 2n x 2n restatement: use_q 0 / 1 / 2 x (coupling | lean | split outputs) x n = 70 (one panel block),
    82 (ragged panel), 300 (two outer blocks of lu_solve_right), 530 (three, short tail) x batch 1 / 3 x both dtypes; S11, S21, V and
    Cplus / Cminus; info[0..3B) zero and written; guard words behind every output, piv, info and the exactly sized workspace.
    Worst err / max(e_plain, n eps) on MI355X: see WORST_MI355X at the end of this file.
    Finding (include/trx.h): the library forms S11 = M+ - M-, M+- = W (I +- X) T+-^-1, where the reference algebra has S11 = W X c+ + W c-.
    When EVERY mode is strongly evanescent S11 is small against M+- and the difference cancels: with phases drawn log-uniformly one point of
    n = 70 had max |x| = 6.5e-3, max |S11| = 0.066 against max |M+| = 3.6, and err / max |S11| = 9.8e-13 = 62 e_plain (the same two solves
    in LAPACK: 4.5e-13), i.e. 1.8e-14 of max |M+|, while S21, V, C+- stayed within 2 e_plain.  The error is of the size eps cond(T) |M+-| that
    the two-solve form promises; it is stated in trx.h rather than bounded here, and the phases below reach |x| = 1 at every size."""
    be = get_backend(backend)
    if backend == "emu" and (N > 150 or (N == 150 and (dtype == np.complex64 or batch > 1))):
        pytest.skip("emulator: n = 300, batch 1 in complex128 covers the outer-block schedule of every branch (the CPU suite stays within "
                    "minutes); the GPU runs all")
    n = 2 * N
    pts = [_layer_point(N, b, use_q, np.dtype(dtype).name) for b in range(batch)]
    for inp, ref, e_plain, conds, swaps in pts:              # guards on the reference data: a bad seed is a bad test input, not a skip
        assert max(conds.values()) <= 1e4, conds
        assert swaps >= n // 2, (swaps, n)
    out = _call_layer_smatrix(be, dtype, [p[0] for p in pts], use_q, N, mode)
    assert (out["info"] == 0).all(), out["info"]             # pre-filled with -7: slots 0..B-1 must have been written for use_q 1 and 2 too
    ratios = []
    for b, (inp, ref, e_plain, conds, swaps) in enumerate(pts):
        for k in ("V", "S11", "S21") + (("Cplus", "Cminus") if mode == "coupling" else ()):
            _check(f"{k}[{b}]", out[k][b], ref[k], e_plain[k], n, dtype, ratios)
    print(f"layer_smatrix worst err/max(e_plain, n eps) = {max(ratios):.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["coupling", "lean", "split"])
def test_layer_smatrix_singular_point(backend, mode):
    """A mode without field (column 9 of W and of V zero) makes column 9 of Tp and of Tm exactly zero for point 1 of 2: info[B + 1] and
    info[2B + 1] report the zero pivot at column 10 (LAPACK numbering), every other slot is 0 and point 0 stays correct."""
    be = get_backend(backend)
    N, B, dtype = 41, 2, np.complex128
    n = 2 * N
    inps = [_layer_inputs(N, 0, 2, dtype), _layer_inputs(N, 1, 2, dtype, zero_col=9)]
    ref, (Tp, Tm, C) = _layer_formulas(inps[0], 2, *_arith(dtype, True))
    plain, _ = _layer_formulas(inps[0], 2, *_arith(dtype, False))
    assert max(np.linalg.cond(np.asarray(M, dtype=np.complex128)) for M in (Tp, Tm, C)) <= 1e4
    out = _call_layer_smatrix(be, dtype, inps, 2, N, mode)
    info = out["info"]
    assert info[B + 1] == 10 and info[2 * B + 1] == 10, info
    assert info[0] == 0 and info[1] == 0 and info[B] == 0 and info[2 * B] == 0, info
    ratios = []
    for k in ("S11", "S21") + (("Cplus", "Cminus") if mode == "coupling" else ()):
        _check(k, out[k][0], ref[k].astype(np.complex128), relmax(plain[k], ref[k]), n, dtype, ratios)


# ---- 2. trx_redheffer and its XY factors ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n", [70, 75, 300])
@pytest.mark.parametrize("batch", [3, 1])
def test_redheffer_dense(backend, dtype, n, batch):
    """trx_redheffer (one LU + push-through) against the reference's formulas with BOTH inverses explicit, S blocks and X | Y.  n = 75: odd,
    the second half X + n of a complex64 [n, 2n] buffer is then only 8-byte aligned; n = 300 in complex128: the products with ld = 2n
    operands go through gemm_big.  S blocks are complex normal / sqrt(n); Sm12 and Sn21 carry a factor 2 so that K = I - Sm12 Sn21 is neither
    within 0.75 of the identity (no interchanges: what a factor 0.3 gives) nor ill-conditioned (cond 3e2 ... 6e3, 57 - 71 of 70 - 75 and
    290 of 300 steps interchange).  Worst ratio on MI355X: see WORST_MI355X."""
    be = get_backend(backend)
    if backend == "emu" and n == 300 and (dtype == np.complex64 or batch > 1):
        pytest.skip("emulator: n = 300 runs with batch 1 in complex128 (the CPU suite stays within minutes); the GPU runs all")
    nn = n * n
    Sm = np.empty((4, batch, n, n), dtype=dtype)
    Sn = np.empty((4, batch, n, n), dtype=dtype)
    for b in range(batch):
        rng = np.random.default_rng([20262, n, b])
        Sm[:, b] = crandn(rng, (4, n, n)) / np.sqrt(n)
        Sn[:, b] = crandn(rng, (4, n, n)) / np.sqrt(n)
    Sm[2] *= 2
    Sn[1] *= 2
    dSm, dSn = [be.dev(Sm[k]) for k in range(4)], [be.dev(Sn[k]) for k in range(4)]
    out = [Guarded(be, batch * nn, dtype) for _ in range(4)]
    XY = Guarded(be, 2 * batch * n * 2 * n, dtype)
    piv, info = Guarded(be, batch * n, np.int32), Guarded(be, batch, np.int32, body=np.full(batch, -7))
    nws = be.lib.redheffer_ws_bytes(dtcode(dtype), n, batch)
    assert nws == np.dtype(dtype).itemsize * batch * nn
    ws = Guarded(be, nws, np.uint8)
    arr = ctypes.c_void_p * 4
    pm, pn, po = arr(*[be.ptr(x) for x in dSm]), arr(*[be.ptr(x) for x in dSn]), arr(*[x.ptr() for x in out])
    rc = be.lib.redheffer(dtcode(dtype), ctypes.addressof(pm), ctypes.addressof(pn), ctypes.addressof(po), XY.ptr(), n, batch, piv.ptr(), info.ptr(),
                          ws.ptr(), nws, be.stream)
    assert rc == 0 and (info.host() == 0).all()
    ws.host()
    piv.host()
    hS = [x.host((batch, n, n)) for x in out]
    hXY = XY.host((2, batch, n, 2 * n))
    ratios = []
    for b in range(batch):
        wd, solve = _arith(dtype, True)
        I = np.eye(n, dtype=wd)
        ref = star_full([Sm[k, b].astype(wd) for k in range(4)], [Sn[k, b].astype(wd) for k in range(4)], lambda M: solve(M, I))
        wp, solvep = _arith(dtype, False)
        Ip = np.eye(n, dtype=wp)
        plain = star_full([Sm[k, b] for k in range(4)], [Sn[k, b] for k in range(4)], lambda M: solvep(M, Ip))
        K = np.eye(n) - Sm[2, b].astype(np.complex128) @ Sn[1, b].astype(np.complex128)
        K2 = np.eye(n) - Sn[1, b].astype(np.complex128) @ Sm[2, b].astype(np.complex128)
        assert max(np.linalg.cond(K), np.linalg.cond(K2)) <= 1e4
        assert lu_interchanges(K) >= n // 2
        got = hS + [hXY[0], hXY[1]]
        for k, name in enumerate(("S11", "S21", "S12", "S22", "X", "Y")):
            r = np.asarray(ref[k], dtype=np.complex128)
            _check(f"{name}[{b}]", got[k][b], r, relmax(plain[k], r), n, dtype, ratios)
    print(f"redheffer worst err/max(e_plain, n eps) = {max(ratios):.3f}")


# ---- 3. trx_eig_backward ----------------------------------------------------------------------------------------------------------------

def _eigbwd_formulas(w, V, gw, gV, eps, wd, solve):
    """include/trx.h: gA = (V^H)^-1 (diag(gw) + conj(F) o (V^H gV)) V^H, F_ij = conj(w_j - w_i) / (|w_j - w_i|^2 + eps), F_ii = 0."""
    w, V, gw, gV = [np.asarray(a, dtype=wd) for a in (w, V, gw, gV)]
    rd = np.zeros(1, dtype=wd).real.dtype
    Vh = V.conj().T
    s = w[None, :] - w[:, None]                              # s_ij = w_j - w_i
    den = s.real * s.real + s.imag * s.imag + rd.type(eps)
    np.fill_diagonal(den, 1)                                 # F_ii = 0 (s_ii = 0; keeps 0 / eps out of the un-broadened case)
    Fc = s / den                                             # conj(F)
    inner = np.diag(gw) + Fc * (Vh @ gV)
    return solve(Vh, inner @ Vh), Vh


def _spectrum(rng, n, kind):
    """gapped: a jittered grid in the complex plane, all gaps >= 2e-2.  close: the same with one exactly equal and one 1e-9-close pair."""
    side = int(np.ceil(np.sqrt(n)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    w = 0.05 * (gx.reshape(-1) + 1j * gy.reshape(-1))[:n] + 0.015 * (rng.random(n) - 0.5 + 1j * (rng.random(n) - 0.5)) - (1.0 + 0.5j)
    w = w[rng.permutation(n)]
    if kind == "close":
        w[7] = w[3]
        w[n - 2] = w[11] + 1e-9
    return w


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n", [70, 300])
@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("case", ["default", "unbroadened", "close", "gw0", "gV0"])
def test_eig_backward(backend, dtype, n, batch, case):
    """trx_eig_backward against the formula of include/trx.h with w and V as inputs (no eigensolver): default broadening 1e-10; the smallest
    positive number of the dtype on a spectrum with gaps >= 2e-2 (the reference's un-broadened branch); an exactly equal and a 1e-9-close
    pair under the default broadening (F finite, up to 10); gw = 0 and gV = 0 (each term alone).  info written and zero.
    Worst ratio on MI355X: see WORST_MI355X."""
    be = get_backend(backend)
    if backend == "emu" and n == 300 and (dtype == np.complex64 or batch > 1 or case in ("gw0", "gV0")):
        pytest.skip("emulator: n = 300 runs the three broadening cases with batch 1 in complex128 (the CPU suite stays within minutes); the GPU runs all")
    nn = n * n
    eps = 1e-10
    if case == "unbroadened":
        eps = 1.4e-45 if dtype == np.complex64 else 4.9e-324
    w, V, gw, gV = [np.empty(s, dtype=dtype) for s in ((batch, n), (batch, n, n), (batch, n), (batch, n, n))]
    for b in range(batch):
        rng = np.random.default_rng([20263, n, b])
        w[b] = _spectrum(rng, n, "close" if case == "close" else "gapped")
        Vb = crandn(rng, (n, n))
        V[b] = Vb / np.linalg.norm(Vb, axis=0)[None, :]
        gw[b] = 0 if case == "gw0" else crandn(rng, (n,))
        gV[b] = 0 if case == "gV0" else crandn(rng, (n, n)) / np.sqrt(n)
    dw, dV, dgw, dgV = [be.dev(a) for a in (w, V, gw, gV)]
    gA = Guarded(be, batch * nn, dtype)
    piv, info = Guarded(be, batch * n, np.int32), Guarded(be, batch, np.int32, body=np.full(batch, -7))
    nws = be.lib.eig_backward_ws_bytes(dtcode(dtype), n, batch)
    ws = Guarded(be, nws, np.uint8)
    rc = be.lib.eig_backward(dtcode(dtype), be.ptr(dw), be.ptr(dV), be.ptr(dgw), be.ptr(dgV), eps, n, batch, gA.ptr(), piv.ptr(), info.ptr(),
                             ws.ptr(), nws, be.stream)
    assert rc == 0 and (info.host() == 0).all()
    ws.host()
    piv.host()
    got = gA.host((batch, n, n))
    ratios = []
    for b in range(batch):
        ref, Vh = _eigbwd_formulas(w[b], V[b], gw[b], gV[b], eps, *_arith(dtype, True))
        ref = ref.astype(np.complex128)
        plain, _ = _eigbwd_formulas(w[b], V[b], gw[b], gV[b], eps, *_arith(dtype, False))
        Vh = Vh.astype(np.complex128)
        assert np.linalg.cond(Vh) <= 1e4
        assert lu_interchanges(Vh) >= n // 2
        if case == "unbroadened":
            d = np.abs(w[b][None, :] - w[b][:, None]) + np.eye(n)
            assert d.min() >= 1e-2
        _check(f"gA[{b}]", got[b], ref, relmax(plain, ref), n, dtype, ratios)
    print(f"eig_backward worst err/max(e_plain, n eps) = {max(ratios):.3f}")


# ---- 4. trx_build_pq*, trx_build_a*: the one assembly implementation through the entries of the three Fourier rules ------------------------

RULES = ["laurent", "li", "normal"]
_SUFFIX = {"laurent": "", "li": "_aniso", "normal": "_tensor"}


def _pq_dense(Exx, Exy, Eyy, Ei, Mx, My, Mi, kx, ky):
    """include/trx.h, trx_build_pq_aniso and trx_build_pq_tensor in one:
    P = [[Kx Ei Ky, My - Kx Ei Kx],[Ky Ei Ky - Mx, -Ky Ei Kx]],  Q = [[-Kx Mi Ky - Exy, Kx Mi Kx - Eyy],[Exx - Ky Mi Ky, Ky Mi Kx + Exy]]."""
    Kx, Ky = np.diag(kx), np.diag(ky)
    P = np.block([[Kx @ Ei @ Ky, My - Kx @ Ei @ Kx], [Ky @ Ei @ Ky - Mx, -Ky @ Ei @ Kx]])
    Q = np.block([[-Kx @ Mi @ Ky - Exy, Kx @ Mi @ Kx - Eyy], [Exx - Ky @ Mi @ Ky, Ky @ Mi @ Kx + Exy]])
    return P, Q


def _rule_tensor(rule, eps):
    """(Exx, Exy, Eyy) that the entry of `rule` stands for, from its own permittivity arguments `eps` (include/trx.h): trx_build_pq / _a take
    E (Exx = Eyy = E, Exy = 0), the _aniso entries Ex, Ey (Exy = 0), the _tensor entries Exx, Exy, Eyy."""
    if rule == "laurent":
        return eps[0], np.zeros_like(eps[0]), eps[0]
    if rule == "li":
        return eps[0], np.zeros_like(eps[0]), eps[1]
    return eps


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", [(np.complex128, 1e-13), (np.complex64, 2e-5)])
@pytest.mark.parametrize("N", [37, 300])
@pytest.mark.parametrize("rule", RULES)
def test_build_pq_dense_formula(backend, dtype, tol, N, rule):
    """trx_build_pq / _aniso / _tensor against np.block of the dense products (general, unrelated matrices: E, Einv, Mu, Muinv, and per rule
    Ex, Ey, Mx, My or Exx, Exy, Eyy -- the kernel must not assume that any two are equal or inverses of each other).  N = 300: the second
    column block of the assembly kernel.  Tolerances of test_gemm."""
    be = get_backend(backend)
    batch, n = 2, 2 * N
    rng = np.random.default_rng([20264, N] + ([RULES.index(rule)] if rule != "laurent" else []))
    draw = lambda: crandn(rng, (batch, N, N)).astype(dtype)
    eps = [draw() for _ in range({"laurent": 1, "li": 2, "normal": 3}[rule])]
    Ei = draw()
    mus = [draw() for _ in range(2 if rule == "li" else 1)]           # M, or Li's Mx, My
    Mi = draw()
    kx, ky = crandn(rng, (batch, N)).astype(dtype), crandn(rng, (batch, N)).astype(dtype)
    dev = [be.dev(a) for a in (*eps, Ei, *mus, Mi, kx, ky)]
    P, Q = Guarded(be, batch * n * n, dtype), Guarded(be, batch * n * n, dtype)
    rc = getattr(be.lib, "build_pq" + _SUFFIX[rule])(dtcode(dtype), *[be.ptr(d) for d in dev], N, batch, P.ptr(), Q.ptr(), be.stream)
    assert rc == 0
    hP, hQ = P.host((batch, n, n)), Q.host((batch, n, n))
    for b in range(batch):
        rP, rQ = _pq_dense(*[a[b].astype(np.complex128) for a in (*_rule_tensor(rule, eps), Ei, mus[0], mus[-1], Mi, kx, ky)])
        assert relmax(hP[b], rP) < tol and relmax(hQ[b], rQ) < tol, (relmax(hP[b], rP), relmax(hQ[b], rQ))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", [(np.complex128, 1e-13), (np.complex64, 2e-5)])
@pytest.mark.parametrize("N", [37, 300])
@pytest.mark.parametrize("rule", RULES)
def test_build_a_is_p_times_q(backend, dtype, tol, N, rule):
    """trx_build_a / _aniso / _tensor (N^3-sized products from the block structure) against the dense A = P Q with Mu = mu I, two different mu
    in the batch.  Laurent's Einv is the inverse of E as before; Li's Ex, Ey and the tensor Exx, Exy, Eyy are unrelated to the matrix Einv
    inverts.  The 2N-deep product of the complex128 case is formed in clongdouble.  Tolerances of test_gemm."""
    be = get_backend(backend)
    batch, n = 2, 2 * N
    rng = np.random.default_rng([20265, N] + ([RULES.index(rule)] if rule != "laurent" else []))
    diag_dominant = lambda: (crandn(rng, (batch, N, N)) * (0.5 / np.sqrt(N)) + 3.0 * np.eye(N)).astype(dtype)
    E = diag_dominant()
    Ei = np.linalg.inv(E.astype(np.complex128)).astype(dtype)
    if rule == "laurent":
        eps = [E]
    elif rule == "li":
        eps = [diag_dominant(), diag_dominant()]
    else:
        eps = [diag_dominant(), (crandn(rng, (batch, N, N)) * (0.5 / np.sqrt(N))).astype(dtype), diag_dominant()]
    mu = np.array([1.0 + 0.0j, 1.3 - 0.2j]).astype(dtype)
    kx, ky = crandn(rng, (batch, N)).astype(dtype), crandn(rng, (batch, N)).astype(dtype)
    dev = [be.dev(a) for a in (*eps, Ei, mu, kx, ky)]
    A = Guarded(be, batch * n * n, dtype)
    nws = getattr(be.lib, "build_a" + _SUFFIX[rule] + "_ws_bytes")(dtcode(dtype), N, batch)
    ws = Guarded(be, nws, np.uint8)
    rc = getattr(be.lib, "build_a" + _SUFFIX[rule])(dtcode(dtype), *[be.ptr(d) for d in dev], N, batch, A.ptr(), ws.ptr(), nws, be.stream)
    assert rc == 0
    ws.host()
    hA = A.host((batch, n, n))
    wd = LD if dtype == np.complex128 else np.complex128
    for b in range(batch):
        m = mu[b].astype(np.complex128)
        I = np.eye(N)
        rP, rQ = _pq_dense(*[a[b].astype(np.complex128) for a in (*_rule_tensor(rule, eps), Ei)], m * I, m * I, I / m,
                           kx[b].astype(np.complex128), ky[b].astype(np.complex128))
        ref = (rP.astype(wd) @ rQ.astype(wd)).astype(np.complex128)
        assert relmax(hA[b], ref) < tol, relmax(hA[b], ref)


# Worst err / max(e_plain, n eps) per test over all its cases (the bound is 16).  On the emulator (every case it runs): test_layer_smatrix
# 3.8, the other tests below 4.  MI355X: from the `-m gpu -s` run that first recorded tests/test_eig_blocks.py, rounded up.
WORST_MI355X = {"test_layer_smatrix": 6.3, "test_redheffer_dense": 4.6, "test_eig_backward": 2.6}
