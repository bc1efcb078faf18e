"""trx_thickness_prepare / trx_thickness_columns (include/trx.h) on random data, against the stack REBUILT at every thickness.

Policy: the block tests' ("Block tests"; tests/test_smatrix_blocks.py).
  * independent algebra: the reference builds the layer S-matrix of every thickness from the 2n x 2n definition of torcwa/rcwa.py:1266-1281,
    star-multiplies it with the left and the right operand (rcwa.py:1287-1294, both inverses explicit) and takes the requested columns; the
    kernels never form a layer S-matrix (reflection operators in the mode basis, one n x n system per thickness);
  * reference precision: complex128 for a complex64 kernel, clongdouble products and helpers.solve_hp for a complex128 kernel;
  * tolerance: err <= 16 * max(e_plain, n * eps(dtype)), e_plain = the error of the same reference formulas through LAPACK in the kernel's dtype;
    errors are max-abs over the requested columns divided by max-abs of the reference BLOCK they belong to (tests/test_redheffer_columns.py);
  * guards on the reference data, asserted for every case: cond(P_L), cond(P_R), cond(K_t) <= 1e4 and |x| <= 1;
  * out, info, piv and the exactly sized workspaces carry guard words.
Data: W a random unitary with column scales 0.5 ... 2; F = Vf^-1 V = W diag(g) + 0.2 x complex normal / sqrt(n) with Re g in [0.3, 1.5] (V is
formed from F and the Vf^-1 diagonals, 0.5 x complex normal); dense operand blocks 0.15 sqrt(12 / n) x complex normal (the same spectral norm,
about 1, at every n), block-diagonal operands 0.4 x complex normal; kz with |Re| <= 3 and Im from 0 (a quarter of the modes propagate) to 10,
thicknesses 0.1 ... 30, so |x| runs from 1 down to underflow.  Checked on the CPU over every operand pair, point and thickness used here:
cond(P) <= 10 and cond(K_t) <= 185 up to n = 286.  (With V an unrelated Gaussian matrix and dense blocks of 0.3 sqrt(12 / n), what holds at
n = 12, cond(K_t) reaches 1.5e5 at n = 70.)
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, crandn, solve_hp, star_full
from tests.test_smatrix_blocks import Guarded, _arith, _bound, _eps

ABSENT, BD, DENSE = 0, 1, 2
KINDS = [(l, r) for l in (BD, DENSE, ABSENT) for r in (BD, DENSE, ABSENT)]
KNAME = {ABSENT: "absent", BD: "bd", DENSE: "dense"}
DIRPORT = [(0, 0), (0, 1), (1, 1), (1, 0)]                   # (direction, port) -> block 0, 1, 2, 3
BLOCK = {(0, 0): 0, (0, 1): 1, (1, 1): 2, (1, 0): 3}
THICK = [0.1, 1.0, 3.0, 10.0, 30.0]
# (batch, T, m) dealt to the operand combinations in turn: batch 1 and 3, T = 1, 3, 5, m = 1 and 2
SHAPES = [(1, 1, 1), (3, 3, 2), (1, 5, 1), (3, 1, 2), (1, 3, 2), (2, 5, 1)]


def _point(N, b):
    """Data of one sweep point in complex128 (rounded to the kernel's dtype by the caller), from a generator of its own."""
    n = 2 * N
    rng = np.random.default_rng([20266, N, b])
    W = np.linalg.qr(crandn(rng, (n, n)))[0] * (0.5 + 1.5 * rng.random(n))[None, :]
    # F = Vf^-1 V = W G + a dense perturbation, Re g > 0: every mode is mostly its own impedance match (|(1 - g) / (1 + g)| < 1), as in a real layer
    g = 0.3 + 1.2 * rng.random(n) + 0.5j * rng.standard_normal(n)
    F = W * g[None, :] + 0.2 * crandn(rng, (n, n)) / np.sqrt(n)
    vf = 0.5 * crandn(rng, (4, N))
    det = vf[0] * vf[3] - vf[1] * vf[2]                          # V = Vf F with Vf the inverse of the 2x2-block-diagonal Vf^-1
    V = np.concatenate([(vf[3] / det)[:, None] * F[:N] - (vf[1] / det)[:, None] * F[N:], (vf[0] / det)[:, None] * F[N:] - (vf[2] / det)[:, None] * F[:N]])
    im = 10.0 ** (-3.0 + 4.0 * rng.random(n))
    im[rng.permutation(n)[: max(2, n // 4)]] = 0.0
    kz = 3.0 * (2 * rng.random(n) - 1) + 1j * im
    ops = {}
    for side in ("L", "R"):
        ops[side + "bd"] = 0.4 * crandn(rng, (4, 4, N))
        ops[side + "dn"] = 0.15 * np.sqrt(12.0 / n) * crandn(rng, (4, n, n))
    return dict(W=W, V=V, vf=vf, kz=kz, **ops)


@functools.lru_cache(maxsize=None)
def _inputs(N, batch, T, dtname):
    dtype = np.dtype(dtname).type
    pts = [_point(N, b) for b in range(batch)]
    with np.errstate(under="ignore"):
        st = {k: np.stack([p[k] for p in pts]).astype(dtype) for k in ("W", "V", "Ldn", "Rdn")}
        st["vf"] = np.stack([p["vf"] for p in pts], axis=1).astype(dtype)                  # [4, B, N]
        for side in "LR":
            st[side + "bd"] = np.stack([p[side + "bd"] for p in pts], axis=2).astype(dtype)   # [4, 4, B, N]
            st[side + "dn"] = np.ascontiguousarray(np.swapaxes(st[side + "dn"], 0, 1))        # [4, B, n, n]
        st["x"] = np.stack([np.stack([np.exp(1j * p["kz"] * d) for d in THICK[:T]]) for p in pts]).astype(dtype)   # [B, T, n]
    assert (np.abs(st["x"]) <= 1.0 + 4 * _eps(dtype)).all()       # |x| <= 1 (a propagating mode's exp(i theta) rounds to within an ulp or two of 1)
    return st


def _operand(st, side, kind, b, wd):
    n = st["W"].shape[1]
    if kind == ABSENT:
        return [np.eye(n, dtype=wd), np.zeros((n, n), dtype=wd), np.zeros((n, n), dtype=wd), np.eye(n, dtype=wd)]
    if kind == BD:
        return [_bd_dense(st[side + "bd"][k, :, b].astype(wd)) for k in range(4)]
    return [st[side + "dn"][k, b].astype(wd) for k in range(4)]


def _stack_formulas(st, kinds, b, t, wd, solve):
    """Lft * layer(d_t) * Rgt from the reference's definitions, in the working dtype `wd`.  Returns the four blocks and (A, B) = (W + F, W - F)."""
    W, V, x = st["W"][b].astype(wd), st["V"][b].astype(wd), st["x"][b, t].astype(wd)
    vf = st["vf"][:, b].astype(wd)
    n = W.shape[0]
    N = n // 2
    I = np.eye(n, dtype=wd)
    F = np.concatenate([vf[0][:, None] * V[:N] + vf[1][:, None] * V[N:], vf[2][:, None] * V[:N] + vf[3][:, None] * V[N:]])
    A, Bm = W + F, (W - F) * x[None, :]
    C = np.block([[A, Bm], [Bm, A]])
    c = solve(C, np.concatenate([2 * I, np.zeros((n, n), dtype=wd)]))
    cp, cm = c[:n], c[n:]
    WX = W * x[None, :]
    S11, S21 = WX @ cp + W @ cm, W @ cp + WX @ cm - I
    inv = lambda M: solve(M, I)
    S = star_full(_operand(st, "L", kinds[0], b, wd), [S11, S21, S21, S11], inv)[:4]
    S = star_full(S, _operand(st, "R", kinds[1], b, wd), inv)[:4]
    return S, (A, W - F)


@functools.lru_cache(maxsize=None)
def _reference(N, batch, T, dtname, kinds):
    """Per (point, thickness): the reference blocks (complex128), the LAPACK-in-dtype blocks, and the guards."""
    dtype = np.dtype(dtname).type
    st = _inputs(N, batch, T, dtname)
    n = 2 * N
    ref, plain = {}, {}
    for b in range(batch):
        for t in range(T):
            S, (A, Bb) = _stack_formulas(st, kinds, b, t, *_arith(dtype, True))
            ref[b, t] = [np.asarray(s, dtype=np.complex128) for s in S]
            plain[b, t] = [np.asarray(s, dtype=np.complex128) for s in _stack_formulas(st, kinds, b, t, *_arith(dtype, False))[0]]
            # guards (complex128): the matrices the kernels factor
            A, Bb = np.asarray(A, dtype=np.complex128), np.asarray(Bb, dtype=np.complex128)
            RL = _operand(st, "L", kinds[0], b, np.complex128)[2]
            RR = _operand(st, "R", kinds[1], b, np.complex128)[1]
            PL, PR = A - RL @ Bb, A - RR @ Bb
            rhoL, rhoR = np.linalg.solve(PL, RL @ A - Bb), np.linalg.solve(PR, RR @ A - Bb)
            x = st["x"][b, t].astype(np.complex128)
            K = np.eye(n) - (rhoL * x[None, :]) @ (rhoR * x[None, :])
            conds = [float(np.linalg.cond(M)) for M in (PL, PR, K)]
            assert max(conds) <= 1e4, (N, b, t, kinds, conds)
    return ref, plain


def _ptr4(be, arrs):
    return (ctypes.c_void_p * 4)(*[be.ptr(a) for a in arrs])


class _Dev:
    """Device copies of one input set and the (kind, pointer) pairs of both operands."""

    def __init__(self, be, st, kinds):
        self.be, self.st = be, st
        self.W, self.V, self.vf, self.x = be.dev(st["W"]), be.dev(st["V"]), be.dev(st["vf"]), be.dev(st["x"])
        self.keep, self.op = [], []
        for side, kind in zip("LR", kinds):
            if kind == BD:
                d = be.dev(st[side + "bd"])
                self.keep.append(d)
                self.op.append((BD, be.ptr(d)))
            elif kind == DENSE:
                ds = [be.dev(st[side + "dn"][k]) for k in range(4)]
                arr = _ptr4(be, ds)
                self.keep += [ds, arr]
                self.op.append((DENSE, ctypes.addressof(arr)))
            else:
                self.op.append((ABSENT, None))


def _prepare(be, dv, dtype, N, batch, direction, cols, m=None, ws_short=0, lkind=None):
    n, m = 2 * N, len(cols) if m is None else m
    mm = max(m, 1)
    out = dict(rhoL=Guarded(be, batch * n * n, dtype), rhoR=Guarded(be, batch * n * n, dtype), src=Guarded(be, 2 * batch * n * mm, dtype),
               AB=Guarded(be, 2 * batch * n * n, dtype), piv=Guarded(be, batch * n, np.int32),
               info=Guarded(be, 2 * batch, np.int32, body=np.full(2 * batch, -7)))
    nws = be.lib.thickness_prepare_ws_bytes(dtcode(dtype), N, batch)
    assert nws == np.dtype(dtype).itemsize * batch * n * n
    ws = Guarded(be, nws, np.uint8)
    pc = (ctypes.c_int * max(len(cols), 1))(*cols)
    (lk, lp), (rk, rp) = dv.op
    rc = be.lib.thickness_prepare(dtcode(dtype), be.ptr(dv.W), be.ptr(dv.V), be.ptr(dv.vf), lk if lkind is None else lkind, lp, rk, rp, direction,
                                  ctypes.addressof(pc), m, N, batch, out["rhoL"].ptr(), out["rhoR"].ptr(), out["src"].ptr(), out["AB"].ptr(),
                                  out["piv"].ptr(), out["info"].ptr(), ws.ptr(), nws - ws_short, be.stream)
    be.sync()
    ws.host()
    out["piv"].host()
    return rc, out


def _columns(be, dv, dtype, prep, N, batch, T, m, direction, port, chunk=None, ws_short=0, port_arg=None):
    """trx_thickness_columns over the T axis in chunks of `chunk` (default: one call); every call has an exactly sized guarded workspace."""
    n = 2 * N
    out = Guarded(be, batch * T * n * m, dtype)
    info = Guarded(be, batch * T, np.int32, body=np.full(batch * T, -7))
    chunk = T if chunk is None else chunk
    (lk, lp), (rk, rp) = dv.op
    esz = np.dtype(dtype).itemsize
    rcs = []
    for t0 in range(0, max(T, 1), max(chunk, 1)):
        Tc = min(chunk, T - t0)
        nws = be.lib.thickness_columns_ws_bytes(dtcode(dtype), N, batch, Tc, m)
        assert nws == esz * batch * Tc * (2 * n * n + 5 * n * m)
        ws = Guarded(be, nws, np.uint8)
        piv = Guarded(be, batch * Tc * (n + 1), np.int32)
        rc = be.lib.thickness_columns(dtcode(dtype), prep["rhoL"].ptr(), prep["rhoR"].ptr(), prep["src"].ptr(), prep["AB"].ptr(),
                                      be.ptr(dv.x) + t0 * n * esz, T, Tc, direction, port if port_arg is None else port_arg, lk, lp, rk, rp, m, N, batch,
                                      out.ptr(t0 * n * m), piv.ptr(), info.ptr(t0), ws.ptr(), nws - ws_short, be.stream)
        be.sync()
        ws.host()
        piv.host()
        rcs.append(rc)
    return rcs, out.host((batch, T, n, m)), info.host().reshape(batch, T)


def _compare(got, ref, plain, block, cols, batch, T, n, dtype, what):
    ratios = []
    for b in range(batch):
        for t in range(T):
            r, p = ref[b, t][block], plain[b, t][block]
            scale = np.abs(r).max()
            e_plain = float(np.abs(p[:, cols] - r[:, cols]).max() / scale)
            err = float(np.abs(got[b, t].astype(np.complex128) - r[:, cols]).max() / scale)
            floor = max(e_plain, n * _eps(dtype))
            ratios.append(err / floor)
            print(f"{what} point {b} thickness {t}: err {err:.3e}  e_plain {e_plain:.3e}  err/max(e_plain, n eps) {err / floor:.2f}")
            assert err <= _bound(e_plain, n, dtype), (what, b, t, err, e_plain, _bound(e_plain, n, dtype))
    return max(ratios)


def _cols_for(N, m, i):
    """m = 1: a column of the lower or the upper half in turn; m = 2: one of each."""
    return [[3], [N + 2]][i % 2] if m == 1 else [[N + 1, 4], [0, 2 * N - 1]][i % 2]


def _cases():
    out = []
    for dtype in (np.complex128, np.complex64):
        for N in (9, 35):
            for i, kinds in enumerate(KINDS):
                batch, T, m = SHAPES[(i + (N == 35)) % len(SHAPES)]
                for dp in DIRPORT:
                    out.append(pytest.param(dtype, N, kinds, batch, T, m, dp, i,
                                            id=f"{np.dtype(dtype).name}-N{N}-{KNAME[kinds[0]]}-{KNAME[kinds[1]]}-b{batch}-T{T}-m{m}-d{dp[0]}p{dp[1]}"))
    return out


def _run_case(backend, dtype, N, kinds, batch, T, m, dp, i, chunk=None):
    be = get_backend(backend)
    n, dtname = 2 * N, np.dtype(dtype).name
    st = _inputs(N, batch, T, dtname)
    ref, plain = _reference(N, batch, T, dtname, kinds)
    cols = _cols_for(N, m, i)
    dv = _Dev(be, st, kinds)
    rc, prep = _prepare(be, dv, dtype, N, batch, dp[0], cols)
    assert rc == 0
    assert (prep["info"].host() == 0).all()
    rcs, got, info = _columns(be, dv, dtype, prep, N, batch, T, m, dp[0], dp[1], chunk=chunk)
    assert all(r == 0 for r in rcs), rcs
    assert (info == 0).all(), info
    for k in ("rhoL", "rhoR", "src", "AB"):                      # guard words of the prepare outputs, after the columns call read them
        prep[k].host()
    for key, arr in (("W", dv.W), ("V", dv.V), ("x", dv.x)):     # the inputs are not modified
        assert (be.host(arr) == st[key]).all()
    worst = _compare(got, ref, plain, BLOCK[dp], cols, batch, T, n, dtype, f"{KNAME[kinds[0]]}|{KNAME[kinds[1]]} d{dp[0]} p{dp[1]}")
    print(f"thickness worst err/max(e_plain, n eps) = {worst:.3f}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,kinds,batch,T,m,dp,i", _cases())
def test_thickness_columns(backend, dtype, N, kinds, batch, T, m, dp, i):
    """n = 18 and n = 70, both dtypes, every pair of operand kinds {block-diagonal, dense, absent}, both directions and ports; batch 1 - 3,
    T = 1, 3, 5 and m = 1, 2 dealt over the operand pairs (SHAPES)."""
    _run_case(backend, dtype, N, kinds, batch, T, m, dp, i)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("dp", DIRPORT)
def test_thickness_columns_long_rows(backend, dtype, dp):
    """n = 286 (N = 143), batch 2, T = 2: rows longer than one 256-thread pass of the elementwise kernels, more than four 64-lane passes of the
    skinny products; block-diagonal on the left, dense on the right."""
    if backend == "emu":
        pytest.skip("emulator: n = 286 is left to the GPU (the CPU suite stays within minutes); n = 70 runs the same kernels here")
    _run_case(backend, dtype, 143, (BD, DENSE), 2, 2, 2, dp, 0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("dp", [(0, 1), (1, 0)])
def test_thickness_columns_chunked(backend, dtype, dp):
    """T = 5 through workspaces sized for two thicknesses: three calls (2, 2, 1) with ldt = 5 and offset phase / out / info pointers."""
    _run_case(backend, dtype, 9, (DENSE, BD), 2, 5, 2, dp, 1, chunk=2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_thickness_empty_and_arguments(backend):
    """batch = 0 and T = 0 return TRX_OK and touch nothing; argument errors return TRX_ERR_ARG / TRX_ERR_WORKSPACE and touch nothing."""
    be, dtype, N, batch, T, m = get_backend(backend), np.complex128, 9, 2, 3, 2
    n = 2 * N
    st = _inputs(N, batch, T, "complex128")
    dv = _Dev(be, st, (BD, DENSE))
    cols = [1, N + 1]

    def untouched(prep):
        for k in ("rhoL", "rhoR", "src", "AB"):
            assert np.isnan(prep[k].host()).all()
        assert (prep["info"].host() == -7).all()

    rc, prep = _prepare(be, dv, dtype, N, 0, 0, cols)
    assert rc == 0
    untouched(prep)
    for kw, want in ((dict(ws_short=1), -3), (dict(cols=[n, 0]), -2), (dict(cols=[-1, 0]), -2), (dict(m=0), -2), (dict(cols=list(range(17))), -2),
                     (dict(direction=2), -2), (dict(lkind=3), -2)):
        kw = dict(dict(direction=0, cols=cols), **kw)
        rc, prep = _prepare(be, dv, dtype, N, batch, **kw)
        assert rc == want, (kw, rc)
        untouched(prep)
    dvn = _Dev(be, st, (BD, DENSE))
    dvn.op[1] = (DENSE, None)                                    # a dense operand without its pointer array
    rc, prep = _prepare(be, dvn, dtype, N, batch, 0, cols)
    assert rc == -2
    untouched(prep)

    rc, prep = _prepare(be, dv, dtype, N, batch, 0, cols)
    assert rc == 0
    for kw in (dict(T=0), dict(batch=0)):
        kw = dict(dict(batch=batch, T=T), **kw)
        rcs, got, info = _columns(be, dv, dtype, prep, N, kw["batch"], kw["T"], m, 0, 0)
        assert rcs == [0] and np.isnan(got).all() and (info == -7).all()
    for kw, want in ((dict(ws_short=1), -3), (dict(port_arg=2), -2), (dict(port_arg=-1), -2)):
        rcs, got, info = _columns(be, dv, dtype, prep, N, batch, T, m, 0, 0, **kw)
        assert rcs == [want], (kw, rcs)
        assert np.isnan(got).all() and (info == -7).all()
    rcs, got, info = _columns(be, dv, dtype, prep, N, batch, T, m, 2, 0)         # direction out of range
    assert rcs == [-2] and np.isnan(got).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_thickness_info_of_singular_K(backend, dtype):
    """W = I, V = 0 and no operand on either side: A = B = I, both reflection operators are -I exactly and K = diag(1 - x^2).  With every phase
    equal to 1 at (point 1, thickness 2) that K is exactly zero: info flags that entry alone (zero pivot at column 1), its columns are not
    finite, and every other entry's columns are correct."""
    be, N, batch, T, m = get_backend(backend), 9, 2, 3, 1
    n = 2 * N
    st = dict(_inputs(N, batch, T, np.dtype(dtype).name))
    st["W"] = np.stack([np.eye(n, dtype=dtype)] * batch)
    st["V"] = np.zeros((batch, n, n), dtype=dtype)
    st["x"] = st["x"].copy()
    st["x"][1, 2] = 1.0
    dv = _Dev(be, st, (ABSENT, ABSENT))
    rc, prep = _prepare(be, dv, dtype, N, batch, 0, [2])
    assert rc == 0 and (prep["info"].host() == 0).all()
    rcs, got, info = _columns(be, dv, dtype, prep, N, batch, T, m, 0, 0)
    assert rcs == [0]
    assert info[1, 2] == 1 and (np.delete(info.reshape(-1), 1 * T + 2) == 0).all(), info
    assert not np.isfinite(got[1, 2]).all()
    for b in range(batch):
        for t in range(T):
            if (b, t) != (1, 2):
                r = np.asarray(_stack_formulas(st, (ABSENT, ABSENT), b, t, *_arith(dtype, True))[0][0], dtype=np.complex128)
                p = np.asarray(_stack_formulas(st, (ABSENT, ABSENT), b, t, *_arith(dtype, False))[0][0], dtype=np.complex128)
                err = np.abs(got[b, t, :, 0] - r[:, 2]).max() / np.abs(r).max()
                e_plain = np.abs(p[:, 2] - r[:, 2]).max() / np.abs(r).max()
                assert err <= _bound(e_plain, n, dtype), (b, t, err, e_plain)
