"""trx_thickness_columns_keep / trx_thickness_columns_backward (include/trx.h) on the random data of tests/test_thickness_blocks.py.

Policy: the block tests' ("Block tests"; tests/test_thickness_blocks.py).
  * complex64 kernel: the reference is torch CPU complex128 autograd of L = Re <G, out>, with out restated from the stack REBUILT at every
    thickness (the layer S-matrix from the 2n x 2n definition, two full star products with explicit inverses: _stack_formulas of
    tests/test_thickness_blocks.py in torch -- no reflection operators).  That gives gradients with respect to W, V, the phase and the operand
    blocks; the kernel's gradients with respect to rho_L, rho_R, src and AB are carried to the same tensors through a complex128 torch
    restatement of the prepare step (a vector-Jacobian product, linear in what the kernel returned), its gO joins the operand block and its
    phase gradient is compared as it is.
  * complex128 kernel: the adjoint formulas of include/trx.h in numpy clongdouble with helpers.solve_hp, compared output by output.  That
    restatement is itself held to the torch-autograd reference above, on the CPU, at the project's gradient gate 1e-6 of max |ref|.
  * bound per tensor: max |got - ref| <= 16 max(e_plain, n eps(dtype)) max |ref|, e_plain = the error of the same adjoint formulas through numpy
    in the kernel's dtype; a reference that is zero throughout is met exactly.
  * <out(s, y0), G> = <s, gs> + <y0, gy0> from the kernels' own outputs (out is linear in src), summed in clongdouble, at the tolerance of
    tests/test_symmetry_grad_blocks.py: ties the adjoint to the forward kernel.
  * guards on the data, asserted per case: cond(P_L), cond(P_R) <= 10, cond(K_t) <= 185 (K^H has the condition of K), |x| <= 1.
  * every output, piv, info and the exactly sized workspace carry guard words.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, dtcode, get_backend
from tests.helpers import _bd_dense, crandn, solve_hp
from tests.test_smatrix_blocks import Guarded, _arith, _bound, _eps
from tests.test_thickness_blocks import ABSENT, BD, DENSE, DIRPORT, KINDS, KNAME, SHAPES, _Dev, _inputs, _operand, _prepare

LD = np.clongdouble
NSK = 15                                                         # skinny buffers of the backward's workspace (include/trx.h)
GRADS = ("grhoL", "grhoR", "gsrc", "gAB", "gphase", "gop")


def _out_side(dp):
    """(side, block) of the operand the forward multiplies the column with: Rgt11 or Lft22."""
    return ("R", 0) if (dp[0] == 0) != (dp[1] == 1) else ("L", 3)


@functools.lru_cache(maxsize=None)
def _cotangent(N, batch, T, m, dtname):
    rng = np.random.default_rng([41077, N, batch, T, m])
    return crandn(rng, (batch, T, 2 * N, m)).astype(np.dtype(dtname).type)


# ---- the adjoint formulas of include/trx.h in numpy ------------------------------------------------------------------------------------------
def _adjoint_formulas(rhoL, rhoR, src, AB, x, O, G, dp, wd, solve):
    """Forward and adjoint of one point over its T thicknesses in the working dtype `wd`.  rhoL, rhoR [n,n]; src [2,n,m]; AB [2,n,n];
    x [T,n]; O [n,n] or None; G [T,n,m].  Returns out, cp [T,n,m] and the gradients (gop dense)."""
    c = lambda a: np.asarray(a).astype(wd)
    rhoL, rhoR, src, AB, x, G = c(rhoL), c(rhoR), c(src), c(AB), c(x), c(G)
    O = None if O is None else c(O)
    H = lambda a: a.conj().T
    direction, port = dp
    rA, rB = (rhoR, rhoL) if direction else (rhoL, rhoR)
    A, Bm, s, y0 = AB[0], AB[1], src[0], src[1]
    n, T = A.shape[0], x.shape[0]
    I = np.eye(n, dtype=wd)
    z = lambda a: np.zeros_like(a)
    res = dict(out=[], cp=[], grA=z(A), grB=z(A), gs=z(s), gy0=z(s), gA=z(A), gB=z(A), gx=[], gop=None if O is None else z(A))
    for t in range(T):
        xt, xc = x[t][:, None], x[t].conj()[:, None]
        K = I - rA @ (xt * rB * x[t][None, :])
        cp = solve(K, s)
        u = xt * cp
        cs = rB @ u
        w = xt * cs
        g = (A @ u + Bm @ cs) / 2 if port == 0 else (Bm @ cp + A @ w) / 2
        out = g if O is None else O @ g
        res["out"].append(out + y0 if port == 1 else out)
        res["cp"].append(cp)
        Gt = G[t]
        gb = Gt if O is None else H(O) @ Gt
        if O is not None:
            res["gop"] += Gt @ H(g)
        if port == 0:
            ub, csb, cpb, gx = H(A) @ gb / 2, H(Bm) @ gb / 2, 0, 0
            res["gA"] += gb @ H(u) / 2
            res["gB"] += gb @ H(cs) / 2
        else:
            res["gy0"] += Gt
            cpb, wb = H(Bm) @ gb / 2, H(A) @ gb / 2
            res["gB"] += gb @ H(cp) / 2
            res["gA"] += gb @ H(w) / 2
            csb, gx, ub = xc * wb, (wb * cs.conj()).sum(1), 0
        res["grB"] += csb @ H(u)
        ub = ub + H(rB) @ csb
        gx = gx + (ub * cp.conj()).sum(1)
        cpb = cpb + xc * ub
        lam = solve(H(K), cpb)
        res["gs"] += lam
        res["grA"] += lam @ H(w)
        mu = H(rA) @ lam
        nu = xc * mu
        res["grB"] += nu @ H(u)
        res["gx"].append(gx + (mu * cs.conj()).sum(1) + (cp.conj() * (H(rB) @ nu)).sum(1))
    gL, gR = (res["grB"], res["grA"]) if direction else (res["grA"], res["grB"])
    return dict(out=np.stack(res["out"]), cp=np.stack(res["cp"]), grhoL=gL, grhoR=gR, gsrc=np.stack([res["gs"], res["gy0"]]),
                gAB=np.stack([res["gA"], res["gB"]]), gphase=np.stack(res["gx"]), gop=res["gop"])


def _bd_diags(M):
    """The four diagonals [4,N] of the blocks of a dense 2N x 2N matrix, in the order of a block-diagonal operand."""
    N = M.shape[0] // 2
    return np.stack([np.diagonal(M[r * N:(r + 1) * N, c * N:(c + 1) * N]) for r in (0, 1) for c in (0, 1)])


def _formulas_all(st, prep_h, kinds, G, dp, hp, dtype, batch):
    """_adjoint_formulas over the points, in the kernel's layouts: hp -> the high-precision arithmetic of a kernel of `dtype`."""
    wd, solve = _arith(dtype, hp)
    side, blk = _out_side(dp)
    kind = kinds[0] if side == "L" else kinds[1]
    per = []
    for b in range(batch):
        O = None if kind == ABSENT else _operand(st, side, kind, b, wd)[blk]
        r = _adjoint_formulas(prep_h["rhoL"][b], prep_h["rhoR"][b], prep_h["src"][:, b], prep_h["AB"][:, b], st["x"][b], O, G[b], dp, wd, solve)
        if kind == BD:
            r["gop"] = _bd_diags(r["gop"])
        per.append(r)
    out = {k: np.stack([p[k] for p in per]) for k in ("out", "cp", "grhoL", "grhoR", "gphase")}
    out["gsrc"], out["gAB"] = np.stack([p["gsrc"] for p in per], axis=1), np.stack([p["gAB"] for p in per], axis=1)
    out["gop"] = None if kind == ABSENT else np.stack([p["gop"] for p in per], axis=1 if kind == BD else 0)
    return out


# ---- the torch-autograd reference: the stack rebuilt at every thickness, and the prepare step ------------------------------------------------
def _leaf_ops(st, kinds, b):
    """Leaves and dense blocks of both operands of point b in torch complex128: ([leaf or None] * 2, [four blocks] * 2)."""
    n = st["W"].shape[1]
    N = n // 2
    leaves, blocks = [], []
    for side, kind in zip("LR", kinds):
        if kind == ABSENT:
            I, Z = torch.eye(n, dtype=torch.complex128), torch.zeros((n, n), dtype=torch.complex128)
            leaves.append(None)
            blocks.append([I, Z, Z, I])
        elif kind == BD:
            lf = torch.from_numpy(st[side + "bd"][:, :, b].astype(np.complex128)).requires_grad_(True)       # [4 blocks, 4 diagonals, N]
            leaves.append(lf)
            blocks.append([torch.cat((torch.cat((torch.diag(lf[k, 0]), torch.diag(lf[k, 1])), 1),
                                      torch.cat((torch.diag(lf[k, 2]), torch.diag(lf[k, 3])), 1)), 0) for k in range(4)])
        else:
            lf = torch.from_numpy(st[side + "dn"][:, b].astype(np.complex128)).requires_grad_(True)          # [4, n, n]
            leaves.append(lf)
            blocks.append([lf[k] for k in range(4)])
    return leaves, blocks


def _modes_torch(W, V, vf):
    N = W.shape[0] // 2
    F = torch.cat((vf[0][:, None] * V[:N] + vf[1][:, None] * V[N:], vf[2][:, None] * V[:N] + vf[3][:, None] * V[N:]))
    return W + F, W - F


def _star_torch(Sm, Sn):
    I = torch.eye(Sm[0].shape[0], dtype=Sm[0].dtype)
    t1, t2 = torch.linalg.inv(I - Sm[2] @ Sn[1]), torch.linalg.inv(I - Sn[1] @ Sm[2])
    return [Sn[0] @ t1 @ Sm[0], Sm[1] + Sm[3] @ t2 @ Sn[1] @ Sm[0], Sn[2] + Sn[0] @ t1 @ Sm[2] @ Sn[3], Sm[3] @ t2 @ Sn[3]]


def _stack_torch(W, V, vf, x, Lb, Rb):
    """tests/test_thickness_blocks.py::_stack_formulas in torch: the four blocks of Lft * layer(x) * Rgt."""
    n = W.shape[0]
    I, Z = torch.eye(n, dtype=W.dtype), torch.zeros((n, n), dtype=W.dtype)
    A, B0 = _modes_torch(W, V, vf)
    Bm = B0 * x[None, :]
    c = torch.linalg.solve(torch.cat((torch.cat((A, Bm), 1), torch.cat((Bm, A), 1)), 0), torch.cat((2 * I, Z), 0))
    cp, cm = c[:n], c[n:]
    WX = W * x[None, :]
    S11, S21 = WX @ cp + W @ cm, W @ cp + WX @ cm - I
    return _star_torch(_star_torch(Lb, [S11, S21, S21, S11]), Rb)


def _prepare_torch(W, V, vf, Lb, Rb, direction, cols):
    """(rhoL, rhoR, s, y0, A, B): the formulas of trx_thickness_prepare in torch."""
    A, Bm = _modes_torch(W, V, vf)
    rho = []
    for side, R in enumerate((Lb[2], Rb[1])):
        P = A - R @ Bm
        rho.append(torch.linalg.solve(P, R @ A - Bm))
        if side == direction:
            Tm, Cm = (Rb[3], Rb[2]) if side else (Lb[0], Lb[1])
            s, y0 = torch.linalg.solve(P, 2 * Tm[:, cols]), Cm[:, cols]
    return rho[0], rho[1], s, y0, A, Bm


def _point_leaves(st, kinds, b):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.complex128)).requires_grad_(True)
    W, V, x = t(st["W"][b]), t(st["V"][b]), t(st["x"][b])
    vf = torch.from_numpy(st["vf"][:, b].astype(np.complex128))
    ops, blocks = _leaf_ops(st, kinds, b)
    return W, V, vf, x, ops, blocks


def _np(g, like):
    return np.zeros(tuple(like.shape), dtype=np.complex128) if g is None else g.detach().numpy()


def _autograd_reference(st, kinds, G, dp, cols, batch, block):
    """Per point: dict(W, V, x, L, R) of d Re <G, out> / d conj(.), out = the columns `cols` of `block` of the rebuilt stack."""
    refs = []
    for b in range(batch):
        W, V, vf, x, ops, blocks = _point_leaves(st, kinds, b)
        Gb = torch.from_numpy(G[b].astype(np.complex128))
        loss = 0
        for t in range(x.shape[0]):
            out = _stack_torch(W, V, vf, x[t], blocks[0], blocks[1])[block][:, cols]
            loss = loss + torch.real(torch.sum(torch.conj(Gb[t]) * out))
        leaves = [W, V, x] + [o for o in ops if o is not None]
        gr = list(torch.autograd.grad(loss, leaves, allow_unused=True))
        r = dict(W=_np(gr[0], W), V=_np(gr[1], V), x=_np(gr[2], x))
        rest = gr[3:]
        for side, o in zip("LR", ops):
            r[side] = None if o is None else _np(rest.pop(0), o)
        refs.append(r)
    return refs


def _chain(st, kinds, res, dp, cols, batch):
    """The gradients `res` of the columns step (kernel or formulas) carried to the tensors of _autograd_reference through the prepare step."""
    side, blk = _out_side(dp)
    outs = []
    for b in range(batch):
        W, V, vf, x, ops, blocks = _point_leaves(st, kinds, b)
        prep = _prepare_torch(W, V, vf, blocks[0], blocks[1], dp[0], cols)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.complex128)))
        cot = [t(res["grhoL"][b]), t(res["grhoR"][b]), t(res["gsrc"][0, b]), t(res["gsrc"][1, b]), t(res["gAB"][0, b]), t(res["gAB"][1, b])]
        leaves = [W, V] + [o for o in ops if o is not None]
        live = [(p, c) for p, c in zip(prep, cot) if p.requires_grad]
        gr = list(torch.autograd.grad([p for p, _ in live], leaves, grad_outputs=[c for _, c in live], allow_unused=True))
        r = dict(W=_np(gr[0], W), V=_np(gr[1], V), x=np.asarray(res["gphase"][b]).astype(np.complex128))
        rest = gr[2:]
        for s_, o in zip("LR", ops):
            r[s_] = None if o is None else _np(rest.pop(0), o).copy()
        if r[side] is not None:
            gop = np.asarray(res["gop"]).astype(np.complex128)
            r[side][blk] += gop[:, b] if (kinds[0] if side == "L" else kinds[1]) == BD else gop[b]
        outs.append(r)
    return outs


# ---- running the kernels ---------------------------------------------------------------------------------------------------------------------
def _pad_t(a, ldt):
    """[B, T, ...] -> [B, ldt, ...], NaN behind T."""
    if ldt == a.shape[1]:
        return a
    out = np.full((a.shape[0], ldt) + a.shape[2:], np.nan, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _keep(be, dv, dtype, prep, N, batch, T, m, dp, ldt=None, plain=False, want_cp=True):
    """trx_thickness_columns_keep (plain: trx_thickness_columns) in one call: (rc, out [B,T,n,m], cp [B,T,n,m])."""
    n, ldt = 2 * N, T if ldt is None else ldt
    x = be.dev(_pad_t(dv.st["x"], ldt))
    out, cp = Guarded(be, batch * ldt * n * m, dtype), Guarded(be, batch * ldt * n * m, dtype)
    info = Guarded(be, batch * ldt, np.int32, body=np.full(batch * ldt, -7))
    nws = be.lib.thickness_columns_ws_bytes(dtcode(dtype), N, batch, T, m)
    ws, piv = Guarded(be, nws, np.uint8), Guarded(be, batch * T * (n + 1), np.int32)
    (lk, lp), (rk, rp) = dv.op
    head = (dtcode(dtype), prep["rhoL"].ptr(), prep["rhoR"].ptr(), prep["src"].ptr(), prep["AB"].ptr(), be.ptr(x), ldt, T, dp[0], dp[1], lk, lp, rk, rp,
            m, N, batch, out.ptr())
    tail = (piv.ptr(), info.ptr(), ws.ptr(), nws, be.stream)
    rc = be.lib.thickness_columns(*head, *tail) if plain else be.lib.thickness_columns_keep(*head, cp.ptr() if want_cp else None, *tail)
    be.sync()
    ws.host()
    piv.host()
    return rc, out.host((batch, ldt, n, m))[:, :T], cp.host((batch, ldt, n, m))[:, :T], info.host().reshape(batch, ldt)[:, :T]


def _gop_count(kinds, dp, batch, N):
    side, _ = _out_side(dp)
    kind = kinds[0] if side == "L" else kinds[1]
    return {ABSENT: 0, BD: 4 * batch * N, DENSE: batch * 4 * N * N}[kind], kind


def _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, ldt=None, chunks=None, null=(), ws_short=0, bufs=None, **over):
    """trx_thickness_columns_backward over the T axis in the chunks [(t0, Tc), ...] (default: one call; the first chunk writes, the later ones
    accumulate).  null: names of GRADS passed as null pointers.  Returns (rcs, {name: host array or None}, info, buffers)."""
    n, ldt = 2 * N, T if ldt is None else ldt
    esz = np.dtype(dtype).itemsize
    x, cpd, Gd = be.dev(_pad_t(dv.st["x"], ldt)), be.dev(_pad_t(cp, ldt)), be.dev(_pad_t(G, ldt))
    ngop, okind = _gop_count(kinds, dp, batch, N)
    counts = dict(grhoL=batch * n * n, grhoR=batch * n * n, gsrc=2 * batch * n * m, gAB=2 * batch * n * n, gphase=batch * ldt * n, gop=ngop)
    if bufs is None:
        bufs = {k: Guarded(be, c, dtype) for k, c in counts.items()}
        bufs["info"] = Guarded(be, batch * ldt, np.int32, body=np.full(batch * ldt, -7))
    (lk, lp), (rk, rp) = dv.op
    rcs = []
    for j, (t0, Tc) in enumerate(chunks or [(0, T)]):
        nws = be.lib.thickness_columns_backward_ws_bytes(dtcode(dtype), N, batch, Tc, m)
        assert nws == esz * batch * Tc * (2 * n * n + NSK * n * m)
        ws, piv = Guarded(be, nws, np.uint8), Guarded(be, batch * Tc * (n + 1), np.int32)
        p = lambda k, off=0: None if (k in null or counts[k] == 0) else bufs[k].ptr(off)
        args = dict(direction=dp[0], port=dp[1], lk=lk, rk=rk, m=m, acc=int(j > 0), T=Tc, ldt=ldt)
        args.update({k[2:]: v for k, v in over.items()})         # a_<name>: the argument as passed, whatever the buffers were sized for
        rc = be.lib.thickness_columns_backward(dtcode(dtype), prep["rhoL"].ptr(), prep["rhoR"].ptr(), prep["AB"].ptr(), be.ptr(x) + t0 * n * esz,
                                               args["ldt"], args["T"], args["direction"], args["port"], args["lk"], lp, args["rk"], rp, args["m"], N,
                                               batch, be.ptr(cpd) + t0 * n * m * esz, be.ptr(Gd) + t0 * n * m * esz, p("grhoL"), p("grhoR"), p("gsrc"),
                                               p("gAB"), p("gphase", t0 * n), p("gop"), args["acc"], piv.ptr(), bufs["info"].ptr(t0), ws.ptr(),
                                               nws - ws_short, be.stream)
        be.sync()
        ws.host()
        piv.host()
        rcs.append(rc)
    shapes = dict(grhoL=(batch, n, n), grhoR=(batch, n, n), gsrc=(2, batch, n, m), gAB=(2, batch, n, n), gphase=(batch, ldt, n),
                  gop=(4, batch, N) if okind == BD else (batch, n, n))
    res = {k: (bufs[k].host(shapes[k]) if counts[k] else None) for k in GRADS}
    if res["gphase"] is not None:
        res["gphase"] = res["gphase"][:, :T]
    return rcs, res, bufs["info"].host().reshape(batch, ldt)[:, :T], bufs


def _guards(st, prep_h, kinds, batch, T, dtype):
    """cond(P_L), cond(P_R) <= 10, cond(K_t) <= 185 and |x| <= 1 for the data of this case (complex128; K^H has the condition of K)."""
    n = st["W"].shape[1]
    assert (np.abs(st["x"]) <= 1.0 + 4 * _eps(dtype)).all()
    for b in range(batch):
        A, Bm = prep_h["AB"][0, b].astype(np.complex128), prep_h["AB"][1, b].astype(np.complex128)
        rL, rR = prep_h["rhoL"][b].astype(np.complex128), prep_h["rhoR"][b].astype(np.complex128)
        for R in (_operand(st, "L", kinds[0], b, np.complex128)[2], _operand(st, "R", kinds[1], b, np.complex128)[1]):
            c = float(np.linalg.cond(A - R @ Bm))
            assert c <= 10.0, (b, c)
        for t in range(T):
            x = st["x"][b, t].astype(np.complex128)
            c = float(np.linalg.cond(np.eye(n) - (rL * x[None, :]) @ (rR * x[None, :])))
            assert c <= 185.0, (b, t, c)


def _cmp(name, got, ref, plain, n, dtype):
    """One tensor against its reference at the block-test bound; returns err / max(e_plain, n eps)."""
    ref = np.asarray(ref).astype(np.complex128)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    got = np.asarray(got).astype(np.complex128)
    if scale == 0.0:
        assert not np.abs(got).any(), f"{name}: the reference is zero throughout, got max |.| = {np.abs(got).max():.3e}"
        return 0.0
    e_plain = float(np.abs(np.asarray(plain).astype(np.complex128) - ref).max() / scale)
    err = float(np.abs(got - ref).max() / scale)
    floor = max(e_plain, n * _eps(dtype))
    print(f"  {name}: err {err:.3e}  e_plain {e_plain:.3e}  err/max(e_plain, n eps) {err / floor:.2f}")
    assert err <= _bound(e_plain, n, dtype), (name, err, e_plain, _bound(e_plain, n, dtype))
    return err / floor


def _dot(a, b):
    return complex(np.sum(np.conj(np.asarray(a).astype(LD)) * np.asarray(b).astype(LD)))


def _cols_for(N, m, i):
    if m > 2:
        return [(5 * q + i) % (2 * N) for q in range(m)]
    return [[3], [N + 2]][i % 2] if m == 1 else [[N + 1, 4], [0, 2 * N - 1]][i % 2]


def _run_case(backend, dtype, N, kinds, batch, T, m, dp, i):
    be = get_backend(backend)
    n, dtname = 2 * N, np.dtype(dtype).name
    st = _inputs(N, batch, T, dtname)
    cols = _cols_for(N, m, i)
    G = _cotangent(N, batch, T, m, dtname)
    dv = _Dev(be, st, kinds)
    rc, prep = _prepare(be, dv, dtype, N, batch, dp[0], cols)
    assert rc == 0 and (prep["info"].host() == 0).all()
    prep_h = dict(rhoL=prep["rhoL"].host((batch, n, n)), rhoR=prep["rhoR"].host((batch, n, n)), src=prep["src"].host((2, batch, n, m)),
                  AB=prep["AB"].host((2, batch, n, n)))
    _guards(st, prep_h, kinds, batch, T, dtype)
    rc, out, cp, info = _keep(be, dv, dtype, prep, N, batch, T, m, dp)
    assert rc == 0 and (info == 0).all()
    rcs, got, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp)
    assert rcs == [0] and (info == 0).all(), (rcs, info)
    for k in ("rhoL", "rhoR", "src", "AB"):                      # the inputs keep their guard words and their values
        assert np.array_equal(prep[k].host().reshape(prep_h[k].shape), prep_h[k], equal_nan=True)
    ref = _formulas_all(st, prep_h, kinds, G, dp, True, dtype, batch)
    plain = _formulas_all(st, prep_h, kinds, G, dp, False, dtype, batch)
    what = f"{KNAME[kinds[0]]}|{KNAME[kinds[1]]} d{dp[0]} p{dp[1]} {dtname} n={n} b{batch} T{T} m{m}"
    print(what)
    worst = [_cmp("cp", cp, ref["cp"], plain["cp"], n, dtype)]
    if dtype == np.complex128:
        for k in GRADS:
            if ref[k] is not None:
                worst.append(_cmp(k, got[k], ref[k], plain[k], n, dtype))
    else:
        block = {(0, 0): 0, (0, 1): 1, (1, 1): 2, (1, 0): 3}[dp]
        aref = _autograd_reference(st, kinds, G, dp, cols, batch, block)
        cg, cpl = _chain(st, kinds, got, dp, cols, batch), _chain(st, kinds, plain, dp, cols, batch)
        for b in range(batch):
            for k in ("W", "V", "x", "L", "R"):
                if aref[b][k] is not None:
                    worst.append(_cmp(f"point {b} d/d{k}", cg[b][k], aref[b][k], cpl[b][k], n, dtype))
    # out is linear in (s, y0): <G, out> = <gs, s> + <gy0, y0> from the kernels' own outputs
    lhs = _dot(G, out)
    rhs = _dot(got["gsrc"][0], prep_h["src"][0]) + _dot(got["gsrc"][1], prep_h["src"][1])
    tol = 16 * n * _eps(dtype) * (float(np.abs(out).max()) * float(np.abs(G).sum()) + float(np.abs(got["gsrc"][0]).max()) * float(np.abs(prep_h["src"][0]).sum())
                                  + float(np.abs(got["gsrc"][1]).max()) * float(np.abs(prep_h["src"][1]).sum()))
    print(f"  <G, out> = {lhs:.6g}, <gsrc, src> = {rhs:.6g}, |difference| {abs(lhs - rhs):.2e}, bound {tol:.2e}")
    assert abs(lhs - rhs) <= tol
    print(f"thickness backward worst err/max(e_plain, n eps) = {max(worst):.3f}")


def _cases():
    out = []
    for dtype in (np.complex128, np.complex64):
        for i, kinds in enumerate(KINDS):
            batch, T, m = SHAPES[i % len(SHAPES)]
            for dp in DIRPORT:
                out.append(pytest.param(dtype, 6, kinds, batch, T, m, dp, i,
                                        id=f"{np.dtype(dtype).name}-N6-{KNAME[kinds[0]]}-{KNAME[kinds[1]]}-b{batch}-T{T}-m{m}-d{dp[0]}p{dp[1]}"))
        for i, kinds in enumerate(KINDS):                        # n = 70: ragged against 64 lanes; one (direction, port) per pair of kinds, in turn
            batch, T, m = SHAPES[(i + 1) % len(SHAPES)]
            dp = DIRPORT[i % 4]
            out.append(pytest.param(dtype, 35, kinds, batch, T, m, dp, i,
                                    id=f"{np.dtype(dtype).name}-N35-{KNAME[kinds[0]]}-{KNAME[kinds[1]]}-b{batch}-T{T}-m{m}-d{dp[0]}p{dp[1]}"))
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,N,kinds,batch,T,m,dp,i", _cases())
def test_thickness_columns_backward(backend, dtype, N, kinds, batch, T, m, dp, i):
    """n = 12: every pair of operand kinds x every (direction, port); T m = 6 and 10 leave a partial tile of the skinny products.  n = 70 once
    per pair of kinds."""
    _run_case(backend, dtype, N, kinds, batch, T, m, dp, i)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_thickness_columns_backward_sixteen_columns(backend, dtype):
    """m = 16, the column limit: two full tiles of (thickness, column) pairs per thickness."""
    _run_case(backend, dtype, 6, (DENSE, BD), 1, 3, 16, (0, 1), 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_thickness_columns_backward_long_rows(backend, dtype):
    """n = 286 (N = 143): rows longer than one 256-thread pass of the row-parallel kernels."""
    if backend == "emu":
        pytest.skip("emulator: n = 286 is left to the GPU (the CPU suite stays within minutes); n = 70 runs the same kernels here")
    _run_case(backend, dtype, 143, (BD, DENSE), 1, 2, 2, (0, 0) if dtype == np.complex128 else (1, 1), 0)


def _setup(backend, dtype, N, kinds, batch, T, m, dp, i=0):
    be = get_backend(backend)
    n = 2 * N
    st = _inputs(N, batch, T, np.dtype(dtype).name)
    dv = _Dev(be, st, kinds)
    rc, prep = _prepare(be, dv, dtype, N, batch, dp[0], _cols_for(N, m, i))
    assert rc == 0
    prep_h = dict(rhoL=prep["rhoL"].host((batch, n, n)), rhoR=prep["rhoR"].host((batch, n, n)), src=prep["src"].host((2, batch, n, m)),
                  AB=prep["AB"].host((2, batch, n, n)))
    rc, out, cp, info = _keep(be, dv, dtype, prep, N, batch, T, m, dp)
    assert rc == 0 and (info == 0).all()
    return be, st, dv, prep, prep_h, out, cp, _cotangent(N, batch, T, m, np.dtype(dtype).name)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("kinds,dp", [((DENSE, BD), (0, 1)), ((BD, DENSE), (0, 0)), ((DENSE, ABSENT), (1, 0))])
def test_thickness_columns_backward_ldt_and_chunks(backend, dtype, kinds, dp):
    """T = 5 inside arrays of ldt = 7; and the chunks (3, 2) with accumulate against the one call: every output within the bound of the
    one-call reference, the phase gradient (never accumulated) bit-equal."""
    N, batch, T, m = 6, 2, 5, 2
    be, st, dv, prep, prep_h, out, cp, G = _setup(backend, dtype, N, kinds, batch, T, m, dp)
    n = 2 * N
    rcs, one, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp)
    assert rcs == [0] and (info == 0).all()
    rc, out7, cp7, _ = _keep(be, dv, dtype, prep, N, batch, T, m, dp, ldt=7)
    assert rc == 0 and np.array_equal(out7, out) and np.array_equal(cp7, cp)
    rcs, wide, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, ldt=7)
    assert rcs == [0] and (info == 0).all()
    for k in GRADS:
        assert (one[k] is None and wide[k] is None) or np.array_equal(one[k], wide[k]), k
    rcs, two, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, ldt=7, chunks=[(0, 3), (3, 2)])
    assert rcs == [0, 0] and (info == 0).all()
    assert np.array_equal(two["gphase"], one["gphase"])
    ref = _formulas_all(st, prep_h, kinds, G, dp, True, dtype, batch)
    plain = _formulas_all(st, prep_h, kinds, G, dp, False, dtype, batch)
    for k in GRADS:                                              # two chunks against the one call, at the bound of the formulas' own error
        if one[k] is None:
            continue
        scale = float(np.abs(one[k]).max())
        e_plain = float(np.abs(np.asarray(plain[k]).astype(np.complex128) - np.asarray(ref[k]).astype(np.complex128)).max() / np.abs(ref[k]).max())
        err = float(np.abs(two[k].astype(np.complex128) - one[k].astype(np.complex128)).max() / scale)
        print(f"  {k}: two chunks - one call {err:.3e}, e_plain {e_plain:.3e}")
        assert err <= _bound(e_plain, n, dtype), (k, err, e_plain)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("kinds,dp", [((BD, DENSE), (0, 0)), ((DENSE, BD), (0, 1)), ((BD, ABSENT), (1, 1))])
def test_thickness_columns_backward_null_pointers_and_repeat(backend, dtype, kinds, dp):
    """A repeated call is bit-equal; each gradient pointer null in turn leaves the other outputs bit-equal and its own buffer untouched; all
    null writes nothing at all, info and piv included."""
    N, batch, T, m = 6, 2, 3, 2
    be, st, dv, prep, prep_h, out, cp, G = _setup(backend, dtype, N, kinds, batch, T, m, dp)
    rcs, one, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp)
    rcs2, again, _, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp)
    assert rcs == [0] and rcs2 == [0]
    for k in GRADS:
        assert (one[k] is None and again[k] is None) or np.array_equal(one[k], again[k]), k
    for skip in GRADS:
        if one[skip] is None:
            continue
        rcs, got, _, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, null=(skip,))
        assert rcs == [0]
        assert np.isnan(got[skip]).all(), skip
        for k in GRADS:
            if k != skip and one[k] is not None:
                assert np.array_equal(one[k], got[k]), (skip, k)
    rcs, got, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, null=GRADS)
    assert rcs == [0] and (info == -7).all()
    assert all(v is None or np.isnan(v).all() for v in got.values())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_thickness_columns_keep_matches_columns(backend, dtype):
    """trx_thickness_columns_keep returns the bits of trx_thickness_columns; both leave their guard words."""
    N, batch, T, m = 6, 3, 3, 2
    for kinds, dp in (((BD, DENSE), (0, 0)), ((DENSE, BD), (1, 1)), ((ABSENT, ABSENT), (0, 1))):
        be, st, dv, prep, prep_h, out, cp, G = _setup(backend, dtype, N, kinds, batch, T, m, dp)
        rc, plain_out, untouched, info = _keep(be, dv, dtype, prep, N, batch, T, m, dp, plain=True)
        assert rc == 0 and (info == 0).all()
        assert np.array_equal(plain_out, out) and np.isnan(untouched).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_thickness_columns_backward_arguments(backend):
    """batch = 0 and T = 0 return TRX_OK and touch nothing; malformed arguments return TRX_ERR_ARG / TRX_ERR_WORKSPACE and touch nothing."""
    dtype, N, batch, T, m, kinds, dp = np.complex128, 6, 2, 3, 2, (BD, DENSE), (0, 0)
    be, st, dv, prep, prep_h, out, cp, G = _setup(backend, dtype, N, kinds, batch, T, m, dp)

    def untouched(got, info):
        assert all(v is None or np.isnan(v).all() for v in got.values()) and (info == -7).all()

    for kw, want in ((dict(ws_short=1), -3), (dict(a_port=2), -2), (dict(a_port=-1), -2), (dict(a_direction=2), -2), (dict(a_m=0), -2),
                     (dict(a_m=17), -2), (dict(a_acc=2), -2), (dict(a_lk=3), -2), (dict(a_ldt=T - 1), -2), (dict(a_T=-1), -2)):
        rcs, got, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, **kw)
        assert rcs == [want], (kw, rcs)
        untouched(got, info)
    rcs, got, info, _ = _backward(be, dv, dtype, prep, cp, G, kinds, N, batch, T, m, dp, a_T=0)
    assert rcs == [0]
    untouched(got, info)
    dvn = _Dev(be, st, kinds)
    dvn.op[1] = (DENSE, None)                                    # a dense operand without its pointer array
    rcs, got, info, _ = _backward(be, dvn, dtype, prep, cp, G, kinds, N, batch, T, m, dp)
    assert rcs == [-2]
    untouched(got, info)
    rc, o, c, info = _keep(be, dv, dtype, prep, N, batch, T, m, dp, want_cp=False)      # keep without its cp pointer
    assert rc == -2 and np.isnan(o).all() and (info == -7).all()
    # batch = 0
    nws = be.lib.thickness_columns_backward_ws_bytes(dtcode(dtype), N, 0, T, m)
    assert nws == 0
    rc = be.lib.thickness_columns_backward(dtcode(dtype), None, None, None, None, T, T, 0, 0, 0, None, 0, None, m, N, 0, None, None, None, None, None, None,
                                           None, None, 0, None, None, None, 0, be.stream)
    assert rc == 0


# ---- the high-precision restatement against autograd (CPU only) ------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,dp,shape", [((BD, DENSE), (0, 0), (2, 3, 2)), ((DENSE, BD), (0, 1), (1, 5, 1)), ((DENSE, DENSE), (1, 1), (2, 3, 2)),
                                            ((ABSENT, BD), (1, 0), (1, 3, 2)), ((BD, ABSENT), (0, 1), (3, 1, 2))])
def test_adjoint_formulas_against_autograd(kinds, dp, shape):
    """The clongdouble adjoint formulas (the reference of the complex128 kernels), fed with the prepare step in complex128 and carried through
    it, against torch autograd of the rebuilt stack: the project's gradient gate, 1e-6 of max |ref| per tensor."""
    N, (batch, T, m) = 6, shape
    n = 2 * N
    st = _inputs(N, batch, T, "complex128")
    cols = _cols_for(N, m, 1)
    G = _cotangent(N, batch, T, m, "complex128")
    prep_h = dict(rhoL=[], rhoR=[], s=[], y0=[], A=[], B=[])
    for b in range(batch):
        W, V, vf, x, ops, blocks = _point_leaves(st, kinds, b)
        for k, v in zip(prep_h, _prepare_torch(W, V, vf, blocks[0], blocks[1], dp[0], cols)):
            prep_h[k].append(v.detach().numpy())
    prep_h = dict(rhoL=np.stack(prep_h["rhoL"]), rhoR=np.stack(prep_h["rhoR"]), src=np.stack([np.stack(prep_h["s"]), np.stack(prep_h["y0"])]),
                  AB=np.stack([np.stack(prep_h["A"]), np.stack(prep_h["B"])]))
    res = _formulas_all(st, prep_h, kinds, G, dp, True, np.complex128, batch)
    block = {(0, 0): 0, (0, 1): 1, (1, 1): 2, (1, 0): 3}[dp]
    aref = _autograd_reference(st, kinds, G, dp, cols, batch, block)
    mine = _chain(st, kinds, res, dp, cols, batch)
    for b in range(batch):
        for t in range(T):                                       # the forward of the formulas is the rebuilt stack's column
            W, V, vf, x, ops, blocks = _point_leaves(st, kinds, b)
            want = _stack_torch(W, V, vf, x[t], blocks[0], blocks[1])[block][:, cols].detach().numpy()
            assert np.abs(res["out"][b, t].astype(np.complex128) - want).max() <= 1e-9 * np.abs(want).max()
        for k in ("W", "V", "x", "L", "R"):
            if aref[b][k] is None:
                continue
            scale = np.abs(aref[b][k]).max()
            err = np.abs(mine[b][k] - aref[b][k]).max()
            print(f"point {b} d/d{k}: {err / scale if scale else err:.2e}")
            assert err <= 1e-6 * scale, (b, k, err, scale)
