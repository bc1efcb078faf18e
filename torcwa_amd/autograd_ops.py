"""torch.autograd.Function wrappers around the libtrx primitives (forward AND backward run on the HIP kernels).

Used by the differentiable path of `BatchedRCWA` (Examples 4-6 of the reference: gradients w.r.t. permittivity grids,
thickness, ...).  PyTorch's complex-autograd convention applies: for C = f(A) holomorphic, grad_A = conj(f') applied to
grad_C, i.e. for C = A B: grad_A = grad_C B^H, grad_B = A^H grad_C.
"""
import math

import torch


class ConvMatFn(torch.autograd.Function):
    """E = convmat(grid) (torcwa/rcwa.py:1183-1204).  Linear in the grid; the backward is its adjoint: Toeplitz-diagonal
    sums of grad_E followed by the conjugate (inverse-direction) pruned DFT."""

    @staticmethod
    def forward(ctx, grid, ox, oy, cdtype, engine):
        ctx.meta = (ox, oy, grid.shape, grid.is_complex(), grid.dtype)
        return engine.convmat(grid, ox, oy, cdtype)

    @staticmethod
    def backward(ctx, gE):
        ox, oy, (B, nx, ny), cplx, gdt = ctx.meta
        dev = gE.device
        wy = 2 * oy + 1
        N = (2 * ox + 1) * wy
        idx = torch.arange(N, device=dev)
        m, n_ = idx // wy, idx % wy
        dm = (m[:, None] - m[None, :] + 2 * ox).reshape(-1)
        dn = (n_[:, None] - n_[None, :] + 2 * oy).reshape(-1)
        nq = 4 * oy + 1
        G = torch.zeros((B, (4 * ox + 1) * nq), dtype=gE.dtype, device=dev)
        G.index_add_(1, dm * nq + dn, gE.reshape(B, -1))                    # G[p,q] = sum_{(i,j): diff = (p,q)} gE[i,j]
        G = G.reshape(B, 4 * ox + 1, nq)
        rdt = torch.float64 if gE.dtype == torch.complex128 else torch.float32
        x = torch.arange(nx, device=dev, dtype=rdt)[:, None]
        p = torch.arange(-2 * ox, 2 * ox + 1, device=dev, dtype=rdt)[None, :]
        y = torch.arange(ny, device=dev, dtype=rdt)[None, :]
        q = torch.arange(-2 * oy, 2 * oy + 1, device=dev, dtype=rdt)[:, None]
        Fx = torch.exp(2j * math.pi * (x * p) / nx).to(gE.dtype)             # conj of the forward twiddle
        Fy = torch.exp(2j * math.pi * (q * y) / ny).to(gE.dtype)
        g = (Fx[None] @ G @ Fy[None]) / (nx * ny)                            # [B, nx, ny]  (tiny: 4ox+1 inner dims)
        if not cplx:
            g = torch.real(g)
        return g.to(gdt), None, None, None, None


class ConvMatOrdersFn(torch.autograd.Function):
    """E = convmat_orders(grid, mn) (include/trx.h: trx_convmat_orders) for an [N,2] harmonic list.  The backward mirrors ConvMatFn: the
    scatter-add of grad_E over the differences (m_i - m_j, n_i - n_j), then the conjugate pruned DFT over the coefficient box."""

    @staticmethod
    def forward(ctx, grid, mn, cdtype, engine):
        mn = torch.as_tensor(mn)
        ctx.meta = (mn, grid.shape, grid.is_complex(), grid.dtype)
        return engine.convmat_orders(grid, mn, cdtype)

    @staticmethod
    def backward(ctx, gE):
        mn, (B, n1, n2), cplx, gdt = ctx.meta
        dev = gE.device
        mn = mn.to(device=dev, dtype=torch.int64)
        mmax, nmax = (int(v) for v in mn.abs().amax(dim=0).cpu())
        nq = 4 * nmax + 1
        dm = (mn[:, None, 0] - mn[None, :, 0] + 2 * mmax).reshape(-1)
        dn = (mn[:, None, 1] - mn[None, :, 1] + 2 * nmax).reshape(-1)
        G = torch.zeros((B, (4 * mmax + 1) * nq), dtype=gE.dtype, device=dev)
        G.index_add_(1, dm * nq + dn, gE.reshape(B, -1))                    # G[p,q] = sum_{(i,j): diff = (p,q)} gE[i,j]
        G = G.reshape(B, 4 * mmax + 1, nq)
        rdt = torch.float64 if gE.dtype == torch.complex128 else torch.float32
        x = torch.arange(n1, device=dev, dtype=rdt)[:, None]
        p = torch.arange(-2 * mmax, 2 * mmax + 1, device=dev, dtype=rdt)[None, :]
        y = torch.arange(n2, device=dev, dtype=rdt)[None, :]
        q = torch.arange(-2 * nmax, 2 * nmax + 1, device=dev, dtype=rdt)[:, None]
        Fx = torch.exp(2j * math.pi * (x * p) / n1).to(gE.dtype)             # conj of the forward twiddle
        Fy = torch.exp(2j * math.pi * (q * y) / n2).to(gE.dtype)
        g = (Fx[None] @ G @ Fy[None]) / (n1 * n2)                            # [B, n1, n2]
        if not cplx:
            g = torch.real(g)
        return g.to(gdt), None, None, None


class ShapeConvFn(torch.autograd.Function):
    """E = convmat_shapes(par, val) (include/trx.h: trx_convmat_shapes) of a packed shape list (shapes.ShapeLayer.pack).  The backward is the
    adjoint of the gather (trx_toeplitz_sums) followed by the adjoint of the closed forms (trx_convmat_shapes_backward): exact derivatives with
    respect to radii, widths, centres, rotations, polygon vertices and the permittivities, both kernels bit-reproducible.  Once differentiable."""

    @staticmethod
    def forward(ctx, par, val, packed, mn, mmax, nmax, cdtype, engine):
        packed = packed._replace(par=par.detach(), val=val.detach())
        ctx.meta = (packed, mn, mmax, nmax, engine, par.dtype, val.dtype)
        return engine.convmat_shapes(packed, mn, cdtype, mmax, nmax)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gE):
        packed, mn, mmax, nmax, engine, pdt, vdt = ctx.meta
        gbox = engine.toeplitz_sums(gE, mn, mmax, nmax)
        gpar, gval = engine.convmat_shapes_backward(packed, gbox, mmax, nmax)
        gval = gval if vdt.is_complex else torch.real(gval)
        return gpar.to(pdt), gval.to(vdt), None, None, None, None, None, None


def _twiddle(n, o, dev):
    """[n, 4o+1] complex128: exp(+2 pi i (q-2o) r / n) with exact integer phase reduction (the conjugate of the forward twiddle)."""
    r = torch.arange(n, device=dev, dtype=torch.int64)[:, None]
    q = torch.arange(-2 * o, 2 * o + 1, device=dev, dtype=torch.int64)[None, :]
    return torch.exp(2j * math.pi * ((r * q) % n).to(torch.float64) / n)


class ShapeNormalFieldFn(torch.autograd.Function):
    """nn = shape_normal_field(par) (include/trx.h: trx_shape_normal_field), the [B,3,n1,n2] products of the blended normal field of a packed
    shape list, differentiable in the parameter rows par [B, npar]: the backward is trx_shape_normal_field_backward, the derivative of the
    piece of the (piecewise smooth) forward the parameters lie on, bit-reproducible.  Once differentiable."""

    @staticmethod
    def forward(ctx, par, packed, lattice, n1, n2, engine):
        packed = packed._replace(par=par.detach())
        ctx.meta = (packed, lattice, engine, par.dtype)
        return engine.shape_normal_field(packed, lattice, n1, n2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gnn):
        packed, lattice, engine, pdt = ctx.meta
        return engine.shape_normal_field_backward(packed, lattice, gnn).to(pdt), None, None, None, None, None


class FieldConvFn(torch.autograd.Function):
    """C = convmat_orders(g, mn) of REAL grids g [B,n1,n2] (the products of a normal field), differentiable in g.  The backward is the adjoint of
    the gather by trx_toeplitz_sums (fixed-order sums: ConvMatOrdersFn's index_add_ is an atomic scatter on the GPU and would cost the path its
    bit-reproducibility), then the conjugate pruned DFT over the coefficient box as two small twiddle products, real part.  Once differentiable."""

    @staticmethod
    def forward(ctx, grid, mn, mmax, nmax, cdtype, engine):
        ctx.meta = (mn, mmax, nmax, engine, tuple(grid.shape), grid.dtype)
        return engine.convmat_orders(grid, mn, cdtype, mmax, nmax)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gC):
        mn, mmax, nmax, engine, (B, n1, n2), gdt = ctx.meta
        G = engine.toeplitz_sums(gC, mn, mmax, nmax)                          # [B, 4mmax+1, 4nmax+1] complex128
        Fx, Fy = _twiddle(n1, mmax, gC.device), _twiddle(n2, nmax, gC.device)
        g = torch.real(Fx[None] @ G @ Fy.transpose(0, 1)[None]) / (n1 * n2)   # [B, n1, n2]
        return g.to(gdt), None, None, None, None, None


def _diag_index(w, o, dev):
    """Flattened (a, a') of a w x w block -> a - a' + 2o (w = 2o+1): the Toeplitz diagonal of each entry."""
    a = torch.arange(w, device=dev)
    return (a[:, None] - a[None, :] + 2 * o).reshape(-1)


class ConvMatLiFn(torch.autograd.Function):
    """(Ex, Ey) = Li's inverse-rule convolution matrices of a grid (include/trx.h: trx_convmat_li).  The backward is the adjoint chain of
    the forward: scatter (index_add), inverse transform along the other axis, gT = -U^H gU U^H per Toeplitz block (batched trx_gemm),
    Toeplitz-diagonal sums, inverse pruned DFT, and the derivative of 1/g (times conj(-1/g^2); the real part for a real grid)."""

    @staticmethod
    def forward(ctx, grid, ox, oy, cdtype, engine):
        Ex, Ey, Ux, Uy = engine.convmat_li(grid, ox, oy, cdtype, keep_inverses=True)
        ctx.meta = (ox, oy, grid.is_complex(), grid.dtype)
        ctx.engine = engine
        ctx.save_for_backward(grid, Ux, Uy)
        return Ex, Ey

    @staticmethod
    def _block_grad(eng, gF, U, tw):
        """gF [B, w^2, nq2] (adjoint of the scatter), U [B, R, w, w], tw [R, nq2] conjugate twiddles -> gT [B, R, w, w]."""
        B, R, w, _ = U.shape
        gU = (tw[None] @ gF.transpose(1, 2)).reshape(B * R, w, w).contiguous() / R      # [B, R, w^2] adjoint of the transform
        Uf = U.reshape(B * R, w, w)
        gT = -eng.gemm(eng.gemm(Uf, gU, opA=2), Uf, opB=2)                                  # -U^H gU U^H
        return gT.reshape(B, R, w * w)

    @staticmethod
    def backward(ctx, gEx, gEy):
        ox, oy, cplx, gdt = ctx.meta
        grid, Ux, Uy = ctx.saved_tensors
        eng = ctx.engine
        B, nx, ny = grid.shape
        dev, z = grid.device, torch.complex128
        wx, wy = 2 * ox + 1, 2 * oy + 1
        np_, nq = 4 * ox + 1, 4 * oy + 1
        ix, iy = _diag_index(wx, ox, dev), _diag_index(wy, oy, dev)
        gr = torch.zeros((B, nx, ny), dtype=z, device=dev)
        if gEx is not None:                      # Ex[(m,n),(m',n')] = F[m,m',n-n'],  F = transform along y of Uy
            g = gEx.to(z).reshape(B, wx, wy, wx, wy).permute(0, 1, 3, 2, 4).reshape(B, wx * wx, wy * wy)
            gF = torch.zeros((B, wx * wx, nq), dtype=z, device=dev).index_add_(2, iy, g)
            gT = ConvMatLiFn._block_grad(eng, gF, Uy, _twiddle(ny, oy, dev))             # [B, ny, wx^2]
            ga = torch.zeros((B, ny, np_), dtype=z, device=dev).index_add_(2, ix, gT)      # Toeplitz-diagonal sums
            gr += (_twiddle(nx, ox, dev)[None] @ ga.transpose(1, 2)) / nx                 # inverse pruned DFT along x
        if gEy is not None:                      # Ey[(m,n),(m',n')] = G[n,n',m-m'],  G = transform along x of Ux
            g = gEy.to(z).reshape(B, wx, wy, wx, wy).permute(0, 2, 4, 1, 3).reshape(B, wy * wy, wx * wx)
            gG = torch.zeros((B, wy * wy, np_), dtype=z, device=dev).index_add_(2, ix, g)
            gT = ConvMatLiFn._block_grad(eng, gG, Ux, _twiddle(nx, ox, dev))             # [B, nx, wy^2]
            ga = torch.zeros((B, nx, nq), dtype=z, device=dev).index_add_(2, iy, gT)
            gr += (ga @ _twiddle(ny, oy, dev).transpose(0, 1)[None]) / ny                 # inverse pruned DFT along y
        r = 1 / grid.to(z)
        gg = torch.conj(-r * r) * gr                                                       # d(1/g)/dg = -1/g^2 (holomorphic)
        if not cplx:
            gg = torch.real(gg)
        return gg.to(gdt), None, None, None, None


def _strip_weights(brk, o, L):
    """[B, K+1] float64 breakpoints -> [B, K, 4o+1] complex128 strip weights w_k[q] = (h_k/L) sinc(pi q h_k/L) e^{-2 pi i q y_k/L}."""
    f = ((brk[:, 1:] - brk[:, :-1]) / L)[:, :, None]
    mid = ((brk[:, 1:] + brk[:, :-1]) / 2)[:, :, None]
    q = torch.arange(-2 * o, 2 * o + 1, device=brk.device, dtype=torch.float64)[None, None, :]
    return f * torch.sinc(q * f) * torch.exp(-2j * math.pi * q * mid / L)


class ShapeLiFn(torch.autograd.Function):
    """(Ex, Ey) = Li's inverse-rule matrices of a packed list of axis-aligned rectangles in closed form (include/trx.h:
    trx_convmat_li_shapes), differentiable in the parameter rows par [B, npar] and the reciprocal values rval [B, S+1].  The backward is
    ConvMatLiFn's composition with the strips in the place of the grid rows and the strip weights in the place of the twiddles -- the scatter
    (index_add), gT = -U^H gU U^H per Toeplitz block (batched trx_gemm), the Toeplitz-diagonal sums, and one more small product for the
    adjoint of the weights, gw_k[q] = sum conj(U_k) gF -- followed by trx_convmat_li_shapes_backward (widths, centres, values; theta gets 0).
    Once differentiable."""

    @staticmethod
    def forward(ctx, par, rval, packed, Lx, Ly, ox, oy, cdtype, engine):
        packed = packed._replace(par=par.detach(), val=packed.val.detach())          # kind, voff and par are read; nothing of the graph is held
        Ex, Ey, Ux, Uy, brk, rec = engine.convmat_li_shapes(packed, rval, Lx, Ly, ox, oy, cdtype, keep=True)
        ctx.meta = (packed, Lx, Ly, ox, oy, engine, par.dtype, rval.dtype)
        ctx.save_for_backward(rval.detach(), Ux, Uy, brk, rec)
        return Ex, Ey

    @staticmethod
    def _direction(eng, g, U, wgt, i_scatter, i_diag, n_diag):
        """g [B, w^2, w'^2] (gE sorted by block entry and by the pair of the other axis), U [B, K, w, w], wgt [B, K, nq2] -> the adjoints
        (ga [B, K, n_diag], gw [B, K, nq2]) of the Toeplitz rows and of the weights."""
        B, K, w, _ = U.shape
        z = torch.complex128
        gF = torch.zeros((B, w * w, wgt.shape[2]), dtype=z, device=g.device).index_add_(2, i_scatter, g)          # adjoint of the scatter
        gU = (torch.conj(wgt) @ gF.transpose(1, 2)).reshape(B * K, w, w).contiguous()                             # adjoint of F = sum_k U_k w_k
        Uf = U.reshape(B * K, w, w)
        gT = -eng.gemm(eng.gemm(Uf, gU, opA=2), Uf, opB=2)                                                        # -U^H gU U^H
        ga = torch.zeros((B, K, n_diag), dtype=z, device=g.device).index_add_(2, i_diag, gT.reshape(B, K, w * w))
        gw = torch.conj(U.reshape(B, K, w * w)) @ gF
        return ga, gw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gEx, gEy):
        packed, Lx, Ly, ox, oy, eng, pdt, vdt = ctx.meta
        rval, Ux, Uy, brk, rec = ctx.saved_tensors
        B, K = Ux.shape[:2]
        dev, z = Ux.device, torch.complex128
        wx, wy = 2 * ox + 1, 2 * oy + 1
        np_, nq = 4 * ox + 1, 4 * oy + 1
        ix, iy = _diag_index(wx, ox, dev), _diag_index(wy, oy, dev)
        zeros = lambda n: torch.zeros((B, K, n), dtype=z, device=dev)
        ga_x, gw_y, ga_y, gw_x = zeros(np_), zeros(nq), zeros(nq), zeros(np_)
        if gEx is not None:                      # Ex[(m,n),(m',n')] = F[m,m',n-n'],  F = sum over the y-strips of Uy w_y
            g = gEx.to(z).reshape(B, wx, wy, wx, wy).permute(0, 1, 3, 2, 4).reshape(B, wx * wx, wy * wy)
            ga_x, gw_y = ShapeLiFn._direction(eng, g, Uy, _strip_weights(brk[:, 0], oy, Ly), iy, ix, np_)
        if gEy is not None:                      # Ey[(m,n),(m',n')] = G[n,n',m-m'],  G = sum over the x-strips of Ux w_x
            g = gEy.to(z).reshape(B, wx, wy, wx, wy).permute(0, 2, 4, 1, 3).reshape(B, wy * wy, wx * wx)
            ga_y, gw_x = ShapeLiFn._direction(eng, g, Ux, _strip_weights(brk[:, 1], ox, Lx), ix, iy, nq)
        gpar, grval = eng.convmat_li_shapes_backward(packed, rval, Lx, Ly, ox, oy, brk, rec, ga_x, gw_y, ga_y, gw_x)
        grval = grval if vdt.is_complex else torch.real(grval)
        return gpar.to(pdt), grval.to(vdt), None, None, None, None, None, None, None


class GemmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, engine):
        ctx.engine = engine
        ctx.save_for_backward(A, B)
        return engine.gemm(A, B)

    @staticmethod
    def backward(ctx, G):
        A, B = ctx.saved_tensors
        eng = ctx.engine
        G = G.contiguous()
        gA = eng.gemm(G, B, opB=2) if ctx.needs_input_grad[0] else None      # G B^H
        gB = eng.gemm(A, G, opA=2) if ctx.needs_input_grad[1] else None      # A^H G
        return gA, gB, None


class InverseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, engine):
        Y = engine.inverse(A)
        ctx.engine = engine
        ctx.save_for_backward(Y)
        return Y

    @staticmethod
    def backward(ctx, G):
        (Y,) = ctx.saved_tensors
        eng = ctx.engine
        T = eng.gemm(Y, G.contiguous(), opA=2)                               # Y^H G
        return -eng.gemm(T, Y, opB=2), None                                   # - Y^H G Y^H


class SolveFn(torch.autograd.Function):
    """X = A^-1 B."""

    @staticmethod
    def forward(ctx, A, B, engine):
        X = engine.solve(A, B)
        ctx.engine = engine
        ctx.save_for_backward(A, X)
        return X

    @staticmethod
    def backward(ctx, G):
        A, X = ctx.saved_tensors
        eng = ctx.engine
        AH = torch.conj(A).transpose(-2, -1).contiguous()
        gB = eng.solve(AH, G.contiguous())                                    # A^-H G
        gA = -eng.gemm(gB, X, opB=2) if ctx.needs_input_grad[0] else None     # - gB X^H
        return gA, gB, None


class SymFoldFn(torch.autograd.Function):
    """(blocks of T^H A T per size group ..., resid) = engine.sym_fold(A, plan); resid is not differentiable.
    backward: gA = sum_k T_k gB_k T_k^H (trx_sym_fold_backward)."""

    @staticmethod
    def forward(ctx, A, plan, engine):
        ctx.engine, ctx.plan = engine, plan
        blocks, resid = engine.sym_fold(A, plan)
        ctx.mark_non_differentiable(resid)
        return (*blocks, resid)

    @staticmethod
    def backward(ctx, *grads):
        return ctx.engine.sym_fold_backward([g.contiguous() for g in grads[:-1]], ctx.plan), None, None


class SymUnfoldFn(torch.autograd.Function):
    """(lam, W) = engine.sym_unfold(Wk, lamk, plan) for per-group lists, passed flat: SymUnfoldFn.apply(plan, engine, *Wk, *lamk).
    backward: gW_k = T_k^H gW[:, block k], glam_k = the slices of glam (trx_sym_unfold_backward)."""

    @staticmethod
    def forward(ctx, plan, engine, *parts):
        ctx.engine, ctx.plan = engine, plan
        g = len(plan.groups)
        return engine.sym_unfold(list(parts[:g]), list(parts[g:]), plan)

    @staticmethod
    def backward(ctx, glam, gW):
        gWk, glamk = ctx.engine.sym_unfold_backward(gW, glam, ctx.plan)
        return (None, None, *gWk, *glamk)


class SymFoldPairsFn(torch.autograd.Function):
    """One [B, n_kl, n_kr] tensor per (kl, kr) of `pairs`: T_kl^H M T_kr (engine.sym_fold_pair per pair).  A fold is linear: nothing is saved,
    and the full-size M is not kept alive.  backward: ONE trx_sym_fold_pairs_backward, gM = sum_p T_kl_p G_p T_kr_p^H; an output that took no
    gradient travels as a null pointer."""

    @staticmethod
    def forward(ctx, M, plan, engine, pairs):
        ctx.engine, ctx.plan, ctx.pairs = engine, plan, [(int(kl), int(kr)) for kl, kr in pairs]
        ctx.meta = (M.shape[0], M.dtype)
        ctx.set_materialize_grads(False)
        return tuple(engine.sym_fold_pair(M, plan, kl, kr) for kl, kr in ctx.pairs)

    @staticmethod
    def backward(ctx, *grads):
        B, dt = ctx.meta
        return ctx.engine.sym_fold_pairs_backward(list(grads), ctx.plan, ctx.pairs, B=B, dtype=dt), None, None, None


class SymFoldPairBdFn(torch.autograd.Function):
    """[B, n_kl, n_kr] = T_kl^H M T_kr of a 2x2-block-diagonal M given as its four diagonals bd [4,B,N] (engine.sym_fold_pair_bd); nothing is
    saved.  backward: the four diagonals of T_kl G T_kr^H (trx_sym_fold_pair_bd_backward)."""

    @staticmethod
    def forward(ctx, bd, plan, engine, kl, kr):
        ctx.engine, ctx.plan, ctx.pair = engine, plan, (int(kl), int(kr))
        return engine.sym_fold_pair_bd(bd, plan, kl, kr)

    @staticmethod
    def backward(ctx, G):
        return ctx.engine.sym_fold_pair_bd_backward(G, ctx.plan, *ctx.pair), None, None, None, None


class ThicknessColumnsFn(torch.autograd.Function):
    """out [B,T,n,m] = engine.thickness_columns_keep(rho [2,B,n,n], src [2,B,n,m], AB [2,B,n,n], phase [B,T,n], op): the per-thickness step of
    a swept solve (include/trx.h: trx_thickness_columns).  op: the output-side block, dense [B,n,n], the four diagonals [4,B,N] of a
    block-diagonal one, or None.  The solved amplitude cp is the only forward intermediate saved; backward: ONE trx_thickness_columns_backward
    per chunk of thicknesses, a gradient that is not needed travels as a null pointer.  No double backward."""

    @staticmethod
    def forward(ctx, rho, src, AB, phase, op, engine, direction, port, chunk):
        out, cp = engine.thickness_columns_keep(rho, src, AB, phase, direction, port, op, chunk=chunk)
        ctx.engine, ctx.meta = engine, (int(direction), int(port), chunk, op is not None)
        ctx.save_for_backward(rho, AB, phase, cp, *([op] if op is not None else []))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        direction, port, chunk, has_op = ctx.meta
        rho, AB, phase, cp, *rest = ctx.saved_tensors
        grads = ctx.engine.thickness_columns_backward(rho, AB, phase, cp, gout, direction, port, rest[0] if has_op else None,
                                                      needs=ctx.needs_input_grad[:5], chunk=chunk)
        return (*grads, None, None, None, None)
