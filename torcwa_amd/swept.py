"""Thickness sweeps (BatchedRCWA.add_layer(..., swept=True)): the one layer whose thickness is a sweep axis [B, T].  It keeps its modes W, kz,
V, forms no layer S-matrix and is not folded; the layers after it fold into a running product of their own (fold_layers), and
solve_S_parameters returns [B, T, len(orders)] from one GEMM and one LU per thickness (include/trx.h: trx_thickness_prepare /
trx_thickness_columns).

With swept_grad=True (opt-in) a differentiable stack is served too: the prepare step is restated from the differentiable primitives
(_swept_prepare_diff: GemmFn, SolveFn, elementwise torch), the per-thickness step is ag.ThicknessColumnsFn over the same kernels and their
adjoint (trx_thickness_columns_backward), so the eigenproblem and its adjoint still run once per point whatever T is.

What the mode refuses is stated here: _check_swept (the layer itself), _refuse_swept_diff (a differentiable stack without swept_grad) and
_refuse_swept (every method that needs the one stack a swept solver does not have)."""
import torch

from . import autograd_ops as ag
from .memory import auto_thickness_chunk


class SweptMixin:
    def _check_swept(self):
        if self._swept is not None:
            raise ValueError(f"add_layer(swept=True): layer {self._swept['index']} is already swept; one swept layer per solver "
                             "(two thickness axes would need a K per pair of thicknesses)")
        if self.keep_coupling:
            raise ValueError("add_layer(swept=True) needs keep_coupling=False: the coupling matrices of a stack depend on the thickness, "
                             "and a swept solve keeps none")
        if self.avoid_Pinv_instability:
            raise ValueError("add_layer(swept=True) is not available with avoid_Pinv_instability=True (the swept layer takes V = P^-1 W Kz only)")

    def _refuse_swept_diff(self, swept):
        if (swept or self._swept is not None) and self._diff and not self.swept_grad:
            raise ValueError("swept=True is not available on a differentiable stack (a tensor of this layer or another one requires grad): "
                             "the adjoint of the thickness sweep is opt-in, BatchedRCWA(..., swept_grad=True)")

    def _refuse_swept(self, what):
        if self._swept is not None:
            raise ValueError(f"{what} is not available on a solver with a swept layer (add_layer(..., swept=True)): there is no single stack to "
                             "solve; solve_S_parameters(...) returns the S-parameters of every thickness")

    def _swept_thickness(self, thickness):
        """The thickness axis [B, T] of the swept layer from [T] (shared by the points) or [B, T]."""
        d = torch.as_tensor(thickness, dtype=self._rdtype, device=self._device)
        if d.dim() == 1:
            d = d[None, :].expand(self.B, -1)
        if d.dim() != 2 or d.shape[0] != self.B:
            raise ValueError(f"add_layer(swept=True): thickness must be [T] or [{self.B}, T], got {list(d.shape)}")
        return d.contiguous()

    def _keep_swept_modes(self, P, W, kz, mu_s, E, diff=False):
        """V of the swept layer: P^-1 W Kz (rcwa.py:1248, 1264; trx_hmodes from E for a homogeneous mu mu_s); no layer S-matrix.  diff: through
        SolveFn, as _solve_layer_smatrix_diff forms it."""
        if diff:
            return ag.SolveFn.apply(P, W * kz[:, None, :], self.engine)
        if mu_s is not None:
            return self.engine.hmodes(E, mu_s, self.Kx_norm_dn, self.Ky_norm_dn, W, kz)
        return self.engine.solve(P, W * kz[:, None, :])

    def _swept_sides(self):
        """(Lft, Rgt): everything left / right of the swept layer as one S-matrix each -- None (nothing there), a list of four BlockDiag2
        (half-space and homogeneous layers only) or of four [B,n,n] tensors."""
        i = self._swept["index"]
        none = [[], []]
        Lft, _ = self._star_chain(self._running, none, self._stored_layers(self._n_folded, i))
        if self.has_in:
            Lft = self._Sin if Lft is None else self._star(self._Sin, Lft, none, none)[0]
        Rgt, _ = self._star_chain(self._right_running, none, self._stored_layers(i + 1 + self._n_right_folded, self.layer_N))
        if self.has_out:
            Rgt = self._Sout if Rgt is None else self._star(Rgt, self._Sout, none, none)[0]
        return Lft, Rgt

    def _solve_swept(self, orders, direction, port, polarization, ref_order, power_norm, evanscent):
        """solve_S_parameters of a solver with a swept layer: [B, T, len(orders)]."""
        orders, polarization, oi, ri, k = self._sparam_args(orders, direction, port, polarization, ref_order)
        cols = self._sparam_columns(ri, polarization)
        sw = self._swept
        i = sw["index"]
        ops = []
        for S in self._swept_sides():
            if S is not None and self._is_bd(S):
                S = self._pack_bd(S)
            ops.append(S)
        if self._diff:
            return self._solve_swept_diff(cols, k, oi, ri, polarization, power_norm, evanscent)
        vfinv = self._Vfinv.packed(self._cdtype)                                                                        # [4,B,N]
        prep = self.engine.thickness_prepare(self.E_eigvec[i], self.H_eigvec[i], vfinv, ops[0], ops[1], 0 if k < 2 else 1, cols)
        phase = torch.exp(1j * (self.omega[:, None] * sw["d"])[:, :, None] * self.kz_norm[i][:, None, :])               # [B, T, n]   rcwa.py:1246
        chunk = self.thickness_chunk or auto_thickness_chunk(self.B, sw["d"].shape[1], self.n, len(cols), self._cdtype, self._device)
        out = self.engine.thickness_columns(prep, phase, 0 if k in (0, 3) else 1, chunk=chunk)                          # [B, T, n, m]
        vals = [self._sparam_values(lambda c, t=t: out[:, t, :, cols.index(c)], k, oi, ri, polarization, power_norm, evanscent)
                for t in range(out.shape[1])]
        return torch.stack(vals, dim=1)

    # ---- swept_grad=True: the same solve on a differentiable stack --------------------------------------------------------------------------
    def _swept_mul(self, blk, X):
        """blk @ X for a block of a side's S-matrix: O(n^2) for a BlockDiag2, GemmFn for a dense one."""
        if torch.is_tensor(blk):
            return ag.GemmFn.apply(blk.contiguous(), X.contiguous(), self.engine)
        return blk.apply(X)

    def _swept_cols(self, S, blk, cols, ident):
        """[B, n, m]: the columns `cols` of block `blk` of a side; S None: of the identity (ident) or of zero."""
        if S is None:
            I = torch.eye(self.n, dtype=self._cdtype, device=self._device)[:, cols]
            return (I if ident else torch.zeros_like(I))[None].expand(self.B, -1, -1)
        M = S[blk] if torch.is_tensor(S[blk]) else S[blk].dense().to(self._cdtype)
        return M[:, :, cols]

    def _swept_prepare_diff(self, Lft, Rgt, direction, cols):
        """(rho [2,B,n,n], src [2,B,n,m], AB [2,B,n,n]): what trx_thickness_prepare returns, restated from the differentiable primitives (the
        algebra of the header comment of thickness.hip).  One factorisation of P per side: the incident side solves its m source columns next
        to the n columns of rho."""
        eng, i, n = self.engine, self._swept["index"], self.n
        W = self.E_eigvec[i]
        F = self._Vfinv.apply(self.H_eigvec[i])                                         # Vf^-1 V
        A, Bm = W + F, W - F
        rho, src = [], None
        for side, S in enumerate((Lft, Rgt)):
            if S is None:
                P, Nn = A, -Bm
            else:
                R = S[1] if side else S[2]                                              # the reflection the layer sees: Rgt21 / Lft12
                P, Nn = A - self._swept_mul(R, Bm), self._swept_mul(R, A) - Bm
            if side != direction:
                rho.append(ag.SolveFn.apply(P.contiguous(), Nn.contiguous(), eng))
                continue
            tblk, cblk = (3, 2) if side else (0, 1)
            rhs = torch.cat((Nn, 2 * self._swept_cols(S, tblk, cols, True)), dim=2).contiguous()
            X = ag.SolveFn.apply(P.contiguous(), rhs, eng)
            rho.append(X[:, :, :n])
            src = torch.stack((X[:, :, n:], self._swept_cols(S, cblk, cols, False)))
        return torch.stack(rho), src, torch.stack((A, Bm))

    def _solve_swept_diff(self, cols, k, oi, ri, polarization, power_norm, evanscent):
        """_solve_swept on a differentiable stack (swept_grad=True): [B, T, len(orders)] carrying a graph."""
        sw = self._swept
        i = sw["index"]
        direction, port = (0 if k < 2 else 1), (0 if k in (0, 3) else 1)
        Lft, Rgt = self._swept_sides()
        rho, src, AB = self._swept_prepare_diff(Lft, Rgt, direction, cols)
        # the output-side block the per-thickness step multiplies with: Rgt11 or Lft22, dense, its four diagonals, or absent
        side, blk = (Rgt, 0) if (direction == 0) != (port == 1) else (Lft, 3)
        op = None
        if side is not None:
            op = side[blk].contiguous() if torch.is_tensor(side[blk]) else side[blk].packed(self._cdtype)
        phase = torch.exp(1j * (self.omega[:, None] * sw["d"])[:, :, None] * self.kz_norm[i][:, None, :])               # [B, T, n]   rcwa.py:1246
        chunk = self.thickness_chunk or auto_thickness_chunk(self.B, sw["d"].shape[1], self.n, len(cols), self._cdtype, self._device, backward=True)
        out = ag.ThicknessColumnsFn.apply(rho, src, AB, phase, op, self.engine, direction, port, chunk)                 # [B, T, n, m]
        vals = [self._sparam_values(lambda c, t=t: out[:, t, :, cols.index(c)], k, oi, ri, polarization, power_norm, evanscent)
                for t in range(out.shape[1])]
        return torch.stack(vals, dim=1)
