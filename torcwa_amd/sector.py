"""Sector solves (BatchedRCWA(symmetry_sector=True)): the caller states that the WHOLE stack shares the mirrors of symmetry=.  The global
S-matrix is then block diagonal in the mirror basis, and solve_S_parameters solves -- eigenproblem, layer S-matrices, star products -- only
the sectors the requested columns touch (one of about n / 4 for an x- or y-polarised (0, 0) order under "xy").  A patterned layer keeps the
folded P_k, Q_k of every block (include/trx.h: trx_sym_fold_pair) instead of P, Q, A and its modes; there is no global S-matrix, so
everything that reads one is refused.  symmetry_residual is None for such layers: the grid check with
symmetry_tol is the guard.

What the mode refuses is stated here: _check_sector (the constructor), _add_layer_sector (a layer) and _refuse_sector (every method that
reads a global S-matrix or coupling matrices).

Gradients (sector_grad=True, opt-in): a layer whose tensors require grad is factorised through the differentiable primitives, its P, Q are
folded by SymFoldPairsFn (one trx_sym_fold_pairs_backward per matrix on the way back), and _sector_layer / the star products of its sectors run
on GemmFn, Eig, InverseFn and SolveFn at the sector's size; a homogeneous layer and the half-spaces are plain torch up to SymFoldPairBdFn.  The
fold acts on P and Q themselves, so the RAW gradient of a per-pixel density is mirror-symmetric: it is the mirror average of the unfolded
path's gradient, and no averaging is left to the caller (symmetry_grad=True projects the eigen-part only).  Without sector_grad the refusals of a
differentiable stack stand as they were.  Still refused with it: add_layer(swept=True), everything _refuse_sector names, the drop-in class rcwa
(it keeps coupling matrices) and the sweep drivers, whose interface is not differentiable and takes no sector_grad."""
import torch

from . import autograd_ops as ag
from . import symmetry as _sym
from .blockdiag import _kz_branch
from .torch_eig import Eig


class SectorMixin:
    def _check_sector(self, keep_coupling, avoid_Pinv_instability):
        if self.symmetry is None:
            raise ValueError('symmetry_sector=True needs symmetry="x" | "y" | "xy"')
        if keep_coupling:
            raise ValueError("symmetry_sector=True needs keep_coupling=False: the coupling matrices of a stack live in the original basis, "
                             "and a sector solve keeps none (the drop-in class rcwa always keeps them)")
        if avoid_Pinv_instability is True:
            raise ValueError("symmetry_sector=True is not available with avoid_Pinv_instability=True (a sector takes V = Q W Kz^-1 only)")
        if self.symmetry_grad and not self.sector_grad:            # with sector_grad either value is accepted: no full-size fold is run
            raise ValueError("symmetry_sector=True is not available on a differentiable stack (symmetry_grad=True): the adjoint of the "
                             "sector cascade is not implemented")

    def _refuse_sector(self, what):
        if self.symmetry_sector:
            raise ValueError(f"{what} is not available with symmetry_sector=True: only the mirror sectors a source excites are solved, so there is "
                             "no global S-matrix and there are no coupling matrices; solve_S_parameters(...) is the read-out of a sector solve")

    def _add_layer_sector(self, thickness, eps, mu, normal_field, swept):
        """add_layer of a sector solver: a patterned layer is factorised and its P, Q are built as always (any fourier_rule, a patterned mu),
        then every block keeps P_k = T_k^H P T_k', Q_k = T_k'^H Q T_k and the full-size P, Q are dropped: no A, no eigen call here.  A
        homogeneous layer keeps its block-diagonal S-matrix.  sector_grad=True: a layer with a tensor that requires grad takes the same steps
        through ConvMat*Fn, InverseFn, _pq_torch and SymFoldPairsFn; any other layer the plain calls."""
        eng = self.engine
        if swept:
            raise ValueError("add_layer(swept=True) is not available with symmetry_sector=True: the thickness sweep works on the modes of the "
                             "original basis")
        self._refuse_normal_field(normal_field)
        diff = self._requires_grad(thickness, eps, mu, self.freq, self.Kx_norm_dn, self.Ky_norm_dn)
        if diff and not self.sector_grad:
            raise ValueError("symmetry_sector=True is not available on a differentiable stack (a tensor of this layer requires grad): the "
                             "adjoint of the sector cascade is not implemented")
        self._diff = self._diff or diff
        eps_h, mu_h = self._is_homogeneous(eps), self._is_homogeneous(mu)
        self._sector_S = {}
        if eps_h and mu_h:                                  # O(N) diagonals in plain torch: differentiable as they are
            self._add_homogeneous_layer_bd(thickness, self._bvec(eps), self._bvec(mu))
            return
        eye = torch.eye(self.order_N, dtype=self._cdtype, device=self._device)
        fac, plan = self._factorise(eps, mu, eps_h, mu_h, None, diff, eye)
        inv = (lambda A: ag.InverseFn.apply(A, eng)) if diff else eng.inverse
        if fac.Einv is None:
            fac = fac._replace(Einv=inv(fac.E))
        if fac.Minv is None:
            fac = fac._replace(Minv=inv(fac.M))
        P, Q = self._pq(fac, diff)
        del fac
        opp = [_sym.opposite_block(plan.nblk, k) for k in range(plan.nblk)]
        if diff:
            rec = dict(P=list(ag.SymFoldPairsFn.apply(P, plan, eng, [(k, opp[k]) for k in range(plan.nblk)])),
                       Q=list(ag.SymFoldPairsFn.apply(Q, plan, eng, [(opp[k], k) for k in range(plan.nblk)])), diff=True)
        else:
            rec = dict(P=[eng.sym_fold_pair(P, plan, k, opp[k]) for k in range(plan.nblk)],
                       Q=[eng.sym_fold_pair(Q, plan, opp[k], k) for k in range(plan.nblk)])
        del P, Q
        self._push_layer(thickness=self._bvec(thickness, self._rdtype), _sector_layers=rec)

    def _sector_plan(self):
        """The one plan of the stack: that of the first patterned layer's centres; centres 0 when no layer is patterned."""
        key = self._sector_centres if self._sector_centres is not None else (0, 1, 0, 1)
        if key not in self._sym_plans:
            self._sym_plans[key] = _sym.build_plan(self._mn, self.symmetry, *key)
        return self._sym_plans[key]

    def _sector_bd(self, blk, kl, kr):
        """Dense sector block T_kl^H M T_kr of a BlockDiag2 M (through SymFoldPairBdFn when M carries a gradient)."""
        bd = blk.packed(self._cdtype)
        if self._requires_grad(bd):
            return ag.SymFoldPairBdFn.apply(bd, self._sector_plan(), self.engine, kl, kr)
        return self.engine.sym_fold_pair_bd(bd, self._sector_plan(), kl, kr)

    def _sector_layer(self, i, k):
        """[S11, S21] of layer i in sector k (cached): the lean formulation of SURVEY.md section 7.2 on the folded operators, with
        V_k = Q_k W_k Kz^-1 and the dense Vf^-1 block (k, k').  A differentiable layer: the same algebra on GemmFn, Eig and InverseFn."""
        if (i, k) in self._sector_layer_S:
            return self._sector_layer_S[(i, k)]
        eng, rec = self.engine, self._sector_layers[i]
        if rec is None:
            S = [self._sector_bd(self.layer_S11[i], k, k), self._sector_bd(self.layer_S21[i], k, k)]
        elif rec.get("diff"):
            plan = self._sector_plan()
            mm = lambda a, b: ag.GemmFn.apply(a.contiguous(), b.contiguous(), eng)
            Eig.engine = eng
            A = mm(rec["P"][k], rec["Q"][k])
            lam, W = Eig.apply(A) if self.stable_eig_grad else Eig.apply(A, Eig.UNBROADENED)    # as add_layer: bound to this graph node
            kz = _kz_branch(torch.sqrt(lam), negate=True)                               # rcwa.py:1241
            X = torch.exp(1j * (self.omega * self.thickness[i])[:, None] * kz)          # rcwa.py:1246
            V = mm(rec["Q"][k], W / kz[:, None, :])
            F = mm(self._sector_bd(self._Vfinv, k, _sym.opposite_block(plan.nblk, k)), V)
            A_, B_ = W + F, (W - F) * X[:, None, :]
            Tip, Tim = ag.InverseFn.apply((A_ + B_).contiguous(), eng), ag.InverseFn.apply((A_ - B_).contiguous(), eng)
            cp, cm = Tip + Tim, Tip - Tim
            I = torch.eye(W.shape[-1], dtype=self._cdtype, device=self._device)
            S = [mm(W, X[:, :, None] * cp + cm), mm(W, cp + X[:, :, None] * cm) - I]
        else:
            plan = self._sector_plan()
            A = eng.gemm(rec["P"][k], rec["Q"][k])
            lam, W = self._eig_call(A, refine_steps=3 if self._dtype == torch.complex128 else 2)
            del A
            kz = _kz_branch(torch.sqrt(lam), negate=True)                               # rcwa.py:1241
            X = torch.exp(1j * (self.omega * self.thickness[i])[:, None] * kz)          # rcwa.py:1246
            V = eng.gemm(rec["Q"][k], (W / kz[:, None, :]).contiguous())                # Q W Kz^-1, in the coordinates of block k'
            F = eng.gemm(self._sector_bd(self._Vfinv, k, _sym.opposite_block(plan.nblk, k)), V)
            A_, B_ = W + F, (W - F) * X[:, None, :]
            I = torch.eye(W.shape[-1], dtype=self._cdtype, device=self._device).expand(self.B, -1, -1).contiguous()
            Tip, Tim = eng.solve(A_ + B_, I), eng.solve(A_ - B_, I)
            cp, cm = Tip + Tim, Tip - Tim
            S = [eng.gemm(W, X[:, :, None] * cp + cm), eng.gemm(W, cp + X[:, :, None] * cm) - I]
        self._sector_layer_S[(i, k)] = S
        return S

    def _sector_global(self, k):
        """Sector k of the whole stack's S-matrix (cached): the star products of the layers' sectors and the folded half-spaces."""
        if k in self._sector_S:
            return self._sector_S[k]
        none = [[], []]

        def layer(i):
            S11, S21 = self._sector_layer(i, k)
            return [S11, S21, S21, S11], none
        S, _ = self._star_chain(None, none, (layer(i) for i in range(self.layer_N)))
        if S is None:
            nk = self._sector_plan().sizes[k]
            I = torch.eye(nk, dtype=self._cdtype, device=self._device).expand(self.B, -1, -1).contiguous()
            Z = torch.zeros_like(I)
            S = [I, Z, Z.clone(), I.clone()]
        if self.has_in:
            S, _ = self._star([self._sector_bd(blk, k, k) for blk in self._Sin], S, none, none)
        if self.has_out:
            S, _ = self._star(S, [self._sector_bd(blk, k, k) for blk in self._Sout], none, none)
        self._sector_S[k] = S
        return S

    def _solve_sector(self, orders, direction, port, polarization, ref_order, power_norm, evanscent):
        """solve_S_parameters of a sector solver: column c of block kb of the global S-matrix is sum_k T_k S^(k)_kb T_k^H e_c over the sectors
        that c touches; the expansion is plain indexing, O(n) per column, and a row no sector reaches is exactly 0."""
        orders, polarization, oi, ri, kb = self._sparam_args(orders, direction, port, polarization, ref_order)
        plan = self._sector_plan()
        full = {}
        for c in self._sparam_columns(ri, polarization):
            col = torch.zeros((self.B, self.n), dtype=self._cdtype, device=self._device)
            for k, j, w in _sym.sector_coordinates(plan, c):
                rows, src, wts = plan.expansion(k, self._device, self._cdtype)
                y = w * self._sector_global(k)[kb][:, :, j]
                col[:, rows] += wts[None, :] * y[:, src]
            full[c] = col
        return self._sparam_values(lambda c: full[c], kb, oi, ri, polarization, power_norm, evanscent)
