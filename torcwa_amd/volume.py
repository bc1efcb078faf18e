"""Per-layer volume integrals and absorption by region of `BatchedRCWA` (and, as its B = 1 view, of the drop-in `rcwa`).

Inside an internal layer every field component set is F(z) = Phi (a + s b) with the mode amplitudes of flux.py,

    a = c+ . e^{i w kz z},   b = c- . e^{i w kz (d - z)},   [c+; c-] = C_layer E_i,
    [ex; ey] = W (a + b),   [hx; hy] = V (a - b),   ez = [eps]^-1 (Ky V_x - Kx V_y)(a - b),   hz = [mu]^-1 (Kx W_y - Ky W_x)(a + b)

(the formulas of fields.py), so the integral of w |F|^2 over the cell (as a cell average, by Parseval) and over a z range has the closed form

    I = (1 / cell) int_{z0}^{z1} int int w |F|^2 dx dy dz = sum_kl M_kl T_kl(z0, z1),    M = Phi^H Gamma Phi,

Gamma the (Laurent) convolution matrix of the weight grid w and T the products of c+- with the z integrals of the mode exponentials
(include/trx.h: trx_modal_overlap, one libtrx call per field set and region; M is two trx_gemm products).  No spatial grid and no z quadrature
are involved.  When the stack was built on the differentiable path the same expressions are evaluated with GemmFn, InverseFn, ConvMat*Fn and
torch ops, with the same end-point and phi rule for the z integrals.
"""
import operator

import torch

from . import autograd_ops as ag
from .shapes import ShapeLayer


def _phi(x):
    """(e^x - 1) / x for Re x <= 0: the series for |x| < 1/2 (phi(0) = 1 exactly), the quotient elsewhere."""
    small = x.abs() < 0.5
    xs = torch.where(small, x, torch.zeros_like(x))
    p = torch.ones_like(x)
    for j in range(16, 1, -1):
        p = 1 + xs * p / j
    xl = torch.where(small, torch.ones_like(x), x)
    return torch.where(small, p, (torch.exp(xl) - 1) / xl)


def overlap_torch(M, cp, cm, kz, omega, d, zr, s):
    """[B, nr] sum_kl M_kl T_kl(z0, z1) in torch ops (differentiable): the expressions and the end-point rule of trx_modal_overlap."""
    c = torch.conj
    z0, z1 = zr[:, :, 0], zr[:, :, 1]                                             # [B, nr]
    lo, hi = torch.minimum(z0, z1), torch.maximum(z0, z1)
    D = hi - lo
    sg = torch.where(z1 < z0, -torch.ones_like(D), torch.ones_like(D))
    w, q = omega[:, None, None], kz[:, None, :]
    e = lambda z: torch.exp(1j * w * q * z[:, :, None])                           # [B, nr, n], modulus <= 1 inside the layer
    alo, ahi = cp[:, None, :] * e(lo), cp[:, None, :] * e(hi)
    blo, bhi = cm[:, None, :] * e(d[:, None] - lo), cm[:, None, :] * e(d[:, None] - hi)
    wr, wi = w * torch.real(q) * D[:, :, None], w * torch.imag(q) * D[:, :, None]
    k, l = (lambda t: t[..., :, None]), (lambda t: t[..., None, :])
    p1 = _phi(torch.complex(-(k(wi) + l(wi)), l(wr) - k(wr)))
    re2, im2 = l(wi) - k(wi), -(k(wr) + l(wr))
    first = re2 <= 0
    p2 = _phi(torch.complex(torch.where(first, re2, -re2), torch.where(first, im2, -im2)))
    t1 = k(c(alo)) * l(alo) + k(c(bhi)) * l(bhi)
    t2 = torch.where(first, k(c(alo)) * l(blo) + k(c(bhi)) * l(ahi), k(c(ahi)) * l(bhi) + k(c(blo)) * l(alo))
    return (M[:, None] * (p1 * t1 + s * (p2 * t2))).sum(dim=(-2, -1)) * (sg * D)


class VolumeMixin:
    # ---- helpers -------------------------------------------------------------------------------------------------------------------------
    def _vol_layer(self, layer_num):
        try:
            layer_num = operator.index(layer_num)
        except TypeError:
            raise ValueError(f"layer_num must be an internal layer 0 .. {self.layer_N - 1}, got {layer_num!r}") from None
        if layer_num < 0 or layer_num >= self.layer_N:
            raise ValueError(f"layer_num must be an internal layer 0 .. {self.layer_N - 1}, got {layer_num!r} "
                             "(the volume of a half-space is infinite)")
        return layer_num

    def _vol_inverses(self, l, diff):
        """([eps]^-1, [mu]^-1) of layer l (Laurent matrices: they act on ez / hz), cached per layer on the plain path."""
        E, Mu = self.eps_conv[l], self.mu_conv[l]
        if diff:
            return ag.InverseFn.apply(E, self.engine), ag.InverseFn.apply(Mu, self.engine)        # graph-bound: not cached
        cache = self.__dict__.setdefault("_vol_inv_cache", {})
        key = (l, id(E), id(Mu))
        if key not in cache:
            cache[key] = (self.engine.inverse(E), self.engine.inverse(Mu))
        return cache[key]

    def _vol_mm(self, A, X, diff):
        if diff:
            return ag.GemmFn.apply(A.contiguous(), X.contiguous(), self.engine)
        return self.engine.gemm(A, X)

    def _vol_sets(self, l, field, components, diff):
        """[(s, [Phi blocks [B, N, n]])]: the requested components grouped by the sign s of F = Phi (a + s b)."""
        N = self.order_N
        W, V = self.E_eigvec[l], self.H_eigvec[l]
        kx, ky = self.Kx_norm_dn[:, :, None], self.Ky_norm_dn[:, :, None]
        T, Z, st, sz = (W, V, 1, -1) if field == "E" else (V, W, -1, 1)
        tr = [T[:, :N] for c in components if c == "x"] + [T[:, N:] for c in components if c == "y"]
        sets = [(st, tr)] if tr else []
        if "z" in components:
            Einv, Minv = self._vol_inverses(l, diff)
            if field == "E":
                zb = self._vol_mm(Einv, ky * Z[:, :N] - kx * Z[:, N:], diff)                         # fields.py: Ez = E^-1 (Ky Hx - Kx Hy)
            else:
                zb = self._vol_mm(Minv, kx * Z[:, N:] - ky * Z[:, :N], diff)                         # Hz = M^-1 (Kx Ey - Ky Ex)
            sets.append((sz, [zb]))
        return sets

    def _vol_gamma(self, g, diff):
        """Laurent convolution matrix [B, N, N] of a weight grid [B, nx, ny] (or [1, nx, ny], shared by the batch)."""
        eng, cdt = self.engine, self._cdtype
        if not (g.is_complex() or g.is_floating_point()):
            g = g.to(self._rdtype)
        g = g.to(self._device).expand(self.B, -1, -1).contiguous()
        if self._general:
            if diff:
                return ag.ConvMatOrdersFn.apply(g, self.orders, cdt, eng)
            return eng.convmat_orders(g, self._mn_dev, cdt, self._mmax, self._nmax)
        if diff:
            return ag.ConvMatFn.apply(g, self.order[0], self.order[1], cdt, eng)
        return eng.convmat(g, self.order[0], self.order[1], cdt)

    def _vol_ranges(self, l, z_range):
        d = self.thickness[l].to(self._rdtype)
        if z_range is None:
            return torch.stack((torch.zeros_like(d), d), dim=1)[:, None, :]                          # [B, 1, 2]
        zr = torch.as_tensor(z_range, device=self._device).to(self._rdtype)
        if zr.dim() == 2:
            zr = zr[None]
        if zr.dim() != 3 or zr.shape[2] != 2 or zr.shape[0] not in (1, self.B):
            raise ValueError(f"z_range must be [nr, 2] or [{self.B}, nr, 2], got {list(zr.shape)}")
        return zr.expand(self.B, -1, -1)

    def _vol_weights(self, weight, stacked=None):
        """weight -> ([B or 1, R, nx, ny] or None, region axis in the result?).  stacked: True when a 3-D tensor is a stack [R, nx, ny]."""
        if weight is None:
            return None, False
        w = torch.as_tensor(weight, device=self._device)
        if w.dim() == 2:
            return w[None, None], False
        if w.dim() == 3:
            if stacked is None:
                stacked = w.shape[0] != self.B
            return (w[None], True) if stacked else (w[:, None], False)
        if w.dim() == 4 and w.shape[0] in (1, self.B):
            return w, True
        raise ValueError(f"weight must be [nx, ny], [{self.B}, nx, ny], a stack [R, nx, ny] or [{self.B}, R, nx, ny], got {list(w.shape)}")

    def _vol_integrals(self, l, field, components, w4, zr):
        """[B, R, nr] complex: the integral for every region of w4 [B or 1, R, nx, ny] (None: w = 1, R = 1)."""
        eng, n = self.engine, self.n
        fwd = self.source_direction == "forward"
        Cl = self.C[0][l] if fwd else self.C[1][l]
        c = self._mv(Cl, self._E_i)
        cp, cm = c[:, :n], c[:, n:]
        kz, d = self.kz_norm[l], self.thickness[l].to(self._rdtype)
        diff = self._flux_diff(self.E_eigvec[l], self.H_eigvec[l], kz, d, c, zr, w4, self.eps_conv[l], self.mu_conv[l])
        sets = self._vol_sets(l, field, components, diff)
        out = []
        for r in range(1 if w4 is None else w4.shape[1]):
            G = None if w4 is None else self._vol_gamma(w4[:, r], diff)
            tot = 0
            for s, blocks in sets:
                Phi = torch.cat(blocks, dim=1) if len(blocks) > 1 else blocks[0]
                GP = Phi if G is None else torch.cat([self._vol_mm(G, blk, diff) for blk in blocks], dim=1)      # Gamma Phi, block by block
                if diff:
                    M = ag.GemmFn.apply(torch.conj(Phi).transpose(1, 2).contiguous(), GP.contiguous(), eng)
                    tot = tot + overlap_torch(M, cp, cm, kz, self.omega, d, zr, s)
                else:
                    M = eng.gemm(Phi, GP, opA=2)                                                                    # Phi^H (Gamma Phi)
                    tot = tot + eng.modal_overlap(M, cp, cm, kz, self.omega, d, zr, s)
            out.append(tot)
        return torch.stack(out, dim=1)

    # ---- public ------------------------------------------------------------------------------------------------------------------------------
    def volume_integral(self, layer_num, field="E", components="xyz", weight=None, z_range=None, normalize=False, *, _stacked=None):
        """[B, nr] (real for a real weight, complex otherwise): (1 / cell) int int int w |F|^2 dx dy dz over the in-layer ranges z_range of
        internal layer `layer_num`, |F|^2 summed over `components` (a non-empty subset of "xyz") of field "E" or "H", in closed form.
        weight: None (w = 1), a real or complex grid [nx, ny] or [B, nx, ny], or a stack of regions [R, nx, ny] / [B, R, nx, ny], which adds a
        region axis to the result ([B, R, nr]); a 3-D weight whose leading size equals B is read as one grid per point.  The weight enters
        through its Laurent convolution matrix, i.e. as the truncated Fourier series the solver itself works with.  z_range: None (the
        whole layer), [nr, 2] or [B, nr, 2] offsets (z0, z1) inside the layer; z1 < z0 gives the negated integral.  normalize=True divides
        by incident_flux().  H carries the free-space impedance as in power_flux.  Needs keep_coupling=True, a solved stack and a source;
        a half-space has no finite volume (ValueError)."""
        self._flux_ready()
        l = self._vol_layer(layer_num)
        if field not in ("E", "H"):
            raise ValueError(f'field must be "E" or "H", got {field!r}')
        comps = "".join(sorted(set(components)))
        if not comps or any(ch not in "xyz" for ch in comps) or len(comps) != len(components):
            raise ValueError(f'components must be a non-empty subset of "xyz", got {components!r}')
        w4, region_axis = self._vol_weights(weight, _stacked)
        val = self._vol_integrals(l, field, comps, w4, self._vol_ranges(l, z_range))
        val = val.to(self._cdtype) if (w4 is not None and w4.is_complex()) else torch.real(val).to(self._rdtype)
        if normalize:
            val = val / self.incident_flux()[:, None, None]
        return val if region_axis else val[:, 0]

    def absorption_by_region(self, layer_num, masks=None, z_range=None, *, _stacked=None):
        """[B, R, nr] ([B, nr] for masks=None): the fraction of the incident flux absorbed inside the regions masks [R, nx, ny] or
        [B, R, nx, ny] (on the layer's eps grid) and the ranges z_range of internal layer `layer_num`, signed like absorption()["layers"]:

            A_r = w ( I_E[Im(eps) m_r] + I_H[Im(mu) m_r] ) / |incident_flux|        (all three components; the H term only if Im mu != 0)

        with the eps and mu given to add_layer (kept by reference, not copied); a homogeneous layer takes masks=None only.  With Laurent's
        rule the truncated system dissipates exactly sum_r A_r: complementary masks, masks=None and a z profile all sum to
        absorption()["layers"][:, layer_num] to rounding.  With fourier_rule="li" / "normal" the transverse dissipation of the truncated
        system is the anti-Hermitian part of Li's matrices or of the tensor, not a masked Laurent matrix, so the split sums to the layer
        absorption only up to the truncation error there."""
        self._flux_ready()
        l = self._vol_layer(layer_num)
        eps, mu = self.eps_grid[l], self.mu_grid[l]
        if isinstance(eps, ShapeLayer):              # masks stay grids: the layer's Im(eps) is sampled on theirs (hard edges, the DFT's positions)
            if masks is None:
                raise ValueError("absorption_by_region of a ShapeLayer takes grid masks (ShapeLayer.rasterise gives eps on any grid); "
                                 "absorption() has the whole layer")
            shp = tuple(torch.as_tensor(masks).shape[-2:])
            eps = eps.rasterise(self._lattice[0], self._lattice[1], shp[0], shp[1], device=self._device)
        eps_h, mu_h = self._is_homogeneous(eps), self._is_homogeneous(mu)
        zr = self._vol_ranges(l, z_range)
        m4 = None
        if masks is not None:
            if eps_h and mu_h:
                raise ValueError("a homogeneous layer has no grid to mask: absorption_by_region takes masks=None there")
            m = torch.as_tensor(masks, device=self._device)
            shp = tuple((mu if eps_h else eps).shape[-2:])
            if m.dim() == 3 and (_stacked or _stacked is None):
                m = m[None]
            if m.dim() != 4 or m.shape[0] not in (1, self.B) or tuple(m.shape[-2:]) != shp:
                raise ValueError(f"masks must be [R, {shp[0]}, {shp[1]}] or [{self.B}, R, {shp[0]}, {shp[1]}] (the layer's grid), got {list(m.shape)}")
            m4 = m if (m.is_complex() or m.is_floating_point()) else m.to(self._rdtype)
        tot = 0
        for field, v, homog in (("E", eps, eps_h), ("H", mu, mu_h)):
            v = torch.as_tensor(v, device=self._device)
            if not v.is_complex():
                continue
            im = torch.imag(v)
            if not v.requires_grad and not bool((im != 0).any()):
                continue
            if homog:
                w4, scale = m4, im.to(self._rdtype).reshape(self.B, 1, 1)
            else:
                g = im if im.dim() == 3 else im[None]                                     # [B or 1, nx, ny]
                w4, scale = (g[:, None] if m4 is None else g[:, None] * m4), 1.0
            tot = tot + scale * torch.real(self._vol_integrals(l, field, "xyz", w4, zr))
        if not torch.is_tensor(tot):
            tot = torch.zeros((self.B, 1 if m4 is None else m4.shape[1], zr.shape[1]), dtype=torch.float64, device=self._device)
        val = (self.omega[:, None, None] * tot / self.incident_flux().abs()[:, None, None]).to(self._rdtype)
        return val if masks is not None else val[:, 0]
