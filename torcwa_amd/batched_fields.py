"""Field maps of `BatchedRCWA`: field_xy / field_xz / field_yz for every sweep point in one call.

The formulas are those of fields.py (torcwa/rcwa.py:598-1112), per sweep point b,

    [ex; ey](z) = W (a + b),   [hx; hy](z) = V (a - b),   a = c+ . e^{i w kz z},   b = c- . e^{i w kz (d - z)},   [c+; c-] = C_layer E_i,
    ez = [eps]^-1 (Ky hx - Kx hy),   hz = [mu]^-1 (Kx ey - Ky ex),        F(x, y, z) = sum_m f_m(z) e^{i w (kx_m x + ky_m y)},

on two kernels of their own (include/trx.h): trx_layer_field forms the coefficients of all depths of a layer from W and V streamed once per 16
depths, and trx_field_synth sums the Bloch series with the phases formed in the kernel, all six components from one phase.  Between them lies
one trx_gemm per z component with the inverse of Laurent's [eps] / [mu] (under every fourier_rule, as in fields.py; a homogeneous layer divides
by the scalar).  The half-spaces need one skinny product S_block E_i (trx_matvec) and O(n nz) torch ops.  The source is the one of
source_planewave / source_fourier (flux.py), which may differ per point.  When the stack was built on the differentiable path and an input
requires grad, the same expressions are evaluated with GemmFn, InverseFn and torch ops; there are no adjoint kernels.
"""
import operator

import torch

from . import autograd_ops as ag


class BatchedFieldMixin:
    # ---- helpers -------------------------------------------------------------------------------------------------------------------------
    def _field_k(self):
        """(kx, ky) [B, N] real: the in-plane wave vectors are stored in the compute dtype with a zero imaginary part."""
        return torch.real(self.Kx_norm_dn), torch.real(self.Ky_norm_dn)

    def _field_layer_num(self, layer_num):
        try:
            layer_num = operator.index(layer_num)
        except TypeError:
            raise ValueError(f"layer_num must be an integer in -1 .. {self.layer_N}, got {layer_num!r}") from None
        if layer_num < -1 or layer_num > self.layer_N:
            raise ValueError(f"layer_num must be an integer in -1 .. {self.layer_N}, got {layer_num!r}")
        return layer_num

    def _axis(self, a, name):
        a = torch.as_tensor(a, device=self._device).to(self._rdtype).reshape(-1)
        if a.numel() == 0:
            raise ValueError(f"{name} must hold at least one sample")
        return a

    def _gemm(self, A, X, diff):
        return ag.GemmFn.apply(A.contiguous(), X.contiguous(), self.engine) if diff else self.engine.gemm(A, X.contiguous())

    def _is_scalar_medium(self, grid):
        return torch.is_tensor(grid) and grid.dim() == 1

    def _batched_conv_inverses(self, l, diff):
        """([eps]^-1, [mu]^-1) [B, N, N] of layer l, None for a homogeneous medium; cached per layer like fields.py:_conv_inverses."""
        eng = self.engine
        mats = [None if self._is_scalar_medium(g) else M for g, M in ((self.eps_grid[l], self.eps_conv[l]), (self.mu_grid[l], self.mu_conv[l]))]
        if diff and self._requires_grad(*mats):
            return tuple(None if M is None else ag.InverseFn.apply(M, eng) for M in mats)        # graph-bound: not cached
        cache = self.__dict__.setdefault("_field_inv_cache", {})
        key = (l, id(self.eps_conv[l]), id(self.mu_conv[l]))
        if key not in cache:
            cache[key] = tuple(None if M is None else eng.inverse(M.detach()) for M in mats)
        return cache[key]

    def _layer_coeffs(self, l, z):
        """[B, 6, N, nz] (Ex, Ey, Ez, Hx, Hy, Hz) Fourier coefficients of internal layer l at in-layer offsets z [B, nz]."""
        n, N = self.n, self.order_N
        fwd = self.source_direction == "forward"
        Cl = self.C[0][l] if fwd else self.C[1][l]                                                # [B, 2n, n]
        W, V, kz, d = self.E_eigvec[l], self.H_eigvec[l], self.kz_norm[l], self.thickness[l]
        c = self._mv(Cl, self._E_i)                                                               # [B, 2n]
        cp, cm = c[:, :n], c[:, n:]
        kx, ky = self._field_k()
        scal = [g if self._is_scalar_medium(g) else None for g in (self.eps_grid[l], self.mu_grid[l])]
        diff = self._flux_diff(W, V, kz, d, c, z, kx, ky, self.eps_conv[l], self.mu_conv[l], *scal)
        if diff:
            w = self.omega[:, None, None]
            a = cp[:, :, None] * torch.exp(1j * w * kz[:, :, None] * z[:, None, :])
            b = cm[:, :, None] * torch.exp(1j * w * kz[:, :, None] * (d[:, None, None] - z[:, None, :]))
            e, h = self._gemm(W, a + b, True), self._gemm(V, a - b, True)
            ex, ey, hx, hy = e[:, :N], e[:, N:], h[:, :N], h[:, N:]
            ez = ky[:, :, None] * hx - kx[:, :, None] * hy
            hz = kx[:, :, None] * ey - ky[:, :, None] * ex
        else:
            raw = self.engine.layer_field(W, V, cp, cm, kz, self.omega, d, z, kx, ky)             # [B, 6, N, nz]
            ex, ey, hx, hy, ez, hz = raw.unbind(dim=1)
        Einv, Minv = self._batched_conv_inverses(l, diff)
        ez = ez / scal[0][:, None, None] if Einv is None else self._gemm(Einv, ez, diff)
        hz = hz / scal[1][:, None, None] if Minv is None else self._gemm(Minv, hz, diff)
        return torch.stack((ex, ey, ez, hx, hy, hz), dim=1)

    def _halfspace_coeffs(self, side, z):
        """The same in the input (side -1) / output half-space at offsets z [B, nz] (fields.py:103-139, rcwa.py:639-696)."""
        N = self.order_N
        Ep, Em, Vh, kz = self._halfspace_waves(side)
        ph = torch.exp(1j * self.omega[:, None, None] * kz[:, :, None] * z[:, None, :].to(self._rdtype))      # [B, n, nz]
        Ep, Em = Ep[:, :, None] * ph, Em[:, :, None] * torch.conj(ph)
        e, h = Ep + Em, Vh.apply(Ep) - Vh.apply(Em)
        ex, ey, hx, hy = e[:, :N], e[:, N:], h[:, :N], h[:, N:]
        eps, mu = (self.eps_in, self.mu_in) if side == -1 else (self.eps_out, self.mu_out)
        kx, ky = self._field_k()
        hz = (kx[:, :, None] * ey - ky[:, :, None] * ex) / mu[:, None, None]
        ez = (ky[:, :, None] * hx - kx[:, :, None] * hy) / eps[:, None, None]
        return torch.stack((ex, ey, ez, hx, hy, hz), dim=1).to(self._cdtype)

    def _coeffs_of(self, layer_num, z):
        if layer_num == -1:
            return self._halfspace_coeffs(-1, torch.clamp(z, max=0.0))
        if layer_num == self.layer_N:
            return self._halfspace_coeffs(1, torch.clamp(z, min=0.0))
        return self._layer_coeffs(layer_num, z)

    def _synth(self, coef, ku, kv, u, v):
        """[B, 6, nu, nv, T] from coef [B, 6, N, T]: trx_field_synth, or GemmFn per component when a gradient is wanted."""
        if not self._flux_diff(coef, ku, kv):
            return self.engine.field_synth(coef, ku, kv, self.omega, u, v)
        w = self.omega[:, None, None]
        Pu = torch.exp(1j * w * ku[:, None, :] * u[None, :, None]).to(self._cdtype)                # [B, nu, N]
        Pv = torch.exp(1j * w * kv[:, :, None] * v[None, None, :]).to(self._cdtype)                # [B, N, nv]
        if coef.shape[3] == 1:
            out = [self._gemm(Pu * coef[:, c, None, :, 0], Pv, True)[:, :, :, None] for c in range(coef.shape[1])]
        else:
            P = Pu * Pv[:, None, :, 0]
            out = [self._gemm(P, coef[:, c], True)[:, :, None, :] for c in range(coef.shape[1])]
        return torch.stack(out, dim=1)

    def _field_ready(self, what):
        self._global_only(what)
        self._flux_ready()

    def _shared_thicknesses(self, what):
        """[layer_N] python floats; ValueError when a layer's thickness differs between the sweep points (a z sample would then lie in
        different layers at different points)."""
        if self.layer_N == 0:
            return []
        th = torch.stack([t.detach().to(torch.float64) for t in self.thickness], dim=0)          # [layer_N, B]
        same = (th == th[:, :1]).all(dim=1).cpu().tolist()
        for l, ok in enumerate(same):
            if not ok:
                raise ValueError(f"{what} needs every layer thickness to be the same at all {self.B} sweep points (the layer of a z sample would "
                                 f"differ per point); the thickness of layer {l} differs.  field_xy has no such limit")
        return th[:, 0].cpu().tolist()

    def _field_layer_of(self, z_axis, th):
        """Layer index of every z sample (fields.py:_layer_of, rcwa.py:623-634): -1 input, 0..L-1 internal, L output."""
        dev = self._device
        zp = torch.zeros(len(th), device=dev, dtype=z_axis.dtype)
        for i in range(len(th)):
            zp[i:] += th[i]
        zm = torch.zeros_like(zp)
        if len(th) > 0:
            zm[1:] = zp[:-1]
        layer = torch.zeros(len(z_axis), dtype=torch.int64, device=dev)
        layer[z_axis < 0.] = -1
        for i in range(len(zp)):
            layer[z_axis > zp[i]] += 1
        return layer, zp, zm

    def _field_plane(self, what, axis, z_axis, fixed, swap):
        self._field_ready(what)
        th = self._shared_thicknesses(what)
        u = self._axis(axis, "the in-plane axis")
        z_axis = torch.as_tensor(z_axis, device=self._device).reshape(-1)
        if not z_axis.is_floating_point():
            z_axis = z_axis.to(self._rdtype)
        v = torch.as_tensor([float(fixed)], dtype=self._rdtype, device=self._device)
        kx, ky = self._field_k()
        ku, kv = (ky, kx) if swap else (kx, ky)
        layer, zp, zm = self._field_layer_of(z_axis, th)
        parts, sels = [], []
        for ln in sorted(set(layer.tolist())):
            sel = torch.nonzero(layer == ln).reshape(-1)
            z = z_axis[sel]
            if ln == -1:
                zprop = torch.where(z <= 0., z, torch.zeros_like(z))
            elif ln == self.layer_N:
                zprop = z if len(zp) == 0 else torch.where(z - zp[-1] >= 0., z - zp[-1], torch.zeros_like(z))
            else:
                zprop = z - zm[ln]
            zb = zprop.to(self._rdtype)[None, :].expand(self.B, -1)
            parts.append(self._synth(self._coeffs_of(ln, zb), ku, kv, u, v)[:, :, :, 0, :])        # [B, 6, nu, nz_l]
            sels.append(sel)
        out = torch.cat(parts, dim=3)[:, :, :, torch.argsort(torch.cat(sels))] if parts else \
            torch.zeros((self.B, 6, u.shape[0], 0), dtype=self._cdtype, device=self._device)
        out = out.to(self._dtype)
        return [out[:, 0], out[:, 1], out[:, 2]], [out[:, 3], out[:, 4], out[:, 5]]

    # ---- public ------------------------------------------------------------------------------------------------------------------------------
    def field_xy(self, layer_num, x_axis, y_axis, z_prop=0.):
        """([Ex, Ey, Ez], [Hx, Hy, Hz]), each [B, nx, ny] in the solver's dtype: the fields of every sweep point on the grid x_axis x y_axis at
        the in-layer offset z_prop (a scalar or [B]) of layer `layer_num` (-1: input half-space, 0 .. layer_N - 1, layer_N: output half-space;
        z_prop is clamped to <= 0 / >= 0 in the half-spaces as in power_flux).  Needs keep_coupling=True, a solved stack and a source."""
        self._field_ready("field_xy")
        layer_num = self._field_layer_num(layer_num)
        z = torch.as_tensor(z_prop, device=self._device).to(self._rdtype)
        if z.dim() > 1 or (z.dim() == 1 and z.shape[0] not in (1, self.B)):
            raise ValueError(f"z_prop must be a scalar or [{self.B}], got {list(z.shape)}")
        z = z.reshape(-1, 1).expand(self.B, 1)
        x, y = self._axis(x_axis, "x_axis"), self._axis(y_axis, "y_axis")
        kx, ky = self._field_k()
        out = self._synth(self._coeffs_of(layer_num, z), kx, ky, x, y)[:, :, :, :, 0].to(self._dtype)
        return [out[:, 0], out[:, 1], out[:, 2]], [out[:, 3], out[:, 4], out[:, 5]]

    def field_xz(self, x_axis, z_axis, y):
        """([Ex, Ey, Ez], [Hx, Hy, Hz]), each [B, nx, nz]: the cut y = const through the whole stack; z_axis is measured from the top of the
        first layer as in rcwa.field_xz (negative: input half-space).  Every layer thickness must be the same at all sweep points."""
        return self._field_plane("field_xz", x_axis, z_axis, y, swap=False)

    def field_yz(self, y_axis, z_axis, x):
        """([Ex, Ey, Ez], [Hx, Hy, Hz]), each [B, ny, nz]: the cut x = const through the whole stack (see field_xz)."""
        return self._field_plane("field_yz", y_axis, z_axis, x, swap=True)
