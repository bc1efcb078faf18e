"""Sources, per-plane power flux and per-layer absorption of `BatchedRCWA` (and, as its B = 1 view, of the drop-in `rcwa`).

The flux through a plane needs no spatial grid: by Parseval the cell average of Ex Hy* - Ey Hx* is a sum over harmonics in which the Bloch
phases cancel,

    Phi(z) = Re sum_j ( ex_j(z) conj(hy_j(z)) - ey_j(z) conj(hx_j(z)) ),    [ex; ey] = W (a + b),   [hx; hy] = V (a - b),
    a = c+ . e^{i w kz z},   b = c- . e^{i w kz (d - z)},   [c+; c-] = C_layer E_i

-- the formulas of fields.py for Ex, Ey, Hx, Hy (torcwa/rcwa.py:708-755).  Internal layers are one libtrx call per layer (trx_layer_flux: W and V
streamed once per 16 planes, nothing of size [n, nz] written); the half-spaces need one skinny product S_block E_i (trx_matvec) and O(n) work.
H carries the free-space impedance as in the reference, so a unit plane wave in a medium of index n_in at angle theta has Phi = n_in cos(theta).
Phi is positive along +z.  When the stack was built on the differentiable path the same expressions are evaluated with GemmFn and torch ops.
"""
import operator
import warnings

import torch

from ._lib import TrxError
from . import autograd_ops as ag


class FluxMixin:
    # ---- sources (semantics of FieldMixin / torcwa/rcwa.py:526-596, one source per sweep point) ---------------------------------------
    def source_planewave(self, *, amplitude=[1., 0.], direction="forward", notation="xy"):
        self.source_fourier(amplitude=amplitude, orders=[0, 0], direction=direction, notation=notation)

    def source_fourier(self, *, amplitude, orders, direction="forward", notation="xy"):
        """amplitude: [M, 2] (or [2] for one order) shared by the batch, or with a leading B: [B, M, 2] / [B, 2]."""
        cdt, dev, N, B = self._cdtype, self._device, self.order_N, self.B
        orders = torch.as_tensor(orders, dtype=torch.int64, device=dev).reshape([-1, 2])
        M = orders.shape[0]
        # python scalars / lists: built directly in the compute dtype like FieldMixin.source_fourier (no fp32 detour: 0.3 would arrive as 0.3f)
        amp = amplitude.to(device=dev, dtype=cdt) if torch.is_tensor(amplitude) else torch.as_tensor(amplitude, dtype=cdt, device=dev)
        if amp.numel() == 2 * M:
            amp = amp.reshape(1, M, 2).expand(B, M, 2)
        elif amp.numel() == 2 * M * B:
            amp = amp.reshape(B, M, 2)
        else:
            raise ValueError(f"amplitude must hold [{M}, 2] values (shared) or [{B}, {M}, 2] (per point), got {list(amp.shape)}")
        if direction in ("f", "forward"):
            direction = "forward"
        elif direction in ("b", "backward"):
            direction = "backward"
        else:
            warnings.warn("Invalid source direction. Set as forward.", UserWarning)
            direction = "forward"
        if notation not in ("xy", "ps"):
            warnings.warn("Invalid amplitude notation. Set as xy notation.", UserWarning)
            notation = "xy"
        idx = self._matching_indices(orders)
        self.source_direction = direction
        E_i = torch.zeros([B, 2 * N], dtype=cdt, device=dev)
        E_i[:, idx] = amp[:, :, 0]
        E_i[:, idx + N] = amp[:, :, 1]
        if notation == "ps":                           # rcwa.py:575-594 with every point's own kx, ky, eps, mu
            eps, mu, sign = (self.eps_in, self.mu_in, 1) if direction == "forward" else (self.eps_out, self.mu_out, -1)
            kx, ky = self.Kx_norm_dn, self.Ky_norm_dn
            kt = torch.sqrt(kx ** 2 + ky ** 2)
            kz = sign * torch.abs(torch.real(torch.sqrt((eps * mu)[:, None] - kx ** 2 - ky ** 2)))
            inc = torch.atan2(torch.real(kt), kz)
            azi = torch.atan2(torch.real(ky), torch.real(kx))
            Ep, Es = E_i[:, :N], E_i[:, N:]
            Ex = torch.cos(inc) * torch.cos(azi) * Ep - torch.sin(azi) * Es
            Ey = torch.cos(inc) * torch.sin(azi) * Ep + torch.cos(azi) * Es
            E_i = torch.cat((Ex, Ey), dim=1).to(cdt)
        self._E_i = E_i                                # [B, n]

    @property
    def E_i(self):
        return self._E_i.to(self._dtype)

    # ---- helpers -------------------------------------------------------------------------------------------------------------------------
    def _flux_ready(self):
        missing = []
        if not self.keep_coupling:
            missing.append("keep_coupling=True (this solver was built with keep_coupling=False: W, V and the coupling matrices were dropped)")
        if not hasattr(self, "C") or not hasattr(self, "S"):
            missing.append("a solved stack (call solve_global_smatrix() first)")
        if missing:
            raise TrxError("power_flux / absorption need " + " and ".join(missing))
        if not hasattr(self, "_E_i"):
            raise TrxError("power_flux / absorption need a source (call source_planewave() or source_fourier() first)")

    def _flux_diff(self, *tensors):
        return self._diff and self._requires_grad(*tensors)

    def _mv(self, A, x):
        """A [B,m,n] times x [B,n] -> [B,m]: trx_matvec, or GemmFn when a gradient is wanted."""
        if self._flux_diff(A, x):
            return ag.GemmFn.apply(A.contiguous(), x[:, :, None].contiguous(), self.engine)[:, :, 0]
        return self.engine.matvec(A, x[:, :, None])[:, :, 0]

    @staticmethod
    def _poynting(E, H, N):
        """Re sum_j (Ex_j conj(Hy_j) - Ey_j conj(Hx_j)) over dim 1 of [B, n, nz]."""
        return torch.real(E[:, :N] * torch.conj(H[:, N:]) - E[:, N:] * torch.conj(H[:, :N])).sum(dim=1)

    def _halfspace_waves(self, side):
        """(E+ [B,n], E- [B,n], Vh, kz [B,n]) at z = 0 of the input (side -1) / output half-space: the amplitudes of fields.py (rcwa.py:639-696)."""
        E_i, S = self._E_i, self.S
        fwd = self.source_direction == "forward"
        kx, ky = self.Kx_norm_dn, self.Ky_norm_dn
        zero = torch.zeros_like(E_i)
        if side == -1:
            Vh = self._Vi if self.has_in else self._Vf
            kz = torch.sqrt((self.eps_in * self.mu_in)[:, None] - kx ** 2 - ky ** 2)
            kz = torch.where(torch.imag(kz) > 0, torch.conj(kz), kz)
            Ep, Em = (E_i, self._mv(S[1], E_i)) if fwd else (zero, self._mv(S[3], E_i))
        else:
            Vh = self._Vo if self.has_out else self._Vf
            kz = torch.sqrt((self.eps_out * self.mu_out)[:, None] - kx ** 2 - ky ** 2)
            kz = torch.where(torch.imag(kz) < 0, torch.conj(kz), kz)
            Ep, Em = (self._mv(S[0], E_i), zero) if fwd else (self._mv(S[2], E_i), E_i)
        return Ep, Em, Vh, torch.cat((kz, kz), dim=1)

    def _halfspace_flux(self, side, z, parts="both"):
        """Phi [B, nz] in a half-space at offsets z [B, nz]; parts: "both", or "+" / "-" for the flux of one wave alone."""
        Ep, Em, Vh, kz = self._halfspace_waves(side)
        ph = torch.exp(1j * self.omega[:, None, None] * kz[:, :, None] * z[:, None, :].to(self._rdtype))      # [B, n, nz]
        Ep = Ep[:, :, None] * ph if parts != "-" else torch.zeros_like(ph)
        Em = Em[:, :, None] * torch.conj(ph) if parts != "+" else torch.zeros_like(ph)
        return self._poynting(Ep + Em, Vh.apply(Ep) - Vh.apply(Em), self.order_N)

    def _layer_flux(self, l, z):
        """Phi [B, nz] of internal layer l at offsets z [B, nz]."""
        n, N = self.n, self.order_N
        fwd = self.source_direction == "forward"
        Cl = self.C[0][l] if fwd else self.C[1][l]                                                # [B, 2n, n]
        W, V, kz, d = self.E_eigvec[l], self.H_eigvec[l], self.kz_norm[l], self.thickness[l]
        c = self._mv(Cl, self._E_i)                                                               # [B, 2n]
        cp, cm = c[:, :n], c[:, n:]
        if self._flux_diff(W, V, kz, d, c, z):
            w = self.omega[:, None, None]
            a = cp[:, :, None] * torch.exp(1j * w * kz[:, :, None] * z[:, None, :])
            b = cm[:, :, None] * torch.exp(1j * w * kz[:, :, None] * (d[:, None, None] - z[:, None, :]))
            mm = lambda A, X: ag.GemmFn.apply(A.contiguous(), X.contiguous(), self.engine)
            return self._poynting(mm(W, a + b), mm(V, a - b), N)
        return self.engine.layer_flux(W, V, cp, cm, kz, self.omega, d, z).to(self._rdtype)

    def incident_flux(self):
        """[B] Phi of the source wave alone in its own half-space: Re sum (E_i,x conj(H_i,y) - E_i,y conj(H_i,x)) with H_i = +V_in E_i for a
        forward source and -V_out E_i for a backward one (negative then: Phi is counted along +z)."""
        if not hasattr(self, "_E_i"):
            raise TrxError("incident_flux needs a source (call source_planewave() or source_fourier() first)")
        fwd = self.source_direction == "forward"
        Vh = (self._Vi if self.has_in else self._Vf) if fwd else (self._Vo if self.has_out else self._Vf)
        E = self._E_i[:, :, None]
        H = Vh.apply(E)
        return self._poynting(E, H if fwd else -H, self.order_N)[:, 0]

    def _z_arg(self, z_prop):
        z = torch.as_tensor(z_prop, device=self._device).to(self._rdtype)
        if z.dim() == 0:
            z = z.reshape(1, 1)
        elif z.dim() == 1:
            z = z[None, :]
        if z.dim() != 2 or z.shape[0] not in (1, self.B):
            raise ValueError(f"z_prop must be a scalar, [nz] or [{self.B}, nz], got {list(z.shape)}")
        return z.expand(self.B, -1)

    # ---- public ------------------------------------------------------------------------------------------------------------------------------
    def power_flux(self, layer_num, z_prop=0.0, *, normalize=True):
        """Real [B, nz]: the power flux (cell average of the z component of Re(E x H*), positive along +z) through the planes at in-layer
        offsets z_prop (scalar, [nz] or [B, nz]) of layer `layer_num` (-1: input half-space, 0 .. layer_N - 1, layer_N: output half-space;
        z_prop is clamped to <= 0 / >= 0 in the half-spaces as in field_xy).  normalize=True divides by incident_flux(), so the result is
        positive along the propagation direction of the source; a purely evanescent source has zero incident flux and the normalised result is
        then whatever IEEE division gives (inf / nan).  Needs keep_coupling=True, a solved stack and a source."""
        self._flux_ready()
        try:
            layer_num = operator.index(layer_num)              # python, numpy and torch integer scalars
        except TypeError:
            raise ValueError(f"layer_num must be an integer in -1 .. {self.layer_N}, got {layer_num!r}") from None
        if layer_num < -1 or layer_num > self.layer_N:
            raise ValueError(f"layer_num must be an integer in -1 .. {self.layer_N}, got {layer_num!r}")
        z = self._z_arg(z_prop)
        if layer_num == -1:
            phi = self._halfspace_flux(-1, torch.clamp(z, max=0.0))
        elif layer_num == self.layer_N:
            phi = self._halfspace_flux(1, torch.clamp(z, min=0.0))
        else:
            phi = self._layer_flux(layer_num, z)
        return phi / self.incident_flux()[:, None] if normalize else phi

    def absorption(self):
        """{"layers": [B, layer_N], "R": [B], "T": [B], "A": [B]}, all normalised by the incident flux: the flux entering minus the flux
        leaving each layer (one trx_layer_flux call per layer with z = {0, d}); the flux of the outgoing wave alone on the source side (R)
        and the flux on the far side (T); A = the sum over layers.  R + T + A = 1 when the source half-space is lossless and the source
        has no evanescent part."""
        self._flux_ready()
        inc = self.incident_flux()
        fwd = self.source_direction == "forward"
        z0 = torch.zeros((self.B, 1), dtype=self._rdtype, device=self._device)
        lay = []
        for l in range(self.layer_N):
            phi = self._layer_flux(l, torch.cat((z0, self.thickness[l][:, None].to(self._rdtype)), dim=1)) / inc[:, None]
            lay.append(phi[:, 0] - phi[:, 1] if fwd else phi[:, 1] - phi[:, 0])
        layers = torch.stack(lay, dim=1) if lay else torch.zeros((self.B, 0), dtype=self._rdtype, device=self._device)
        if fwd:
            R = -self._halfspace_flux(-1, z0, parts="-")[:, 0] / inc
            T = self._halfspace_flux(1, z0)[:, 0] / inc
        else:
            R = -self._halfspace_flux(1, z0, parts="+")[:, 0] / inc
            T = self._halfspace_flux(-1, z0)[:, 0] / inc
        return {"layers": layers, "R": R, "T": T, "A": layers.sum(dim=1)}
