"""Read-out of a solved stack: S-parameters (rcwa.py:300-524) and diffraction angles (rcwa.py:214-262) of BatchedRCWA.

_sparam_args / _sparam_columns / _sparam_values are what every solve mode shares: a mode hands _sparam_values the columns of the one block
of the global S-matrix that the read-out takes, however it came by them (the global S-matrix, a probed half-space product, a thickness
sweep, the mirror sectors)."""
import warnings

import torch

# torcwa/rcwa.py:5 -- the reference's pi (typo in the 9th decimal) is part of its observable behaviour
PI_REF = 3.141592652589793

_DIRS = {"f": "forward", "forward": "forward", "b": "backward", "backward": "backward"}
_PORTS = {"t": "transmission", "transmission": "transmission", "r": "reflection", "reflection": "reflection"}
_SBLOCK = {("forward", "transmission"): 0, ("forward", "reflection"): 1, ("backward", "reflection"): 2, ("backward", "transmission"): 3}
# (numerator side, denominator side) of the power normalisation for S[k]            rcwa.py:377-388
_KZ_SIDES = {0: ("out", "in"), 1: ("in", "in"), 2: ("out", "out"), 3: ("in", "out")}


class ReadoutMixin:
    def _matching_indices(self, orders):                                                # rcwa.py:1115-1122
        if self._general:         # position in the order list; the reference's clamping into the box applies to the rectangular path only
            idx = []
            for p, q in orders.reshape(-1, 2).tolist():
                if (p, q) not in self._index:
                    raise ValueError(f"harmonic ({p}, {q}) is not in this solver's order set")
                idx.append(self._index[(p, q)])
            return torch.as_tensor(idx, dtype=torch.int64, device=orders.device)
        ox, oy = self.order
        orders[orders[:, 0] < -ox, 0] = -ox
        orders[orders[:, 0] > ox, 0] = ox
        orders[orders[:, 1] < -oy, 1] = -oy
        orders[orders[:, 1] > oy, 1] = oy
        return len(self.order_y) * (orders[:, 0] + ox) + orders[:, 1] + oy

    def _kz_real(self, side, evan, abs_when_evanescent=False):
        em = self.eps_in * self.mu_in if side == "in" else self.eps_out * self.mu_out
        kzc = torch.sqrt(em[:, None] - self.Kx_norm_dn ** 2 - self.Ky_norm_dn ** 2)
        ev = torch.abs(torch.real(kzc) / torch.imag(kzc)) < evan
        repl = torch.abs(torch.real(kzc)) if abs_when_evanescent else torch.zeros_like(torch.real(kzc))
        kz = torch.where(ev, repl, torch.real(kzc))
        return torch.cat((kz, kz), dim=1)                                               # [B, n]

    def _sparam_args(self, orders, direction, port, polarization, ref_order):
        """Argument handling of S_parameters (rcwa.py:300-340): warnings and defaults for invalid names, the order -> index map (clamps `orders`
        in place).  Returns (orders, polarization, oi, ri, k) with k the block of S the (direction, port) pair reads."""
        dev = self._device
        orders = torch.as_tensor(orders, dtype=torch.int64, device=dev).reshape([-1, 2])
        if direction in _DIRS:
            direction = _DIRS[direction]
        else:
            warnings.warn("Invalid propagation direction. Set as forward.", UserWarning)
            direction = "forward"
        if port in _PORTS:
            port = _PORTS[port]
        else:
            warnings.warn("Invalid port. Set as tramsmission.", UserWarning)
            port = "transmission"
        if polarization not in ("xx", "yx", "xy", "yy", "pp", "sp", "ps", "ss"):
            warnings.warn("Invalid polarization. Set as xx.", UserWarning)
            polarization = "xx"
        ref_order = torch.as_tensor(ref_order, dtype=torch.int64, device=dev).reshape([1, 2])
        oi = self._matching_indices(orders)
        ri = self._matching_indices(ref_order)
        return orders, polarization, oi, ri, _SBLOCK[(direction, port)]

    def _sparam_columns(self, ri, polarization):
        """Columns of the S block that _sparam_values reads: one in the xy basis, r0 and r0 + N in the ps basis."""
        r0 = int(ri[0])
        if polarization in ("xx", "yx", "xy", "yy"):
            return [r0 + (self.order_N if polarization[1] == "y" else 0)]
        return [r0, r0 + self.order_N]

    def S_parameters(self, orders, *, direction="forward", port="transmission", polarization="xx", ref_order=[0, 0],
                     power_norm=True, evanscent=1e-3):                                  # rcwa.py:300-524
        self._refuse_sector("S_parameters")
        orders, polarization, oi, ri, k = self._sparam_args(orders, direction, port, polarization, ref_order)
        Sk = self.S[k]
        return self._sparam_values(lambda c: Sk[:, :, c], k, oi, ri, polarization, power_norm, evanscent)

    def _sparam_values(self, col, k, oi, ri, polarization, power_norm, evanscent):
        """Read-out and normalisation of S_parameters from the columns of block k: col(c) -> [B, n], column c of S[k] (one of _sparam_columns)."""
        N = self.order_N
        num_side, den_side = _KZ_SIDES[k]

        if polarization in ("xx", "yx", "xy", "yy"):
            if polarization[0] == "y":
                oi = oi + N
            if polarization[1] == "y":
                ri = ri + N
            val = col(int(ri[0]))[:, oi]                                                 # [B, M]
            if power_norm:
                kzn, kzd = self._kz_real(num_side, evanscent), self._kz_real(den_side, evanscent)
                kxr = torch.cat((torch.real(self.Kx_norm_dn),) * 2, dim=1)
                kyr = torch.cat((torch.real(self.Ky_norm_dn),) * 2, dim=1)
                pn = kxr if polarization[0] == "x" else kyr                              # rcwa.py:368-375
                pd = kxr if polarization[1] == "x" else kyr
                norm = torch.sqrt((1 + (pn[:, oi] / kzn[:, oi]) ** 2) / (1 + (pd[:, ri] / kzd[:, ri]) ** 2))
                norm = norm * torch.sqrt(kzn[:, oi] / kzd[:, ri])
                val = val * norm
            val = torch.where(torch.isinf(val), torch.zeros_like(val), val)
            val = torch.where(torch.isnan(val), torch.zeros_like(val), val)
            return val.to(self._dtype)

        # ps basis                                                                         rcwa.py:410-521
        osign, rsign = {0: (1, 1), 1: (-1, 1), 2: (1, -1), 3: (-1, -1)}[k]
        em_in, em_out = self.eps_in * self.mu_in, self.eps_out * self.mu_out
        ok2 = {0: em_out, 1: em_in, 2: em_out, 3: em_in}[k]
        rk2 = {0: em_in, 1: em_in, 2: em_out, 3: em_out}[k]

        def angles(idx, k2, sign):
            kx_, ky_ = self.Kx_norm_dn[:, idx], self.Ky_norm_dn[:, idx]
            kt = torch.sqrt(kx_ ** 2 + ky_ ** 2)
            kzc = torch.sqrt(k2[:, None] - kx_ ** 2 - ky_ ** 2)
            kzs = sign * torch.abs(torch.real(kzc))
            ev = torch.abs(torch.real(kzc) / torch.imag(kzc)) < evanscent
            return torch.atan2(torch.real(kt), kzs), torch.atan2(torch.real(ky_), torch.real(kx_)), ev

        o_inc, o_azi, o_ev = angles(oi, ok2, osign)
        r_inc, r_azi, r_ev = angles(ri, rk2, rsign)
        r0 = int(ri[0])
        c0, c1 = col(r0), col(r0 + N)
        xx, xy = c0[:, oi], c1[:, oi]
        yx, yy = c0[:, oi + N], c1[:, oi + N]
        zero = torch.zeros_like(xx)
        xx, xy, yx, yy = (torch.where(o_ev, zero, t) for t in (xx, xy, yx, yy))
        co, so, ci = torch.cos(o_azi), torch.sin(o_azi), torch.cos(o_inc)
        cr, sr, cri = torch.cos(r_azi), torch.sin(r_azi), torch.cos(r_inc)
        if polarization == "pp":
            val = co / ci * cri * cr * xx + so / ci * cri * cr * yx + co / ci * cri * sr * xy + so / ci * cri * sr * yy
        elif polarization == "ps":
            val = co / ci * (-1) * sr * xx + so / ci * (-1) * sr * yx + co / ci * cr * xy + so / ci * cr * yy
        elif polarization == "sp":
            val = -so * cri * cr * xx + co * cri * cr * yx + -so * cri * sr * xy + co * cri * sr * yy
        else:
            val = -so * (-1) * sr * xx + co * (-1) * sr * yx + -so * cr * xy + co * cr * yy
        val = torch.where(torch.isinf(val), torch.zeros_like(val), val)
        val = torch.where(torch.isnan(val), torch.zeros_like(val), val)
        if power_norm:
            kz_in = self._kz_real("in", evanscent)
            kz_out = self._kz_real("out", evanscent, abs_when_evanescent=True)          # rcwa.py:495
            kzn = kz_out if num_side == "out" else kz_in
            kzd = kz_out if den_side == "out" else kz_in
            val = val * torch.sqrt(kzn[:, oi] / kzd[:, ri])
        val = torch.where(r_ev, torch.zeros_like(val), val)                             # rcwa.py:462-464 (per point)
        return val.to(self._dtype)

    def diffraction_angle(self, orders, *, layer="output", unit="radian"):               # rcwa.py:214-262
        orders = torch.as_tensor(orders, dtype=torch.int64, device=self._device).reshape([-1, 2])
        if layer in ("i", "in", "input"):
            layer = "input"
        elif layer in ("o", "out", "output"):
            layer = "output"
        else:
            warnings.warn("Invalid layer. Set as output layer.", UserWarning)
            layer = "output"
        if unit in ("r", "rad", "radian"):
            unit = "radian"
        elif unit in ("d", "deg", "degree"):
            unit = "degree"
        else:
            warnings.warn("Invalid unit. Set as radian.", UserWarning)
            unit = "radian"
        idx = self._matching_indices(orders)
        eps = self.eps_in if layer == "input" else self.eps_out
        mu = self.mu_in if layer == "input" else self.mu_out
        kx, ky = self.Kx_norm_dn[:, idx], self.Ky_norm_dn[:, idx]
        kt = torch.sqrt(kx ** 2 + ky ** 2)
        kz = torch.sqrt((eps * mu)[:, None] - kx ** 2 - ky ** 2)
        inc = torch.atan2(torch.real(kt), torch.real(kz))
        azi = torch.atan2(torch.real(ky), torch.real(kx))
        if unit == "degree":
            inc, azi = (180. / PI_REF) * inc, (180. / PI_REF) * azi
        return inc, azi
