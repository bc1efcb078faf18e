"""Batched RCWA solver: B independent sweep points (frequency / angle / geometry) advance in lock-step.

This is the MI355X-native restatement of the hot path of torcwa.rcwa (kch3782/torcwa 0.1.4.2, torcwa/rcwa.py).  The
reference is un-batched (one object per sweep point, a Python `for` loop over points, e.g. example/Example1.ipynb
cell "lamb0 sweep"); here the sweep axis is the leading tensor dimension and every heavy operation is one batched
libtrx call (include/trx.h).  The drop-in class `torcwa_amd.rcwa` is the B=1 view of this class.

All per-point scalars (`freq`, angles, homogeneous eps/mu, thickness) may be python scalars or [B] tensors.
"""
import warnings
from collections import namedtuple

import numpy as np
import torch

from .engine import Engine, default_engine
from . import autograd_ops as ag
from . import lattice as _lat
from . import shapes as _shapes
from . import symmetry as _sym
from .blockdiag import BlockDiag2, _halfspace_V, _kz_branch, _star_bd
from .batched_fields import BatchedFieldMixin
from .flux import FluxMixin
from .readout import PI_REF, ReadoutMixin  # noqa: F401  (PI_REF: part of this module's interface)
from .sector import SectorMixin
from .swept import SweptMixin
from .torch_eig import Eig
from .volume import VolumeMixin

FOURIER_RULES = ("laurent", "li", "normal")
# fourier_rule="normal": default width (grid cells) of the Gaussian that smooths the structure tensor of a grid into the normal-vector field
# (include/trx.h: trx_normal_field); chosen by the CPU study in profiles/normal_vector.txt
NV_SIGMA_DEFAULT = 6.0
# fourier_rule="normal" on a shapes.ShapeLayer: the grid (an int or (n1, n2)) on which the three smooth products of the layer's normal field are
# sampled (include/trx.h: trx_shape_normal_field).  128, 256 and 512 give the same digits at orders [5,5] .. [9,9] for a disk and an ellipse of
# eps = 12, and 256 vs 512 differ by < 1e-5 at [13,13] (profiles/shape_nv_study.txt).  The keyword itself defaults to None -- the rule on shapes
# is opt-in, so that a solver built as before behaves as before -- and this is the value to pass: shape_nv_grid=SHAPE_NV_GRID_DEFAULT.
SHAPE_NV_GRID_DEFAULT = 256


# The factorised medium of one layer: Laurent's E, M and their inverses (None until needed; M = Minv = None for a lean layer, see
# BatchedRCWA._factorise), the per-point scalars of a homogeneous eps / mu (else None), and the matrices that stand for eps and mu per field
# component in P, Q and A (include/trx.h).  Laurent's rule: exx = eyy = E, mx = my = M, exy = None; Li's rule: its own exx, eyy (mx, my) for a
# patterned eps (mu); the normal-vector rule: the tensor exx, exy, eyy.
Medium = namedtuple("Medium", "E Einv M Minv eps_s mu_s exx exy eyy mx my")

# The per-layer record: every one of these attributes is a list with one entry per layer (None where a layer has no such thing), and
# BatchedRCWA._push_layer is the one place that appends to them.  flux.py, volume.py, fields.py and rcwa.py index them by layer.
#   thickness [B] (None: the swept layer, see _swept["d"]); eps_conv, mu_conv: Laurent's matrices; eps_grid, mu_grid (keep_coupling): the eps / mu
#   handed to add_layer, by reference (a grid or a shapes.ShapeLayer) or as the per-point scalar [B] (absorption_by_region); eps_conv_x / _y (fourier_rule="li" with
#   keep_coupling): Li's Ex, Ey; eps_conv_xx / _xy / _yy (fourier_rule="normal" with keep_coupling): the tensor Exx, Exy (= Eyx), Eyy;
#   symmetry_residual: resid [B] of trx_sym_fold (the discarded part of T^H A T relative to max |A|); _sector_layers (symmetry_sector):
#   dict(P=[P_k], Q=[Q_k]) of a patterned layer, with diff=True when they came through SymFoldPairsFn (sector_grad)
_CONV_FIELDS = ("eps_conv", "eps_conv_x", "eps_conv_y", "eps_conv_xx", "eps_conv_xy", "eps_conv_yy")     # what a folded layer drops
_LAYER_FIELDS = ("thickness", "mu_conv", "eps_grid", "mu_grid", "P", "Q", "kz_norm", "E_eigvec", "H_eigvec", "Cplus", "Cminus",
                 "layer_S11", "layer_S21", "symmetry_residual", "_sector_layers") + _CONV_FIELDS


def check_fourier_rule(rule):
    if rule not in FOURIER_RULES:
        raise ValueError(f"fourier_rule must be one of {FOURIER_RULES}, got {rule!r}")


def _propagate_coupling(mm, Cm, Cn, X1, X2, Y1, Y2):
    """The coupling lists of Sm * Sn (rcwa.py:1298-1304) from the factors X, Y of the star product: the lists Cm of the left operand take
    Y1, Y2, the lists Cn of the right operand X1, X2 (an operand without lists: [[], []], and its factors are not read).  mm: the product."""
    C = [[], []]
    for cf, cb in zip(*Cm):
        C[0].append(cf + mm(cb, Y1))
        C[1].append(mm(cb, Y2))
    for cf, cb in zip(*Cn):
        C[0].append(mm(cf, X1))
        C[1].append(cb + mm(cf, X2))
    return C


class BatchedRCWA(FluxMixin, BatchedFieldMixin, VolumeMixin, ReadoutMixin, SectorMixin, SweptMixin):
    def __init__(self, freq, order, L, *, batch=None, dtype=torch.complex64, device=None, stable_eig_grad=True,
                 avoid_Pinv_instability=False, max_Pinv_instability=0.005, precision="high", engine=None,
                 keep_coupling=True, fold_layers=False, eig_route="auto", route_hint=None, fourier_rule="laurent", nv_sigma=NV_SIGMA_DEFAULT,
                 symmetry=None, symmetry_tol=1e-6, symmetry_grad=False, symmetry_sector=False, sector_grad=False, swept_grad=False,
                 shape_nv_grid=None, shape_nv_grad=False):
        check_fourier_rule(fourier_rule)
        # symmetry (extension): None | "x" | "y" | "xy" -- the caller states that every patterned layer is invariant under x -> -x (y -> -y) about
        # a plane and that kx0 = 0 (ky0 = 0) at every sweep point.  A = P Q of such a layer is then folded into 2 / 4 independent eigenproblems
        # (include/trx.h: trx_sym_fold; torcwa_amd/symmetry.py) and the modes are unfolded into the original basis, so nothing downstream changes.
        # Checked, not trusted: the lattice, the order set, the wave vector and every grid (to symmetry_tol, relative to max |grid|); a grid that is
        # symmetric only to within the tolerance yields the solution of its symmetrised structure.  None: today's path, untouched.
        _sym.check_symmetry(symmetry)
        self.symmetry = symmetry
        self.symmetry_tol = float(symmetry_tol)
        self._sym_plans = {}
        # symmetry_grad=True (opt-in): a differentiable stack folds its eigenproblems too (SymFoldFn -> Eig per block size -> SymUnfoldFn).
        # The fold drops the part of A outside the diagonal blocks, so the eigen-part of the gradient is the one of the mirror-constrained
        # problem: gradients with respect to symmetric parameters (radii, widths, thicknesses, a symmetrised density) and the mirror average of
        # a per-pixel gradient are those of the unfolded path, a raw per-pixel gradient is not.
        self.symmetry_grad = bool(symmetry_grad)
        if self.symmetry_grad and symmetry is None:
            raise ValueError('symmetry_grad=True needs symmetry="x" | "y" | "xy"')
        # symmetry_sector=True (opt-in; needs symmetry=): only the mirror sectors a read-out touches are solved (sector.py).  False: the
        # paths below.
        self.symmetry_sector = bool(symmetry_sector)
        # sector_grad=True (opt-in; needs symmetry_sector=True): a layer whose tensors require grad goes through the differentiable twin of the
        # sector path (SymFoldPairsFn, GemmFn, Eig, InverseFn on the sector's block).  P and Q themselves are folded, so the RAW per-pixel
        # gradient is the mirror average of the unfolded path's gradient (sector.py).  symmetry_grad is then accepted and not read.
        self.sector_grad = bool(sector_grad)
        if self.sector_grad and not self.symmetry_sector:
            raise ValueError("sector_grad=True needs symmetry_sector=True")
        # swept_grad=True (opt-in): add_layer(..., swept=True) is accepted on a differentiable stack; solve_S_parameters then restates the
        # prepare step from the differentiable primitives and runs the per-thickness step through ThicknessColumnsFn (swept.py).  A stack
        # without a tensor that requires grad takes the fused path, bit for bit.
        self.swept_grad = bool(swept_grad)
        if self.swept_grad and self.symmetry_sector:
            raise ValueError("swept_grad=True is not available with symmetry_sector=True: add_layer(swept=True) itself is not (the thickness "
                             "sweep works on the modes of the whole layer, a sector solve never forms them)")
        if self.symmetry_sector:
            self._check_sector(keep_coupling, avoid_Pinv_instability)
        self._sector_centres = None      # (cx, nx, cy, ny) of the first patterned layer: the one plan of the whole stack
        self._sector_layer_S = {}        # (layer, block) -> [S11, S21] of the sector
        self._sector_S = {}              # block -> the sector of the whole stack's S-matrix, [S11, S21, S12, S22]
        # fourier_rule="li" needs the rectangular order box on a rectangular lattice (ValueError otherwise, see the order / lattice below).
        # fourier_rule="li": Li's inverse rule for the x / y components of D in every patterned layer (Ex, Ey convolution matrices,
        # include/trx.h trx_convmat_li); Ez / Hz keep Laurent's matrices (E^-1 in P, trx_hmodes, eps_conv).  "laurent": the reference's rule.
        # fourier_rule="normal": the normal-vector method (in-plane tensor Exx, Exy, Eyy of the permittivity, trx_convmat_nv) with the field
        # derived from each grid, smoothed over nv_sigma cells, unless add_layer(normal_field=...) supplies one; a patterned mu keeps
        # Laurent's matrix, and so do Ez / Hz.
        self.fourier_rule = fourier_rule
        self.nv_sigma = float(nv_sigma)
        if not (0.0 <= self.nv_sigma <= 256.0):
            raise ValueError(f"nv_sigma must lie in [0, 256] grid cells, got {nv_sigma!r}")
        # a ShapeLayer under fourier_rule="normal": [eps] and [1/eps] in closed form, the field of the shape list sampled on this grid
        # (trx_convmat_nv_shapes) unless add_layer(normal_field=...) supplies one on a grid of its own
        # None (the default): a ShapeLayer without a supplied field stays refused under this rule, as before the rule reached shapes
        self.shape_nv_grid = None if shape_nv_grid is None else _shapes.nv_grid(shape_nv_grid)
        # shape_nv_grad=True (opt-in): the field a ShapeLayer derives on shape_nv_grid stays in the autograd graph (ShapeNormalFieldFn ->
        # FieldConvFn), so the gradient with respect to the geometry is the derivative of the forward, the dependence of the blend on the
        # parameters included -- wherever the piecewise smooth forward is differentiable.  False: the derived field is a constant of the
        # graph, as before, bit for bit.  A field supplied with add_layer(normal_field=...) is a constant whatever this keyword says.
        self.shape_nv_grad = bool(shape_nv_grad)
        if self.shape_nv_grad and fourier_rule != "normal":
            raise ValueError(f'shape_nv_grad=True needs fourier_rule="normal", got {fourier_rule!r}: only that rule derives a normal field')
        if dtype != torch.complex64 and dtype != torch.complex128:                      # rcwa.py:37-41
            warnings.warn("Invalid simulation data type. Set as torch.complex64.", UserWarning)
            dtype = torch.complex64
        self._dtype = dtype
        # eigensolver route of THIS solver: "auto" | "mixed" | "fp64" (see _eig_call); route_hint: a dict shared by the chunks of one sweep call
        self.eig_route = eig_route
        self._route_hint = route_hint if route_hint is not None else {}
        self.engine = engine if engine is not None else (default_engine() if device is None else Engine(device=device))
        self._device = self.engine.device
        # precision="high": c64 problems are computed in complex128 internally (the reference's own c64 path is only
        # ~1e-3 accurate at order 15; the <=1e-5 parity gate needs fp64 in eig and LU).
        self._cdtype = torch.complex128 if (precision == "high" or dtype == torch.complex128) else torch.complex64
        self._rdtype = torch.float64 if self._cdtype == torch.complex128 else torch.float32
        self.stable_eig_grad = bool(stable_eig_grad)
        self.avoid_Pinv_instability = avoid_Pinv_instability is True
        self.max_Pinv_instability = max_Pinv_instability if self.avoid_Pinv_instability else None
        self.Pinv_instability = [] if self.avoid_Pinv_instability else None
        self.Qinv_instability = [] if self.avoid_Pinv_instability else None
        self.keep_coupling = keep_coupling
        # fold_layers (sweep drivers; needs keep_coupling=False): every layer's S-matrix is folded into the running cascade as soon as it
        # exists and is then dropped together with the layer's convolution matrix, so a K-layer stack holds ONE layer at a time instead
        # of K (configs[2]: 4 layers at n = 3698).  The per-layer attributes of such a solver are None.
        self.fold_layers = bool(fold_layers) and not keep_coupling
        self._running = None
        self._n_folded = 0            # layers 0 .. _n_folded-1 live in _running; the rest are stored layers
        # add_layer(..., swept=True): the one layer whose thickness is a sweep axis [B, T] (swept.py).  None: no such layer.
        self._swept = None            # dict(index, d [B,T])
        self._right_running = None    # the layers right of the swept one fold into a running product of their own
        self._n_right_folded = 0
        self.thickness_chunk = None   # thicknesses per library call of a swept solve (None: as many as the free HBM holds, memory.auto_thickness_chunk)
        self._diff = False            # a layer so far went through the differentiable primitives
        self._zero_layer_S = False    # the last cascade was the one of no layer and no half-space (rcwa.py:187-188)

        if batch is None:
            batch = freq.numel() if (torch.is_tensor(freq) and freq.dim() > 0) else (len(freq) if isinstance(freq, (list, tuple)) else 1)
        self.B = int(batch)
        self.freq = self._bvec(freq)                                                    # [B] complex
        self.omega = (2 * PI_REF) * torch.real(self.freq)                               # rcwa.py:61  [B] real
        # L: [Lx, Ly] or a 2 x 2 array of lattice vectors (rows a1, a2); order: [ox, oy] or an [N, 2] list of harmonics (m, n) in the lattice
        # basis (torcwa_amd.lattice).  [ox, oy] on a rectangular lattice is the reference's path, unchanged; anything else is the general path:
        # an order list, the convolution matrices of trx_convmat_orders, G_norm = (b1, b2) / f, and order_x / order_y / Gx_norm / Gy_norm None.
        kind, box, mn = _lat.parse_order(order)
        A = _lat.lattice_matrix(L)
        rect_lattice = _lat.is_rectangular(A)
        flat_L = _lat._host(L).shape == (2,)
        Lx, Ly = (L[0], L[1]) if flat_L else ((L[0][0], L[1][1]) if rect_lattice else (None, None))
        self._general = kind == "list" or not rect_lattice
        self.L = L
        self._lattice = A
        self._Lxy = (Lx, Ly)          # the rectangle's periods (None, None on an oblique lattice), whichever form L took
        if not self._general:
            self.order = [int(box[0]), int(box[1])]
            self.order_x = torch.arange(-self.order[0], self.order[0] + 1, dtype=torch.int64, device=self._device)
            self.order_y = torch.arange(-self.order[1], self.order[1] + 1, dtype=torch.int64, device=self._device)
            self.order_N = len(self.order_x) * len(self.order_y)
            self.Gx_norm = 1 / (Lx * self.freq)                                         # rcwa.py:72
            self.Gy_norm = 1 / (Ly * self.freq)
            mn = _lat.rect_orders(*self.order)
            G = torch.zeros((self.B, 2, 2), dtype=self.Gx_norm.dtype, device=self._device)
            G[:, 0, 0], G[:, 1, 1] = self.Gx_norm, self.Gy_norm
        else:
            if self.fourier_rule == "li":
                raise ValueError('fourier_rule="li" needs the rectangular order box [ox, oy] on a rectangular lattice')
            if kind == "rect":
                mn = _lat.rect_orders(*box)
            self.order = self.order_x = self.order_y = self.Gx_norm = self.Gy_norm = None
            self.order_N = int(mn.shape[0])
            if rect_lattice:          # a diagonal lattice keeps the reference's expression: kx, ky bit-identical to the rectangular path
                G = torch.zeros((self.B, 2, 2), dtype=self._cdtype, device=self._device)
                G[:, 0, 0], G[:, 1, 1] = 1 / (Lx * self.freq), 1 / (Ly * self.freq)
            else:
                G = torch.as_tensor(_lat.reciprocal(A), dtype=self._cdtype, device=self._device)[None] / self.freq[:, None, None]
        self.G_norm = G                                                                 # [B, 2, 2]: rows b1 / f, b2 / f
        self.orders = torch.as_tensor(mn, dtype=torch.int64, device=self._device)       # [N, 2] (m, n) of every harmonic, in matrix order
        self._mn = mn
        self._mn_dev = self.orders.to(torch.int32).contiguous()
        self._mmax, self._nmax = int(np.abs(mn[:, 0]).max()), int(np.abs(mn[:, 1]).max())
        if self.symmetry is not None:
            if not rect_lattice:
                raise ValueError(f'symmetry="{self.symmetry}" needs a rectangular lattice (the mirrors x -> -x, y -> -y do not map an oblique lattice onto itself)')
            _sym.check_orders_closed(mn, self.symmetry)
        self._index = {(int(p), int(q)): i for i, (p, q) in enumerate(mn)} if self._general else None
        one = torch.ones(self.B, dtype=self._cdtype, device=self._device)
        self.eps_in, self.mu_in, self.eps_out, self.mu_out = one, one.clone(), one.clone(), one.clone()
        self.has_in = self.has_out = False
        self.layer_N = 0
        for name in _LAYER_FIELDS:
            setattr(self, name, [])

    # ---- helpers -----------------------------------------------------------------------------------------
    def _bvec(self, v, dtype=None):
        """python scalar / 0-d / [B] tensor -> [B] tensor of the compute dtype."""
        dt = dtype if dtype is not None else self._cdtype
        if torch.is_tensor(v):
            t = v.to(device=self._device, dtype=dt)
        else:                      # python scalars / lists: build directly in the target precision (no fp32 detour)
            t = torch.as_tensor(v, dtype=dt, device=self._device)
        if t.dim() == 0:
            t = t.expand(self.B).clone()
        return t.reshape(self.B)

    @property
    def n(self):
        return 2 * self.order_N

    @staticmethod
    def _requires_grad(*values):
        return torch.is_grad_enabled() and any(isinstance(v, (torch.Tensor, _shapes.ShapeLayer)) and v.requires_grad for v in values)

    def _push_layer(self, **fields):
        """Append one layer to every per-layer list: fields[name] where given, None elsewhere."""
        unknown = set(fields) - set(_LAYER_FIELDS)
        if unknown:
            raise KeyError(f"not a per-layer attribute: {sorted(unknown)}")
        for name in _LAYER_FIELDS:
            getattr(self, name).append(fields.get(name))
        self.layer_N += 1

    # ---- a2 / a3 -----------------------------------------------------------------------------------------
    def add_input_layer(self, eps=1., mu=1.):                                           # rcwa.py:95-107
        self.eps_in, self.mu_in, self.has_in = self._bvec(eps), self._bvec(mu), True
        self._sector_S = {}

    def add_output_layer(self, eps=1., mu=1.):                                          # rcwa.py:109-121
        self.eps_out, self.mu_out, self.has_out = self._bvec(eps), self._bvec(mu), True
        self._sector_S = {}

    def set_incident_angle(self, inc_ang, azi_ang, angle_layer="input"):                # rcwa.py:123-144
        self.inc_ang, self.azi_ang = self._bvec(inc_ang), self._bvec(azi_ang)
        if angle_layer in ("i", "in", "input"):
            self.angle_layer = "input"
        elif angle_layer in ("o", "out", "output"):
            self.angle_layer = "output"
        else:
            warnings.warn("Invalid angle layer. Set as input layer.", UserWarning)
            self.angle_layer = "input"
        self._kvectors()
        self._sector_S, self._sector_layer_S = {}, {}
        if self.symmetry is not None:
            # the mirror x -> -x maps kx0 + m Gx onto -(kx0 + m Gx) only for kx0 = 0 (ky0 is free: an angle sweep in the yz plane qualifies)
            bad = torch.stack([(k != 0).any() for k, nm in ((self.kx0_norm, "x"), (self.ky0_norm, "y")) if nm in self.symmetry]).cpu().tolist()
            for flag, nm in zip(bad, [nm for nm in "xy" if nm in self.symmetry]):
                if flag:
                    raise ValueError(f'symmetry="{self.symmetry}": k{nm}0_norm must be exactly 0 at every sweep point for the {nm} mirror '
                                     f"(the incident wave vector must lie in the mirror plane), got max |k{nm}0_norm| = "
                                     f"{float(torch.abs(self.kx0_norm if nm == 'x' else self.ky0_norm).max()):.3g}")

    def _kvectors(self):                                                                # rcwa.py:1124-1181
        em = self.eps_in * self.mu_in if self.angle_layer == "input" else self.eps_out * self.mu_out
        nref = torch.real(torch.sqrt(em))
        self.kx0_norm = nref * torch.sin(self.inc_ang) * torch.cos(self.azi_ang)
        self.ky0_norm = nref * torch.sin(self.inc_ang) * torch.sin(self.azi_ang)
        if self._general:         # k = k0 + m b1 / f + n b2 / f per listed harmonic; kx_norm / ky_norm (the axes of a box) do not exist
            m, n, G = self.orders[None, :, 0], self.orders[None, :, 1], self.G_norm
            self.kx_norm = self.ky_norm = None
            self.Kx_norm_dn = (self.kx0_norm[:, None] + m * G[:, 0, 0, None] + n * G[:, 1, 0, None]).contiguous()
            self.Ky_norm_dn = (self.ky0_norm[:, None] + m * G[:, 0, 1, None] + n * G[:, 1, 1, None]).contiguous()
        else:
            kx = self.kx0_norm[:, None] + self.order_x[None, :] * self.Gx_norm[:, None]     # [B, 2ox+1]
            ky = self.ky0_norm[:, None] + self.order_y[None, :] * self.Gy_norm[:, None]     # [B, 2oy+1]
            self.kx_norm, self.ky_norm = kx, ky
            self.Kx_norm_dn = kx[:, :, None].expand(-1, -1, ky.shape[1]).reshape(self.B, -1).contiguous()   # x-major
            self.Ky_norm_dn = ky[:, None, :].expand(-1, kx.shape[1], -1).reshape(self.B, -1).contiguous()
        kxd, kyd = self.Kx_norm_dn, self.Ky_norm_dn
        self._Vf = _halfspace_V(kxd, kyd, 1.0)
        self._Vfinv = self._Vf.inv()
        self._Sin = self._Sout = None
        if self.has_in:                                                                 # rcwa.py:1149-1164
            self._Vi = _halfspace_V(kxd, kyd, (self.eps_in * self.mu_in)[:, None])
            T = (self._Vf + self._Vi).inv()
            D = self._Vf - self._Vi
            self._Sin = [(T @ self._Vi).scale(2), -(T @ D), T @ D, (T @ self._Vf).scale(2)]
        if self.has_out:                                                                # rcwa.py:1166-1181
            self._Vo = _halfspace_V(kxd, kyd, (self.eps_out * self.mu_out)[:, None])
            T = (self._Vf + self._Vo).inv()
            D = self._Vf - self._Vo
            self._Sout = [(T @ self._Vf).scale(2), T @ D, -(T @ D), (T @ self._Vo).scale(2)]

    # ---- a4-a8 -------------------------------------------------------------------------------------------
    def add_layer(self, thickness, eps=1., mu=1., normal_field=None, *, swept=False):  # rcwa.py:146-170
        """normal_field (fourier_rule="normal" only): (Nx, Ny), each [nx, ny] or [B, nx, ny] on the eps grid, a caller-supplied in-plane field
        for the normal-vector method (e.g. the analytic radial field of a disk), used as given (not normalised) and treated as constant by
        autograd.  None: the field is derived from the eps grid (trx_normal_field, nv_sigma).  With eps a ShapeLayer the grids may have any
        size n1 > 2 mmax, n2 > 2 nmax (at most 2048), sampled at (i / n1) a1 + (j / n2) a2 like ShapeLayer.rasterise; None: the blended field
        of the shape list on shape_nv_grid (trx_shape_normal_field); one tensor [3, n1, n2] or [B, 3, n1, n2] is taken as the
        products (Nx^2, Nx Ny, Ny^2) themselves, as shapes.normal_products returns them.  A supplied field is a constant of the graph; the
        derived one is too unless the solver was built with shape_nv_grad=True (then gradients include the field's dependence on the
        geometry, trx_shape_normal_field_backward).
        swept=True: `thickness` is a sweep axis, [T] (shared by the points) or [B, T].  The layer's modes are computed once, exactly as for a
        plain layer, and solve_S_parameters returns [B, T, len(orders)] (one GEMM and one LU per thickness, include/trx.h:
        trx_thickness_prepare / trx_thickness_columns).  At most one swept layer; needs keep_coupling=False, and a non-differentiable stack
        unless the solver was built with swept_grad=True: then gradients reach the swept thicknesses, the layer's eps / mu, every other layer's
        tensors, freq and the incidence wave vector (one eigenproblem and one eigen-adjoint per point, trx_thickness_columns_backward per
        thickness)."""
        eng, N, B, cdt = self.engine, self.order_N, self.B, self._cdtype
        self._refuse_shapes(eps, mu, normal_field)
        if self.symmetry_sector:
            return self._add_layer_sector(thickness, eps, mu, normal_field, swept)
        if swept:
            self._check_swept()
        eps_h, mu_h = self._is_homogeneous(eps), self._is_homogeneous(mu)
        if normal_field is not None and self.fourier_rule != "normal":
            raise ValueError('add_layer(normal_field=...) needs fourier_rule="normal"')
        if normal_field is not None and eps_h:
            raise ValueError("add_layer(normal_field=...) needs a patterned eps grid")
        eye = torch.eye(N, dtype=cdt, device=self._device)
        # differentiable path (Examples 4-6): every O(n^3) primitive is an autograd.Function over the same HIP kernels
        diff = self._requires_grad(thickness, eps, mu, self.freq, self.Kx_norm_dn, self.Ky_norm_dn)
        self._diff = self._diff or diff
        self._refuse_swept_diff(swept)
        if self.symmetry is not None:
            if self._diff and not self.symmetry_grad:
                raise ValueError("symmetry= is not available on a differentiable stack (a tensor of this layer or an earlier one requires grad): "
                                 "the adjoint of the folded eigenproblem is not implemented for a raw per-pixel gradient; symmetry_grad=True "
                                 "opts in to the gradient of the mirror-constrained problem")
            self._refuse_normal_field(normal_field)
        if eps_h and mu_h and not diff and not self.keep_coupling and not swept:
            self._add_homogeneous_layer_bd(thickness, self._bvec(eps), self._bvec(mu))
            self._fold_last_layer()
            return
        fac, plan = self._factorise(eps, mu, eps_h, mu_h, normal_field, diff, eye)
        keep = self.keep_coupling
        E, mu_s = fac.E, fac.mu_s          # homogeneous mu: V = P^-1 W Kz from the rank-N structure of P (trx_hmodes)
        keep_li = keep and fac.exy is None and fac.exx is not fac.E          # Li's Ex, Ey of a patterned eps
        keep_nv = keep and fac.exy is not None
        rec = dict(eps_conv=E, mu_conv=fac.M,
                   eps_grid=(self._bvec(eps) if eps_h else eps) if keep else None, mu_grid=(self._bvec(mu) if mu_h else mu) if keep else None,
                   eps_conv_x=fac.exx if keep_li else None, eps_conv_y=fac.eyy if keep_li else None,
                   eps_conv_xx=fac.exx if keep_nv else None, eps_conv_xy=fac.exy if keep_nv else None, eps_conv_yy=fac.eyy if keep_nv else None)
        d = self._swept_thickness(thickness) if swept else self._bvec(thickness, self._rdtype)
        kxd, kyd = self.Kx_norm_dn, self.Ky_norm_dn
        inv = (lambda A: ag.InverseFn.apply(A, eng)) if diff else eng.inverse
        if fac.Einv is None:
            fac = fac._replace(Einv=inv(fac.E))
        if fac.Minv is None and fac.M is not None:
            fac = fac._replace(Minv=inv(fac.M))
        P, Q = self._pq(fac, diff)
        resid = None
        if eps_h and mu_h:                                                              # rcwa.py:1206-1222
            W = torch.eye(2 * N, dtype=cdt, device=self._device).expand(B, -1, -1).contiguous()
            kz = _kz_branch(torch.sqrt((fac.eps_s * mu_s)[:, None] - kxd ** 2 - kyd ** 2))
            kz = torch.cat((kz, kz), dim=1)
        else:                                                                           # rcwa.py:1224-1242
            if diff:
                Eig.engine = eng
                A = ag.GemmFn.apply(P, Q, eng)
                # stable_eig_grad=False is the reference's plain torch.linalg.eig branch (rcwa.py:1238): its backward is never
                # broadened.  The choice is bound to this graph node (not to the process-global at backward time).
                eig = Eig.apply if self.stable_eig_grad else (lambda M: Eig.apply(M, Eig.UNBROADENED))
                if plan is None:
                    lam, W = eig(A)
                else:
                    lam, W, resid = self._eig_folded_diff(A, plan, eig)
            else:
                A = self._a(fac, P, Q)
                # the factorised medium dies here, before the eigensolver's peak: E, M live on in eps_conv / mu_conv, Li's / the
                # normal-vector matrices only in eps_conv_x / _y / _xx / _xy / _yy (keep_coupling)
                del fac
                # mixed-precision eigensolver: two Newton steps for a complex64 problem (1e-5 gate), three for complex128 (engine.eig)
                steps = 3 if self._dtype == torch.complex128 else 2
                if plan is None:
                    lam, W = self._eig_call(A, refine_steps=steps)                          # torch_eig.py:14
                else:
                    lam, W, resid = self._eig_folded(A, plan, steps)
                del A
            kz = _kz_branch(torch.sqrt(lam), negate=True)                               # rcwa.py:1241
        if swept:
            V = self._keep_swept_modes(P, W, kz, mu_s, E, diff)
            self._push_layer(P=P, Q=Q, kz_norm=kz, E_eigvec=W, H_eigvec=V, symmetry_residual=resid, **rec)
            self._swept = dict(index=self.layer_N - 1, d=d)
            if self.fold_layers:              # as a folded layer: the matrices the modes came from are not read again
                self._drop_layer_matrices(self.layer_N - 1, modes=True)
            return
        S11, S21, V, cp, cm, W_kept = (self._solve_layer_smatrix_diff if diff else self._solve_layer_smatrix)(P, Q, W, kz, d, mu_s, E)
        self._push_layer(thickness=d, P=P, Q=Q, kz_norm=kz, E_eigvec=W_kept, H_eigvec=V, Cplus=cp, Cminus=cm, layer_S11=S11, layer_S21=S21,
                         symmetry_residual=resid, **rec)
        self._fold_last_layer()

    def _refuse_shapes(self, eps, mu, normal_field):
        """What a ShapeLayer cannot be combined with, each refused by name (DESIGN.md section 8 lists them as follow-ups)."""
        if isinstance(mu, _shapes.ShapeLayer):
            raise ValueError("a ShapeLayer cannot be given as mu: vector shapes describe the permittivity only")
        if not isinstance(eps, _shapes.ShapeLayer):
            return
        if self.fourier_rule == "li":
            # Li's rule has a closed form for axis-aligned rectangles only (trx_convmat_li_shapes): strips of piecewise constant 1/eps
            names = {_shapes.ELLIPSE: "an ellipse", _shapes.POLYGON: "a polygon"}
            for i, s in enumerate(eps.shapes):
                what = names.get(s.kind)
                if what is None and s.params[4].requires_grad:
                    what = "a rectangle whose theta requires grad"
                elif what is None and bool((s.params[4].detach() != 0).any()):
                    what = "a rotated rectangle"
                if what is not None:
                    raise ValueError('a ShapeLayer needs fourier_rule="laurent" or "normal", got \'li\': the per-row inverses of Li\'s rule are built '
                                     f"from grids, and in closed form only for axis-aligned rectangles (theta identically 0); shape {i} is {what} "
                                     '-- fourier_rule="normal" takes any shape')
            for i, t in enumerate([eps.background] + [s.eps for s in eps.shapes]):
                if not bool(torch.isfinite(t.detach()).all()):      # 1/eps = 0: trx_convmat_li_shapes sees sums of rval only and cannot tell
                    raise ValueError('a ShapeLayer under fourier_rule="li" needs finite permittivities: '
                                     f'{"the background" if i == 0 else f"shape {i - 1}"} has a medium with 1/eps = 0')
        if self.symmetry is not None or self.symmetry_sector:
            raise ValueError("a ShapeLayer cannot be combined with symmetry= / symmetry_sector=True: the mirror is detected from grids")
        if self.fourier_rule == "normal" and self.shape_nv_grid is None and normal_field is None:
            # opt-in: a solver built without a field grid keeps refusing shapes under this rule, as it did before the rule reached them
            raise ValueError('a ShapeLayer needs fourier_rule="laurent", or under fourier_rule="normal" a grid for the products of its normal '
                             f"field: shape_nv_grid= (an int or (n1, n2); {SHAPE_NV_GRID_DEFAULT} is the measured choice, SHAPE_NV_GRID_DEFAULT) "
                             "or add_layer(normal_field=...)")

    def _refuse_normal_field(self, normal_field):
        if normal_field is not None:
            raise ValueError("symmetry= cannot be combined with add_layer(normal_field=...): a caller-supplied field is not checked for the mirror; "
                             "let the field be derived from the grid")

    def _grid(self, v):
        """eps / mu grid [nx, ny] or [B, nx, ny] -> contiguous [B, nx, ny] on the device."""
        g = torch.as_tensor(v, device=self._device)
        if g.dim() == 2:
            g = g[None].expand(self.B, -1, -1)
        return g.contiguous()

    def _factorise(self, eps, mu, eps_h, mu_h, normal_field, diff, eye):
        """(Medium, plan): the convolution matrices of a layer under this solver's Fourier rule, and its symmetry folding plan (None without
        symmetry=; a grid without the claimed mirror raises here, before the per-component matrices are built).  eye: the N x N identity.
        Sweep drivers (keep_coupling=False) with a homogeneous mu never read P, Q, the dense mu matrices or, after the layer's S-matrix, the
        mode matrices W, V: A = PQ and V = P^-1 W Kz come from E directly (trx_build_a / trx_hmodes).  Not building / not keeping them takes
        4 of ~16 n^2-sized tensors per sweep point out of the peak: M = Minv = None in the record of such a layer."""
        eng, cdt = self.engine, self._cdtype

        def conv(v, homog):
            if homog:
                s = self._bvec(v)
                return s[:, None, None] * eye, (1 / s)[:, None, None] * eye, s
            if isinstance(v, _shapes.ShapeLayer):      # closed-form coefficients; the rectangle of `order` and an order list both as mn
                packed = v.pack(self._lattice, self.B, self._device)
                if diff:
                    return ag.ShapeConvFn.apply(packed.par, packed.val, packed, self._mn_dev, self._mmax, self._nmax, cdt, eng), None, None
                return eng.convmat_shapes(packed, self._mn_dev, cdt, self._mmax, self._nmax), None, None
            g = self._grid(v)
            if self._general:
                if diff:
                    return ag.ConvMatOrdersFn.apply(g, self.orders, cdt, eng), None, None
                return eng.convmat_orders(g, self._mn_dev, cdt, self._mmax, self._nmax), None, None
            if diff:
                return ag.ConvMatFn.apply(g, self.order[0], self.order[1], cdt, eng), None, None
            C = eng.convmat(g, self.order[0], self.order[1], cdt)                       # rcwa.py:1183-1204
            return C, None, None

        def conv_li(v, homog, C):
            """Li's (Cx, Cy) of a patterned grid or of a ShapeLayer of axis-aligned rectangles; a homogeneous layer has Cx = Cy = C (the scaled
            identity)."""
            if homog:
                return C, C
            if isinstance(v, _shapes.ShapeLayer):      # axis-aligned rectangles (_refuse_shapes): strips in closed form, no grid
                packed = v.pack(self._lattice, self.B, self._device)
                rval = v.reciprocal_values(self.B, self._device)
                Lx, Ly = float(self._Lxy[0]), float(self._Lxy[1])
                if diff:
                    return ag.ShapeLiFn.apply(packed.par, rval, packed, Lx, Ly, self.order[0], self.order[1], cdt, eng)
                return eng.convmat_li_shapes(packed, rval, Lx, Ly, self.order[0], self.order[1], cdt)
            g = self._grid(v)
            if diff:
                return ag.ConvMatLiFn.apply(g, self.order[0], self.order[1], cdt, eng)
            return eng.convmat_li(g, self.order[0], self.order[1], cdt)[:2]

        def conv_nv(v):
            """(Exx, Exy, Eyy) of a patterned eps grid with the normal-vector rule."""
            if isinstance(v, _shapes.ShapeLayer):      # closed-form [eps], [1/eps]; only the field's products are sampled (both lattice paths)
                packed = v.pack(self._lattice, self.B, self._device)
                rval = v.reciprocal_values(self.B, self._device)
                nn, (n1, n2) = self._shape_nv_products(normal_field)
                if diff:
                    if nn is None and self.shape_nv_grad:      # the derived field carries its dependence on the parameters
                        nn = ag.ShapeNormalFieldFn.apply(packed.par, packed, self._lattice, n1, n2, eng)
                    elif nn is None:           # the field derived from the shape list is a constant of the differentiable path (detached)
                        nn = eng.shape_normal_field(packed, self._lattice, n1, n2)
                    return self._nv_tensor_shapes_torch(packed, rval, nn)
                return eng.convmat_nv_shapes(packed, rval, self._lattice, self._mn_dev, cdt, n1, n2, nn=nn, mmax=self._mmax, nmax=self._nmax)
            g = self._grid(v)
            nn = self._nv_products(g, normal_field)
            if self._general:
                h = self._nv_spacing(g)
                if diff:
                    if nn is None:
                        nn = eng.normal_field_lattice(g.detach(), self.nv_sigma, h)
                    return self._nv_tensor_torch(g, nn)
                return eng.convmat_nv_orders(g, self._mn_dev, cdt, sigma=self.nv_sigma, h=h, nn=nn, mmax=self._mmax, nmax=self._nmax)
            hx, hy = self._nv_spacing(g)
            if diff:
                if nn is None:                 # the field derived from the grid is a constant of the differentiable path (detached)
                    nn = eng.normal_field(g.detach(), self.nv_sigma, hx, hy)
                return self._nv_tensor_torch(g, nn)
            return eng.convmat_nv(g, self.order[0], self.order[1], cdt, sigma=self.nv_sigma, hx=hx, hy=hy, nn=nn)

        lean = ((not diff) and (not self.keep_coupling) and mu_h and (not eps_h) and (not self.avoid_Pinv_instability)
                and not self.symmetry_sector)                               # a sector layer folds the finished P, Q
        E, Einv, eps_s = conv(eps, eps_h)
        if lean:
            M, Minv, mu_s = None, None, self._bvec(mu)
        else:
            M, Minv, mu_s = conv(mu, mu_h)
        plan = None
        if self.symmetry is not None and not (eps_h and mu_h):          # before any heavy work: a grid without the mirror raises here
            plan = self._sym_plan([torch.as_tensor(v, device=self._device).detach() for v, h in ((eps, eps_h), (mu, mu_h)) if not h])
        exx, exy, eyy, mx, my = E, None, E, M, M
        if self.fourier_rule == "li" and not (eps_h and mu_h):
            exx, eyy = conv_li(eps, eps_h, E)
            if M is not None:
                mx, my = conv_li(mu, mu_h, M)
        elif self.fourier_rule == "normal" and not eps_h:      # a homogeneous eps has the tensor eps I: Laurent's matrices as they are
            exx, exy, eyy = conv_nv(eps)
        return Medium(E, Einv, M, Minv, eps_s, mu_s, exx, exy, eyy, mx, my), plan

    def _pq(self, fac, diff):
        """P, Q of a layer (rcwa.py:1226-1232) from its Medium, through the entry of its rule; (None, None) for a lean layer."""
        kxd, kyd = self.Kx_norm_dn, self.Ky_norm_dn
        if diff:
            return self._pq_torch(fac.E, fac.Einv, fac.M, fac.Minv, kxd, kyd, fac.exx, fac.eyy, fac.mx, fac.my, fac.exy)
        if fac.M is None:
            return None, None
        eng = self.engine
        if fac.exy is not None:
            return eng.build_pq_tensor(fac.exx, fac.exy, fac.eyy, fac.Einv, fac.M, fac.Minv, kxd, kyd)
        if fac.exx is not fac.E or fac.mx is not fac.M:
            return eng.build_pq_aniso(fac.exx, fac.eyy, fac.Einv, fac.mx, fac.my, fac.Minv, kxd, kyd)
        return eng.build_pq(fac.E, fac.Einv, fac.M, fac.Minv, kxd, kyd)

    def _a(self, fac, P, Q):
        """A = P Q (rcwa.py:1236): with a homogeneous mu the block structure needs two N^3 products, not one (2N)^3."""
        eng, kxd, kyd = self.engine, self.Kx_norm_dn, self.Ky_norm_dn
        if fac.mu_s is None:
            return eng.gemm(P, Q)
        if fac.exy is not None:
            return eng.build_a_tensor(fac.exx, fac.exy, fac.eyy, fac.Einv, fac.mu_s, kxd, kyd)
        if fac.exx is not fac.E:
            return eng.build_a_aniso(fac.exx, fac.eyy, fac.Einv, fac.mu_s, kxd, kyd)
        return eng.build_a(fac.E, fac.Einv, fac.mu_s, kxd, kyd)

    def _drop_layer_matrices(self, i, modes=False):
        """The convolution matrices of a folded layer are not read again; modes: nor are the P, Q its modes came from (the swept layer)."""
        for name in _CONV_FIELDS + (("P", "Q") if modes else ()):
            getattr(self, name)[i] = None

    def _pack_bd(self, S):
        """Four BlockDiag2 blocks -> [4,4,B,N] diagonals in the compute dtype, as the library takes a block-diagonal S-matrix."""
        return torch.stack([torch.stack(blk.d, dim=0) for blk in S], dim=0).to(self._cdtype).contiguous()

    def _fold_last_layer(self):
        """Streaming cascade: fold the layer just added into the running star product and drop it.  Decided PER LAYER: a layer is folded
        only while the stack so far is a plain (non-differentiable) prefix 0 .. i-1 that has itself been folded; from the first
        differentiable layer on, layers stay stored and solve_global_smatrix continues the cascade from the folded prefix over them
        (a global early return here used to leave such layers out of the cascade altogether).  Right of the swept layer: the same
        streaming cascade into a product of its own."""
        i = self.layer_N - 1
        right = self._swept is not None and i > self._swept["index"]
        if right:
            ready = self._n_right_folded == i - self._swept["index"] - 1
        else:
            ready = not self._diff and self._n_folded == i
        if not (self.fold_layers and ready):
            return
        S, run = self._layer_S(i), self._right_running if right else self._running
        if run is not None:
            S = self._star(run, S, [[], []], [[], []])[0]
        if right:
            self._right_running, self._n_right_folded = S, self._n_right_folded + 1
        else:
            self._running, self._n_folded = S, i + 1
        self.layer_S11[i] = self.layer_S21[i] = None
        self._drop_layer_matrices(i)

    def _add_homogeneous_layer_bd(self, thickness, eps_s, mu_s):
        """Homogeneous layer without field bookkeeping (keep_coupling=False): every operator of rcwa.py:1206-1222 and 1244-1281
        is 2x2-block-diagonal (W = I, V = P^-1 Kz = Q Kz^-1 in closed form), so the layer S-matrix is four [B,N] diagonals per
        block and costs O(N) instead of the dense eigen/LU path; the cascade then uses the half-space star product.  The dense
        per-layer attributes (P, Q, E_eigvec, H_eigvec, eps_conv, mu_conv) are not materialised for such a layer (None)."""
        kxd, kyd = self.Kx_norm_dn, self.Ky_norm_dn
        d = self._bvec(thickness, self._rdtype)
        epsmu = (eps_s * mu_s)[:, None]
        kz = _kz_branch(torch.sqrt(epsmu - kxd ** 2 - kyd ** 2))                        # rcwa.py:1218
        x = torch.exp(1j * (self.omega * d)[:, None] * kz)                              # rcwa.py:1246, [B,N] (same for both field components)
        V = _halfspace_V(kxd, kyd, epsmu).scale(1 / mu_s[:, None])                      # Q Kz^-1 = P^-1 Kz
        I = BlockDiag2.identity_like(kz)
        F = self._Vfinv @ V
        A_, B_ = I + F, (I - F).scale(x)
        Tip, Tim = (A_ + B_).inv(), (A_ - B_).inv()
        cp, cm = Tip + Tim, Tip - Tim
        self._push_layer(thickness=d, kz_norm=torch.cat((kz, kz), dim=1),
                         layer_S11=cp.scale(x) + cm,                                    # rcwa.py:1276 with W = I
                         layer_S21=cp + cm.scale(x) - I)                                # rcwa.py:1277

    def _nv_spacing(self, g):
        """Grid spacings (hx, hy) of a [B, nx, ny] grid over the unit cell: they orient the gradient of the normal-vector field.  On the
        general path the cell matrix instead: [2, 2], rows a1 / n1 and a2 / n2 (include/trx.h: trx_normal_field_lattice)."""
        if self._general:
            return self._lattice / np.array([[g.shape[1]], [g.shape[2]]], dtype=np.float64)
        return float(self._Lxy[0]) / g.shape[1], float(self._Lxy[1]) / g.shape[2]

    def _nv_products(self, g, normal_field):
        """[B,3,nx,ny] float64 (Nx^2, Nx Ny, Ny^2): from a caller-supplied field, or None (the library derives it from the grid)."""
        if normal_field is None:
            return None
        Nx, Ny = (torch.as_tensor(t, device=self._device).detach().to(torch.float64) for t in normal_field)
        shp = tuple(g.shape[1:])
        if tuple(Nx.shape[-2:]) != shp or tuple(Ny.shape[-2:]) != shp:
            raise ValueError(f"normal_field components must be {list(shp)} grids like eps, got {list(Nx.shape)} and {list(Ny.shape)}")
        Nx, Ny = Nx.expand(self.B, -1, -1), Ny.expand(self.B, -1, -1)
        return torch.stack((Nx * Nx, Nx * Ny, Ny * Ny), dim=1).contiguous()

    def _shape_nv_products(self, normal_field):
        """(nn, (n1, n2)) for a ShapeLayer: the [B,3,n1,n2] float64 products of a caller-supplied field on its own grid, or None and
        shape_nv_grid (the library samples the field of the shape list).  ValueError for a grid the order set does not fit on."""
        def fits(n1, n2, factor, what):
            if n1 <= factor * self._mmax or n2 <= factor * self._nmax or max(n1, n2) > 2048:
                raise ValueError(f"{what} ({n1}, {n2}) is too small for the order set: it needs n1 > {factor * self._mmax}, n2 > "
                                 f"{factor * self._nmax} ({factor} x the largest |m|, |n|) and at most 2048 points a side")
        if normal_field is None:
            # the box of the products reaches +-2 mmax: on fewer than 4 mmax + 1 points its outer coefficients would alias
            fits(*self.shape_nv_grid, 4, "shape_nv_grid")
            return None, self.shape_nv_grid
        if torch.is_tensor(normal_field):             # the products themselves, as shapes.normal_products returns them
            nn = normal_field.detach().to(device=self._device, dtype=torch.float64)
            if nn.dim() not in (3, 4) or nn.shape[-3] != 3 or (nn.dim() == 4 and nn.shape[0] != self.B):
                raise ValueError(f"normal_field products of a ShapeLayer must be [3, n1, n2] or [{self.B}, 3, n1, n2], got {list(nn.shape)}")
            fits(int(nn.shape[-2]), int(nn.shape[-1]), 2, "the normal_field grid")
            return nn.expand(self.B, -1, -1, -1).contiguous(), (int(nn.shape[-2]), int(nn.shape[-1]))
        if len(normal_field) != 2:
            raise ValueError("normal_field is (Nx, Ny)")
        Nx, Ny = (torch.as_tensor(t, device=self._device).detach().to(torch.float64) for t in normal_field)
        if Nx.dim() not in (2, 3) or Nx.shape != Ny.shape or (Nx.dim() == 3 and Nx.shape[0] != self.B):
            raise ValueError(f"normal_field components of a ShapeLayer must be two [n1, n2] or [{self.B}, n1, n2] grids of one size, got "
                             f"{list(Nx.shape)} and {list(Ny.shape)}")
        n1, n2 = int(Nx.shape[-2]), int(Nx.shape[-1])
        fits(n1, n2, 2, "the normal_field grid")         # the bound of trx_convmat_orders, as for a grid layer
        Nx, Ny = Nx.expand(self.B, -1, -1), Ny.expand(self.B, -1, -1)
        return torch.stack((Nx * Nx, Nx * Ny, Ny * Ny), dim=1).contiguous(), (n1, n2)

    def _nv_tensor_shapes_torch(self, packed, rval, nn):
        """(Exx, Exy, Eyy) of a ShapeLayer from the differentiable primitives: ShapeConvFn of the values and of the reciprocal values,
        InverseFn, GemmFn.  Field products nn that carry no graph are constants (the gradient is the derivative at a fixed field, INTEGRATION.md
        section A); those of ShapeNormalFieldFn (shape_nv_grad=True) pass their gradient on through FieldConvFn and GemmFn's second operand."""
        eng, cdt, B = self.engine, self._cdtype, self.B
        conv_d = lambda val: ag.ShapeConvFn.apply(packed.par, val, packed, self._mn_dev, self._mmax, self._nmax, cdt, eng)
        E = conv_d(packed.val)
        D = E - ag.InverseFn.apply(conv_d(rval), eng)
        if nn.requires_grad:
            C = ag.FieldConvFn.apply(nn.reshape(3 * B, *nn.shape[2:]), self._mn_dev, self._mmax, self._nmax, cdt, eng)
        else:
            C = eng.convmat_orders(nn.reshape(3 * B, *nn.shape[2:]), self._mn_dev, cdt, self._mmax, self._nmax)
        C = C.reshape(B, 3, E.shape[1], E.shape[2])
        DC = [0.5 * (ag.GemmFn.apply(D, C[:, c].contiguous(), eng) + ag.GemmFn.apply(C[:, c].contiguous(), D, eng)) for c in range(3)]
        return E - DC[0], -DC[1], E - DC[2]

    def _nv_tensor_torch(self, g, nn):
        """(Exx, Exy, Eyy) from the differentiable primitives: ConvMatFn of eps and 1/eps, InverseFn, GemmFn (the symmetrised products
        (D C + C D) / 2 of include/trx.h: trx_convmat_nv); the field products nn are constants."""
        eng, cdt = self.engine, self._cdtype
        B = g.shape[0]
        if self._general:         # ConvMatOrdersFn / convmat_orders of the order list in place of the rectangle's
            conv_d = lambda x: ag.ConvMatOrdersFn.apply(x, self.orders, cdt, eng)
            conv_c = lambda x: eng.convmat_orders(x, self._mn_dev, cdt, self._mmax, self._nmax)
        else:
            ox, oy = self.order
            conv_d = lambda x: ag.ConvMatFn.apply(x, ox, oy, cdt, eng)
            conv_c = lambda x: eng.convmat(x, ox, oy, cdt)
        E = conv_d(g)
        D = E - ag.InverseFn.apply(conv_d((1 / g).contiguous()), eng)
        C = conv_c(nn.reshape(3 * B, *nn.shape[2:])).reshape(B, 3, E.shape[1], E.shape[2])
        DC = [0.5 * (ag.GemmFn.apply(D, C[:, c].contiguous(), eng) + ag.GemmFn.apply(C[:, c].contiguous(), D, eng)) for c in range(3)]
        return E - DC[0], -DC[1], E - DC[2]

    @staticmethod
    def _pq_torch(E, Ei, M, Mi, kx, ky, Ex=None, Ey=None, Mx=None, My=None, Exy=None):
        """P, Q (rcwa.py:1226-1232) with broadcasting instead of dense diagonal products (differentiable).  Ex, Ey, Mx, My: Li's
        per-component matrices (default: the Laurent E, M in both places); with Exy, (Ex, Exy, Ey) is the normal-vector tensor
        (Exx, Exy = Eyx, Eyy) and Q gains its off-diagonal blocks."""
        Ex, Ey = (E, E) if Ex is None else (Ex, Ey)
        Mx, My = (M, M) if Mx is None else (Mx, My)
        kxi, kyi, kxj, kyj = kx[:, :, None], ky[:, :, None], kx[:, None, :], ky[:, None, :]
        P = torch.cat((torch.cat((kxi * Ei * kyj, My - kxi * Ei * kxj), dim=2),
                       torch.cat((kyi * Ei * kyj - Mx, -(kyi * Ei * kxj)), dim=2)), dim=1)
        Q = torch.cat((torch.cat((-(kxi * Mi * kyj), kxi * Mi * kxj - Ey), dim=2),
                       torch.cat((Ex - kyi * Mi * kyj, kyi * Mi * kxj), dim=2)), dim=1)
        if Exy is not None:
            Q = Q + torch.cat((torch.cat((-Exy, torch.zeros_like(Exy)), dim=2), torch.cat((torch.zeros_like(Exy), Exy), dim=2)), dim=1)
        return P, Q

    def _solve_layer_smatrix_diff(self, P, Q, W, kz, d, mu_s, E):
        """Layer S-matrix (rcwa.py:1244-1281) from differentiable primitives; same lean algebra as trx_layer_smatrix.  Arguments and
        return value as _solve_layer_smatrix (mu_s and E are not read: this path always solves with P)."""
        eng, n = self.engine, self.n
        X = torch.exp(1j * (self.omega * d)[:, None] * kz)                              # [B, n]
        WKz = W * kz[:, None, :]
        bad = None
        if self.avoid_Pinv_instability:                                                 # rcwa.py:1249-1262 (metrics are detached diagnostics)
            with torch.no_grad():
                Pd, Qd = P.detach(), Q.detach()
                I = torch.eye(n, dtype=self._cdtype, device=self._device)
                Pinv = eng.inverse(Pd)
                ins = torch.maximum(torch.amax(torch.abs(eng.gemm(Pd, Pinv) - I), dim=(1, 2)),
                                    torch.amax(torch.abs(eng.gemm(Pinv, Pd) - I), dim=(1, 2)))
                qins = torch.amax(torch.abs(eng.gemm(Qd, eng.inverse(Qd)) - I), dim=(1, 2))
            self.Pinv_instability.append(ins)
            self.Qinv_instability.append(qins)
            bad = ins >= self.max_Pinv_instability
            bad = bad if bool(bad.any()) else None
        if bad is None:
            V = ag.SolveFn.apply(P, WKz, eng)                                           # P^-1 W Kz
        else:
            # V = Q W Kz^-1 for the ill-conditioned points.  The reference routes the graph of such a point through that branch only;
            # in a batch both branches are evaluated, so the discarded P-solve of a bad point must not be able to produce Inf / NaN
            # (0 * NaN in SolveFn.backward would poison the gradient of every point): those points solve with the identity instead
            sel = bad[:, None, None]
            I = torch.eye(n, dtype=self._cdtype, device=self._device)
            V = torch.where(sel, ag.GemmFn.apply(Q, (W / kz[:, None, :]).contiguous(), eng),
                            ag.SolveFn.apply(torch.where(sel, I, P), WKz, eng))
        F = self._Vfinv.apply(V)                                                        # Vf^-1 V
        A_, B_ = W + F, (W - F) * X[:, None, :]
        Tip, Tim = ag.InverseFn.apply(A_ + B_, eng), ag.InverseFn.apply(A_ - B_, eng)
        cp, cm = Tip + Tim, Tip - Tim
        I = torch.eye(n, dtype=self._cdtype, device=self._device)
        S11 = ag.GemmFn.apply(W, X[:, :, None] * cp + cm, eng)
        S21 = ag.GemmFn.apply(W, cp + X[:, :, None] * cm, eng) - I
        return S11, S21, V, cp, cm, W

    def _RS_prod_diff(self, Sm, Sn, Cm, Cn):
        """Star product (rcwa.py:1283-1306) from differentiable primitives (one factorisation, push-through identity).  The size comes from
        the operand: the blocks of a sector (sector.py) are about n / 4."""
        eng, n = self.engine, Sm[0].shape[-1]
        I = torch.eye(n, dtype=self._cdtype, device=self._device)
        mm = lambda a, b: ag.GemmFn.apply(a.contiguous(), b.contiguous(), eng)
        K = I - mm(Sm[2], Sn[1])
        X12 = ag.SolveFn.apply(K, torch.cat((Sm[0], mm(Sm[2], Sn[3])), dim=2).contiguous(), eng)
        X1, X2 = X12[:, :, :n], X12[:, :, n:]
        Y1, Y2 = mm(Sn[1], X1), Sn[3] + mm(Sn[1], X2)
        S = [mm(Sn[0], X1), Sm[1] + mm(Sm[3], Y1), Sn[2] + mm(Sn[0], X2), mm(Sm[3], Y2)]
        return S, _propagate_coupling(mm, Cm, Cn, X1, X2, Y1, Y2)

    def _eig_call(self, A, refine_steps, out=None):
        """trx_eig with this solver's route policy.  "fp64" / "mixed": as named.  "auto": the library's mixed-precision route, and -- scoped to THIS
        solver object (or to the one sweep call whose chunks share `route_hint`), never beyond -- once a call had to redo matrices in fp64
        (clusters of close eigenvalues beyond the refinement's exact treatment: symmetric meta-atoms, the dense spectra of large orders), the
        following eigenproblems of the same size go to the all-fp64 route directly instead of paying for another failed attempt.  The hint is
        created with the solver / sweep call and dies with it: results never depend on what the process solved before."""
        eng = self.engine
        key = int(A.shape[-1])
        route = {"auto": 0, "mixed": 3, "fp64": 1}[self.eig_route]
        if self.eig_route == "auto" and self._route_hint.get(key):
            route = 1
        lam, W = eng.eig(A, destroy=True, refine_steps=refine_steps, route=route, **({} if out is None else {"out": out}))
        if self.eig_route == "auto" and route == 0 and eng.eig_fallback_of_last_call() > 0:
            self._route_hint[key] = True
        return lam, W

    def _sym_plan(self, grids):
        """The folding plan of a patterned layer: the centre c of every claimed mirror is detected from the layer's grids (ValueError if a grid
        does not have the mirror), and the plan of (c, grid size) is built once per solver."""
        key = _sym.grid_centres(grids, self.symmetry, self.symmetry_tol)
        if self.symmetry_sector:
            if self._sector_centres is None:
                self._sector_centres = key
            elif key != self._sector_centres:
                raise ValueError(f'symmetry_sector=True: the mirror planes of this layer, (cx, nx, cy, ny) = {key}, differ from those of the first '
                                 f"patterned layer, {self._sector_centres}: the sector cascade needs one symmetry basis for the whole stack "
                                 "(sample every grid about the same centre)")
        if key not in self._sym_plans:
            self._sym_plans[key] = _sym.build_plan(self._mn, self.symmetry, *key)
        return self._sym_plans[key]

    def _eig_folded(self, A, plan, refine_steps):
        """(lam, W, resid) of A through its symmetry blocks: fold, one trx_eig call per distinct block size (the route hint is keyed by size),
        unfold into the original basis."""
        eng = self.engine
        blocks, resid = eng.sym_fold(A, plan)
        Wp, lp, Wk, lamk = eng.sym_packed(plan, A.shape[0], A.dtype)       # trx_eig writes straight into the buffers trx_sym_unfold reads
        for Bk, wk, lk in zip(blocks, Wk, lamk):
            if Bk.shape[-1] > 0:
                self._eig_call(Bk, refine_steps=refine_steps, out=(lk, wk))
        del blocks
        lam, W = eng.sym_unfold(Wp, lp, plan)
        return lam, W, resid

    def _eig_folded_diff(self, A, plan, eig):
        """_eig_folded for a differentiable A: every step is an autograd.Function over the HIP kernels (trx_sym_fold / _backward, Eig per
        distinct block size, trx_sym_unfold / _backward).  resid carries no gradient."""
        eng = self.engine
        *blocks, resid = ag.SymFoldFn.apply(A, plan, eng)
        pairs = [eig(Bk) if Bk.shape[-1] > 0 else (Bk.new_empty(Bk.shape[:2]), Bk) for Bk in blocks]
        lam, W = ag.SymUnfoldFn.apply(plan, eng, *[p[1] for p in pairs], *[p[0] for p in pairs])
        return lam, W, resid


    def _is_homogeneous(self, v):
        if isinstance(v, (float, complex)):
            return True
        if isinstance(v, _shapes.ShapeLayer):
            return False
        if isinstance(v, int):                     # the reference raises AttributeError here (rcwa.py:156)
            raise AttributeError("'int' object has no attribute 'dim'")
        t = torch.as_tensor(v)
        # rcwa.py:156-157: a 0-d tensor or a 1-D tensor of length 1.  Batched extension: a 1-D tensor of length B is one homogeneous value per
        # sweep point; any other 1-D tensor is NOT homogeneous, exactly as in the reference (it then fails in the grid path like there).
        return t.dim() == 0 or (t.dim() == 1 and t.shape[0] in (1, self.B))

    def _solve_layer_smatrix(self, P, Q, W, kz, d, mu_s, E):                            # rcwa.py:1244-1281
        """(S11, S21, V, c+, c-, W) of a layer of thickness d [B] from its modes W, kz and P (or Q where P is ill-conditioned:
        avoid_Pinv_instability); with a homogeneous mu, mu_s [B], V comes from E instead (trx_hmodes; P, Q may be None then).  The W that
        comes back is the one to store: None, like V, where the sweep drivers do not read the mode matrices again."""
        eng = self.engine
        phase = torch.exp(1j * (self.omega * d)[:, None] * kz)                          # rcwa.py:1246
        vfinv = self._Vfinv.packed(self._cdtype)                                        # [4,B,N]
        if not self.avoid_Pinv_instability:
            if mu_s is not None:                                                        # rcwa.py:1264, structured (include/trx.h: trx_hmodes)
                Vh = eng.hmodes(E, mu_s, self.Kx_norm_dn, self.Ky_norm_dn, W, kz)
                S11, S21, V, cp, cm = eng.layer_smatrix(None, None, W, kz, vfinv, phase, want_c=self.keep_coupling, V=Vh)
            else:
                S11, S21, V, cp, cm = eng.layer_smatrix(P, None, W, kz, vfinv, phase, use_q=False, want_c=self.keep_coupling)
        else:                                                                           # rcwa.py:1249-1262
            n = self.n
            I = torch.eye(n, dtype=self._cdtype, device=self._device)
            Pinv = eng.inverse(P)
            ins1 = torch.amax(torch.abs(eng.gemm(P, Pinv) - I), dim=(1, 2))
            ins2 = torch.amax(torch.abs(eng.gemm(Pinv, P) - I), dim=(1, 2))
            qins = torch.amax(torch.abs(eng.gemm(Q, eng.inverse(Q)) - I), dim=(1, 2))   # computed twice in the reference
            self.Pinv_instability.append(torch.maximum(ins1, ins2))
            self.Qinv_instability.append(qins)
            bad = self.Pinv_instability[-1] >= self.max_Pinv_instability
            S11, S21, V, cp, cm = eng.layer_smatrix(P, None, W, kz, vfinv, phase, use_q=False, want_c=self.keep_coupling)
            if bool(bad.any()):
                alt = eng.layer_smatrix(None, Q, W, 1 / kz, vfinv, phase, use_q=True, want_c=self.keep_coupling)
                sel = bad[:, None, None]
                S11, S21, V = torch.where(sel, alt[0], S11), torch.where(sel, alt[1], S21), torch.where(sel, alt[2], V)
                if self.keep_coupling:
                    cp, cm = torch.where(sel, alt[3], cp), torch.where(sel, alt[4], cm)
        if not self.keep_coupling and not self.avoid_Pinv_instability and mu_s is not None:
            W = V = None                      # sweep drivers: the mode matrices are not read again (see _factorise)
        return S11, S21, V, cp, cm, W

    # ---- a9 / a10 ----------------------------------------------------------------------------------------
    def _RS_prod(self, Sm, Sn, Cm, Cn):                                                 # rcwa.py:1283-1306
        if self._diff:
            return self._RS_prod_diff(Sm, Sn, Cm, Cn)
        S, X1, X2, Y1, Y2 = self.engine.redheffer(Sm, Sn)
        return S, _propagate_coupling(self._mm_plain, Cm, Cn, X1, X2, Y1, Y2)

    def _mm_plain(self, a, b):
        return self.engine.gemm(a, b.contiguous())

    def _RS_halfspace(self, side, Sbd, S, C):
        """Star product with Sin (side 0) / Sout (side 1), whose blocks are 2x2-block-diagonal: O(n^2) products with them.  C: the lists
        of the dense operand -- the right one for side 0 (rcwa.py:1302-1304), the left one for side 1 (rcwa.py:1298-1300)."""
        none = [[], []]
        Cm, Cn = (none, C) if side == 0 else (C, none)
        if self._diff:
            dense = [blk.dense().to(self._cdtype) for blk in Sbd]
            return self._RS_prod_diff(dense, S, Cm, Cn) if side == 0 else self._RS_prod_diff(S, dense, Cm, Cn)
        Sn, X1, X2, Y1, Y2 = self.engine.redheffer_halfspace(side, self._pack_bd(Sbd), S, want_xy=len(C[0]) > 0)
        return Sn, _propagate_coupling(self._mm_plain, Cm, Cn, X1, X2, Y1, Y2)

    @staticmethod
    def _is_bd(S):
        return isinstance(S[0], BlockDiag2)

    def _star(self, Sm, Sn, Cm, Cn):
        """Sm * Sn for any mix of dense ([B,n,n] tensors) and block-diagonal (BlockDiag2) operands."""
        bm, bn = self._is_bd(Sm), self._is_bd(Sn)
        if bm and bn:
            return _star_bd(Sm, Sn), [[], []]
        if bm:
            return self._RS_halfspace(0, Sm, Sn, Cn)
        if bn:
            return self._RS_halfspace(1, Sn, Sm, Cm)
        return self._RS_prod(Sm, Sn, Cm, Cn)

    def _layer_S(self, i):
        # the layer S-matrix is symmetric under port exchange: S22 = S11, S12 = S21
        return [self.layer_S11[i], self.layer_S21[i], self.layer_S21[i], self.layer_S11[i]]

    def _layer_C(self, i):
        if not self.keep_coupling or self.Cplus[i] is None:
            return [[], []]
        return [[torch.cat((self.Cplus[i], self.Cminus[i]), dim=1)], [torch.cat((self.Cminus[i], self.Cplus[i]), dim=1)]]

    def _stored_layers(self, lo, hi):
        """(S, C) of the stored layers lo .. hi - 1, each formed when the chain reaches it."""
        return ((self._layer_S(i), self._layer_C(i)) for i in range(lo, hi))

    def _star_chain(self, S, C, items):
        """(S, C) * (S_1, C_1) * (S_2, C_2) ... from left to right over the (S_i, C_i) of `items`; S None: the first item starts the chain
        (and None comes back when there is none)."""
        for Sn, Cn in items:
            S, C = (Sn, Cn) if S is None else self._star(S, Sn, C, Cn)
        return S, C

    def _cascade(self, defer_last=False):
        """The cascade of solve_global_smatrix (rcwa.py:173-211): returns (S, C, None).  defer_last: when the LAST star product is one with a
        half-space on the plain path -- a dense running S, no coupling lists to propagate (keep_coupling=False), no differentiable layer -- it is
        not formed: (S before it, C, side) comes back, side 0 for the pending Sin * S, 1 for S * Sout (solve_S_parameters probes it)."""
        n, B = self.n, self.B
        # the folded prefix (None when nothing is folded), then the stored layers
        S, C = self._star_chain(self._running, [[], []], self._stored_layers(self._n_folded, self.layer_N))
        self._zero_layer_S = S is None and not (self.has_in or self.has_out)           # reference stores 1-D zeros (rcwa.py:187-188)
        if S is None:
            I = torch.eye(n, dtype=self._cdtype, device=self._device).expand(B, -1, -1).contiguous()
            Z = torch.zeros((B, n, n), dtype=self._cdtype, device=self._device)
            S = [I, Z, Z.clone(), I.clone()]
        sides = ([0] if self.has_in else []) + ([1] if self.has_out else [])           # rcwa.py:198-202, 204-208
        for j, side in enumerate(sides):
            if (defer_last and j == len(sides) - 1 and not self.keep_coupling and not self._diff
                    and not self._is_bd(S) and not C[0] and not C[1]):
                return S, C, side
            S, C = self._star(self._Sin, S, [[], []], C) if side == 0 else self._star(S, self._Sout, C, [[], []])
        return S, C, None

    def solve_global_smatrix(self):                                                     # rcwa.py:173-211
        self._global_only("solve_global_smatrix")
        S, C, _ = self._cascade()
        if self._is_bd(S):                                                              # only homogeneous media: densify for the read-out
            S = [blk.dense().to(self._cdtype) for blk in S]
        self.S = S
        self.C = C

    def solve_S_parameters(self, orders, *, direction="forward", port="transmission", polarization="xx", ref_order=[0, 0],
                           power_norm=True, evanscent=1e-3):
        """solve_global_smatrix() followed by S_parameters(...) -- same arguments, warnings, in-place order clamping and values -- without the
        global S-matrix where the read-out does not need it.  When the last star product of the cascade is one with a half-space on the plain
        path (keep_coupling=False, no differentiable layer, a dense S before it), only the one or two columns of the one block that the
        read-out takes are computed (Engine.redheffer_halfspace_columns: one LU instead of the 4.33 n^3 product), and `self.S` / `self.C` are
        NOT set (they keep whatever an earlier solve_global_smatrix left).  Every other case -- keep_coupling, a differentiable stack, no
        half-space, only homogeneous layers -- runs solve_global_smatrix() and reads out of self.S as S_parameters does.
        On a solver with a swept layer (add_layer(..., swept=True)) the result is [B, T, len(orders)], one row per thickness.
        With symmetry_sector=True only the mirror sectors that the requested columns touch are solved, cached per (layer, sector), and
        `self.S` / `self.C` are not set; with sector_grad=True the result carries the graph of those sectors (read-outs of one sector share it)."""
        solve = self._solve_sector if self.symmetry_sector else (self._solve_swept if self._swept is not None else self._solve_plain)
        return solve(orders, direction, port, polarization, ref_order, power_norm, evanscent)

    def _solve_plain(self, orders, direction, port, polarization, ref_order, power_norm, evanscent):
        orders, polarization, oi, ri, k = self._sparam_args(orders, direction, port, polarization, ref_order)
        S, C, side = self._cascade(defer_last=True)
        if side is None:
            if self._is_bd(S):
                S = [blk.dense().to(self._cdtype) for blk in S]
            self.S, self.C = S, C
            Sk = S[k]
            return self._sparam_values(lambda c: Sk[:, :, c], k, oi, ri, polarization, power_norm, evanscent)
        cols = self._sparam_columns(ri, polarization)
        bd = self._pack_bd(self._Sin if side == 0 else self._Sout)
        out = self.engine.redheffer_halfspace_columns(side, bd, S, k, cols)             # [B, n, len(cols)]
        return self._sparam_values(lambda c: out[:, :, cols.index(c)], k, oi, ri, polarization, power_norm, evanscent)

    # ---- what a mode cannot serve: a swept solver has no single stack, a sector solver no global S-matrix and no coupling matrices.  Each mode
    # states its refusal next to its code (_refuse_swept in swept.py, _refuse_sector in sector.py); S_parameters (readout.py) and
    # solve_global_smatrix above call them as well
    def _global_only(self, what):
        self._refuse_swept(what)
        self._refuse_sector(what)

    def power_flux(self, *a, **kw):
        self._global_only("power_flux")
        return super().power_flux(*a, **kw)

    def incident_flux(self, *a, **kw):
        self._global_only("incident_flux")
        return super().incident_flux(*a, **kw)

    def absorption(self, *a, **kw):
        self._global_only("absorption")
        return super().absorption(*a, **kw)

    def volume_integral(self, *a, **kw):
        self._global_only("volume_integral")
        return super().volume_integral(*a, **kw)

    def absorption_by_region(self, *a, **kw):
        self._global_only("absorption_by_region")
        return super().absorption_by_region(*a, **kw)

    def source_planewave(self, *a, **kw):
        self._refuse_sector("source_planewave")
        return super().source_planewave(*a, **kw)

    def source_fourier(self, *a, **kw):
        self._refuse_sector("source_fourier")
        return super().source_fourier(*a, **kw)
