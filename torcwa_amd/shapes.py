"""Vector-shape layers: ellipses, rectangles and simple polygons whose Fourier coefficients are evaluated in closed form
(include/trx.h: trx_convmat_shapes), so a patterned layer needs no pixel grid, has no staircase error and has exact derivatives with respect to
its radii, widths, centres, rotations, vertices and permittivities.

    layer = ShapeLayer(1.0, [circle(120., 350., 330., 12.0 + 0.5j)])
    sim.add_layer(thickness=200., eps=layer)

Coordinates are those of the field maps (`x_axis`, `y_axis`): the origin is the cell corner.  A grid from `geometry` with nominal centre
(Cx, Cy) is the structure centred at (Cx - Lx/2nx, Cy - Ly/2ny) in these coordinates; `ShapeLayer.rasterise`
samples at the DFT's own positions and has no such shift.

Every scalar may be a python number, a 0-d tensor or a [B] tensor (a geometry sweep); polygon vertices are [K, 2] or [B, K, 2].  Any of them
may require grad.  Contributions add: shapes that overlap without being nested are the caller's error and are not checked.  A shape that lies
wholly inside another names it with `host=` (core-shell); its contrast is then taken against the host's permittivity.
"""
import math
from collections import namedtuple

import numpy as np
import torch

ELLIPSE, RECTANGLE, POLYGON = 0, 1, 2

# the operands of trx_convmat_shapes: kind [S], voff [S+1] (int32), par [B, npar] fp64, val [B, S+1] complex128, recip = (b1x, b1y, b2x, b2y)
Packed = namedtuple("Packed", "kind voff par val recip cell_area")


def _t(v, dtype):
    return v.to(dtype) if torch.is_tensor(v) else torch.as_tensor(v, dtype=dtype)


def _batch_of(t, lead):
    """Batch size a parameter carries: `lead` is the number of dimensions of its unbatched form."""
    return int(t.shape[0]) if t.dim() == lead + 1 else 1


class Shape:
    """One shape: its kind, its parameters (five scalars, or the vertex array of a polygon), its permittivity and the shape it sits in."""

    def __init__(self, kind, params, eps, host=None):
        if host is not None and not isinstance(host, Shape):
            raise TypeError("host= names the Shape this one lies inside")
        self.kind, self.eps, self.host = kind, _t(eps, torch.complex128), host
        if kind == POLYGON:
            v = _t(params, torch.float64)
            if v.dim() not in (2, 3) or v.shape[-1] != 2 or v.shape[-2] < 3:
                raise ValueError(f"polygon vertices must be [K, 2] or [B, K, 2] with K >= 3, got {list(v.shape)}")
            self.params = v
        else:
            self.params = [_t(p, torch.float64) for p in params]
            for p in self.params:
                if p.dim() > 1:
                    raise ValueError("a shape parameter is a number, a 0-d tensor or a [B] tensor")
        if self.eps.dim() > 1:
            raise ValueError("eps of a shape is a number, a 0-d tensor or a [B] tensor")

    def _tensors(self):
        return ([self.params] if self.kind == POLYGON else list(self.params)) + [self.eps]

    @property
    def batch(self):
        sizes = [_batch_of(self.params, 2)] if self.kind == POLYGON else [_batch_of(p, 0) for p in self.params]
        return max(sizes + [_batch_of(self.eps, 0)])

    @property
    def depth(self):
        return 0 if self.host is None else self.host.depth + 1

    def _row(self, B, device):
        """[B, 5] or [B, 2K] parameter rows; a clockwise polygon is reversed (the kernel's edge sum takes counter-clockwise lists)."""
        if self.kind == POLYGON:
            v = self.params.to(device)
            v = (v[None] if v.dim() == 2 else v).expand(B, -1, -1)
            x, y = v.detach()[..., 0], v.detach()[..., 1]
            area = (x * torch.roll(y, -1, 1) - torch.roll(x, -1, 1) * y).sum(1)
            v = torch.where((area < 0)[:, None, None], v.flip(1), v)
            return v.reshape(B, -1)
        return torch.stack([p.to(device).expand(B) for p in self.params], dim=1)

    def _sliced(self, lo, hi, B, memo):
        if id(self) in memo:
            return memo[id(self)]
        cut = lambda t, lead: t[lo:hi] if (t.dim() == lead + 1 and t.shape[0] == B) else t
        params = cut(self.params, 2) if self.kind == POLYGON else [cut(p, 0) for p in self.params]
        memo[id(self)] = Shape(self.kind, params, cut(self.eps, 0), None if self.host is None else self.host._sliced(lo, hi, B, memo))
        return memo[id(self)]

    def _inside(self, X, Y, B):
        """[B, n1, n2] bool: the points (X, Y) [n1, n2] strictly inside the shape."""
        row = self._row(B, X.device).detach()
        if self.kind == POLYGON:
            v = row.reshape(B, -1, 2)
            w = torch.roll(v, -1, 1)
            odd = torch.zeros((B,) + tuple(X.shape), dtype=torch.bool, device=X.device)
            for k in range(v.shape[1]):                                    # edge by edge: [B, n1, n2] temporaries whatever K is
                ax, ay, bx, by = (t[:, k, None, None] for t in (v[..., 0], v[..., 1], w[..., 0], w[..., 1]))
                odd ^= ((ay > Y) != (by > Y)) & (X < (bx - ax) * (Y - ay) / torch.where(by == ay, torch.ones_like(by), by - ay) + ax)
            return odd                                                     # even-odd rule
        a, b, cx, cy, th = (row[:, i, None, None] for i in range(5))
        dx, dy = X - cx, Y - cy
        u, w = torch.cos(th) * dx + torch.sin(th) * dy, -torch.sin(th) * dx + torch.cos(th) * dy
        if self.kind == ELLIPSE:
            return (u / a) ** 2 + (w / b) ** 2 < 1
        return (u.abs() < a / 2) & (w.abs() < b / 2)


def ellipse(Rx, Ry, Cx, Cy, eps, theta=0., host=None):
    """Ellipse with semi-axes Rx, Ry about (Cx, Cy), rotated by theta (radians, counter-clockwise)."""
    return Shape(ELLIPSE, [Rx, Ry, Cx, Cy, theta], eps, host)


def circle(R, Cx, Cy, eps, host=None):
    return Shape(ELLIPSE, [R, R, Cx, Cy, 0.], eps, host)


def rectangle(Wx, Wy, Cx, Cy, eps, theta=0., host=None):
    """Rectangle of full widths Wx, Wy about (Cx, Cy), rotated by theta."""
    return Shape(RECTANGLE, [Wx, Wy, Cx, Cy, theta], eps, host)


def square(W, Cx, Cy, eps, theta=0., host=None):
    return Shape(RECTANGLE, [W, W, Cx, Cy, theta], eps, host)


def polygon(vertices, eps, host=None):
    """Simple polygon, vertices [K, 2] or [B, K, 2] in either orientation."""
    return Shape(POLYGON, vertices, eps, host)


def rhombus(Wx, Wy, Cx, Cy, eps, theta=0., host=None):
    """Rhombus with diagonals Wx, Wy about (Cx, Cy), rotated by theta: the 4-gon (+-Wx/2, 0), (0, +-Wy/2)."""
    Wx, Wy, Cx, Cy, theta = (_t(v, torch.float64) for v in (Wx, Wy, Cx, Cy, theta))
    c, s = torch.cos(theta), torch.sin(theta)
    pts = [(Wx / 2, 0 * Wy), (0 * Wx, Wy / 2), (-Wx / 2, 0 * Wy), (0 * Wx, -Wy / 2)]
    verts = torch.stack([torch.stack(torch.broadcast_tensors(Cx + c * u - s * w, Cy + s * u + c * w), dim=-1) for u, w in pts], dim=-2)
    return Shape(POLYGON, verts, eps, host)


class ShapeLayer:
    """eps of a patterned layer as a background permittivity and a list of shapes: `add_layer(d, eps=ShapeLayer(background, shapes))`."""

    def __init__(self, background, shapes):
        self.background = _t(background, torch.complex128)
        if self.background.dim() > 1:
            raise ValueError("background is a number, a 0-d tensor or a [B] tensor")
        self.shapes = list(shapes)
        if not self.shapes or not all(isinstance(s, Shape) for s in self.shapes):
            raise ValueError("ShapeLayer needs a non-empty list of shapes (circle, ellipse, rectangle, square, rhombus, polygon)")
        for s in self.shapes:
            if s.host is not None and not any(s.host is h for h in self.shapes):
                raise ValueError("host= must name a shape of the same layer")

    @property
    def batch(self):
        return max([_batch_of(self.background, 0)] + [s.batch for s in self.shapes])

    @property
    def requires_grad(self):
        return any(t.requires_grad for s in self.shapes for t in s._tensors()) or self.background.requires_grad

    def slice(self, lo, hi):
        """The layer of sweep points lo .. hi-1 (per-point parameters are cut, shared ones kept)."""
        B, memo = self.batch, {}
        cut = self.background[lo:hi] if (self.background.dim() == 1 and self.background.shape[0] == B) else self.background
        return ShapeLayer(cut, [s._sliced(lo, hi, B, memo) for s in self.shapes])

    def pack(self, lattice, B, device):
        """The operands of trx_convmat_shapes for a lattice (rows a1, a2) and B sweep points; par and val stay in the autograd graph."""
        if self.batch not in (1, B):
            raise ValueError(f"ShapeLayer carries {self.batch} sweep points, the solver {B}")
        A = np.asarray(lattice, dtype=np.float64).reshape(2, 2)
        area = abs(A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0])
        recip = 2 * math.pi * np.linalg.inv(A).T                              # rows b1, b2: b_i . a_j = 2 pi delta_ij
        rows = [s._row(B, device) for s in self.shapes]
        voff = np.concatenate(([0], np.cumsum([r.shape[1] for r in rows])))
        bvec = lambda t: t.to(device).expand(B)
        bg = bvec(self.background)
        val = torch.stack([bg] + [bvec(s.eps) - (bg if s.host is None else bvec(s.host.eps)) for s in self.shapes], dim=1)
        return Packed(torch.tensor([s.kind for s in self.shapes], dtype=torch.int32, device=device),
                      torch.tensor(voff, dtype=torch.int32, device=device), torch.cat(rows, dim=1), val,
                      tuple(float(v) for v in recip.ravel()), float(area))

    def reciprocal_values(self, B, device):
        """[B, S+1] complex128, the `rval` of trx_convmat_nv_shapes: 1/eps of the background, then 1/eps_s - 1/eps_host per shape -- the
        `val` of pack() for the reciprocal permittivity.  Stays in the autograd graph."""
        bvec = lambda t: t.to(device).expand(B)
        rbg = 1 / bvec(self.background)
        return torch.stack([rbg] + [1 / bvec(s.eps) - (rbg if s.host is None else 1 / bvec(s.host.eps)) for s in self.shapes], dim=1)

    def rasterise(self, a1, a2, n1, n2, device=None):
        """Hard-edged [B, n1, n2] eps grid sampled at (x / n1) a1 + (y / n2) a2 -- the DFT's positions, not the half-pixel-shifted ones of
        `geometry`.  Shapes that cross the cell boundary wrap around (the eight neighbouring images are tested).  For comparisons with the grid
        path, masks for absorption_by_region, and eyeballing; not differentiable."""
        B = self.batch
        a1, a2 = (np.asarray(torch.as_tensor(a).detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (a1, a2))
        u = torch.arange(n1, dtype=torch.float64, device=device)[:, None] / n1
        v = torch.arange(n2, dtype=torch.float64, device=device)[None, :] / n2
        X, Y = u * a1[0] + v * a2[0], u * a1[1] + v * a2[1]
        bvec = lambda t: t.detach().to(X.device).expand(B)
        grid = bvec(self.background)[:, None, None].expand(B, n1, n2).clone()
        for s in sorted(self.shapes, key=lambda s: s.depth):                    # hosts before what they hold
            inside = torch.zeros((B, n1, n2), dtype=torch.bool, device=X.device)
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    inside |= s._inside(X - i * a1[0] - j * a2[0], Y - i * a1[1] - j * a2[1], B)
            grid = torch.where(inside, bvec(s.eps)[:, None, None], grid)
        return grid


def nv_grid(shape_nv_grid):
    """(n1, n2) of the `shape_nv_grid` keyword: an int or a pair of ints, each in 1 .. 2048."""
    g = (shape_nv_grid, shape_nv_grid) if isinstance(shape_nv_grid, (int, np.integer)) else tuple(shape_nv_grid)
    if len(g) != 2 or not all(isinstance(v, (int, np.integer)) and 1 <= v <= 2048 for v in g):
        raise ValueError(f"shape_nv_grid must be an int or (n1, n2) with 1 <= n <= 2048, got {shape_nv_grid!r}")
    return int(g[0]), int(g[1])


def normal_products(layer, lattice, n1, n2, B=None, engine=None):
    """[B, 3, n1, n2] float64 products (Nx^2, Nx Ny, Ny^2) of the blended normal field of a ShapeLayer (include/trx.h:
    trx_shape_normal_field), sampled at (i / n1) a1 + (j / n2) a2 like `rasterise`: what fourier_rule="normal" derives for the layer.  For
    inspection, and for experiments with add_layer(normal_field=...).  lattice: [Lx, Ly] or the 2 x 2 rows a1, a2."""
    from . import lattice as _lat
    from .engine import default_engine
    eng = engine if engine is not None else default_engine()
    A = _lat.lattice_matrix(lattice)
    B = layer.batch if B is None else int(B)
    return eng.shape_normal_field(layer.pack(A, B, eng.device), A, n1, n2)
