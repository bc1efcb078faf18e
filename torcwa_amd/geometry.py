"""Level-set shape generators (input side of the hot path; mirrors the public API of torcwa/geometry.py:4-290).

Every primitive returns sigmoid(edge_sharpness * level) on the cell-centre grid x_i = (i+0.5) Lx/nx, where
`level` is 1 - (normalised distance in the shape's own rotated frame).  Differentiable torch elementwise code.
`geometry` is the instance API; `rcwa_geo` is the legacy class-level twin the notebooks use.
"""
import torch


def _rot(x, y, cx, cy, theta, dtype, device):
    th = torch.as_tensor(theta, dtype=dtype, device=device)
    c, s = torch.cos(th), torch.sin(th)
    return (x - cx) * c + (y - cy) * s, -(x - cx) * s + (y - cy) * c


class _Shapes:
    """Shape algebra shared by the instance and the class-level front-ends; `g` supplies Lx, Ly, nx, ny, ... ."""

    @staticmethod
    def _grid(g):
        g.x = (g.Lx / g.nx) * (torch.arange(g.nx, dtype=g.dtype, device=g.device) + 0.5)
        g.y = (g.Ly / g.ny) * (torch.arange(g.ny, dtype=g.dtype, device=g.device) + 0.5)
        g.x_grid, g.y_grid = torch.meshgrid(g.x, g.y, indexing="ij")

    @staticmethod
    def _level(g, kind, a, b, Cx, Cy, theta=0., power=2.):
        _Shapes._grid(g)
        u, v = _rot(g.x_grid, g.y_grid, Cx, Cy, theta, g.dtype, g.device)
        return _Shapes._shape(g, kind, u, v, a, b, power)

    @staticmethod
    def _shape(g, kind, u, v, a, b, power=2.):
        """sigmoid(edge_sharpness (1 - distance)) of a shape of half-axes / widths a, b at the displacement (u, v) in its own frame."""
        if kind == "ellipse":
            dist = torch.sqrt((u / a) ** 2 + (v / b) ** 2)
        elif kind == "box":
            dist = torch.maximum(torch.abs(u / (a / 2.)), torch.abs(v / (b / 2.)))
        elif kind == "rhombus":
            dist = torch.abs(u / (a / 2.)) + torch.abs(v / (b / 2.))
        else:  # super ellipse
            dist = (torch.abs(u / (a / 2.)) ** power + torch.abs(v / (b / 2.)) ** power) ** (1 / power)
        return torch.sigmoid(g.edge_sharpness * (1. - dist))


class geometry:
    def __init__(self, Lx: float = 1., Ly: float = 1., nx: int = 100, ny: int = 100, edge_sharpness: float = 1000., *,
                 dtype=torch.float32, device=torch.device("cuda" if torch.cuda.is_available() else "cpu")):
        self.Lx, self.Ly, self.nx, self.ny, self.edge_sharpness = Lx, Ly, nx, ny, edge_sharpness
        self.dtype, self.device = dtype, device

    def grid(self):
        _Shapes._grid(self)

    def circle(self, R, Cx, Cy):
        _Shapes._grid(self)
        return torch.sigmoid(self.edge_sharpness * (1. - torch.sqrt(((self.x_grid - Cx) / R) ** 2 + ((self.y_grid - Cy) / R) ** 2)))

    def ellipse(self, Rx, Ry, Cx, Cy, theta=0.):
        return _Shapes._level(self, "ellipse", Rx, Ry, Cx, Cy, theta)

    def square(self, W, Cx, Cy, theta=0.):
        return _Shapes._level(self, "box", W, W, Cx, Cy, theta)

    def rectangle(self, Wx, Wy, Cx, Cy, theta=0.):
        return _Shapes._level(self, "box", Wx, Wy, Cx, Cy, theta)

    def rhombus(self, Wx, Wy, Cx, Cy, theta=0.):
        return _Shapes._level(self, "rhombus", Wx, Wy, Cx, Cy, theta)

    def super_ellipse(self, Wx, Wy, Cx, Cy, theta=0., power=2.):
        return _Shapes._level(self, "super", Wx, Wy, Cx, Cy, theta, power)

    @staticmethod
    def union(A, B):
        return torch.maximum(A, B)

    @staticmethod
    def intersection(A, B):
        return torch.minimum(A, B)

    @staticmethod
    def difference(A, B):
        return torch.minimum(A, 1. - B)


class lattice_geometry:
    """The shape API of `geometry` on an oblique cell spanned by the lattice vectors a1, a2 (torcwa_amd.lattice): an [n1, n2] grid whose axis
    0 runs along a1 and axis 1 along a2, with samples at the cell centres ((i+0.5)/n1) a1 + ((j+0.5)/n2) a2 (physical x_grid, y_grid).  Centres
    Cx, Cy and sizes are physical.  Each shape is evaluated at the minimum-image displacement from its centre: the fractional coordinates are
    reduced to [-1/2, 1/2) and the nearest of the 9 neighbouring images is taken, so a disk on a lattice point or a cell edge is whole.  The
    shapes stay differentiable in their parameters (the choice of image is piecewise constant)."""

    def __init__(self, a1, a2, n1: int = 100, n2: int = 100, edge_sharpness: float = 1000., *, dtype=torch.float32,
                 device=torch.device("cuda" if torch.cuda.is_available() else "cpu")):
        import numpy as np
        from .lattice import lattice_matrix
        A = lattice_matrix([a1, a2])
        self.a1, self.a2, self.n1, self.n2, self.edge_sharpness = A[0].tolist(), A[1].tolist(), int(n1), int(n2), edge_sharpness
        self.dtype, self.device = dtype, device
        self._A, self._Ai = A, np.linalg.inv(A)
        f1 = (torch.arange(self.n1, dtype=torch.float64) + 0.5) / self.n1
        f2 = (torch.arange(self.n2, dtype=torch.float64) + 0.5) / self.n2
        F1, F2 = torch.meshgrid(f1, f2, indexing="ij")
        self.x_grid = (F1 * A[0, 0] + F2 * A[1, 0]).to(dtype=dtype, device=device)
        self.y_grid = (F1 * A[0, 1] + F2 * A[1, 1]).to(dtype=dtype, device=device)

    def _disp(self, Cx, Cy):
        """Minimum-image displacement (u, v) of every sample from the point (Cx, Cy)."""
        A, Ai = self._A, self._Ai
        dx, dy = self.x_grid - Cx, self.y_grid - Cy
        f1 = dx * Ai[0, 0] + dy * Ai[1, 0]                 # d = f1 a1 + f2 a2
        f2 = dx * Ai[0, 1] + dy * Ai[1, 1]
        f1 = f1 - torch.floor(f1.detach() + 0.5)
        f2 = f2 - torch.floor(f2.detach() + 0.5)
        bu = bv = br = None
        for k1 in (-1, 0, 1):
            for k2 in (-1, 0, 1):
                u = (f1 + k1) * A[0, 0] + (f2 + k2) * A[1, 0]
                v = (f1 + k1) * A[0, 1] + (f2 + k2) * A[1, 1]
                r = (u * u + v * v).detach()
                if bu is None:
                    bu, bv, br = u, v, r
                else:
                    sel = r < br
                    bu, bv, br = torch.where(sel, u, bu), torch.where(sel, v, bv), torch.where(sel, r, br)
        return bu, bv

    def _level(self, kind, a, b, Cx, Cy, theta=0., power=2.):
        u, v = self._disp(Cx, Cy)
        u, v = _rot(u, v, 0., 0., theta, self.dtype, self.device)
        return _Shapes._shape(self, kind, u, v, a, b, power)

    def circle(self, R, Cx, Cy):
        u, v = self._disp(Cx, Cy)
        return torch.sigmoid(self.edge_sharpness * (1. - torch.sqrt((u / R) ** 2 + (v / R) ** 2)))

    def ellipse(self, Rx, Ry, Cx, Cy, theta=0.):
        return self._level("ellipse", Rx, Ry, Cx, Cy, theta)

    def square(self, W, Cx, Cy, theta=0.):
        return self._level("box", W, W, Cx, Cy, theta)

    def rectangle(self, Wx, Wy, Cx, Cy, theta=0.):
        return self._level("box", Wx, Wy, Cx, Cy, theta)

    def rhombus(self, Wx, Wy, Cx, Cy, theta=0.):
        return self._level("rhombus", Wx, Wy, Cx, Cy, theta)

    def super_ellipse(self, Wx, Wy, Cx, Cy, theta=0., power=2.):
        return self._level("super", Wx, Wy, Cx, Cy, theta, power)

    union = staticmethod(geometry.union)
    intersection = staticmethod(geometry.intersection)
    difference = staticmethod(geometry.difference)


class rcwa_geo:
    """Legacy class-level API of the notebooks: `rcwa_geo.Lx = ...; rcwa_geo.grid(); rcwa_geo.rectangle(...)` on the class itself."""
    dtype = torch.float32
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    Lx, Ly, nx, ny = 1., 1., 100, 100
    edge_sharpness = 1000.

    @classmethod
    def grid(cls):
        _Shapes._grid(cls)

    @classmethod
    def circle(cls, R, Cx, Cy):
        _Shapes._grid(cls)
        return torch.sigmoid(cls.edge_sharpness * (1. - torch.sqrt(((cls.x_grid - Cx) / R) ** 2 + ((cls.y_grid - Cy) / R) ** 2)))

    @classmethod
    def ellipse(cls, Rx, Ry, Cx, Cy, theta=0.):
        return _Shapes._level(cls, "ellipse", Rx, Ry, Cx, Cy, theta)

    @classmethod
    def square(cls, W, Cx, Cy, theta=0.):
        return _Shapes._level(cls, "box", W, W, Cx, Cy, theta)

    @classmethod
    def rectangle(cls, Wx, Wy, Cx, Cy, theta=0.):
        return _Shapes._level(cls, "box", Wx, Wy, Cx, Cy, theta)

    @classmethod
    def rhombus(cls, Wx, Wy, Cx, Cy, theta=0.):
        return _Shapes._level(cls, "rhombus", Wx, Wy, Cx, Cy, theta)

    @classmethod
    def super_ellipse(cls, Wx, Wy, Cx, Cy, theta=0., power=2.):
        return _Shapes._level(cls, "super", Wx, Wy, Cx, Cy, theta, power)

    union = staticmethod(geometry.union)
    intersection = staticmethod(geometry.intersection)
    difference = staticmethod(geometry.difference)
