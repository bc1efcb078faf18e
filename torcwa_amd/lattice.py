"""Lattices and Fourier-order sets beyond the reference's rectangle.

The reference describes every structure on a rectangular lattice L = [Lx, Ly] with the order box |m| <= ox, |n| <= oy.  Here L may also be a
2 x 2 array whose rows are the lattice vectors a1, a2 (grid axis 0 runs along a1, axis 1 along a2), and the order set may be any list of
harmonic indices (m, n) in the lattice basis: harmonic (m, n) has the in-plane wave vector k0 + m b1 + n b2 with a_i . b_j = delta_ij (the
reference's convention, no factor 2 pi: G = 1 / (L f) in units of the free-space wave number).
"""
import numpy as np
import torch

# |det| / (|a1| |a2|) = |sin| of the angle between the lattice vectors: at or below this the lattice is singular
_SINGULAR = 1e-9
# shells of circular_orders: |G| equal to this relative tolerance are one shell (kept or dropped whole)
_SHELL_RTOL = 1e-9


def _host(v):
    """float64 numpy view of a scalar, tensor or (nested) list of them (real part of complex values)."""
    if torch.is_tensor(v):
        t = v.detach().cpu()
        return (torch.real(t) if t.is_complex() else t).to(torch.float64).numpy()
    if isinstance(v, (list, tuple)):
        return np.stack([_host(x) for x in v])
    return np.real(np.asarray(v)).astype(np.float64)


def lattice_matrix(L):
    """[2, 2] float64 numpy array whose rows are a1, a2: [Lx, Ly] -> diag(Lx, Ly); a 2 x 2 array as given.  ValueError if singular."""
    A = _host(L)
    if A.shape == (2,):
        A = np.diag(A)
    if A.shape != (2, 2):
        raise ValueError(f"L must be [Lx, Ly] or a 2 x 2 array of lattice vectors (rows a1, a2), got shape {list(A.shape)}")
    if not np.isfinite(A).all():
        raise ValueError("L must be finite")
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    if not abs(det) > _SINGULAR * np.linalg.norm(A[0]) * np.linalg.norm(A[1]):
        raise ValueError(f"the lattice vectors {A.tolist()} are (nearly) parallel or zero")
    return A


def is_rectangular(L):
    """True for [Lx, Ly] and for a diagonal 2 x 2 lattice."""
    A = lattice_matrix(L)
    return A[0, 1] == 0.0 and A[1, 0] == 0.0


def reciprocal(L):
    """[2, 2] float64 numpy array whose rows are b1, b2 with a_i . b_j = delta_ij (no factor 2 pi, as the reference's G = 1 / L)."""
    A = lattice_matrix(L)
    if A[0, 1] == 0.0 and A[1, 0] == 0.0:
        return np.diag([1.0 / A[0, 0], 1.0 / A[1, 1]])
    return np.linalg.inv(A).T


def rect_orders(ox, oy):
    """[N, 2] int64 (m, n) of the order box |m| <= ox, |n| <= oy in the reference's x-major enumeration i = (m+ox)(2oy+1) + (n+oy)."""
    ox, oy = int(ox), int(oy)
    if ox < 0 or oy < 0:
        raise ValueError(f"orders must be >= 0, got [{ox}, {oy}]")
    m, n = np.meshgrid(np.arange(-ox, ox + 1), np.arange(-oy, oy + 1), indexing="ij")
    return np.stack((m.ravel(), n.ravel()), axis=1).astype(np.int64)


def circular_orders(L, n_harmonics=None, g_max=None):
    """[N, 2] int64: every (m, n) with |m b1 + n b2| <= R, sorted by (|G|, m, n).

    g_max: R itself (units of 1 / length of L, i.e. of b1, b2).  n_harmonics: the smallest R that holds at least that many harmonics.  Shells
    of equal |G| (to 1e-9 relative) are always kept whole, so the set has the lattice's symmetry; as a set it does not depend on the basis
    chosen for the lattice."""
    if (n_harmonics is None) == (g_max is None):
        raise ValueError("circular_orders needs exactly one of n_harmonics and g_max")
    A = lattice_matrix(L)
    Bm = reciprocal(L)
    la1, la2 = np.linalg.norm(A[0]), np.linalg.norm(A[1])
    if g_max is not None:
        R = float(g_max)
        if not (R >= 0.0 and np.isfinite(R)):
            raise ValueError(f"g_max must be a finite number >= 0, got {g_max!r}")
    else:
        n_harmonics = int(n_harmonics)
        if n_harmonics < 1:
            raise ValueError(f"n_harmonics must be >= 1, got {n_harmonics}")
        cell = abs(np.linalg.det(Bm))                          # reciprocal-cell area: about pi R^2 / cell harmonics lie within R
        R = 1.5 * np.sqrt(n_harmonics * cell / np.pi) + np.linalg.norm(Bm, axis=1).max()
    while True:
        # |m| = |a1 . G| <= |a1| R: the box holds every G of the disk of radius R
        mm, nm = int(np.floor(la1 * R * (1 + 1e-6))) + 1, int(np.floor(la2 * R * (1 + 1e-6))) + 1
        m, n = np.meshgrid(np.arange(-mm, mm + 1), np.arange(-nm, nm + 1), indexing="ij")
        m, n = m.ravel(), n.ravel()
        g = np.hypot(m * Bm[0, 0] + n * Bm[1, 0], m * Bm[0, 1] + n * Bm[1, 1])
        if g_max is not None:
            cut = R
            break
        cut = np.partition(g, n_harmonics - 1)[n_harmonics - 1]
        if cut * (1 + 2 * _SHELL_RTOL) <= R:
            break
        R *= 2.0
    keep = g <= cut * (1 + _SHELL_RTOL)
    m, n, g = m[keep], n[keep], g[keep]
    o = np.argsort(g, kind="stable")
    m, n, g = m[o], n[o], g[o]
    # shell index: consecutive |G| within the tolerance share one (sorting by the raw |G| would order a shell by rounding noise)
    shell = np.concatenate(([0], np.cumsum(np.diff(g) > _SHELL_RTOL * np.maximum(g[1:], 1e-300))))
    o = np.lexsort((n, m, shell))
    return np.stack((m[o], n[o]), axis=1).astype(np.int64)


def parse_order(order):
    """("rect", (ox, oy), None) for the flat 2-element form; ("list", None, mn [N, 2] int64) for a list of (m, n).  Nesting depth decides:
    [ox, oy] is always the rectangle, [[m, n], ...] always a list.  A list must hold integers, contain (0, 0) and have no duplicates."""
    a = order.detach().cpu().numpy() if torch.is_tensor(order) else np.asarray(order)
    if a.ndim == 1:
        if a.shape[0] != 2:
            raise ValueError(f"order must be [ox, oy] or an [N, 2] list of (m, n), got {order!r}")
        return "rect", (int(a[0]), int(a[1])), None
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"an order list must have shape [N, 2], got {list(a.shape)}")
    if a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and np.array_equal(a, np.round(a))):
        raise ValueError("an order list must hold integers")
    mn = a.astype(np.int64)
    if len({(int(p), int(q)) for p, q in mn}) != len(mn):
        raise ValueError("the order list has duplicate harmonics")
    if not ((mn[:, 0] == 0) & (mn[:, 1] == 0)).any():
        raise ValueError("the order list must contain the harmonic (0, 0)")
    return "list", None, mn
