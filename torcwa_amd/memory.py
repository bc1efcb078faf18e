"""The HBM model of the sweep drivers: how many sweep points (auto_chunk) and how many thicknesses of a swept layer (auto_thickness_chunk) fit
the free memory of the device, from footprints measured on MI355X with the caching allocator."""
import torch

from .lattice import parse_order

# HBM footprint of one sweep point, in units of one n x n complex128 matrix (n = 2 (2 ox + 1)(2 oy + 1)): measured on MI355X with the caching
# allocator -- single patterned layer, order [15,15], 128 points: 75.8 GB allocated / 111.8 GB reserved = 10.0 / 14.8 matrices per point; 4-layer stack
# with the streaming cascade, order [21,21], 64 points: 228 / 247 GB = 16.3 / 17.6.  precision="native" halves the element.
_POINT_MATRICES = {1: 15.0, 2: 18.0}          # layers == 1 / layers >= 2 (what the allocator RESERVES, which is what must fit)
# fourier_rule="li": Ex and Ey (two N x N = n^2 / 4 matrices each) live next to E, E^-1 and the assembly workspace until A exists
_LI_EXTRA = 0.5
# fourier_rule="normal": Exx, Exy, Eyy (three N x N) next to E, E^-1 while A is built, and inside trx_convmat_nv the workspace ([1/eps], its
# inverse's workspace and the three product matrices: five more N x N) -- 8 N^2 = 2 n^2
_NV_EXTRA = 2.0
# fourier_rule="normal" on a ShapeLayer (trx_convmat_nv_shapes): the tensor and the workspace matrices are those of _NV_EXTRA; on top, per point,
# the three fp64 products of the field on the shape_nv_grid (24 n1 n2 bytes), the row transforms of their pruned DFT (3 x 16 n1 (4 nmax + 1))
# and the coefficient boxes (4 x 16 (4 mmax + 1)(4 nmax + 1)).  From the workspace layout; not measured on the allocator yet.
def _shape_nv_bytes(shape_nv_grid, mmax, nmax):
    n1, n2 = (shape_nv_grid, shape_nv_grid) if isinstance(shape_nv_grid, int) else shape_nv_grid
    return 24 * n1 * n2 + 48 * n1 * (4 * nmax + 1) + 64 * (4 * mmax + 1) * (4 * nmax + 1)


_HEADROOM = 0.10                               # fraction of the device memory a sweep leaves free
# Thickness sweep (add_layer(..., swept=True)), matrices per (point, thickness) that one trx_thickness_columns call holds, from its workspace
# layout (include/trx.h): X rho X and K, 2 n x n; the amplitudes and the pivots are O(n m) and O(n) next to them.  They come on top of what stays
# per point after the eigendecomposition -- W, V, rho_L, rho_R, A, B and the prepare workspace (7) and up to two dense sides (8) -- which is
# below the eigensolver's peak that _POINT_MATRICES already covers.  Not measured on the allocator yet: auto_thickness_chunk() asks for what is free
# at the time of the call, with the same headroom.
_THICKNESS_MATRICES = 2.0


# absorption=True (keep_coupling=True, no streaming cascade), matrices per point and layer on top of _POINT_MATRICES.  Derived from the code: every
# layer keeps W, V, c+, c- (4), its S11, S21 (2) and, with the lean paths off, P, Q, M, M^-1 (4) = 10; the C lists hold one [2n, n] block per layer
# in each direction (4 per layer), and a star product writes the new lists while the old ones are alive (4 per layer already folded) next to its
# X / Y factors (4, once): 22 for one layer.  Measured on MI355X (profiles/flux_timing.txt: single patterned layer, order [15,15], 120 points):
# 188.1 GB allocated / 210.9 GB reserved = 26.5 / 29.7 matrices per point in all, against 10.0 / 14.2 for the plain sweep -- the derived count was
# too high (not all of its terms are alive at once).  What must fit is what the allocator reserves: 29.7 - 15.0 (_POINT_MATRICES) = 14.7 -> 15.
# Only the one-layer case is measured; the count is applied per layer because every term of the derivation grows with the number of layers.
_ABS_EXTRA_PER_LAYER = 15.0


def auto_chunk(B, order, n_layers, precision, device, dtype=torch.complex64, streams=1, fourier_rule="laurent", absorption=False,
               shape_nv_grid=None):
    """Largest number of points solved in lock-step that fits the free HBM of `device` with _HEADROOM to spare (a multiple of 8 when it
    is cut: the mixed-precision eigensolver and its iteration groups want batches of at least 8).  Raises with the numbers when not even
    one point fits -- instead of an allocator error in the middle of a solve."""
    if device.type != "cuda":
        return B
    kind, box, mn = parse_order(order)          # [ox, oy] or an [N, 2] order list (oblique lattices, circular truncation): n = 2N
    n = 2 * (2 * box[0] + 1) * (2 * box[1] + 1) if kind == "rect" else 2 * len(mn)
    # element size of the COMPUTE dtype: complex128 unless a complex64 problem is solved natively (BatchedRCWA: precision="native" only
    # halves the element of complex64 problems); `streams` chunks are resident at once when the sweep is dealt to several streams
    elem = 8 if (precision == "native" and dtype == torch.complex64) else 16
    mats = _POINT_MATRICES[1 if n_layers <= 1 else 2] + {"li": _LI_EXTRA, "normal": _NV_EXTRA}.get(fourier_rule, 0.0)
    if absorption:
        mats += _ABS_EXTRA_PER_LAYER * max(1, int(n_layers))
    per_point = mats * n * n * elem * max(1, int(streams))
    if fourier_rule == "normal" and shape_nv_grid is not None:      # a ShapeLayer in the stack: its field products and their transforms
        mmax, nmax = (box[0], box[1]) if kind == "rect" else (int(abs(mn[:, 0]).max()), int(abs(mn[:, 1]).max()))
        per_point += _shape_nv_bytes(shape_nv_grid, mmax, nmax) * max(1, int(streams))
    free, total = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)      # the caching allocator's idle blocks are ours to reuse
    budget = free - _HEADROOM * total
    fit = int(budget // per_point)
    if fit < 1:
        raise RuntimeError("torcwa_amd sweep: one sweep point at order %s needs about %.1f GB of HBM (%d x %d complex matrices x %.0f), but only "
                           "%.1f GB are free on %s (%.1f GB total, %.0f %% kept as headroom); free memory or lower the order"
                           % (list(box) if kind == "rect" else "of %d harmonics" % len(mn), per_point / 1e9, n, n, mats, free / 1e9, device, total / 1e9, 100 * _HEADROOM))
    if fit >= B:
        return B
    return fit if fit < 8 else fit - fit % 8


def auto_thickness_chunk(B, T, n, m, cdtype, device, backward=False):
    """Thicknesses per trx_thickness_columns call that fit the free HBM of `device` next to B resident points (_THICKNESS_MATRICES), with
    _HEADROOM to spare; T when everything fits.  Raises with the numbers when not even one thickness fits.  backward: the chunk is also the
    one of trx_thickness_columns_backward, whose workspace holds the same two matrices and 15 skinny buffers instead of 5."""
    if device.type != "cuda":
        return T
    elem = 16 if cdtype == torch.complex128 else 8
    per = B * ((_THICKNESS_MATRICES * n * n + (15 if backward else 5) * n * m) * elem + 4 * (n + 1))
    free, total = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    fit = int((free - _HEADROOM * total) // per)
    if fit < 1:
        raise RuntimeError("torcwa_amd thickness sweep: one thickness of %d points needs about %.1f GB of HBM (%d x %d complex matrices x %.0f per "
                           "point), but only %.1f GB are free on %s; lower the chunk of points" % (B, per / 1e9, n, n, _THICKNESS_MATRICES, free / 1e9, device))
    return min(int(T), fit)
