"""Sweep driver: the reference's user-level `for` loop over sweep points (example/Example1.ipynb lambda sweep,
example/Example3.ipynb (Wx,Wy) sweep) as one batched, optionally multi-GPU job.

Sharding: sweep points are independent, so rank r of R owns a contiguous block of the flattened sweep
(`shard_range`) -- or, when the cost of a point varies along the sweep (geometry sweeps: eigensolver iteration counts and
fp64 re-solves differ per shape), every R-th point (`shard_indices(..., cyclic=True)`); there is no data-path
collective.  The only communication is one all_gather of the requested S-parameters at the end (`gather_sweep`, RCCL over xGMI
on GPUs; payload is a few KB, latency-bound).
"""
import os

import numpy as np
import torch

from .batched import NV_SIGMA_DEFAULT, BatchedRCWA, check_fourier_rule
from .lattice import parse_order

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def shard_range(n_items, rank, world):
    """Contiguous block [lo, hi) of rank `rank`; blocks differ in size by at most one."""
    base, rem = divmod(int(n_items), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_indices(n_items, rank, world, cyclic=False):
    """Global indices (numpy int64, ascending) of the sweep points rank `rank` solves: the contiguous block of `shard_range`, or
    rank, rank + world, rank + 2 world, ... (cyclic: neighbouring points -- similar cost -- go to different ranks)."""
    if cyclic:
        return np.arange(int(rank), int(n_items), int(world), dtype=np.int64)
    lo, hi = shard_range(n_items, rank, world)
    return np.arange(lo, hi, dtype=np.int64)


def gather_sweep(local, n_items, group=None, cyclic=False):
    """all_gather of per-point results: `local` is this rank's [m_r, ...] block, in the order of shard_indices(n_items, rank, world,
    cyclic).  Returns the full [n_items, ...] tensor in sweep order on every rank.  Works with unequal block sizes (pads to the largest)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    counts = [len(shard_indices(n_items, r, world, cyclic)) for r in range(world)]
    sizes = [(0, c) for c in counts]
    mmax = max(counts)
    pad = torch.zeros((mmax,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    if pad.is_complex():
        buf = torch.view_as_real(pad).contiguous()
    else:
        buf = pad.contiguous()
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf, group=group)
    parts = []
    for r, (lo, hi) in enumerate(sizes):
        t = out[r][: hi - lo]
        parts.append(torch.view_as_complex(t) if pad.is_complex() else t)
    full = torch.cat(parts, dim=0)
    if not cyclic:
        return full
    # rank-major -> sweep order
    order = np.concatenate([shard_indices(n_items, r, world, True) for r in range(world)])
    inv = torch.as_tensor(np.argsort(order), device=full.device)
    return full.index_select(0, inv)


def asih_eps_table():
    """eps(lambda) of a-Si:H on linspace(400,700,128) nm (values of example/Materials.py `aSiH.apply(l)**2`, stored as data)."""
    z = np.load(os.path.join(_DATA, "asih_eps_400_700_128.npz"))
    return z["lam"], z["eps"]


def rectangle_density(nx, ny, Lx, Ly, Wx, Wy, Cx, Cy, theta=0.0, edge_sharpness=1000.0, dtype=torch.float64, device="cpu"):
    from .geometry import geometry
    g = geometry(Lx=Lx, Ly=Ly, nx=nx, ny=ny, edge_sharpness=edge_sharpness, dtype=dtype, device=torch.device(device))
    return g.rectangle(Wx=Wx, Wy=Wy, Cx=Cx, Cy=Cy, theta=theta)


def _solve_chunk(freq, layers, order, L, eps_in, eps_out, inc_ang, azi_ang, dtype, precision, engine, orders,
                 polarization, direction, port, check_info, eig_route="auto", route_hint=None, fourier_rule="laurent", nv_sigma=NV_SIGMA_DEFAULT,
                 absorption=False, source=None, symmetry=None, symmetry_tol=1e-6, symmetry_sector=False):
    """layers: list of (thickness, eps[, mu]); thickness scalar or [b]; eps/mu scalar, [b] or [b,nx,ny].  absorption: the chunk keeps W, V and
    the coupling matrices (keep_coupling=True, no streaming cascade) and returns (S-parameters, BatchedRCWA.absorption())."""
    sim = BatchedRCWA(freq, order, L, dtype=dtype, precision=precision, engine=engine, keep_coupling=bool(absorption), fold_layers=not absorption,
                      eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma,
                      symmetry=symmetry, symmetry_tol=symmetry_tol, **({"symmetry_sector": True} if symmetry_sector else {}))
    if eps_in is not None:
        sim.add_input_layer(eps=eps_in)
    if eps_out is not None:
        sim.add_output_layer(eps=eps_out)
    sim.set_incident_angle(inc_ang, azi_ang)
    for lay in layers:
        sim.add_layer(*lay)
    if not absorption:
        # only the column(s) of the one S block the read-out takes: the last half-space star product is probed, not formed
        return sim.solve_S_parameters([list(o) for o in orders], direction=direction, port=port, polarization=polarization)
    sim.solve_global_smatrix()
    sp = sim.S_parameters([list(o) for o in orders], direction=direction, port=port, polarization=polarization)
    src = dict(amplitude=[1.0, 0.0], notation="xy", direction=direction)
    src.update(source or {})
    if "orders" in src:
        sim.source_fourier(**src)
    else:
        sim.source_planewave(**src)
    return sp, sim.absorption()


# HBM footprint of one sweep point, in units of one n x n complex128 matrix (n = 2 (2 ox + 1)(2 oy + 1)): measured on MI355X with the caching
# allocator -- single patterned layer, order [15,15], 128 points: 75.8 GB allocated / 111.8 GB reserved = 10.0 / 14.8 matrices per point; 4-layer stack
# with the streaming cascade, order [21,21], 64 points: 228 / 247 GB = 16.3 / 17.6.  precision="native" halves the element.
_POINT_MATRICES = {1: 15.0, 2: 18.0}          # layers == 1 / layers >= 2 (what the allocator RESERVES, which is what must fit)
# fourier_rule="li": Ex and Ey (two N x N = n^2 / 4 matrices each) live next to E, E^-1 and the assembly workspace until A exists
_LI_EXTRA = 0.5
# fourier_rule="normal": Exx, Exy, Eyy (three N x N) next to E, E^-1 while A is built, and inside trx_convmat_nv the workspace ([1/eps], its
# inverse's workspace and the three product matrices: five more N x N) -- 8 N^2 = 2 n^2
_NV_EXTRA = 2.0
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


def auto_chunk(B, order, n_layers, precision, device, dtype=torch.complex64, streams=1, fourier_rule="laurent", absorption=False):
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


def auto_thickness_chunk(B, T, n, m, cdtype, device):
    """Thicknesses per trx_thickness_columns call that fit the free HBM of `device` next to B resident points (_THICKNESS_MATRICES), with
    _HEADROOM to spare; T when everything fits.  Raises with the numbers when not even one thickness fits."""
    if device.type != "cuda":
        return T
    elem = 16 if cdtype == torch.complex128 else 8
    per = B * ((_THICKNESS_MATRICES * n * n + 5 * n * m) * elem + 4 * (n + 1))
    free, total = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    fit = int((free - _HEADROOM * total) // per)
    if fit < 1:
        raise RuntimeError("torcwa_amd thickness sweep: one thickness of %d points needs about %.1f GB of HBM (%d x %d complex matrices x %.0f per "
                           "point), but only %.1f GB are free on %s; lower the chunk of points" % (B, per / 1e9, n, n, _THICKNESS_MATRICES, free / 1e9, device))
    return min(int(T), fit)


def _slice(v, lo, hi, B):
    """Per-point quantities are [B] vectors or [B,nx,ny] grids; a 2-D tensor is a grid SHARED by all points and is never cut
    (a 128 x 128 grid in a 128-point sweep is not a per-point quantity)."""
    if torch.is_tensor(v) and v.dim() in (1, 3) and v.shape[0] == B:
        return v[lo:hi]
    return v


def _source_amplitudes(source, B):
    """(M, per_point) of a sweep's source keywords: M orders, and whether `amplitude` carries a leading B.  Anything else is refused here,
    before any chunk is solved."""
    if not source or "amplitude" not in source:
        return 1, False
    M = int(torch.as_tensor(source["orders"]).numel() // 2) if "orders" in source else 1
    k = int(torch.as_tensor(source["amplitude"]).numel())
    if k == 2 * M:
        return M, False
    if k == 2 * M * B:
        return M, True
    raise ValueError(f"source amplitude must hold [{M}, 2] values (shared by the sweep) or [{B}, {M}, 2] (one per sweep point), got {k} values")


def solve_stack_sweep(freq, layers, order, L, *, eps_in=None, eps_out=None, inc_ang=0.0, azi_ang=0.0, dtype=torch.complex64,
                      precision="high", engine=None, chunk=None, streams=1, orders=((0, 0),), polarization="xx",
                      direction="forward", port="transmission", check_info=True, eig_route="auto", fourier_rule="laurent",
                      nv_sigma=NV_SIGMA_DEFAULT, absorption=False, source=None, symmetry=None, symmetry_tol=1e-6, symmetry_sector=False):
    """B sweep points of a multi-layer stack (BASELINE.json configs 2-4): the reference's per-point Python loop
    (example/Example1-1.ipynb, Example3.ipynb) as chunks of a batched solve.  `layers` as in `_solve_chunk`, with
    per-point quantities carrying a leading dimension B = len(freq).  Returns the requested S-parameter [B, len(orders)].

    eig_route: "auto" (mixed-precision eigensolver; once a chunk of THIS call had to redo matrices in fp64, the remaining layers and chunks
    of this call use the all-fp64 route -- BatchedRCWA._eig_call), "mixed" or "fp64".

    fourier_rule: "laurent" (default), "li" (Li's inverse rule in every patterned layer, BatchedRCWA) or "normal" (the normal-vector method,
    the field derived from each grid with a Gaussian of nv_sigma cells).

    symmetry: None | "x" | "y" | "xy" -- mirror planes of every patterned layer (kx0 = 0 / ky0 = 0 at every point); each layer eigenproblem is
    folded into 2 / 4 independent blocks (BatchedRCWA, torcwa_amd/symmetry.py).  ValueError from the first chunk if a grid, the order set, the
    lattice or an angle does not have the mirror; symmetry_tol: the relative grid asymmetry that is accepted (and symmetrised away).

    symmetry_sector=True (needs symmetry=, every patterned layer about the same mirror planes; not with absorption=True): only the mirror
    sectors the requested columns excite are solved -- eigenproblem, layer S-matrices and star products of about n / 4 for an x- or
    y-polarised (0, 0) order under "xy" (BatchedRCWA).

    absorption=True: every chunk is solved with keep_coupling=True and without the streaming cascade (more HBM per point: auto_chunk), the source
    is applied -- `source`: keywords of BatchedRCWA.source_planewave, or of source_fourier when it has "orders"; default a unit plane wave,
    amplitude [1, 0], notation "xy", in the call's `direction`; an amplitude with a leading B is cut into the chunks like every other per-point
    input -- and the call returns
    (S-parameters, absorption dict) with the dict's tensors ("layers" [B, n_layers], "R", "T", "A" [B]) concatenated over the chunks.  With the
    default absorption=False the code path, the return value and the memory model are unchanged."""
    from .engine import default_engine
    check_fourier_rule(fourier_rule)
    if symmetry_sector and absorption:
        raise ValueError("symmetry_sector=True is not available with absorption=True: a sector solve keeps no coupling matrices")
    if symmetry_sector and symmetry is None:
        raise ValueError('symmetry_sector=True needs symmetry="x" | "y" | "xy"')
    B = freq.shape[0]
    eng = engine if engine is not None else default_engine()
    old_check, eng.check_info = eng.check_info, check_info         # restored below: the engine may be shared with other solvers
    # chunk=None: as many points in lock-step as the free HBM holds (the reference's per-point loop cannot run out of memory; neither must this)
    chunk = (auto_chunk(B, order, len(layers), precision, freq.device, dtype=dtype, streams=streams, fourier_rule=fourier_rule,
                        **({"absorption": True} if absorption else {})) if not chunk
             else int(chunk))
    if streams > 1 and chunk >= B:
        chunk = -(-B // streams)
    spans = [(lo, min(B, lo + chunk)) for lo in range(0, B, chunk)]
    outs = [None] * len(spans)
    route_hint = {}                     # shared by the chunks of this call only
    n_src, src_per_point = _source_amplitudes(source, B) if absorption else (1, False)

    def run(i):
        lo, hi = spans[i]
        lays = [tuple(_slice(v, lo, hi, B) for v in lay) for lay in layers]
        src = source
        if src_per_point:
            src = dict(source, amplitude=torch.as_tensor(source["amplitude"]).reshape(B, n_src, 2)[lo:hi])
        outs[i] = _solve_chunk(freq[lo:hi], lays, order, L, _slice(eps_in, lo, hi, B), _slice(eps_out, lo, hi, B), _slice(inc_ang, lo, hi, B),
                               _slice(azi_ang, lo, hi, B), dtype, precision, engine, orders, polarization, direction, port, check_info,
                               eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma,
                               **({"absorption": True, "source": src} if absorption else {}),
                               symmetry=symmetry, symmetry_tol=symmetry_tol, **({"symmetry_sector": True} if symmetry_sector else {}))

    dev = freq.device
    try:
        _run_spans(run, spans, streams, dev)
    finally:
        eng.check_info = old_check
    if absorption:
        return (torch.cat([o[0] for o in outs], dim=0), {k: torch.cat([o[1][k] for o in outs], dim=0) for k in outs[0][1]})
    return torch.cat(outs, dim=0)


def _run_spans(run, spans, streams, dev):
    import threading
    if streams <= 1 or len(spans) == 1 or dev.type != "cuda":
        for i in range(len(spans)):
            run(i)
    else:
        cur = torch.cuda.current_stream(dev)
        pool = [torch.cuda.Stream(device=dev) for _ in range(streams)]
        errors = []

        def worker(w):
            try:
                with torch.cuda.device(dev), torch.cuda.stream(pool[w]):
                    pool[w].wait_stream(cur)
                    for i in range(w, len(spans), streams):
                        run(i)
            except BaseException as e:      # noqa: BLE001 - re-raised on the caller's thread
                errors.append(e)

        threads = [threading.Thread(target=worker, args=(w,)) for w in range(streams)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        for st in pool:
            cur.wait_stream(st)


def solve_single_layer_sweep(freq, eps_grids, thickness, order, L, **kw):
    """B sweep points of a 1-patterned-layer stack (configs 2 and 4 of BASELINE.json): freq [B], eps_grids [B,nx,ny].  Keywords as
    solve_stack_sweep (fourier_rule="li": Li's inverse rule; "normal": the normal-vector method, nv_sigma).

    chunk   : points solved in lock-step by one batched solver (bounds the HBM footprint; default None = as many as the free HBM holds with
              10 % headroom, `auto_chunk`).  At order [15,15] (n = 1922) a point costs about 0.6 GB allocated / 0.9 GB reserved, so about 256 points
              fit the 288 GB of an MI355X, and larger chunks are faster (measured, round 5: 15.7 / 22.1 / 27.9 / 32.2 layer-solves/s at 16 / 32 / 64 / 128 points).
    streams : number of HIP streams / host threads the chunks are dealt to (default 1: one lock-step chunk is faster on MI355X -- two half
              sweeps on two threads 18.3 layer-solves/s against 33.6, and 28.9 - 31.3 with CU-masked streams that keep the other half's GEMM
              grids off a reserved set of compute units: profiles/r06_ab/cumask.txt).
    """
    return solve_stack_sweep(freq.to(eps_grids.device), [(thickness, eps_grids)], order, L, **kw)


def solve_thickness_sweep(freq, layers, order, L, *, layer=0, thicknesses, eps_in=None, eps_out=None, inc_ang=0.0, azi_ang=0.0,
                          dtype=torch.complex64, precision="high", engine=None, chunk=None, streams=1, orders=((0, 0),), polarization="xx",
                          direction="forward", port="transmission", check_info=True, eig_route="auto", fourier_rule="laurent",
                          nv_sigma=NV_SIGMA_DEFAULT, symmetry=None, symmetry_tol=1e-6, thickness_chunk=None):
    """B sweep points x T thicknesses of ONE layer of a stack: the modes of `layers[layer]` are computed once per point and every thickness
    costs one GEMM and one LU (BatchedRCWA.add_layer(..., swept=True)) instead of a new eigendecomposition.  Returns [B, T, len(orders)].

    layers as in solve_stack_sweep; the thickness entry of layers[layer] is ignored and may be None.  thicknesses: [T] (shared by the points)
    or [B, T].  Keywords as solve_stack_sweep, without absorption / source (a swept solve keeps no coupling matrices).  chunk: points solved in
    lock-step (default: auto_chunk); thickness_chunk: thicknesses per library call (default: what the free HBM holds, `auto_thickness_chunk`)."""
    from .engine import default_engine
    check_fourier_rule(fourier_rule)
    B = freq.shape[0]
    layer = int(layer)
    if not (-len(layers) <= layer < len(layers)):
        raise ValueError(f"layer must index one of the {len(layers)} layers, got {layer}")
    layer %= len(layers)
    d = torch.as_tensor(thicknesses)
    if d.dim() == 1:
        per_point = False
    elif d.dim() == 2 and d.shape[0] == B:
        per_point = True
    else:
        raise ValueError(f"thicknesses must be [T] or [{B}, T], got {list(d.shape)}")
    eng = engine if engine is not None else default_engine()
    old_check, eng.check_info = eng.check_info, check_info
    chunk = auto_chunk(B, order, len(layers), precision, freq.device, dtype=dtype, streams=streams, fourier_rule=fourier_rule) if not chunk else int(chunk)
    if streams > 1 and chunk >= B:
        chunk = -(-B // streams)
    spans = [(lo, min(B, lo + chunk)) for lo in range(0, B, chunk)]
    outs = [None] * len(spans)
    route_hint = {}

    def run(i):
        lo, hi = spans[i]
        sim = BatchedRCWA(freq[lo:hi], order, L, dtype=dtype, precision=precision, engine=engine, keep_coupling=False, fold_layers=True,
                          eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma, symmetry=symmetry,
                          symmetry_tol=symmetry_tol)
        sim.thickness_chunk = thickness_chunk
        if eps_in is not None:
            sim.add_input_layer(eps=_slice(eps_in, lo, hi, B))
        if eps_out is not None:
            sim.add_output_layer(eps=_slice(eps_out, lo, hi, B))
        sim.set_incident_angle(_slice(inc_ang, lo, hi, B), _slice(azi_ang, lo, hi, B))
        for j, lay in enumerate(layers):
            lay = tuple(_slice(v, lo, hi, B) for v in lay)
            if j == layer:
                sim.add_layer(d[lo:hi] if per_point else d, *lay[1:], swept=True)
            else:
                sim.add_layer(*lay)
        outs[i] = sim.solve_S_parameters([list(o) for o in orders], direction=direction, port=port, polarization=polarization)

    try:
        _run_spans(run, spans, streams, freq.device)
    finally:
        eng.check_info = old_check
    return torch.cat(outs, dim=0)
