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
from .engine import default_engine
from .shapes import ShapeLayer
from .memory import auto_chunk, auto_thickness_chunk  # noqa: F401  (the HBM model: re-exported, the benchmark and the tests take it from here)

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
                 polarization, direction, port, eig_route="auto", route_hint=None, fourier_rule="laurent", nv_sigma=NV_SIGMA_DEFAULT, shape_nv_grid=None,
                 absorption=False, source=None, symmetry=None, symmetry_tol=1e-6, symmetry_sector=False):
    """layers: list of (thickness, eps[, mu]); thickness scalar or [b]; eps/mu scalar, [b] or [b,nx,ny].  absorption: the chunk keeps W, V and
    the coupling matrices (keep_coupling=True, no streaming cascade) and returns (S-parameters, BatchedRCWA.absorption())."""
    sim = BatchedRCWA(freq, order, L, dtype=dtype, precision=precision, engine=engine, keep_coupling=bool(absorption), fold_layers=not absorption,
                      eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma, shape_nv_grid=shape_nv_grid,
                      symmetry=symmetry, symmetry_tol=symmetry_tol, symmetry_sector=symmetry_sector)
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


def _slice(v, lo, hi, B):
    """Per-point quantities are [B] vectors or [B,nx,ny] grids; a 2-D tensor is a grid SHARED by all points and is never cut
    (a 128 x 128 grid in a 128-point sweep is not a per-point quantity)."""
    if torch.is_tensor(v) and v.dim() in (1, 3) and v.shape[0] == B:
        return v[lo:hi]
    if isinstance(v, ShapeLayer) and v.batch == B:          # per-point shape parameters are cut, shared ones kept
        return v.slice(lo, hi)
    return v


def _shape_grid_of(layers, shape_nv_grid):
    """shape_nv_grid for the memory model when a layer of the stack is a ShapeLayer (its field products are sampled per point), else None."""
    return shape_nv_grid if any(isinstance(v, ShapeLayer) for lay in layers for v in lay) else None


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
                      nv_sigma=NV_SIGMA_DEFAULT, shape_nv_grid=None, absorption=False, source=None, symmetry=None, symmetry_tol=1e-6, symmetry_sector=False):
    """B sweep points of a multi-layer stack (BASELINE.json configs 2-4): the reference's per-point Python loop
    (example/Example1-1.ipynb, Example3.ipynb) as chunks of a batched solve.  `layers` as in `_solve_chunk`, with
    per-point quantities carrying a leading dimension B = len(freq).  Returns the requested S-parameter [B, len(orders)].

    eig_route: "auto" (mixed-precision eigensolver; once a chunk of THIS call had to redo matrices in fp64, the remaining layers and chunks
    of this call use the all-fp64 route -- BatchedRCWA._eig_call), "mixed" or "fp64".

    fourier_rule: "laurent" (default), "li" (Li's inverse rule in every patterned layer, BatchedRCWA) or "normal" (the normal-vector method,
    the field derived from each grid with a Gaussian of nv_sigma cells; for a ShapeLayer the blended field of the shape list sampled on
    shape_nv_grid, an int or (n1, n2)).

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
    check_fourier_rule(fourier_rule)
    if symmetry_sector and absorption:
        raise ValueError("symmetry_sector=True is not available with absorption=True: a sector solve keeps no coupling matrices")
    if symmetry_sector and symmetry is None:
        raise ValueError('symmetry_sector=True needs symmetry="x" | "y" | "xy"')
    B = freq.shape[0]
    n_src, src_per_point = _source_amplitudes(source, B) if absorption else (1, False)

    def solve(lo, hi, route_hint):
        lays = [tuple(_slice(v, lo, hi, B) for v in lay) for lay in layers]
        src = source
        if src_per_point:
            src = dict(source, amplitude=torch.as_tensor(source["amplitude"]).reshape(B, n_src, 2)[lo:hi])
        return _solve_chunk(freq[lo:hi], lays, order, L, _slice(eps_in, lo, hi, B), _slice(eps_out, lo, hi, B), _slice(inc_ang, lo, hi, B),
                            _slice(azi_ang, lo, hi, B), dtype, precision, engine, orders, polarization, direction, port,
                            eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma, shape_nv_grid=shape_nv_grid, absorption=absorption,
                            source=src if absorption else None, symmetry=symmetry, symmetry_tol=symmetry_tol, symmetry_sector=symmetry_sector)

    # chunk=None: as many points in lock-step as the free HBM holds (the reference's per-point loop cannot run out of memory; neither must this)
    outs = _solve_chunks(solve, B, freq.device, engine, check_info, streams, chunk or (lambda: auto_chunk(
        B, order, len(layers), precision, freq.device, dtype=dtype, streams=streams, fourier_rule=fourier_rule, absorption=absorption,
        shape_nv_grid=_shape_grid_of(layers, shape_nv_grid))))
    if absorption:
        return (torch.cat([o[0] for o in outs], dim=0), {k: torch.cat([o[1][k] for o in outs], dim=0) for k in outs[0][1]})
    return torch.cat(outs, dim=0)


def _solve_chunks(solve, B, dev, engine, check_info, streams, chunk):
    """What the sweep drivers share: the B points are cut into chunks of `chunk` points (an int, or a callable that chooses it once the engine
    is set), the chunks are dealt to `streams` streams, and solve(lo, hi, route_hint) -> the result of points lo .. hi - 1 is called for each;
    route_hint is the dict the chunks of this one call share (BatchedRCWA._eig_call).  Returns the results in sweep order.  The engine's
    check_info is set for the call and restored: the engine may be shared with other solvers."""
    eng = engine if engine is not None else default_engine()
    old_check, eng.check_info = eng.check_info, check_info
    try:
        chunk = int(chunk() if callable(chunk) else chunk)
        if streams > 1 and chunk >= B:
            chunk = -(-B // streams)
        spans = [(lo, min(B, lo + chunk)) for lo in range(0, B, chunk)]
        outs = [None] * len(spans)
        route_hint = {}

        def run(i):
            outs[i] = solve(*spans[i], route_hint)

        _run_spans(run, spans, streams, dev)
    finally:
        eng.check_info = old_check
    return outs


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
    if isinstance(eps_grids, ShapeLayer):            # vector shapes carry no device of their own: freq goes to the engine's, as to a grid's
        eng = kw.get("engine") or default_engine()
        return solve_stack_sweep(freq.to(eng.device), [(thickness, eps_grids)], order, L, **kw)
    return solve_stack_sweep(freq.to(eps_grids.device), [(thickness, eps_grids)], order, L, **kw)


def solve_thickness_sweep(freq, layers, order, L, *, layer=0, thicknesses, eps_in=None, eps_out=None, inc_ang=0.0, azi_ang=0.0,
                          dtype=torch.complex64, precision="high", engine=None, chunk=None, streams=1, orders=((0, 0),), polarization="xx",
                          direction="forward", port="transmission", check_info=True, eig_route="auto", fourier_rule="laurent",
                          nv_sigma=NV_SIGMA_DEFAULT, shape_nv_grid=None, symmetry=None, symmetry_tol=1e-6, thickness_chunk=None):
    """B sweep points x T thicknesses of ONE layer of a stack: the modes of `layers[layer]` are computed once per point and every thickness
    costs one GEMM and one LU (BatchedRCWA.add_layer(..., swept=True)) instead of a new eigendecomposition.  Returns [B, T, len(orders)].

    layers as in solve_stack_sweep; the thickness entry of layers[layer] is ignored and may be None.  thicknesses: [T] (shared by the points)
    or [B, T].  Keywords as solve_stack_sweep, without absorption / source (a swept solve keeps no coupling matrices).  chunk: points solved in
    lock-step (default: auto_chunk); thickness_chunk: thicknesses per library call (default: what the free HBM holds, `auto_thickness_chunk`)."""
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

    def solve(lo, hi, route_hint):
        sim = BatchedRCWA(freq[lo:hi], order, L, dtype=dtype, precision=precision, engine=engine, keep_coupling=False, fold_layers=True,
                          eig_route=eig_route, route_hint=route_hint, fourier_rule=fourier_rule, nv_sigma=nv_sigma, shape_nv_grid=shape_nv_grid, symmetry=symmetry,
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
        return sim.solve_S_parameters([list(o) for o in orders], direction=direction, port=port, polarization=polarization)

    return torch.cat(_solve_chunks(solve, B, freq.device, engine, check_info, streams, chunk or (lambda: auto_chunk(
        B, order, len(layers), precision, freq.device, dtype=dtype, streams=streams, fourier_rule=fourier_rule,
        shape_nv_grid=_shape_grid_of(layers, shape_nv_grid)))), dim=0)
