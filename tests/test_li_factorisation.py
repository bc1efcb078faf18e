"""Li's inverse-rule Fourier factorisation (fourier_rule="li"): the kernels of trx_convmat_li / trx_build_pq_aniso / trx_build_a_aniso
against an in-test restatement of the formulas (include/trx.h), the full solver against the CPU oracle with Li's matrices swapped into Q,
gradients, physics on the MI355X (convergence in the order, energy, symmetry) and the unchanged default.

`emu` runs the small cases through the CPU kernel-logic emulator; `gpu` runs them, and the large orders, on MI355X.
"""
import math

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, get_backend
from tests.test_pipeline import make_engine

TRX_ERR_UNSUPPORTED = -5


# ---- restatement (torch on CPU, complex128; differentiable) -------------------------------------------------------------------------------
def _dft_matrix(n, o):
    r = torch.arange(n, dtype=torch.int64)[:, None]
    q = torch.arange(-2 * o, 2 * o + 1, dtype=torch.int64)[None, :]
    return torch.exp(-2j * math.pi * ((r * q) % n).to(torch.float64) / n)          # [n, 4o+1]


def _toeplitz_index(o):
    a = torch.arange(2 * o + 1)
    return a[:, None] - a[None, :] + 2 * o


def li_ref(grid, ox, oy):
    """(Ex, Ey) [N,N] of one [nx,ny] grid, straight from the definitions (per-row DFT, torch.linalg.inv per row, DFT along the other axis)."""
    g = grid.to(torch.complex128)
    nx, ny = g.shape
    r = 1 / g
    wx, wy = 2 * ox + 1, 2 * oy + 1
    N = wx * wy
    ay = (r.transpose(0, 1) @ _dft_matrix(nx, ox)) / nx                             # [ny, 4ox+1]
    Uy = torch.linalg.inv(ay[:, _toeplitz_index(ox)])                               # [ny, wx, wx]
    F = torch.einsum("yab,yq->abq", Uy, _dft_matrix(ny, oy)) / ny                   # [wx, wx, 4oy+1]
    Ex = F[:, :, _toeplitz_index(oy)].permute(0, 2, 1, 3).reshape(N, N)             # [m, n, m', n']
    ax = (r @ _dft_matrix(ny, oy)) / ny                                             # [nx, 4oy+1]
    Ux = torch.linalg.inv(ax[:, _toeplitz_index(oy)])                               # [nx, wy, wy]
    G = torch.einsum("xab,xp->abp", Ux, _dft_matrix(nx, ox)) / nx                   # [wy, wy, 4ox+1]
    Ey = G[:, :, _toeplitz_index(ox)].permute(2, 0, 3, 1).reshape(N, N)             # [n, n', m, m'] -> [m, n, m', n']
    return Ex, Ey


def laurent_ref(grid, ox, oy):
    from oracle.rcwa_oracle import conv_matrix
    return conv_matrix(grid.to(torch.complex128), [ox, oy])


def pq_ref(Ex, Ey, E, Mx, My, M, kx, ky):
    """P, Q of a patterned layer with Li's matrices (block formulas of include/trx.h: trx_build_pq_aniso), dense."""
    Kx, Ky = torch.diag(kx), torch.diag(ky)
    Ei, Mi = torch.linalg.inv(E), torch.linalg.inv(M)
    P = torch.cat((torch.cat((Kx @ Ei @ Ky, My - Kx @ Ei @ Kx), 1), torch.cat((Ky @ Ei @ Ky - Mx, -Ky @ Ei @ Kx), 1)), 0)
    Q = torch.cat((torch.cat((-Kx @ Mi @ Ky, Kx @ Mi @ Kx - Ey), 1), torch.cat((Ex - Ky @ Mi @ Ky, Ky @ Mi @ Kx), 1)), 0)
    return P, Q


def _grid(nx, ny, cplx, seed, eps=(4.0, 16.0)):
    """Rectangle-ish high-contrast grid with some texture (no zero)."""
    rng = np.random.default_rng(seed)
    g = np.full((nx, ny), eps[0])
    g[nx // 5: 3 * nx // 5 + 1, ny // 4: ny // 2 + 2] = eps[1]
    g = g + 0.3 * rng.random((nx, ny))
    if cplx:
        g = g + 1j * (0.1 + 0.5 * rng.random((nx, ny)))
    return g


# ---- 1. kernel against the restatement ----------------------------------------------------------------------------------------------------
def _run_li(be, grids, ox, oy, dt, keep=False):
    B, nx, ny = grids.shape
    cplx = np.iscomplexobj(grids)
    rdt = np.float64 if dt == np.complex128 else np.float32
    gin = be.dev(grids.astype(dt if cplx else rdt))
    N = (2 * ox + 1) * (2 * oy + 1)
    Ex, Ey = be.empty((B, N, N), dt), be.empty((B, N, N), dt)
    Ux = be.empty((B, nx, 2 * oy + 1, 2 * oy + 1), np.complex128) if keep else None
    Uy = be.empty((B, ny, 2 * ox + 1, 2 * ox + 1), np.complex128) if keep else None
    info = be.empty((B,), np.int32)
    code = 1 if dt == np.complex128 else 0
    nws = be.lib.convmat_li_ws_bytes(code, B, nx, ny, ox, oy)
    ws = be.empty((max(nws, 16),), np.uint8)
    rc = be.lib.convmat_li(code, int(cplx), be.ptr(gin), B, nx, ny, ox, oy, be.ptr(Ex), be.ptr(Ey), be.ptr(Ux) if keep else None,
                           be.ptr(Uy) if keep else None, be.ptr(info), be.ptr(ws), nws, be.stream)
    if rc != 0:
        return rc, None, None, None
    return rc, be.host(Ex), be.host(Ey), be.host(info)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dt,tol", [(np.complex128, 1e-12), (np.complex64, 2e-6)])
@pytest.mark.parametrize("nx,ny,ox,oy,cplx", [(13, 9, 2, 1, False), (11, 14, 1, 3, True), (12, 10, 0, 2, True), (10, 12, 3, 0, False)])
def test_convmat_li_matches_restatement(backend, dt, tol, nx, ny, ox, oy, cplx):
    be = get_backend(backend)
    grids = np.stack([_grid(nx, ny, cplx, s) for s in range(3)])
    rc, Ex, Ey, info = _run_li(be, grids, ox, oy, dt, keep=(dt == np.complex128))
    assert rc == 0 and not info.any()
    for b in range(3):
        rx, ry = li_ref(torch.as_tensor(grids[b]), ox, oy)
        assert _rel(Ex[b], rx.numpy()) < tol
        assert _rel(Ey[b], ry.numpy()) < tol


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_li_chunked_rows(backend):
    """Small orders on a finer grid: the inverses of one direction are held a chunk of rows at a time (workspace bound)."""
    be = get_backend(backend)
    grids = np.stack([_grid(40, 33, True, s) for s in range(2)])
    rc, Ex, Ey, info = _run_li(be, grids, 1, 1, np.complex128)
    assert rc == 0 and not info.any()
    for b in range(2):
        rx, ry = li_ref(torch.as_tensor(grids[b]), 1, 1)
        assert _rel(Ex[b], rx.numpy()) < 1e-12 and _rel(Ey[b], ry.numpy()) < 1e-12


@pytest.mark.parametrize("backend", BACKENDS)
def test_convmat_li_reports_zero_and_unsupported(backend):
    be = get_backend(backend)
    grids = np.stack([_grid(9, 8, False, s) for s in range(3)])
    grids[1, 4, 3] = 0.0
    rc, _, _, info = _run_li(be, grids, 1, 1, np.complex128)
    assert rc == 0 and info[1] != 0 and info[0] == 0 and info[2] == 0
    # 2*50+1 = 101: one Toeplitz block no longer fits the LDS of a CU
    code = 1
    lib = be.lib
    nws = lib.convmat_li_ws_bytes(code, 1, 128, 8, 50, 1)
    g = be.dev(np.ones((1, 128, 8)))
    out = be.empty((2,), np.complex128)
    info = be.empty((1,), np.int32)
    ws = be.empty((16,), np.uint8)
    rc = lib.convmat_li(code, 0, be.ptr(g), 1, 128, 8, 50, 1, be.ptr(out), be.ptr(out), None, None, be.ptr(info), be.ptr(ws), nws, be.stream)
    assert rc == TRX_ERR_UNSUPPORTED


# ---- 2. identities ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_li_identities(backend):
    be = get_backend(backend)
    ox = oy = 2
    N = 25
    # uniform grid: Ex = Ey = eps I
    rc, Ex, Ey, _ = _run_li(be, np.full((1, 11, 11), 3.5 + 0.2j), ox, oy, np.complex128)
    assert _rel(Ex[0], (3.5 + 0.2j) * np.eye(N)) < 1e-13 and _rel(Ey[0], (3.5 + 0.2j) * np.eye(N)) < 1e-13
    # y-invariant grid: Ey = Laurent E, Ex = inv(Toeplitz_x(1/eps)) (x) I
    row = _grid(11, 1, False, 3)[:, 0]
    g = np.repeat(row[:, None], 12, axis=1)
    rc, Ex, Ey, _ = _run_li(be, g[None], ox, oy, np.complex128)
    assert _rel(Ey[0], laurent_ref(torch.as_tensor(g), ox, oy).numpy()) < 1e-12
    a = np.fft.fft(1 / row) / 11
    T = np.array([[a[(m - mp) % 11] for mp in range(5)] for m in range(5)])
    assert _rel(Ex[0], np.kron(np.linalg.inv(T), np.eye(5))) < 1e-12
    # transposed grid (ox = oy): Ex <-> Ey under (m,n) <-> (n,m)
    g = _grid(12, 10, True, 4)
    _, Ex1, Ey1, _ = _run_li(be, g[None], ox, oy, np.complex128)
    _, Ex2, Ey2, _ = _run_li(be, np.ascontiguousarray(g.T)[None], ox, oy, np.complex128)
    perm = np.arange(N).reshape(5, 5).T.reshape(-1)
    assert _rel(Ex2[0], Ey1[0][np.ix_(perm, perm)]) < 1e-12 and _rel(Ey2[0], Ex1[0][np.ix_(perm, perm)]) < 1e-12
    # real grid: Hermitian
    _, Ex, Ey, _ = _run_li(be, _grid(13, 11, False, 5)[None], ox, oy, np.complex128)
    for M in (Ex[0], Ey[0]):
        assert np.abs(M - M.conj().T).max() < 1e-13 * np.abs(M).max()


# ---- 3. build_pq_aniso / build_a_aniso ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_build_pq_a_aniso(backend):
    eng = make_engine(backend)
    dev = eng.device
    B, ox, oy = 2, 2, 1
    N = (2 * ox + 1) * (2 * oy + 1)
    rng = np.random.default_rng(7)
    grids = [_grid(11, 9, True, s) for s in range(B)]
    mgrid = [1 + 0.5 * _grid(11, 9, False, 10 + s) for s in range(B)]
    E = torch.stack([laurent_ref(torch.as_tensor(g), ox, oy) for g in grids])
    M = torch.stack([laurent_ref(torch.as_tensor(g), ox, oy) for g in mgrid])
    Exy = [li_ref(torch.as_tensor(g), ox, oy) for g in grids]
    Mxy = [li_ref(torch.as_tensor(g), ox, oy) for g in mgrid]
    Ex, Ey = torch.stack([e[0] for e in Exy]), torch.stack([e[1] for e in Exy])
    Mx, My = torch.stack([e[0] for e in Mxy]), torch.stack([e[1] for e in Mxy])
    kx = torch.as_tensor(rng.standard_normal((B, N)) + 0.1j * rng.standard_normal((B, N)))
    ky = torch.as_tensor(rng.standard_normal((B, N)) + 0.1j * rng.standard_normal((B, N)))
    mu = torch.tensor([1.0 + 0j, 1.3 + 0.1j], dtype=torch.complex128)
    Ei, Mi = torch.linalg.inv(E), torch.linalg.inv(M)
    d = lambda t: t.to(dev).contiguous()
    P, Q = eng.build_pq_aniso(d(Ex), d(Ey), d(Ei), d(Mx), d(My), d(Mi), d(kx), d(ky))
    for b in range(B):
        Pr, Qr = pq_ref(Ex[b], Ey[b], E[b], Mx[b], My[b], M[b], kx[b], ky[b])
        assert _rel(P[b].cpu(), Pr) < 1e-12 and _rel(Q[b].cpu(), Qr) < 1e-12
    A = eng.build_a_aniso(d(Ex), d(Ey), d(Ei), d(mu), d(kx), d(ky)).cpu()
    for b in range(B):
        I = torch.eye(N, dtype=torch.complex128)
        Pr, Qr = pq_ref(Ex[b], Ey[b], E[b], mu[b] * I, mu[b] * I, mu[b] * I, kx[b], ky[b])
        assert _rel(A[b], Pr @ Qr) < 1e-12
    # Ex = Ey = E, Mx = My = M: the Laurent entry points (one implementation behind both: identical results)
    P0, Q0 = eng.build_pq(d(E), d(Ei), d(M), d(Mi), d(kx), d(ky))
    P1, Q1 = eng.build_pq_aniso(d(E), d(E), d(Ei), d(M), d(M), d(Mi), d(kx), d(ky))
    assert torch.equal(P1.cpu(), P0.cpu()) and torch.equal(Q1.cpu(), Q0.cpu())
    A0 = eng.build_a(d(E), d(Ei), d(mu), d(kx), d(ky)).cpu()
    A1 = eng.build_a_aniso(d(E), d(E), d(Ei), d(mu), d(kx), d(ky)).cpu()
    assert torch.equal(A1, A0)


# ---- 4. full path against the oracle with Li's matrices in Q (and P for a patterned mu) -----------------------------------------------------
@pytest.fixture
def li_oracle(monkeypatch):
    """oracle.rcwa_oracle with Li's factorisation: conv_matrix tags the Laurent matrix with the restatement's (Ex, Ey) of its grid, and
    pq_patterned uses them (the oracle itself is not edited)."""
    from oracle import rcwa_oracle as orc
    conv0 = orc.conv_matrix

    def conv(grid, order):
        E = conv0(grid, order)
        E._li = li_ref(grid, order[0], order[1])
        return E

    def pq(E, M, kx, ky):
        Ex, Ey = getattr(E, "_li", (E, E))
        Mx, My = getattr(M, "_li", (M, M))
        return pq_ref(Ex, Ey, E, Mx, My, M, kx, ky)

    monkeypatch.setattr(orc, "conv_matrix", conv)
    monkeypatch.setattr(orc, "pq_patterned", pq)
    return orc


ORD = [3, 2]
LAM, LX, LY = 1.0, 0.7, 0.55


def _stack(seed):
    g1 = torch.as_tensor(_grid(24, 20, True, seed, eps=(2.0, 9.0)))
    g2 = torch.as_tensor(_grid(24, 20, False, seed + 1, eps=(1.5, 6.0)))
    return [(0.31, g1), (0.17, g2)]


def _mu_stack(seed):
    g = torch.as_tensor(_grid(24, 20, True, seed, eps=(2.0, 7.0)))
    mu = torch.as_tensor(1.0 + 0.4 * _grid(24, 20, False, seed + 2, eps=(0.0, 1.0)))
    return [(0.23, g, mu)]


def _oracle_s(orc, freq, layers, inc, azi):
    s, _, S, _ = orc.solve_stack(freq, ORD, [LX, LY], layers, eps_in=1.5, eps_out=2.25, inc_ang=inc, azi_ang=azi)
    return torch.stack([orc.s_parameters(s, S, [[0, 0], [1, 0], [0, -1]], polarization=p) for p in ("xx", "xy", "yx", "yy")])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-9), (torch.complex64, 1e-5)])
@pytest.mark.parametrize("stack", ["two_layers", "patterned_mu"])
def test_rcwa_li_against_oracle(backend, dtype, tol, stack, li_oracle):
    import torcwa_amd
    eng = make_engine(backend)
    layers = _stack(1) if stack == "two_layers" else _mu_stack(3)
    inc, azi = 0.35, 0.2
    ref = _oracle_s(li_oracle, 1 / LAM, layers, inc, azi)
    sim = torcwa_amd.rcwa(freq=1 / LAM, order=ORD, L=[LX, LY], dtype=dtype, engine=eng, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=inc, azi_ang=azi)
    for lay in layers:
        d, e = lay[0], lay[1]
        cast = (lambda t: t.to(torch.complex64 if t.is_complex() else torch.float32)) if dtype == torch.complex64 else (lambda t: t)
        kw = {"mu": cast(lay[2]).to(eng.device)} if len(lay) > 2 else {}
        sim.add_layer(thickness=d, eps=cast(e).to(eng.device), **kw)
    sim.solve_global_smatrix()
    got = torch.stack([sim.S_parameters(orders=[[0, 0], [1, 0], [0, -1]], polarization=p).cpu() for p in ("xx", "xy", "yx", "yy")])
    assert float((got.to(torch.complex128) - ref).abs().max() / ref.abs().max()) < tol
    assert sim.eps_conv_x[0] is not None and sim.eps_conv_y[0] is not None


@pytest.mark.parametrize("backend", BACKENDS)
def test_batched_and_sweep_li_against_oracle(backend, li_oracle):
    import torcwa_amd
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    dev = eng.device
    B = 3
    lam = torch.tensor([1.0, 1.1, 0.93], dtype=torch.float64)
    inc = torch.tensor([0.3, 0.1, 0.45], dtype=torch.float64)
    azi = torch.tensor([0.2, 0.0, 0.5], dtype=torch.float64)
    grids = torch.stack([torch.as_tensor(_grid(24, 20, True, 11 + b, eps=(2.0, 9.0))) for b in range(B)])
    ref = torch.stack([li_oracle.s_parameters(*_solve1(li_oracle, 1 / float(lam[b]), grids[b], float(inc[b]), float(azi[b])), [[0, 0], [1, 0]],
                                              polarization="xx") for b in range(B)])
    sim = torcwa_amd.BatchedRCWA(1 / lam, ORD, [LX, LY], dtype=torch.complex128, engine=eng, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc.to(dev), azi.to(dev))
    sim.add_layer(thickness=0.29, eps=grids.to(dev))
    sim.solve_global_smatrix()
    got = sim.S_parameters([[0, 0], [1, 0]], polarization="xx").cpu()
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-9
    sw = solve_stack_sweep((1 / lam).to(dev), [(0.29, grids.to(dev))], ORD, [LX, LY], eps_in=1.5, eps_out=2.25, inc_ang=inc.to(dev),
                           azi_ang=azi.to(dev), dtype=torch.complex128, engine=eng, orders=((0, 0), (1, 0)), fourier_rule="li").cpu()
    assert float((sw - ref).abs().max() / ref.abs().max()) < 1e-9


def _solve1(orc, freq, grid, inc, azi):
    s, _, S, _ = orc.solve_stack(freq, ORD, [LX, LY], [(0.29, grid)], eps_in=1.5, eps_out=2.25, inc_ang=inc, azi_ang=azi)
    return s, S


# ---- 6. gradients -------------------------------------------------------------------------------------------------------------------------
def _fom_gpu(eng, grid, thick):
    import torcwa_amd
    sim = torcwa_amd.rcwa(freq=1 / LAM, order=[3, 3], L=[LX, LX], dtype=torch.complex128, engine=eng, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.set_incident_angle(inc_ang=0.2, azi_ang=0.1)
    sim.add_layer(thickness=thick, eps=grid)
    sim.solve_global_smatrix()
    t = sim.S_parameters(orders=[[0, 0]], polarization="xx")
    r = sim.S_parameters(orders=[[-1, 0]], port="reflection", polarization="xx")
    return (t.abs() ** 2).sum() + (r.abs() ** 2).sum()


def _fom_oracle(orc, grid, thick):
    s, _, S, _ = orc.solve_stack(1 / LAM, [3, 3], [LX, LX], [(thick, grid)], eps_in=1.5, inc_ang=0.2, azi_ang=0.1)
    t = orc.s_parameters(s, S, [[0, 0]], polarization="xx")
    r = orc.s_parameters(s, S, [[-1, 0]], port="reflection", polarization="xx")
    return (t.abs() ** 2).sum() + (r.abs() ** 2).sum()


class _EigRef(torch.autograd.Function):
    """torch.linalg.eig with the Lorentzian-broadened adjoint of torcwa_amd.Eig (include/trx.h: trx_eig_backward), in torch on CPU."""

    @staticmethod
    def forward(ctx, A):
        w, V = torch.linalg.eig(A)
        ctx.save_for_backward(w, V)
        return w, V

    @staticmethod
    def backward(ctx, gw, gV):
        w, V = ctx.saved_tensors
        gw = torch.zeros_like(w) if gw is None else gw
        gV = torch.zeros_like(V) if gV is None else gV
        s = w[None, :] - w[:, None]
        F = s.conj() / (s.abs() ** 2 + 1e-10)
        F.fill_diagonal_(0)
        VH = V.conj().T
        return torch.linalg.solve(VH, (torch.diag(gw) + F.conj() * (VH @ gV)) @ VH)


def _modes_patterned_ref(P, Q):
    lam, W = _EigRef.apply(P @ Q)
    kz = torch.sqrt(lam)
    return torch.where(torch.imag(kz) < 0, -kz, kz), W


@pytest.mark.parametrize("backend", BACKENDS)
def test_li_gradients(backend, li_oracle, monkeypatch):
    monkeypatch.setattr(li_oracle, "modes_patterned", _modes_patterned_ref)
    eng = make_engine(backend)
    dev = eng.device
    g0 = torch.as_tensor(_grid(24, 24, False, 21, eps=(2.0, 6.0)))
    th0 = 0.27
    grid = g0.clone().to(dev).requires_grad_(True)
    thick = torch.tensor(th0, dtype=torch.float64, device=dev, requires_grad=True)
    f = _fom_gpu(eng, grid, thick)
    gg, gt = torch.autograd.grad(f, (grid, thick))
    gg, gt = gg.cpu(), float(gt)
    # CPU autograd through the restatement
    gref = g0.clone().requires_grad_(True)
    tref = torch.tensor(th0, dtype=torch.float64, requires_grad=True)
    fr = _fom_oracle(li_oracle, gref, tref)
    rg, rt = torch.autograd.grad(fr, (gref, tref))
    assert abs(float(f.detach()) - float(fr.detach())) < 1e-10 * abs(float(fr.detach()))
    assert float((gg - rg).abs().max() / rg.abs().max()) < 1e-8
    assert abs(gt - float(rt)) < 1e-8 * abs(float(rt))
    # central finite differences (two grid cells and the thickness)
    h = 1e-5
    with torch.no_grad():
        for (i, j) in [(5, 7), (12, 4)]:
            gp, gm = g0.clone(), g0.clone()
            gp[i, j] += h
            gm[i, j] -= h
            fd = (float(_fom_gpu(eng, gp.to(dev), th0)) - float(_fom_gpu(eng, gm.to(dev), th0))) / (2 * h)
            assert abs(fd - float(gg[i, j])) < 1e-6 * float(gg.abs().max())
        fd = (float(_fom_gpu(eng, g0.to(dev), th0 + h)) - float(_fom_gpu(eng, g0.to(dev), th0 - h))) / (2 * h)
        assert abs(fd - gt) < 1e-6 * abs(gt)


# ---- 7. default unchanged, invalid value --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_default_rule_is_laurent_bit_for_bit(backend):
    import torcwa_amd
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    dev = eng.device
    layers = _stack(5)
    outs = []
    for kw in ({}, {"fourier_rule": "laurent"}):
        sim = torcwa_amd.rcwa(freq=1 / LAM, order=ORD, L=[LX, LY], dtype=torch.complex128, engine=eng, **kw)
        sim.add_input_layer(eps=1.5)
        sim.set_incident_angle(inc_ang=0.3, azi_ang=0.1)
        for d, e in layers:
            sim.add_layer(thickness=d, eps=e.to(dev))
        sim.solve_global_smatrix()
        outs.append(sim.S_parameters(orders=[[0, 0], [1, 0]], polarization="xy").cpu())
        assert all(t is None for t in sim.eps_conv_x)
    assert torch.equal(outs[0], outs[1])
    with pytest.raises(ValueError):
        torcwa_amd.rcwa(freq=1 / LAM, order=ORD, L=[LX, LY], engine=eng, fourier_rule="Li")
    with pytest.raises(ValueError):
        torcwa_amd.BatchedRCWA(1 / LAM, ORD, [LX, LY], engine=eng, fourier_rule="normal-vector")
    with pytest.raises(ValueError):
        solve_stack_sweep(torch.tensor([1.0], device=dev), [(0.2, layers[0][1][None].to(dev))], ORD, [LX, LY], engine=eng, fourier_rule="")


# ---- 5. physics on the MI355X (complex128; orders too large for the emulator) ----------------------------------------------------------------
def _lamellar(eng, order, rule, pol):
    """1-D lamellar metal grating: eps = (0.22+6.71i)^2, period = lambda = 1, fill 0.5, depth 0.3, air / eps 2.25, 0.2 rad incidence."""
    import torcwa_amd
    g = torch.ones((2000, 1), dtype=torch.complex128)
    g[:1000] = (0.22 + 6.71j) ** 2
    sim = torcwa_amd.rcwa(freq=1.0, order=order, L=[1.0, 1.0], dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=0.2, azi_ang=0.0)
    sim.add_layer(thickness=0.3, eps=g.to(eng.device))
    sim.solve_global_smatrix()
    r = sim.S_parameters(orders=[[0, 0]], port="reflection", polarization=pol)
    return float((r.abs() ** 2).sum())


@pytest.mark.gpu
def test_li_lamellar_metal_grating_converges(li_oracle):
    eng = make_engine("gpu")
    # converged reference: Li at [80,0] (a 161 x 161 Toeplitz block: beyond the LDS bound of trx_convmat_li) from the CPU restatement
    g = torch.ones((2000, 1), dtype=torch.complex128)
    g[:1000] = (0.22 + 6.71j) ** 2
    s, _, S, _ = li_oracle.solve_stack(1.0, [80, 0], [1.0, 1.0], [(0.3, g)], eps_in=1.0, eps_out=2.25, inc_ang=0.2, azi_ang=0.0)
    r80 = float((li_oracle.s_parameters(s, S, [[0, 0]], port="reflection", polarization="xx").abs() ** 2).sum())
    r_li, r_la = _lamellar(eng, [20, 0], "li", "xx"), _lamellar(eng, [20, 0], "laurent", "xx")
    assert abs(r_li - r80) < 3e-3, (r_li, r80)
    assert abs(r_la - r80) > 3e-2, (r_la, r80)
    # TE: Ey meets no discontinuity along its own direction, Li's Ey is Laurent's E
    assert abs(_lamellar(eng, [20, 0], "li", "yy") - _lamellar(eng, [20, 0], "laurent", "yy")) < 1e-8


PORTS = [(p, pol) for p in ("transmission", "reflection") for pol in ("xx", "xy", "yx", "yy")]


def _pillar_grid(transpose=False):
    """eps = 16 rectangular pillar of 1/2 x 0.4 of a 0.5 x 0.5 cell (lambda = 1), 120 x 120 binary grid."""
    g = torch.ones((120, 120), dtype=torch.float64)
    g[30:90, 36:84] = 16.0
    return g.T.contiguous() if transpose else g


def _pillar(eng, order, rule, inc, azi, transpose=False):
    import torcwa_amd
    sim = torcwa_amd.rcwa(freq=1.0, order=order, L=[0.5, 0.5], dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=inc, azi_ang=azi)
    sim.add_layer(thickness=0.4, eps=_pillar_grid(transpose).to(eng.device))
    sim.solve_global_smatrix()
    return {(p, pol): sim.S_parameters(orders=[[0, 0]], port=p, polarization=pol).cpu()[0] for p, pol in PORTS}


@pytest.mark.gpu
def test_li_high_contrast_pillar():
    eng = make_engine("gpu")
    ref = _pillar(eng, [12, 12], "li", 0.3, 0.3)
    li8 = _pillar(eng, [8, 8], "li", 0.3, 0.3)
    la8 = _pillar(eng, [8, 8], "laurent", 0.3, 0.3)
    err = lambda s: max(abs(float(s[k].abs() ** 2) - float(ref[k].abs() ** 2)) for k in PORTS)
    assert err(li8) < 1e-2, err(li8)
    assert err(la8) > 5e-2, err(la8)
    # energy at normal incidence (lossless, sub-wavelength: only the zeroth order propagates), x-polarised incidence
    n = _pillar(eng, [8, 8], "li", 0.0, 0.0)
    tot = sum(float(n[k].abs() ** 2) for k in [("reflection", "xx"), ("reflection", "yx"), ("transmission", "xx"), ("transmission", "yx")])
    assert abs(tot - 1.0) < 1e-9, tot
    # the transposed pillar (square cell) at normal incidence exchanges the x and y polarisations
    t = _pillar(eng, [8, 8], "li", 0.0, 0.0, transpose=True)
    for p in ("transmission", "reflection"):
        assert abs(complex(t[(p, "yy")]) - complex(n[(p, "xx")])) < 1e-8
        assert abs(complex(t[(p, "xx")]) - complex(n[(p, "yy")])) < 1e-8
