"""Gradients through vector-shape layers (ShapeConvFn: trx_toeplitz_sums + trx_convmat_shapes_backward) with the project's 1e-6 gradient gate, of
max |reference| per tensor as tests/test_grad.py.

Reference: torch autograd through a float64 torch restatement of the closed forms (torch.special.bessel_j1 with J1' = J0 - J1 / x supplied, torch.sinc, the polygon's edge sum --
so a vertex derivative is the derivative of the edge sum, not the kernels' boundary-velocity form) feeding oracle.rcwa_oracle on the CPU.
Independent check: a central difference of the product's own forward for two parameters.  Step and tolerance: FoM carries a relative error of
about 1e-12 from the solver, the truncation of a central difference is h^2 f''' / 6, so a relative step of 1e-4 balances both near 1e-8 of the
derivative's scale -- two digits inside the 1e-6 gate, which is the one applied.

The product runs with stable_eig_grad=False: torch.linalg.eig in the oracle has the exact eigen-adjoint, and the default Lorentzian broadening
(1e-10 over squared eigenvalue gaps of about 1e-4 in this stack) alone moves d FoM / dR by 1.9e-6 of itself -- measured here, and the property
of the eigen-adjoint that tests/test_grad.py pins per broadening, not of the shape kernels.
"""
import numpy as np
import pytest
import torch

from oracle import rcwa_oracle as orc
from tests.backends import BACKENDS
from tests.test_shapes import DT, EPS_GLASS, FREQ, ORDER, engine, solver

GATE = 1e-6
LATTICE = [[700., 0.], [150., 640.]]
MN = np.array([(m, n) for m in range(-ORDER[0], ORDER[0] + 1) for n in range(-ORDER[1], ORDER[1] + 1)])
NAMES = ("R", "Cx", "theta", "Wx", "verts", "d", "eps_s")


def params(dev="cpu"):
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt, device=dev, requires_grad=True)
    return dict(R=t(150.), Cx=t(260.), theta=t(0.3), Wx=t(120.), verts=t([[520., 120.], [680., 180.], [640., 330.], [560., 260.]]), d=t(120.),
                eps_s=t(12.0116 + 0.5259j, torch.complex128))


def make_layer(S, p):
    return S.ShapeLayer(1.0, [S.ellipse(p["R"], 90., p["Cx"], 250., p["eps_s"], theta=p["theta"]), S.rectangle(p["Wx"], 80., 560., 480., 4.0 + 0.1j, theta=-0.4),
                              S.polygon(p["verts"], 3.0)])


def fom_of(sim):
    t = [sim.S_parameters(orders=[[1, 0]], direction="forward", port="transmission", polarization=pol) for pol in ("xx", "yx", "xy", "yy")]
    return sum((v.abs() ** 2).sum() for v in t)


def product(eng, p):
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    sim = solver(eng, LATTICE, rect_orders(*ORDER).tolist(), stable_eig_grad=False)       # the reference's eigen-adjoint is the exact one
    sim.add_layer(p["d"], eps=make_layer(S, p))
    sim.solve_global_smatrix()
    return fom_of(sim)


# ---- the reference: torch closed forms into the oracle ---------------------------------------------------------------------------------------
def _box():
    A = np.array(LATTICE)
    b = 2 * np.pi * np.linalg.inv(A).T
    P, Q = np.meshgrid(np.arange(-2 * ORDER[0], 2 * ORDER[0] + 1), np.arange(-2 * ORDER[1], 2 * ORDER[1] + 1), indexing="ij")
    return torch.from_numpy(P * b[0, 0] + Q * b[1, 0]), torch.from_numpy(P * b[0, 1] + Q * b[1, 1]), abs(float(np.linalg.det(A)))


def _rot(Gx, Gy, th):
    return torch.cos(th) * Gx + torch.sin(th) * Gy, -torch.sin(th) * Gx + torch.cos(th) * Gy


class BesselJ1(torch.autograd.Function):
    """torch.special.bessel_j1 carries no derivative formula: J1'(x) = J0(x) - J1(x) / x."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.special.bessel_j1(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * (torch.special.bessel_j0(x) - torch.special.bessel_j1(x) / x)


def chi_ellipse(Rx, Ry, Cx, Cy, th, Gx, Gy, area):
    gx, gy = _rot(Gx, Gy, th)
    rho2 = (Rx * gx) ** 2 + (Ry * gy) ** 2
    rho = torch.sqrt(torch.where(rho2 == 0, torch.ones_like(rho2), rho2))
    jinc = torch.where(rho2 == 0, torch.ones_like(rho), 2 * BesselJ1.apply(rho) / rho)
    return np.pi * Rx * Ry / area * jinc * torch.exp(-1j * (Gx * Cx + Gy * Cy))


def chi_rectangle(Wx, Wy, Cx, Cy, th, Gx, Gy, area):
    gx, gy = _rot(Gx, Gy, th)
    return Wx * Wy / area * torch.sinc(gx * Wx / (2 * np.pi)) * torch.sinc(gy * Wy / (2 * np.pi)) * torch.exp(-1j * (Gx * Cx + Gy * Cy))


def chi_polygon(v, Gx, Gy, area):
    w = torch.roll(v, -1, 0)
    e, m = w - v, (w + v) / 2
    G2 = Gx ** 2 + Gy ** 2
    tot = sum((Gx * e[k, 1] - Gy * e[k, 0]) * torch.exp(-1j * (Gx * m[k, 0] + Gy * m[k, 1])) * torch.sinc((Gx * e[k, 0] + Gy * e[k, 1]) / (2 * np.pi))
              for k in range(v.shape[0]))
    shoelace = 0.5 * (v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1]).sum()
    return torch.where(G2 == 0, (shoelace / area).to(DT), 1j * tot / (area * torch.where(G2 == 0, torch.ones_like(G2), G2)))


def reference(p):
    Gx, Gy, area = _box()
    c = lambda v: torch.as_tensor(v, dtype=torch.float64)
    box = ((p["eps_s"] - 1.0) * chi_ellipse(p["R"], c(90.), p["Cx"], c(250.), p["theta"], Gx, Gy, area)
           + (4.0 + 0.1j - 1.0) * chi_rectangle(p["Wx"], c(80.), c(560.), c(480.), c(-0.4), Gx, Gy, area) + (3.0 - 1.0) * chi_polygon(p["verts"], Gx, Gy, area))
    delta = torch.zeros(box.shape, dtype=DT)
    delta[2 * ORDER[0], 2 * ORDER[1]] = 1.0
    box = box + delta
    E = box[MN[:, None, 0] - MN[None, :, 0] + 2 * ORDER[0], MN[:, None, 1] - MN[None, :, 1] + 2 * ORDER[1]]
    s = orc.Setup(freq=FREQ, order=ORDER, L=[1., 1.], dtype=DT, eps_in=EPS_GLASS, eps_out=1.0, has_in=True, has_out=True)
    G = torch.from_numpy(np.linalg.inv(np.array(LATTICE)).T) / FREQ
    m, n = torch.from_numpy(MN[:, 0]), torch.from_numpy(MN[:, 1])
    s.kx, s.ky = (m * G[0, 0] + n * G[1, 0]).to(DT), (m * G[0, 1] + n * G[1, 1]).to(DT)
    s.Vf = orc._halfspace_V(s.kx, s.ky, 1.0)
    s.Vi, s.Vo = orc._halfspace_V(s.kx, s.ky, torch.as_tensor(EPS_GLASS, dtype=DT)), orc._halfspace_V(s.kx, s.ky, torch.as_tensor(1.0, dtype=DT))
    T, D = torch.linalg.inv(s.Vf + s.Vi), s.Vf - s.Vi
    s.Sin = [2 * (T @ s.Vi), -(T @ D), T @ D, 2 * (T @ s.Vf)]
    T, D = torch.linalg.inv(s.Vf + s.Vo), s.Vf - s.Vo
    s.Sout = [2 * (T @ s.Vf), T @ D, -(T @ D), 2 * (T @ s.Vo)]
    M = torch.eye(len(MN), dtype=DT)
    P, Q = orc.pq_patterned(E, M, s.kx, s.ky)
    kz, W = orc.modes_patterned(P, Q)
    lay = orc.layer_smatrix(orc.Layer(thickness=p["d"], E=E, M=M, P=P, Q=Q, kz=kz, W=W), s.Vf, s.omega)
    Sg = orc.global_smatrix(s, [lay])[0]
    return sum((orc.s_parameters(s, Sg, [[1, 0]], polarization=pol).abs() ** 2).sum() for pol in ("xx", "yx", "xy", "yy"))


_REF = {}


def reference_grads():
    """(FoM, {name: gradient}) of the reference, computed once and left unchanged."""
    if not _REF:
        p = params()
        f = reference(p)
        f.backward()
        _REF["fom"], _REF["grads"] = float(f.detach()), {k: p[k].grad.clone() for k in NAMES}
    return _REF["fom"], _REF["grads"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_gradients_match_autograd_through_the_oracle(backend):
    eng = engine(backend)
    p = params(eng.device)
    f = product(eng, p)
    f.backward()
    f_ref, g_ref = reference_grads()
    assert abs(float(f.detach()) - f_ref) <= 1e-9 * max(1.0, abs(f_ref))             # the 1e-9 gate on values, of an O(1) scale as in tests/test_shapes.py
    for k in NAMES:
        got, ref = p[k].grad.cpu(), g_ref[k]
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"d FoM / d {k}: err {err:.2e} of scale {scale:.2e} [{backend}]")
        assert err <= GATE * scale, f"d FoM / d {k}: {err:.3e} against {GATE * scale:.3e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_gradients_match_a_central_difference_of_the_forward(backend):
    eng = engine(backend)
    p = params(eng.device)
    product(eng, p).backward()
    for k, idx in (("R", ()), ("verts", (2, 0))):
        h = 1e-4 * abs(float(p[k].detach()[idx]))
        vals = []
        for sgn in (+1, -1):
            q = {n: v.detach().clone() for n, v in p.items()}
            q[k][idx] += sgn * h
            with torch.no_grad():
                vals.append(float(product(eng, q)))
        cd, got = (vals[0] - vals[1]) / (2 * h), float(p[k].grad[idx])
        scale = float(p[k].grad.abs().max())
        assert abs(got - cd) <= GATE * scale, f"d FoM / d {k}{list(idx)}: autograd {got:.9e}, central difference {cd:.9e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_is_reproducible_and_once_differentiable(backend):
    eng = engine(backend)
    runs = []
    for _ in range(2):
        p = params(eng.device)
        product(eng, p).backward()
        runs.append([p[k].grad.clone() for k in NAMES])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two backward passes differ in their bits"
    p = params(eng.device)
    (g1,) = torch.autograd.grad(product(eng, p), p["R"], create_graph=True)
    # end to end the second pass stops at whichever once-differentiable adjoint of the chain it meets first (the eigen-adjoint and the solves
    # sit downstream of ShapeConvFn and hand it a gradient without a graph), as in tests/test_thickness_grad.py
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g1.sum().backward()
    # ShapeConvFn on its own: the gradient carries a graph, and differentiating it raises in ShapeConvFn itself
    import torcwa_amd.shapes as S
    from torcwa_amd import autograd_ops as ag
    p = params(eng.device)
    pk = make_layer(S, p).pack(np.array(LATTICE), 1, eng.device)
    mn = torch.as_tensor(MN, dtype=torch.int32, device=eng.device)
    E = ag.ShapeConvFn.apply(pk.par, pk.val, pk, mn, ORDER[0], ORDER[1], DT, eng)
    (g2,) = torch.autograd.grad(E.abs().pow(2).sum(), p["R"], create_graph=True)
    assert g2.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.backward()


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_equals_plain_differentiable_solves(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    ds = [100., 120., 145.]
    w = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device=eng.device)        # so that every thickness has its own weight in the FoM
    res = []
    for swept in (True, False):
        p = params(eng.device)
        dd = torch.tensor(ds, dtype=torch.float64, device=eng.device, requires_grad=True)
        if swept:
            sim = solver(eng, [700., 660.], keep_coupling=False, swept_grad=True)
            sim.add_layer(dd, eps=make_layer(S, p), swept=True)
            t = sim.solve_S_parameters([[1, 0]], polarization="xx")[0, :, 0]
        else:
            t = []
            for i in range(len(ds)):
                sim = solver(eng, [700., 660.], keep_coupling=False)
                sim.add_layer(dd[i], eps=make_layer(S, p))
                t.append(sim.solve_S_parameters([[1, 0]], polarization="xx")[0, 0])
            t = torch.stack(t)
        ((t.abs() ** 2) * w).sum().backward()
        res.append({**{k: p[k].grad.clone() for k in NAMES if k != "d"}, "dd": dd.grad.clone()})
    for k in res[0]:
        err, scale = float((res[0][k] - res[1][k]).abs().max()), float(res[1][k].abs().max())
        assert err <= GATE * scale, f"{k}: swept {err:.3e} against {GATE * scale:.3e}"
