"""Gradients through a vector-shape layer under the normal-vector rule: the composition ShapeConvFn (values and reciprocal values) ->
InverseFn -> GemmFn with the field products held constant (BatchedRCWA._nv_tensor_shapes_torch).  The field is supplied (normal_field=, the
products of the nominal structure) and therefore frozen: the gradient is then the exact derivative of the forward with that field.

Check: central differences of the product's own forward with the same field at steps h and h / 2.  The truncation error of FD(h / 2) is a
third of |FD(h) - FD(h / 2)|, so the test passes when |g - FD(h / 2)| <= 4 |FD(h) - FD(h / 2)|, and h is chosen per parameter so that this
estimate is itself below 1e-6 |g| (asserted): no tuned tolerance.  H below: the steps, each some 1e-4 of the parameter's own length scale --
truncation h^2 f''' / 24 near 1e-7 |g| and the forward's rounding (1e-12 / h) well below it.

stable_eig_grad=False as in tests/test_shape_grad.py: the default Lorentzian broadening of the eigen-adjoint alone moves a gradient of this stack
by about 2e-6 of itself, which is the eigen-adjoint's property (tests/test_grad.py), not this composition's.
"""
import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.test_shapes import engine, solver

LATTICE = [[700., 0.], [150., 640.]]
ORDER = [2, 2]
GRID = (40, 36)
# parameter -> (index into the tensor, step h)
H = {"R": ((), 0.04), "Cx": ((), 0.04), "theta": ((), 2e-4), "verts": ((2, 0), 0.04), "eps_re": ((), 2e-3), "eps_im": ((), 2e-3)}


def params(dev="cpu"):
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt, device=dev, requires_grad=True)
    return dict(R=t(150.), Cx=t(260.), theta=t(0.3), verts=t([[520., 120.], [680., 180.], [640., 330.], [560., 260.]]),
                eps_s=t(12.0116 + 0.5259j, torch.complex128))


def make_layer(S, p):
    ell = S.ellipse(p["R"], 90., p["Cx"], 250., p["eps_s"], theta=p["theta"])
    return S.ShapeLayer(1.0, [ell, S.circle(40., 260., 250., 2.0, host=ell), S.polygon(p["verts"], 3.0)])


def frozen_field(eng):
    import torcwa_amd.shapes as S
    with torch.no_grad():
        return S.normal_products(make_layer(S, params(eng.device)), LATTICE, *GRID, engine=eng)


def product(eng, p, nn, **kw):
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    sim = solver(eng, LATTICE, rect_orders(*ORDER).tolist(), fourier_rule="normal", stable_eig_grad=False, **kw)
    sim.add_layer(120., eps=make_layer(S, p), normal_field=nn)
    sim.solve_global_smatrix()
    return (sim.S_parameters(orders=[[0, 0]], direction="forward", port="transmission", polarization="xx").abs() ** 2).sum()


def shifted(p, name, idx, dh):
    q = {n: v.detach().clone() for n, v in p.items()}
    if name.startswith("eps_"):
        q["eps_s"] += dh * (1.0 if name == "eps_re" else 1j)
    else:
        q[name][idx] += dh
    return q


@pytest.mark.parametrize("backend", BACKENDS)
def test_gradients_match_central_differences_of_the_forward(backend):
    eng = engine(backend)
    nn = frozen_field(eng)
    p = params(eng.device)
    product(eng, p, nn).backward()
    for name, (idx, h) in H.items():
        if name.startswith("eps_"):
            g = p["eps_s"].grad
            got = float(g.real if name == "eps_re" else g.imag)
        else:
            got = float(p[name].grad[idx])
        fd = []
        for step in (h, h / 2):
            with torch.no_grad():
                fd.append((float(product(eng, shifted(p, name, idx, +step), nn)) - float(product(eng, shifted(p, name, idx, -step), nn))) / (2 * step))
        est = abs(fd[0] - fd[1])
        print(f"d|t00|^2 / d {name}: g {got:.9e}  FD(h/2) {fd[1]:.9e}  |g - FD(h/2)| {abs(got - fd[1]):.2e}  |FD(h) - FD(h/2)| {est:.2e} "
              f"= {est / abs(got):.1e} |g| [{backend}]")
        assert est < 1e-6 * abs(got), f"{name}: the step {h} does not resolve the derivative to 1e-6 ({est:.2e} of {abs(got):.2e})"
        assert abs(got - fd[1]) <= 4 * est, f"d / d {name}: autograd {got:.9e}, central difference {fd[1]:.9e}, estimate {est:.2e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_is_reproducible_and_once_differentiable(backend):
    eng = engine(backend)
    nn = frozen_field(eng)
    runs = []
    for _ in range(2):
        p = params(eng.device)
        product(eng, p, nn).backward()
        runs.append([p[k].grad.clone() for k in p])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two backward passes differ in their bits"
    p = params(eng.device)
    (g1,) = torch.autograd.grad(product(eng, p, nn), p["R"], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g1.sum().backward()


@pytest.mark.parametrize("backend", BACKENDS)
def test_derived_field_is_a_constant_of_the_graph(backend):
    """normal_field=None on a differentiable stack: the field is derived from the (detached) parameters, and the gradient is the one of the
    same solve with that field supplied, bit for bit."""
    eng = engine(backend)
    nn = frozen_field(eng)
    grads = []
    for field in (None, nn):
        p = params(eng.device)
        product(eng, p, field, shape_nv_grid=GRID).backward()
        grads.append([p[k].grad.clone() for k in p])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_equals_plain_differentiable_solves(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    nn = frozen_field(eng)
    ds = [100., 145.]
    w = torch.tensor([1.0, -0.5], dtype=torch.float64, device=eng.device)
    res = []
    for swept in (True, False):
        p = params(eng.device)
        dd = torch.tensor(ds, dtype=torch.float64, device=eng.device, requires_grad=True)
        kw = dict(fourier_rule="normal", keep_coupling=False)
        if swept:
            sim = solver(eng, LATTICE, [[m, n] for m in range(-2, 3) for n in range(-2, 3)], swept_grad=True, **kw)
            sim.add_layer(dd, eps=make_layer(S, p), normal_field=nn, swept=True)
            t = sim.solve_S_parameters([[0, 0]], polarization="xx")[0, :, 0]
        else:
            t = []
            for i in range(len(ds)):
                sim = solver(eng, LATTICE, [[m, n] for m in range(-2, 3) for n in range(-2, 3)], **kw)
                sim.add_layer(dd[i], eps=make_layer(S, p), normal_field=nn)
                t.append(sim.solve_S_parameters([[0, 0]], polarization="xx")[0, 0])
            t = torch.stack(t)
        ((t.abs() ** 2) * w).sum().backward()
        res.append({**{k: p[k].grad.clone() for k in p}, "dd": dd.grad.clone()})
    for k in res[0]:
        err, scale = float((res[0][k] - res[1][k]).abs().max()), float(res[1][k].abs().max())
        assert err <= 1e-6 * scale, f"{k}: swept {err:.3e} against {1e-6 * scale:.3e}"
