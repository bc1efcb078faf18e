"""The gradient of the forward under the normal-vector rule on vector shapes, derived field included: BatchedRCWA(..., shape_nv_grad=True) keeps
the field the layer derives on shape_nv_grid in the autograd graph (ShapeNormalFieldFn -> FieldConvFn -> GemmFn), end to end in complex128 on
the stack and lattice of tests/test_shape_nv_grad.py, stable_eig_grad=False as there.

Check: central differences of the forward with the field RE-DERIVED at every shifted point (normal_field=None), steps h and h / 2: pass when
|g - FD(h / 2)| <= 4 |FD(h) - FD(h / 2)| (the protocol of tests/test_shape_nv_grad.py), and that estimate is itself below 1e-4 |g| (asserted).
The bound is looser than that file's 1e-6 because the tau = 0 / 1 branch lines of an edge are C0 kinks of the field that sweep over samples
as a vertex moves: the difference is first order in h there.  The field's on / off mask (nn == 0) is asserted equal at p - h and p + h, so no
coherence jump sits inside a difference.  The frozen-field gradient (shape_nv_grad=False) is asserted to miss FD(h / 2) by more than 100 x
the estimate for theta and the vertex: the term this path adds.

Measured on the MI355X with the steps H of that file, |FD(h) - FD(h / 2)| / |g| and |g - FD(h / 2)| / |FD(h) - FD(h / 2)|: R 1.7e-7, 0.33;
Cx 1.2e-6, 0.33; theta 7.4e-8, 0.34; vertex 7.3e-6, 1.05; Re eps 2.3e-8, 0.34; Im eps 1.2e-7, 0.33 (the emulator: the same, vertex 0.99).  Eleven
(sample, image, edge) triples of this grid lie exactly on branch lines of the 4-gon: there the gradient is the mean of the two pieces'
derivatives (include/trx.h), which is what a central difference converges to, at first order in h.  The frozen-field gradient misses
FD(h / 2) by 2.1e7 (theta) and 1.7e5 (vertex) estimates.  Every case prints its figures with `-s`.
"""
import pytest
import torch

from tests.backends import BACKENDS
from tests.test_shape_nv_grad import GRID, H, LATTICE, frozen_field, make_layer, params, product, shifted
from tests.test_shapes import DT, EPS_GLASS, engine, solver

FULL = dict(shape_nv_grid=GRID, shape_nv_grad=True)
_cache = {}


def grad_of(p, name, idx):
    if name.startswith("eps_"):
        g = p["eps_s"].grad
        return float(g.real if name == "eps_re" else g.imag)
    return float(p[name].grad[idx])


def gradients(backend):
    """(full, frozen): the parameter dicts after one backward with and without the keyword, the field derived in both; computed once."""
    if backend not in _cache:
        eng = engine(backend)
        out = []
        for kw in (FULL, dict(shape_nv_grid=GRID)):
            p = params(eng.device)
            product(eng, p, None, **kw).backward()
            out.append(p)
        _cache[backend] = out
    return _cache[backend]


def field_mask(eng, p):
    import torcwa_amd.shapes as S
    with torch.no_grad():
        return S.normal_products(make_layer(S, p), LATTICE, *GRID, engine=eng) == 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(H))
def test_gradient_matches_central_differences_with_the_field_rederived(backend, name):
    eng = engine(backend)
    full, frozen = gradients(backend)
    idx, h = H[name]
    got, got_frozen = grad_of(full, name, idx), grad_of(frozen, name, idx)
    assert torch.equal(field_mask(eng, shifted(full, name, idx, +h)), field_mask(eng, shifted(full, name, idx, -h))), \
        f"{name}: a sample changes its coherence branch between p - h and p + h"
    fd = []
    for step in (h, h / 2):
        with torch.no_grad():
            fd.append((float(product(eng, shifted(full, name, idx, +step), None, shape_nv_grid=GRID))
                       - float(product(eng, shifted(full, name, idx, -step), None, shape_nv_grid=GRID))) / (2 * step))
    est = abs(fd[0] - fd[1])
    print(f"d|t00|^2 / d {name}: g {got:.9e}  FD(h/2) {fd[1]:.9e}  |g - FD(h/2)| {abs(got - fd[1]):.2e}  |FD(h) - FD(h/2)| {est:.2e} "
          f"= {est / abs(got):.1e} |g|;  frozen field g {got_frozen:.9e}, off by {abs(got_frozen - fd[1]) / abs(fd[1]):.2e} of FD "
          f"= {abs(got_frozen - fd[1]) / est:.1e} estimates [{backend}]")
    assert est <= 1e-4 * abs(got), f"{name}: the step {h} does not resolve the derivative to 1e-4 ({est:.2e} of {abs(got):.2e})"
    assert abs(got - fd[1]) <= 4 * est, f"d / d {name}: autograd {got:.9e}, central difference {fd[1]:.9e}, estimate {est:.2e}"
    if name in ("theta", "verts"):         # what the keyword is for: the frozen field's gradient is not the derivative of the forward
        assert abs(got_frozen - fd[1]) > 100 * est, f"{name}: the frozen-field gradient {got_frozen:.9e} is within 100 estimates of {fd[1]:.9e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_eps_gradients_do_not_depend_on_the_keyword(backend):
    """The field does not depend on eps: its gradient is the same bits with and without the keyword."""
    full, frozen = gradients(backend)
    assert torch.equal(full["eps_s"].grad, frozen["eps_s"].grad)
    assert not torch.equal(full["theta"].grad, frozen["theta"].grad)


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_supplied_field_stays_a_constant(backend):
    eng = engine(backend)
    nn = frozen_field(eng)
    grads = []
    for kw in (FULL, dict(shape_nv_grid=GRID)):
        p = params(eng.device)
        product(eng, p, nn, **kw).backward()
        grads.append([p[k].grad.clone() for k in p])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_is_reproducible_and_once_differentiable(backend):
    eng = engine(backend)
    full, _ = gradients(backend)
    p = params(eng.device)
    product(eng, p, None, **FULL).backward()
    assert all(torch.equal(p[k].grad, full[k].grad) for k in p), "two backward passes differ in their bits"
    p = params(eng.device)
    (g1,) = torch.autograd.grad(product(eng, p, None, **FULL), p["theta"], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g1.sum().backward()


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_equals_plain_differentiable_solves(backend):
    import torcwa_amd.shapes as S
    eng = engine(backend)
    ds = [100., 145.]
    w = torch.tensor([1.0, -0.5], dtype=torch.float64, device=eng.device)
    orders = [[m, n] for m in range(-2, 3) for n in range(-2, 3)]
    res = []
    for swept in (True, False):
        p = params(eng.device)
        dd = torch.tensor(ds, dtype=torch.float64, device=eng.device, requires_grad=True)
        kw = dict(fourier_rule="normal", keep_coupling=False, stable_eig_grad=False, **FULL)
        if swept:
            sim = solver(eng, LATTICE, orders, swept_grad=True, **kw)
            sim.add_layer(dd, eps=make_layer(S, p), swept=True)
            t = sim.solve_S_parameters([[0, 0]], polarization="xx")[0, :, 0]
        else:
            t = []
            for i in range(len(ds)):
                sim = solver(eng, LATTICE, orders, **kw)
                sim.add_layer(dd[i], eps=make_layer(S, p))
                t.append(sim.solve_S_parameters([[0, 0]], polarization="xx")[0, 0])
            t = torch.stack(t)
        ((t.abs() ** 2) * w).sum().backward()
        res.append({**{k: p[k].grad.clone() for k in p}, "dd": dd.grad.clone()})
    for k in res[0]:
        err, scale = float((res[0][k] - res[1][k]).abs().max()), float(res[1][k].abs().max())
        assert err <= 1e-6 * scale, f"{k}: swept {err:.3e} against {1e-6 * scale:.3e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_drop_in_gives_the_gradient_of_the_batched_solver(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    from torcwa_amd.lattice import rect_orders
    from tests.test_shapes import FREQ
    eng = engine(backend)
    full, _ = gradients(backend)
    p = params(eng.device)
    drop = torcwa_amd.rcwa(freq=FREQ, order=rect_orders(2, 2).tolist(), L=LATTICE, dtype=DT, engine=eng, fourier_rule="normal",
                           stable_eig_grad=False, **FULL)
    drop.add_input_layer(eps=EPS_GLASS)
    drop.add_output_layer(eps=1.)
    drop.set_incident_angle(inc_ang=0., azi_ang=0.)
    drop.add_layer(thickness=120., eps=make_layer(S, p))
    drop.solve_global_smatrix()
    (drop.S_parameters([[0, 0]], direction="forward", port="transmission", polarization="xx").abs() ** 2).sum().backward()
    for k in p:
        err, scale = float((p[k].grad - full[k].grad).abs().max()), float(full[k].grad.abs().max())
        assert err <= 1e-9 * scale, f"{k}: drop-in {err:.3e} against {scale:.3e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    import torcwa_amd
    from torcwa_amd import sweep
    eng = engine(backend)
    for rule in ("laurent", "li"):
        with pytest.raises(ValueError, match="shape_nv_grad"):
            torcwa_amd.BatchedRCWA(1 / 600., [1, 1], [700., 660.], dtype=DT, engine=eng, fourier_rule=rule, shape_nv_grad=True)
    with pytest.raises(ValueError, match="shape_nv_grad"):
        torcwa_amd.rcwa(freq=1 / 600., order=[1, 1], L=[700., 660.], dtype=DT, engine=eng, shape_nv_grad=True)
    freq = torch.tensor([1 / 600.], dtype=torch.float64, device=eng.device)
    with pytest.raises(TypeError, match="shape_nv_grad"):                # the sweep drivers stay non-differentiable
        sweep.solve_stack_sweep(freq, [(120., 2.0)], [1, 1], [700., 660.], eps_in=EPS_GLASS, eps_out=1., dtype=DT, engine=eng,
                                     fourier_rule="normal", shape_nv_grad=True)
    with pytest.raises(TypeError, match="shape_nv_grad"):
        sweep.solve_thickness_sweep(freq, [(None, 2.0)], [1, 1], [700., 660.], thicknesses=[1.0], engine=eng, fourier_rule="normal",
                                         shape_nv_grad=True)
