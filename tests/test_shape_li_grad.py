"""Gradients through Li's rule on rectangle layers (ShapeLiFn -> trx_convmat_li_shapes_backward), end to end in complex128 at order [2,2]:
d|t00|^2 / d(Wx, Wy, Cx, Cy, eps) of every rectangle of a nested and of a wrapped layer, stable_eig_grad=False (the plain eigen-adjoint).

Check: central differences of the ORACLE's forward with the reference's matrices (tests/test_shape_li.py: rect_oracle; no kernel enters the
difference), steps h and h / 2.  FD(h) = f' + c h^2 + O(h^4) + rho / h, so est = |FD(h) - FD(h / 2)| = 3/4 |c| h^2 is three times the
truncation error of FD(h / 2); rho is the rounding error of the oracle's forward, n eps for its n = 2 N = 50 modes and amplitudes |S| <= 1.
The protocol of tests/test_shape_nv_full_grad.py with the rounding term written out: pass when |g - FD(h / 2)| <= 4 est + n eps / (h / 2)
(the second term is what is left where the derivative is exactly 0: the centre of a single rectangle, by translation invariance), and est
itself is asserted below 1e-6 of the largest component of the layer's gradient (the difference resolves six digits).  Every case prints its
figures with `-s`.
"""
import pytest
import torch

from tests.backends import BACKENDS
from tests.test_pipeline import make_engine
from tests.test_shape_li import AZI, INC, LAM, LX, LY, RectLayer
from tests.test_shape_li import rect_oracle  # noqa: F401  (fixture)

ORDER = [2, 2]
LAYERS = {
    "nested": RectLayer([(0.4, 0.3, 0.33, 0.28), (0.15, 0.1, 0.36, 0.3)], [9.0 + 0.2j, 3.0 + 0.1j], 2.0, [None, 0]),
    "wrapped": RectLayer([(0.4, 0.3, 0.6, 0.5)], [9.0 + 0.2j], 2.0, [None]),
}
H_GEOM, H_EPS = 1e-5, 1e-4                       # est = 3/4 |c| h^2: 1e-5 puts it near 3e-7 of the gradient, rounding at 1e-11 / h = 1e-6 of that
NAMES = ("Wx", "Wy", "Cx", "Cy")
EPS = 2.220446049250313e-16


def forward_gpu(eng, lay, diff, **kw):
    """(|t00|^2, the leaf tensors (par [S, 4] float64, eps [S] complex128)) of glass / layer / eps 2.25 through BatchedRCWA."""
    import torcwa_amd
    import torcwa_amd.shapes as S
    dev = eng.device
    par = torch.tensor(lay.rects, dtype=torch.float64, device=dev, requires_grad=diff)
    eps = torch.tensor(lay.eps, dtype=torch.complex128, device=dev, requires_grad=diff)
    shapes = []
    for s, h in enumerate(lay.hosts):
        shapes.append(S.rectangle(par[s, 0], par[s, 1], par[s, 2], par[s, 3], eps[s], host=None if h is None else shapes[h]))
    sim = torcwa_amd.BatchedRCWA(torch.tensor([1 / LAM], dtype=torch.float64, device=dev), ORDER, [LX, LY], dtype=torch.complex128, engine=eng,
                                 fourier_rule="li", stable_eig_grad=False, **kw)
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(torch.tensor([INC], dtype=torch.float64, device=dev), torch.tensor([AZI], dtype=torch.float64, device=dev))
    return sim, S.ShapeLayer(lay.bg, shapes), par, eps


def fom_gpu(eng, lay, diff):
    sim, layer, par, eps = forward_gpu(eng, lay, diff)
    sim.add_layer(0.31, eps=layer)
    sim.solve_global_smatrix()
    return (sim.S_parameters([[0, 0]], polarization="xx").abs() ** 2).sum(), par, eps


def fom_oracle(orc, lay):
    s, _, S, _ = orc.solve_stack(1 / LAM, ORDER, [LX, LY], [(0.31, lay)], eps_in=1.5, eps_out=2.25, inc_ang=INC, azi_ang=AZI)
    return float((orc.s_parameters(s, S, [[0, 0]], polarization="xx").abs() ** 2).sum())


def shifted(lay, s, j, off):
    rects, eps = [list(r) for r in lay.rects], list(lay.eps)
    if j < 4:
        rects[s][j] += off
    else:
        eps[s] += off * (1.0 if j == 4 else 1j)
    return RectLayer(rects, eps, lay.bg, lay.hosts)


_fd = {}


def differences(orc, name):
    """{(s, j): (FD(h), FD(h / 2))} of the oracle's forward for every parameter of the layer; j = 0 .. 3 the geometry, 4 / 5 Re / Im eps.
    Backend-independent: computed once."""
    if name not in _fd:
        lay = LAYERS[name]
        out = {}
        for s in range(len(lay.rects)):
            for j in range(6):
                h = H_GEOM if j < 4 else H_EPS
                out[(s, j)] = tuple((fom_oracle(orc, shifted(lay, s, j, +st)) - fom_oracle(orc, shifted(lay, s, j, -st))) / (2 * st) for st in (h, h / 2))
        _fd[name] = out
    return _fd[name]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(LAYERS))
def test_gradient_matches_central_differences_of_the_oracle(backend, name, rect_oracle):  # noqa: F811
    eng = make_engine(backend)
    lay = LAYERS[name]
    f, par, eps = fom_gpu(eng, lay, True)
    assert abs(float(f.detach()) - fom_oracle(rect_oracle, lay)) < 1e-9
    gpar, geps = torch.autograd.grad(f, (par, eps))
    gpar, geps = gpar.cpu(), geps.cpu()
    fd = differences(rect_oracle, name)
    got = {(s, j): float(gpar[s, j]) if j < 4 else float(geps[s].real if j == 4 else geps[s].imag) for (s, j) in fd}
    scale = max(abs(v) for v in got.values())
    for (s, j), (d1, d2) in fd.items():
        est = abs(d1 - d2)
        what = f"{name} rectangle {s} {NAMES[j] if j < 4 else ('Re eps', 'Im eps')[j - 4]}"
        print(f"d|t00|^2 / d {what}: g {got[(s, j)]:.9e}  FD(h/2) {d2:.9e}  |g - FD(h/2)| {abs(got[(s, j)] - d2):.2e}  est {est:.2e} "
              f"= {est / scale:.1e} of the largest component [{backend}]")
        assert est <= 1e-6 * scale, f"{what}: the step does not resolve the derivative ({est:.2e} of {scale:.2e})"
        rounding = 2 * (2 * ORDER[0] + 1) * (2 * ORDER[1] + 1) * EPS / ((H_GEOM if j < 4 else H_EPS) / 2)
        assert abs(got[(s, j)] - d2) <= 4 * est + rounding, f"{what}: autograd {got[(s, j)]:.9e}, central difference {d2:.9e}, estimate {est:.2e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_backward_is_reproducible_in_the_shape_entry(backend):
    """Two backward passes of trx_convmat_li_shapes_backward on the same tables give the same bits (the composition before it uses
    index_add, as ConvMatLiFn does, and is not held to that)."""
    eng = make_engine(backend)
    import torcwa_amd.shapes as S
    lay = LAYERS["nested"]
    packed = lay.shape_layer(S).pack([[LX, 0.0], [0.0, LY]], 1, eng.device)
    rval = lay.shape_layer(S).reciprocal_values(1, eng.device)
    Ex, Ey, Ux, Uy, brk, rec = eng.convmat_li_shapes(packed, rval, LX, LY, 2, 2, torch.complex128, keep=True)
    g = torch.Generator().manual_seed(3)
    tabs = [torch.randn((1, 5, 9), dtype=torch.complex128, generator=g).to(eng.device) for _ in range(4)]
    a = eng.convmat_li_shapes_backward(packed, rval, LX, LY, 2, 2, brk, rec, *tabs)
    b = eng.convmat_li_shapes_backward(packed, rval, LX, LY, 2, 2, brk, rec, *tabs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool((a[0][:, 4::5] == 0).all()) and bool((a[0] != 0).any())


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_equals_plain_differentiable_solves(backend):
    eng = make_engine(backend)
    lay = LAYERS["wrapped"]
    ds = [0.2, 0.31]
    w = torch.tensor([1.0, -0.5], dtype=torch.float64, device=eng.device)
    res = []
    for swept in (True, False):
        dd = torch.tensor(ds, dtype=torch.float64, device=eng.device, requires_grad=True)
        if swept:
            sim, layer, par, eps = forward_gpu(eng, lay, True, keep_coupling=False, swept_grad=True)
            sim.add_layer(dd, eps=layer, swept=True)
            t = sim.solve_S_parameters([[0, 0]], polarization="xx")[0, :, 0]
        else:
            t = []
            for i in range(len(ds)):
                sim, layer, par_i, eps_i = forward_gpu(eng, lay, True, keep_coupling=False)
                sim.add_layer(dd[i], eps=layer)
                t.append((sim.solve_S_parameters([[0, 0]], polarization="xx")[0, 0], par_i, eps_i))
            par, eps = [p for _, p, _ in t], [e for _, _, e in t]
            t = torch.stack([v for v, _, _ in t])
        loss = ((t.abs() ** 2) * w).sum()
        if swept:
            g = torch.autograd.grad(loss, (par, eps, dd))
        else:
            g = torch.autograd.grad(loss, (*par, *eps, dd))
            g = (sum(g[:len(ds)]), sum(g[len(ds):2 * len(ds)]), g[-1])
        res.append(g)
    for a, b, what in zip(res[0], res[1], ("par", "eps", "thickness")):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        assert scale > 0 and err <= 1e-6 * scale, f"{what}: swept {err:.3e} against {1e-6 * scale:.3e}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    eng = make_engine(backend)
    head = 'a ShapeLayer needs fourier_rule="laurent" or "normal", got \'li\''

    def solver(**kw):
        sim = torcwa_amd.BatchedRCWA(1 / LAM, [1, 1], [LX, LY], dtype=torch.complex128, engine=eng, fourier_rule="li", **kw)
        sim.add_input_layer(eps=1.5)
        sim.set_incident_angle(0., 0.)
        return sim

    ok = S.rectangle(0.3, 0.2, 0.3, 0.3, 4.0)
    theta = torch.tensor(0.0, dtype=torch.float64, requires_grad=True)
    for shape, what in ((S.rectangle(0.3, 0.2, 0.3, 0.3, 4.0, theta=0.2), "shape 1 is a rotated rectangle"),
                        (S.ellipse(0.1, 0.05, 0.3, 0.3, 4.0), "shape 1 is an ellipse"),
                        (S.polygon([[0.1, 0.1], [0.3, 0.1], [0.2, 0.3]], 4.0), "shape 1 is a polygon"),
                        (S.rectangle(0.3, 0.2, 0.3, 0.3, 4.0, theta=theta), "shape 1 is a rectangle whose theta requires grad")):
        with pytest.raises(ValueError) as e:
            solver().add_layer(0.2, eps=S.ShapeLayer(1.0, [ok, shape]))
        msg = str(e.value)
        assert msg.startswith(head) and what in msg and 'fourier_rule="normal"' in msg, msg
    with pytest.raises(ValueError, match="the mirror is detected from grids"):
        solver(symmetry="xy").add_layer(0.2, eps=S.ShapeLayer(1.0, [ok]))
    with pytest.raises(ValueError, match="cannot be given as mu"):
        solver().add_layer(0.2, eps=2.0, mu=S.ShapeLayer(1.0, [ok]))
    for layer in (S.ShapeLayer(1.0, [ok, S.rectangle(0.1, 0.1, 0.6, 0.45, float("inf"))]), S.ShapeLayer(complex("inf"), [ok])):
        with pytest.raises(ValueError, match="1/eps = 0"):       # the strips see sums of rval only: a medium with 1/eps = 0 is refused here
            solver().add_layer(0.2, eps=layer)
    solver().add_layer(0.2, eps=S.ShapeLayer(1.0, [ok]))          # and the rectangle alone is taken
