"""Differentiable thickness sweeps, end to end: BatchedRCWA(..., swept_grad=True) + add_layer(..., swept=True) + solve_S_parameters, complex128.

Gates: the project's (tests/test_grad.py): 1e-9 on values, 1e-6 on gradients (of max |reference| per gradient tensor).
  1. the stack of tests/golden/grad_o32.npz with its patterned layer swept over [250, 300, 350] and the FoM read at t = 1, against the
     reference's autograd (the fixture of tests/test_grad.py);
  2. against T plain differentiable BatchedRCWA solves (pinned to the reference by tests/test_grad.py), one per thickness: values [B, T, orders]
     and the gradient of sum_t w_t FoM_t with distinct weights, with respect to every differentiable tensor of the stack;
  3. with symmetry="xy", symmetry_grad=True against the unfolded swept_grad run, density gradient mirror-averaged (tests/test_symmetry_grad.py);
  4. the shape of the graph: one eigensolver call and one eigen-adjoint whatever T, read-outs sharing it, the fused path without a gradient;
  5. every refusal, matched on its message.
Bodies run on the emulator and on the MI355X (tests/backends.py).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS
from tests.helpers import GOLDEN
from tests.test_pipeline import make_engine

DIRPORT = [("forward", "transmission"), ("forward", "reflection"), ("backward", "reflection"), ("backward", "transmission")]
WEIGHTS = [1.0, -0.6, 0.35, 0.8, -1.3]
ORDERS = [[1, 0], [0, 0]]


@functools.lru_cache(maxsize=None)
def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _count_eig(eng):
    """The sizes of every eigensolver call of `eng` from now on (as tests/test_sector_grad.py::_count_eig)."""
    sizes, inner = [], eng.eig

    def counted(A, *a, **kw):
        sizes.append(int(A.shape[-1]))
        return inner(A, *a, **kw)
    eng.eig = counted
    return sizes


def _count_eig_backward(eng):
    calls, inner = [], eng.eig_backward

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    eng.eig_backward = counted
    return calls


# ---- 1. the reference's autograd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_matches_reference(backend):
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("grad_o32")
    tag, eps_si = "stable1_bpe-10", complex(g["eps_si"])
    old = torcwa_amd.Eig.broadening_parameter
    torcwa_amd.Eig.broadening_parameter = 1e-10
    try:
        rho = torch.from_numpy(g["rho"]).to(eng.device).requires_grad_(True)
        d = torch.tensor([250., 300., 350.], dtype=torch.float64, device=eng.device, requires_grad=True)
        sim = torcwa_amd.BatchedRCWA(1 / 532., [3, 2], [700., 300.], batch=1, dtype=torch.complex128, engine=eng, keep_coupling=False, swept_grad=True)
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0., 0.)
        sim.add_layer(d, rho * eps_si + (1. - rho), swept=True)
        sim.add_layer(80., 2.25)
        t = [sim.solve_S_parameters([[1, 0]], direction="forward", port="transmission", polarization=p, ref_order=[0, 0]) for p in ("xx", "yx", "xy", "yy")]
        assert all(v.shape == (1, 3, 1) and v.requires_grad for v in t)
        fom = sum(torch.abs(v[:, 1]) ** 2 for v in t)
        fom.sum().backward()
    finally:
        torcwa_amd.Eig.broadening_parameter = old
    fom_v, fom_ref = float(fom.detach().reshape(-1)[0]), float(np.asarray(g[f"{tag}_fom"]).reshape(-1)[0])
    ref = g[f"{tag}_grad_rho"]
    gt_ref = float(np.asarray(g[f"{tag}_grad_thick"]).reshape(-1)[0])
    e_f, e_r = abs(fom_v - fom_ref) / fom_ref, np.abs(rho.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    e_t = abs(float(d.grad[1]) - gt_ref) / abs(gt_ref)
    print(f"FoM {e_f:.2e}, d/d density {e_r:.2e}, d/d thickness {e_t:.2e}")
    assert e_f < 1e-9 and e_r < 1e-6 and e_t < 1e-6
    assert float(d.grad[0]) == 0.0 and float(d.grad[2]) == 0.0          # a thickness that is not read takes exactly no gradient


# ---- 2. T plain differentiable solves --------------------------------------------------------------------------------------------------------
# name -> (B, T, solver keywords, layers in order, half-spaces (input, output), (direction, port) pairs).  Layers: "swept" (patterned, density
# rho_s), "swept_h" (homogeneous, permittivity eps_s), "front" (patterned, density rho_f), "hom" (homogeneous, thickness th_h, permittivity eps_h).
STACKS = {
    "full_b2": (2, 2, {}, ("front", "swept", "hom"), (True, True), [DIRPORT[0], DIRPORT[3]]),
    "full_b1": (1, 2, {}, ("front", "swept", "hom"), (True, True), DIRPORT[1:3]),
    "li_first": (1, 2, dict(fourier_rule="li"), ("swept", "hom"), (True, False), DIRPORT[:1]),
    "hom_last": (1, 3, {}, ("front", "swept_h"), (False, False), DIRPORT[2:3]),
    "only_out": (1, 2, {}, ("swept",), (False, True), [DIRPORT[1], DIRPORT[3]]),
    "only_bare": (1, 2, {}, ("swept",), (False, False), DIRPORT[:1]),
}


def _leaves(g, B, T, dev):
    """The differentiable tensors of a stack, fresh leaves: per-point values differ so that a batch mix-up shows."""
    rho = torch.from_numpy(g["rho"]).to(dev)
    pt = torch.arange(B, dtype=torch.float64, device=dev)
    lv = dict(rho_s=rho[None].repeat(B, 1, 1), rho_f=(rho ** 2)[None].repeat(B, 1, 1),
              d=(torch.tensor([250., 300., 350.][:T], dtype=torch.float64, device=dev)[None] + 13. * pt[:, None]) if B > 1
              else torch.tensor([250., 300., 350.][:T], dtype=torch.float64, device=dev),
              th_h=80. + 7. * pt, eps_h=2.25 + 0.1 * pt, eps_s=3.1 + 0.2 * pt, freq=1 / (532. + 9. * pt))
    return {k: v.clone().requires_grad_(True) for k, v in lv.items()}


def _build(eng, g, lv, layers, halves, d_of_swept, swept, **kw):
    """One solver over the leaves `lv`; the swept layer takes d_of_swept ([T] / [B,T] with swept=True, [B] without)."""
    import torcwa_amd
    eps_si = complex(g["eps_si"])
    B = lv["freq"].shape[0]
    sim = torcwa_amd.BatchedRCWA(lv["freq"], [3, 2], [700., 300.], batch=B, dtype=torch.complex128, engine=eng, keep_coupling=False, **kw)
    if halves[0]:
        sim.add_input_layer(eps=1.46 ** 2)
    if halves[1]:
        sim.add_output_layer(eps=1.7)
    sim.set_incident_angle(0.1, 0.2)
    for name in layers:
        if name == "front":
            sim.add_layer(120., lv["rho_f"] * 2.6 + (1. - lv["rho_f"]))
        elif name == "hom":
            sim.add_layer(lv["th_h"], lv["eps_h"])
        elif name == "swept":
            sim.add_layer(d_of_swept, lv["rho_s"] * eps_si + (1. - lv["rho_s"]), swept=swept)
        else:
            sim.add_layer(d_of_swept, lv["eps_s"], swept=swept)
    return sim


def _read(sim, dr, pt):
    return torch.stack([sim.solve_S_parameters(ORDERS, direction=dr, port=pt, polarization=p, ref_order=[0, 0]) for p in ("xx", "yx")], dim=-1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(STACKS))
def test_swept_gradient_matches_plain_solves(backend, name):
    eng = make_engine(backend)
    g = _golden("grad_o32")
    B, T, kw, layers, halves, dirports = STACKS[name]
    used = {"freq", "d"} | {dict(front="rho_f", swept="rho_s", swept_h="eps_s")[n] for n in layers if n != "hom"} | ({"th_h", "eps_h"} if "hom" in layers else set())
    w = torch.tensor(WEIGHTS[:T], dtype=torch.float64, device=eng.device)
    lv = _leaves(g, B, T, eng.device)
    sim = _build(eng, g, lv, layers, halves, lv["d"], True, swept_grad=True, **kw)
    lp = _leaves(g, B, T, eng.device)
    dp = lp["d"] if B > 1 else lp["d"][None]
    plain = [_build(eng, g, lp, layers, halves, dp[:, t], False, **kw) for t in range(T)]
    for dr, pt in dirports:
        got = _read(sim, dr, pt)                                                        # [B, T, orders, pol]
        assert got.shape == (B, T, len(ORDERS), 2) and got.requires_grad
        ref = torch.stack([_read(p, dr, pt) for p in plain], dim=1)
        e_v = float((got - ref).detach().abs().max()) / max(float(ref.detach().abs().max()), 1e-3)
        keys = sorted(used)
        loss = lambda v: ((v.abs() ** 2).sum(dim=(0, 2, 3)) * w).sum()
        gs = torch.autograd.grad(loss(got), [lv[k] for k in keys], retain_graph=True)
        gp = torch.autograd.grad(loss(ref), [lp[k] for k in keys], retain_graph=True)
        errs = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(keys, gs, gp)}
        print(f"{name} {dr} {pt}: values {e_v:.2e}, gradients " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert e_v < 1e-9
        assert all(float(b.abs().max()) > 0 for b in gp)
        assert max(errs.values()) < 1e-6, errs


# ---- 3. with the folded eigenproblem ---------------------------------------------------------------------------------------------------------
def _mirror_average(g):
    g = (g + np.flip(g, axis=-2)) / 2
    return (g + np.flip(g, axis=-1)) / 2


def _run_sym(eng, g, **kw):
    import torcwa_amd
    eps_si = complex(g["eps_si"])
    rho = torch.from_numpy(g["rho"]).to(eng.device).requires_grad_(True)
    d = torch.tensor([280., 320.], dtype=torch.float64, device=eng.device, requires_grad=True)
    sim = torcwa_amd.BatchedRCWA(1 / float(g["lam0"]), [3, 2], [700., 300.], batch=1, dtype=torch.complex128, engine=eng, keep_coupling=False,
                                 swept_grad=True, **kw)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(d, rho * eps_si + (1. - rho), swept=True)
    sim.add_layer(80., 2.25)
    rxx = sim.solve_S_parameters([[1, 0]], direction="forward", port="reflection", polarization="xx", ref_order=[0, 0])
    ryy = sim.solve_S_parameters([[0, 1]], direction="forward", port="reflection", polarization="yy", ref_order=[0, 0])
    fom = (torch.abs(rxx) ** 2 + 0.5 * torch.abs(ryy) ** 2).reshape(2)               # not mirror-invariant (tests/test_symmetry_grad.py)
    (fom * torch.tensor([1.0, -0.7], dtype=torch.float64, device=eng.device)).sum().backward()
    return fom.detach().cpu().numpy(), d.grad.cpu().numpy(), rho.grad.cpu().numpy()


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_gradient_with_symmetry(backend):
    eng = make_engine(backend)
    g = _golden("symgrad_o32")
    f0, t0, r0 = _run_sym(eng, g)
    f1, t1, r1 = _run_sym(eng, g, symmetry="xy", symmetry_grad=True)
    a0, a1 = _mirror_average(r0), _mirror_average(r1)
    e_f, e_t = np.abs(f1 - f0).max() / np.abs(f0).max(), (np.abs(t1 - t0) / np.abs(t0)).max()
    e_r = np.abs(a1 - a0).max() / np.abs(a0).max()
    raw = np.abs(r0 - a0).max() / np.abs(a0).max()
    print(f"FoM {e_f:.2e}, d/d thickness {e_t:.2e}, mirror-averaged d/d density {e_r:.2e}; unfolded raw - its mirror average {raw:.2e}")
    assert e_f < 1e-9 and e_t < 1e-6 and e_r < 1e-6
    assert raw > 1e-3


# ---- 4. the shape of the graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_graph_has_one_eigenproblem(backend):
    """T = 5: one eigensolver call in the forward, one eigen-adjoint in the backward of two read-outs that share the graph."""
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("grad_o32")
    eps_si = complex(g["eps_si"])
    sizes, adj = _count_eig(eng), _count_eig_backward(eng)
    rho = torch.from_numpy(g["rho"]).to(eng.device).requires_grad_(True)
    d = torch.tensor([240., 270., 300., 330., 360.], dtype=torch.float64, device=eng.device, requires_grad=True)
    sim = torcwa_amd.BatchedRCWA(1 / 532., [3, 2], [700., 300.], batch=1, dtype=torch.complex128, engine=eng, keep_coupling=False, swept_grad=True)
    sim.add_input_layer(eps=1.46 ** 2)
    sim.set_incident_angle(0., 0.)
    sim.add_layer(d, rho * eps_si + (1. - rho), swept=True)
    t = sim.solve_S_parameters([[1, 0]], direction="forward", port="transmission", polarization="xx")
    r = sim.solve_S_parameters([[0, 0]], direction="forward", port="reflection", polarization="yy")
    assert t.shape == r.shape == (1, 5, 1)
    assert sizes == [70]
    ((t.abs() ** 2).sum() + (r.abs() ** 2).sum()).backward()
    assert sizes == [70] and len(adj) == 1
    assert bool((d.grad != 0).all()) and bool(torch.isfinite(rho.grad).all())


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_grad_without_a_gradient_is_the_fused_path(backend):
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("grad_o32")
    eps_si = complex(g["eps_si"])
    rho = torch.from_numpy(g["rho"]).to(eng.device)
    res = []
    for kw in ({}, dict(swept_grad=True)):
        sim = torcwa_amd.BatchedRCWA(1 / 532., [3, 2], [700., 300.], batch=1, dtype=torch.complex128, engine=eng, keep_coupling=False, **kw)
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0., 0.)
        sim.add_layer(torch.tensor([250., 300.], dtype=torch.float64), rho * eps_si + (1. - rho), swept=True)
        sim.add_layer(80., 2.25)
        assert not sim._diff
        res.append(sim.solve_S_parameters(ORDERS, direction="forward", port="reflection", polarization="xx"))
    assert not res[1].requires_grad and torch.equal(res[0], res[1])


# ---- 5. validation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_grad_refusals(backend):
    import torcwa_amd
    eng = make_engine(backend)
    g = _golden("symgrad_o32")
    dev = eng.device
    eps = (torch.from_numpy(g["rho"]) * 3. + 1.).to(dev)
    d = torch.tensor([10.0, 20.0], dtype=torch.float64, device=dev)
    freq = torch.tensor([1 / 532.], dtype=torch.float64, device=dev)

    def new(**kw):
        sim = torcwa_amd.BatchedRCWA(freq, [1, 1], [700., 300.], dtype=torch.complex128, engine=eng, **dict(dict(keep_coupling=False, swept_grad=True), **kw))
        sim.add_input_layer(eps=1.46 ** 2)
        sim.set_incident_angle(0.0, 0.0)
        return sim

    leaf = lambda t: t.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="differentiable"):              # the default still refuses
        new(swept_grad=False).add_layer(leaf(d), eps, swept=True)
    sim = new()
    sim.add_layer(leaf(d), eps, swept=True)
    with pytest.raises(ValueError, match="already swept"):
        sim.add_layer(leaf(d), eps, swept=True)
    with pytest.raises(ValueError, match="keep_coupling"):
        new(keep_coupling=True).add_layer(leaf(d), eps, swept=True)
    with pytest.raises(TypeError, match="swept_grad"):                   # the drop-in class keeps its coupling matrices: no such keyword
        torcwa_amd.rcwa(freq=1 / 532., order=[1, 1], L=[700., 300.], dtype=torch.complex128, engine=eng, swept_grad=True)
    with pytest.raises(ValueError, match="avoid_Pinv_instability"):
        new(avoid_Pinv_instability=True).add_layer(leaf(d), eps, swept=True)
    with pytest.raises(ValueError, match="symmetry_sector"):
        new(symmetry="xy", symmetry_sector=True)
    with pytest.raises(ValueError, match="symmetry_grad"):               # symmetry= on a differentiable stack follows its own rule
        new(symmetry="xy").add_layer(leaf(d), eps, swept=True)
    with pytest.raises(TypeError, match="swept_grad"):                   # the sweep drivers stay non-differentiable
        torcwa_amd.solve_thickness_sweep(freq, [(None, eps)], [1, 1], [700., 300.], thicknesses=[1.0], engine=eng, swept_grad=True)
    with pytest.raises(ValueError, match="differentiable"):
        torcwa_amd.solve_thickness_sweep(freq, [(None, leaf(eps))], [1, 1], [700., 300.], thicknesses=[1.0], engine=eng)
    for call in (lambda: sim.solve_global_smatrix(), lambda: sim.power_flux(0)):
        with pytest.raises(ValueError, match="solve_S_parameters"):
            call()
    t = sim.solve_S_parameters([[0, 0]])
    dd = [p for p in (sim._swept["d"],) if p.requires_grad]
    (g1,) = torch.autograd.grad((t.abs() ** 2).sum(), dd, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g1.sum().backward()
