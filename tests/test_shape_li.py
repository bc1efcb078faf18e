"""Li's rule on axis-aligned rectangle layers end to end (fourier_rule="li" with eps=ShapeLayer([rectangle, ...])): the drop-in `rcwa`,
BatchedRCWA, solve_stack_sweep and a swept=True thickness scan against the CPU oracle with the reference's matrices, convergence of the grid
path towards the closed form, and physics on the MI355X.

Oracle with reference matrices: the construction of li_oracle in tests/test_li_factorisation.py.  oracle.rcwa_oracle is handed a RectLayer in
the place of a grid; its conv_matrix returns the closed-form Laurent E (tests/shape_reference.py, float64) tagged with the (Ex, Ey) of
tests/shape_li_reference.li (long double, rounded), and pq_patterned swaps them into P, Q.  The oracle never sees a kernel's output.
Tolerances: 1e-9 (complex128) and 1e-5 (complex64), those of test_rcwa_li_against_oracle.

Raster convergence: fourier_rule="li" on ShapeLayer.rasterise grids of n = 64, 128, 256 whose edges lie halfway between samples (the rectangle
is snapped to the raster of each n) differs from the closed form by a second-order raster error: the difference must fall to <= 1/3 per
doubling (second order predicts 1/4, first order would give 1/2).  Measured ratios: MEASURED_RATIOS below (from runs with -s).
"""
import numpy as np
import pytest
import torch

from tests import shape_li_reference as lr
from tests import shape_reference as sr
from tests.backends import BACKENDS
from tests.test_li_factorisation import PORTS, _pillar, pq_ref
from tests.test_li_factorisation import li_oracle  # noqa: F401  (the fixture of the lamellar reference)
from tests.test_pipeline import make_engine

MEASURED_RATIOS = {"emu": (0.249, 0.240), "gpu": (0.249, 0.240)}     # diff(128) / diff(64), diff(256) / diff(128)

ORD = [3, 2]
LAM, LX, LY = 1.0, 0.7, 0.55
INC, AZI = 0.35, 0.2
PROBE = [[0, 0], [1, 0], [0, -1]]
POLS = ("xx", "xy", "yx", "yy")


class RectLayer:
    """What the oracle is handed in the place of a grid: rectangles (Wx, Wy, Cx, Cy), their eps, the background and the hosts."""

    def __init__(self, rects, eps, bg, hosts):
        self.rects, self.eps, self.bg, self.hosts = [tuple(float(v) for v in r) for r in rects], [complex(e) for e in eps], complex(bg), list(hosts)

    def dim(self):
        return 2                                   # patterned, to oracle.is_homogeneous

    def matrices(self, order, L):
        """(E, Ex, Ey) complex128 torch: Laurent's closed form and the long-double Li matrices, rounded."""
        ox, oy = order
        mn = np.array([(m, n) for m in range(-ox, ox + 1) for n in range(-oy, oy + 1)])
        recip, area = sr.recip_of((L[0], 0.0), (0.0, L[1]))
        shapes = [(sr.RECTANGLE, list(r) + [0.0]) for r in self.rects]
        val = np.array([self.bg] + [e - (self.bg if h is None else self.eps[h]) for e, h in zip(self.eps, self.hosts)])
        E = sr.gather(sr.plain_box(shapes, val, recip, area, ox, oy), mn, ox, oy)
        Ex, Ey = lr.li(self.rects, lr.rvals(self.eps, self.bg, self.hosts), L[0], L[1], ox, oy)
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)) for a in (E, Ex, Ey))

    def shape_layer(self, S):
        shapes = []
        for r, e, h in zip(self.rects, self.eps, self.hosts):
            shapes.append(S.rectangle(*r, e, host=None if h is None else shapes[h]))
        return S.ShapeLayer(self.bg, shapes)


@pytest.fixture
def rect_oracle(monkeypatch):
    """oracle.rcwa_oracle with Li's closed form for RectLayers on the LX x LY cell (the oracle itself is not edited)."""
    from oracle import rcwa_oracle as orc
    conv0 = orc.conv_matrix

    def conv(grid, order):
        if not isinstance(grid, RectLayer):
            return conv0(grid, order)
        E, Ex, Ey = grid.matrices(order, [LX, LY])
        E._li = (Ex, Ey)
        return E

    def pq(E, M, kx, ky):
        Ex, Ey = getattr(E, "_li", (E, E))
        return pq_ref(Ex, Ey, E, M, M, M, kx, ky)

    monkeypatch.setattr(orc, "conv_matrix", conv)
    monkeypatch.setattr(orc, "pq_patterned", pq)
    return orc


HOST_CORE = RectLayer([(0.4, 0.3, 0.6, 0.5), (0.15, 0.1, 0.65, 0.52)], [9.0 + 0.2j, 3.0], 2.0, [None, 0])     # the host wraps in x and in y
SINGLE = RectLayer([(0.3, 0.25, 0.3, 0.3)], [6.0], 1.5, [None])
STACK = [(0.31, HOST_CORE), (0.17, SINGLE)]


def oracle_s(orc, freq, layers, inc, azi, probe=PROBE, pols=POLS):
    s, _, S, _ = orc.solve_stack(freq, ORD, [LX, LY], layers, eps_in=1.5, eps_out=2.25, inc_ang=inc, azi_ang=azi)
    return torch.stack([orc.s_parameters(s, S, probe, polarization=p) for p in pols])


def rel(got, ref):
    return float((got.to(torch.complex128) - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-9), (torch.complex64, 1e-5)])
def test_rcwa_against_oracle(backend, dtype, tol, rect_oracle):
    import torcwa_amd
    import torcwa_amd.shapes as S
    eng = make_engine(backend)
    ref = oracle_s(rect_oracle, 1 / LAM, STACK, INC, AZI)
    sim = torcwa_amd.rcwa(freq=1 / LAM, order=ORD, L=[LX, LY], dtype=dtype, engine=eng, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=INC, azi_ang=AZI)
    for d, lay in STACK:
        sim.add_layer(thickness=d, eps=lay.shape_layer(S))
    sim.solve_global_smatrix()
    got = torch.stack([sim.S_parameters(orders=PROBE, polarization=p).cpu() for p in POLS])
    assert rel(got, ref) < tol
    assert sim.eps_conv_x[0] is not None and sim.eps_conv_y[0] is not None


def batch_layers(S):
    """B = 3 with per-point widths of the host: (per-point RectLayers, the ShapeLayer of the batch)."""
    wx, wy = [0.4, 0.36, 0.43], [0.3, 0.33, 0.27]
    per_point = [RectLayer([(wx[b], wy[b]) + HOST_CORE.rects[0][2:], HOST_CORE.rects[1]], HOST_CORE.eps, HOST_CORE.bg, HOST_CORE.hosts) for b in range(3)]
    host = S.rectangle(torch.tensor(wx, dtype=torch.float64), torch.tensor(wy, dtype=torch.float64), *HOST_CORE.rects[0][2:], HOST_CORE.eps[0])
    return per_point, S.ShapeLayer(HOST_CORE.bg, [host, S.rectangle(*HOST_CORE.rects[1], HOST_CORE.eps[1], host=host)])


@pytest.mark.parametrize("backend", BACKENDS)
def test_batched_and_sweep_against_oracle(backend, rect_oracle):
    import torcwa_amd
    import torcwa_amd.shapes as S
    from torcwa_amd.sweep import solve_stack_sweep
    eng = make_engine(backend)
    dev = eng.device
    lam = torch.tensor([1.0, 1.1, 0.93], dtype=torch.float64)
    inc = torch.tensor([0.3, 0.1, 0.45], dtype=torch.float64)
    azi = torch.tensor([0.2, 0.0, 0.5], dtype=torch.float64)
    per_point, layer = batch_layers(S)
    ref = torch.stack([oracle_s(rect_oracle, 1 / float(lam[b]), [(0.29, per_point[b]), STACK[1]], float(inc[b]), float(azi[b]), [[0, 0], [1, 0]],
                                ("xx",))[0] for b in range(3)])
    sim = torcwa_amd.BatchedRCWA(1 / lam, ORD, [LX, LY], dtype=torch.complex128, engine=eng, fourier_rule="li")
    sim.add_input_layer(eps=1.5)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc.to(dev), azi.to(dev))
    sim.add_layer(thickness=0.29, eps=layer)
    sim.add_layer(thickness=STACK[1][0], eps=SINGLE.shape_layer(S))
    sim.solve_global_smatrix()
    assert rel(sim.S_parameters([[0, 0], [1, 0]], polarization="xx").cpu(), ref) < 1e-9
    sw = solve_stack_sweep((1 / lam).to(dev), [(0.29, layer), (STACK[1][0], SINGLE.shape_layer(S))], ORD, [LX, LY], eps_in=1.5, eps_out=2.25,
                           inc_ang=inc.to(dev), azi_ang=azi.to(dev), dtype=torch.complex128, engine=eng, orders=((0, 0), (1, 0)),
                           fourier_rule="li").cpu()
    assert rel(sw, ref) < 1e-9


@pytest.mark.parametrize("backend", BACKENDS)
def test_swept_thickness_scan_equals_plain_solves(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    eng = make_engine(backend)
    ds = [0.2, 0.29, 0.41]

    def solver():
        sim = torcwa_amd.BatchedRCWA(torch.tensor([1 / LAM], dtype=torch.float64, device=eng.device), ORD, [LX, LY], dtype=torch.complex128,
                                     engine=eng, fourier_rule="li", keep_coupling=False)
        sim.add_input_layer(eps=1.5)
        sim.add_output_layer(eps=2.25)
        sim.set_incident_angle(torch.tensor([INC], dtype=torch.float64, device=eng.device),
                               torch.tensor([AZI], dtype=torch.float64, device=eng.device))
        return sim

    sim = solver()
    sim.add_layer(torch.tensor(ds, dtype=torch.float64, device=eng.device), eps=HOST_CORE.shape_layer(S), swept=True)
    sim.add_layer(STACK[1][0], eps=SINGLE.shape_layer(S))
    swept = sim.solve_S_parameters(PROBE, polarization="xy").cpu()[0]
    for i, d in enumerate(ds):
        sim = solver()
        sim.add_layer(d, eps=HOST_CORE.shape_layer(S))
        sim.add_layer(STACK[1][0], eps=SINGLE.shape_layer(S))
        plain = sim.solve_S_parameters(PROBE, polarization="xy").cpu()[0]
        assert rel(swept[i], plain) < 1e-9


def snapped(n):
    """The rectangle (0.31, 0.24) about (0.33, 0.29) with every edge moved to the nearest position halfway between two samples of an n x n
    raster of the cell."""
    edge = lambda e, L: (np.floor(e * n / L) + 0.5) * L / n
    x0, x1, y0, y1 = edge(0.175, LX), edge(0.485, LX), edge(0.17, LY), edge(0.41, LY)
    return (x1 - x0, y1 - y0, (x0 + x1) / 2, (y0 + y1) / 2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_grid_path_converges_to_the_closed_form_at_second_order(backend):
    import torcwa_amd
    import torcwa_amd.shapes as S
    eng = make_engine(backend)

    def solve(eps):
        sim = torcwa_amd.rcwa(freq=1 / LAM, order=[3, 3], L=[LX, LY], dtype=torch.complex128, engine=eng, fourier_rule="li")
        sim.add_input_layer(eps=1.5)
        sim.add_output_layer(eps=2.25)
        sim.set_incident_angle(inc_ang=INC, azi_ang=AZI)
        sim.add_layer(thickness=0.31, eps=eps)
        sim.solve_global_smatrix()
        return torch.stack([sim.S_parameters(orders=PROBE, polarization=p, port=port).cpu() for p in POLS for port in ("transmission", "reflection")])

    diffs = []
    for n in (64, 128, 256):
        layer = S.ShapeLayer(2.0, [S.rectangle(*snapped(n), 9.0 + 0.2j)])
        grid = layer.rasterise((LX, 0.0), (0.0, LY), n, n)[0]
        assert abs(float(grid.real.mean()) - (2.0 + 7.0 * snapped(n)[0] * snapped(n)[1] / (LX * LY))) < 1e-12      # the raster holds the exact area
        diffs.append(float((solve(grid.to(eng.device)) - solve(layer)).abs().max()))
    print(f"|S_grid(n) - S_closed| at n = 64, 128, 256: {diffs}; ratios {diffs[1] / diffs[0]:.3f}, {diffs[2] / diffs[1]:.3f} [{backend}]")
    assert diffs[0] > 1e-6                                        # there is a raster error to converge away
    assert diffs[1] <= diffs[0] / 3 and diffs[2] <= diffs[1] / 3, diffs


# ---- physics on the MI355X (complex128; orders too large for the emulator) ---------------------------------------------------------------------
def _lamellar_shapes(eng, order, rule, pol):
    """The lamellar metal grating of tests/test_li_factorisation.py as a rectangle: eps = (0.22 + 6.71i)^2 over 0 <= x < 0.5 of a unit cell."""
    import torcwa_amd
    import torcwa_amd.shapes as S
    sim = torcwa_amd.rcwa(freq=1.0, order=order, L=[1.0, 1.0], dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=0.2, azi_ang=0.0)
    sim.add_layer(thickness=0.3, eps=S.ShapeLayer(1.0, [S.rectangle(0.5, 1.0, 0.25, 0.5, (0.22 + 6.71j) ** 2)]))
    sim.solve_global_smatrix()
    return float((sim.S_parameters(orders=[[0, 0]], port="reflection", polarization=pol).abs() ** 2).sum())


@pytest.mark.gpu
def test_lamellar_metal_grating_converges(li_oracle):  # noqa: F811
    eng = make_engine("gpu")
    g = torch.ones((2000, 1), dtype=torch.complex128)
    g[:1000] = (0.22 + 6.71j) ** 2
    s, _, S, _ = li_oracle.solve_stack(1.0, [80, 0], [1.0, 1.0], [(0.3, g)], eps_in=1.0, eps_out=2.25, inc_ang=0.2, azi_ang=0.0)
    r80 = float((li_oracle.s_parameters(s, S, [[0, 0]], port="reflection", polarization="xx").abs() ** 2).sum())
    r_li, r_la = _lamellar_shapes(eng, [20, 0], "li", "xx"), _lamellar_shapes(eng, [20, 0], "laurent", "xx")
    print(f"lamellar |r00|^2: closed-form Li {r_li:.6f} (off by {abs(r_li - r80):.1e}), closed-form Laurent {r_la:.6f} "
          f"(off by {abs(r_la - r80):.1e}), oracle [80,0] {r80:.6f}")
    assert abs(r_li - r80) < 3e-3, (r_li, r80)
    assert abs(r_la - r80) > 3e-2, (r_la, r80)
    assert abs(_lamellar_shapes(eng, [20, 0], "li", "yy") - _lamellar_shapes(eng, [20, 0], "laurent", "yy")) < 1e-8


def _pillar_shapes(eng, order, rule, inc, azi, transpose=False):
    """The eps = 16 pillar of tests/test_li_factorisation.py (grid cells 30..89 x 36..83 of 120 x 120, sampled at the DFT's positions) as the
    rectangle that has those cells' edges halfway between samples."""
    import torcwa_amd
    import torcwa_amd.shapes as S
    h = 0.5 / 120
    w = (48 * h, 60 * h) if transpose else (60 * h, 48 * h)
    sim = torcwa_amd.rcwa(freq=1.0, order=order, L=[0.5, 0.5], dtype=torch.complex128, engine=eng, fourier_rule=rule)
    sim.add_input_layer(eps=1.0)
    sim.add_output_layer(eps=2.25)
    sim.set_incident_angle(inc_ang=inc, azi_ang=azi)
    sim.add_layer(thickness=0.4, eps=S.ShapeLayer(1.0, [S.rectangle(*w, 59.5 * h, 59.5 * h, 16.0)]))
    sim.solve_global_smatrix()
    return {(p, pol): sim.S_parameters(orders=[[0, 0]], port=p, polarization=pol).cpu()[0] for p, pol in PORTS}


@pytest.mark.gpu
def test_high_contrast_pillar():
    eng = make_engine("gpu")
    ref = _pillar(eng, [12, 12], "li", 0.3, 0.3)                 # the grid path, converged in the order
    li8 = _pillar_shapes(eng, [8, 8], "li", 0.3, 0.3)
    la8 = _pillar_shapes(eng, [8, 8], "laurent", 0.3, 0.3)
    err = lambda s: max(abs(float(s[k].abs() ** 2) - float(ref[k].abs() ** 2)) for k in PORTS)
    print(f"pillar at [8,8] against the grid path at [12,12]: closed-form Li {err(li8):.2e}, closed-form Laurent {err(la8):.2e}")
    assert err(li8) < 1e-2, err(li8)
    assert err(la8) > 5e-2, err(la8)
    n = _pillar_shapes(eng, [8, 8], "li", 0.0, 0.0)
    tot = sum(float(n[k].abs() ** 2) for k in [("reflection", "xx"), ("reflection", "yx"), ("transmission", "xx"), ("transmission", "yx")])
    assert abs(tot - 1.0) < 1e-9, tot
    t = _pillar_shapes(eng, [8, 8], "li", 0.0, 0.0, transpose=True)
    for p in ("transmission", "reflection"):
        assert abs(complex(t[(p, "yy")]) - complex(n[(p, "xx")])) < 1e-8
        assert abs(complex(t[(p, "xx")]) - complex(n[(p, "yy")])) < 1e-8
