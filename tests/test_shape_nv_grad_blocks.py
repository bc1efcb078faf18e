"""Block tests of trx_shape_normal_field_backward, the adjoint of the blended normal field of a shape list, through the C ABI with caller-owned
buffers, guard bytes around gpar and around the exactly sized workspace, on both backends of tests/backends.py.

Policy (DESIGN.md "Block tests", as for the forward field), per parameter k of the packed row:

    |gpar_k - ref_k| / sum_samples |gnn * d nn / d par_k|_ref  <=  16 * max(e_plain_k, T * eps),      T = 9 * (ellipses + edges)

ref the long-double forward-mode restatement of tests/shape_nv_grad_reference.py, e_plain_k the same ratio for its float64 run, eps that of
fp64.  gnn is random normal with a fixed seed.  A sample is left out only where shape_nv_reference.excluded says so (|coherence - 1e-3| < 1e-6,
or within 1e-6 sqrt(area) of an ellipse centre or a polygon vertex of an image), by zeroing gnn there on both sides; at most 1 % of a case,
asserted.  Cases: the structures of tests/test_shape_nv_blocks.py (a disk with Rx = Ry: the tie of min; an ellipse across the cell edge: the
images; a rotated rectangle: the chain rule through its vertices; the L-shape plus triangle; a core-shell pair) on the square and the 60
degree cell, on (32, 32) and (33, 17) (odd, not square, no multiple of a chunk); a batch of 3 with per-point parameters; a 150-gon on 16 x 16
(two staging passes of the recomputed forward, vertices on the pass boundary).  A parameter no sample depends on (theta of a disk: the
reference's tangent is exactly 0) must receive exactly 0, and so must a slot of the row that no shape owns.

Every case prints its worst ratio err / floor with `-s`.  Worst ratios (bound 16), rounded up: WORST_EMU / WORST_MI355X at the end of the file.
"""
import ctypes

import numpy as np
import pytest

from tests import shape_nv_grad_reference as ngr
from tests import shape_nv_reference as nvr
from tests.backends import BACKENDS, get_backend
from tests.test_shape_blocks import CELLS, TRIANGLE, gbuf, gread, pack, regular
from tests.test_shape_nv_blocks import ARG, E, EPS, MARGIN, P, R, STRUCTURES, UNSUPPORTED, WS, lattice_of, terms

GRIDS = [(32, 32), (33, 17)]
RATIOS = {}


def call_backward(be, points, cell, n1, n2, gnn, pad=0, ws_short=0, over=None):
    """(rc, gpar [B, npar + pad]) of trx_shape_normal_field_backward with a guarded gpar and a guarded workspace of exactly the size asked for.
    pad: slots appended to every parameter row that no shape owns; over: arguments passed in place of the valid ones (None: a NULL pointer)."""
    over = over or {}
    kind, voff, par = pack(points)
    par = np.concatenate([par, np.full((par.shape[0], pad), 0.123)], axis=1)
    B, npar = par.shape
    a = dict(S=len(kind), npar=npar, batch=B, n1=n1, n2=n2, lattice=lattice_of(cell))
    nws = be.lib.shape_normal_field_backward_ws_bytes(len(kind), npar, B, n1, n2)
    assert nws > 0
    a.update(over)
    hg, pg = gbuf(be, B * npar * 8)
    hw, pw = gbuf(be, nws)
    bufs = dict(kind=be.dev(kind), voff=be.dev(voff), par=be.dev(par), gnn=be.dev(np.ascontiguousarray(gnn, dtype=np.float64)))
    ptr = {k: (None if k in over and over[k] is None else be.ptr(v)) for k, v in bufs.items()}
    if "gpar" in over:
        pg = None
    if "ws" in over:
        pw = None
    rc = be.lib.shape_normal_field_backward(ptr["kind"], ptr["voff"], a["S"], ptr["par"], a["npar"], a["lattice"], a["batch"], a["n1"], a["n2"],
                                            ptr["gnn"], pg, pw, nws - ws_short, be.stream)
    be.sync()
    ws = gread(be, hw, np.uint8, (nws,))
    gpar = gread(be, hg, np.float64, (B, npar))
    if rc != 0:
        assert (ws == 0xA5).all() and (gpar.view(np.uint8) == 0xA5).all(), "a refused call wrote to its buffers"
    return rc, gpar


def masked_gradient(shapes, cell, n1, n2, seed):
    """gnn [3, n1, n2]: random normal, zero on the samples the policy may leave out (at most 1 % of the case, asserted)."""
    a1, a2 = CELLS[cell]
    coh = nvr.field(shapes, a1, a2, n1, n2)["coh"]
    out = nvr.excluded(shapes, a1, a2, n1, n2, coh)
    assert out.mean() <= 0.01, f"{out.sum()} of {out.size} samples left out"
    gnn = np.random.default_rng(seed).standard_normal((3, n1, n2))
    gnn[:, out] = 0.0
    return gnn, int(out.sum())


def check(backend, what, got, shapes, cell, n1, n2, gnn, left_out):
    a1, a2 = CELLS[cell]
    ref, scale = ngr.gpar(shapes, a1, a2, n1, n2, gnn)
    plain, _ = ngr.gpar(shapes, a1, a2, n1, n2, gnn, dtype=np.float64)
    assert np.isfinite(got).all()
    none = scale == 0                      # a parameter no sample depends on (theta of a disk): the reference's tangent is exactly 0
    assert (got[none] == 0).all(), f"{what}: parameters {np.nonzero(none)[0].tolist()} move no sample and must receive exactly 0, got {got[none]}"
    assert none.sum() <= 1 and (got[~none] != 0).all()
    scale = np.where(none, 1, scale)
    err = np.abs(got - ref) / scale
    floor = np.maximum(np.abs(plain - ref) / scale, terms(shapes) * EPS)
    ratio = (err / floor).astype(np.float64)
    worst = int(ratio.argmax())
    RATIOS[backend] = max(RATIOS.get(backend, 0.0), float(ratio[worst]))
    print(f"shape_normal_field_backward[{backend}] {what}: worst {ratio[worst]:.2f} at parameter {worst} (err {float(err[worst]):.1e}, floor "
          f"{float(floor[worst]):.1e}), left out {left_out} | worst so far {RATIOS[backend]:.2f}  (err / floor; bound {MARGIN:g})")
    assert (err <= MARGIN * floor).all(), f"{what}: parameters {np.nonzero(err > MARGIN * floor)[0].tolist()} exceed the bound; ratios {ratio}"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cell", ["square", "oblique"])
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_shape_normal_field_backward(backend, name, cell):
    be = get_backend(backend)
    shapes = STRUCTURES[name]
    for n1, n2 in GRIDS:
        gnn, left = masked_gradient(shapes, cell, n1, n2, [7, n1, n2])
        rc, gpar = call_backward(be, [shapes], cell, n1, n2, gnn[None], pad=2)
        assert rc == 0
        npar = gpar.shape[1] - 2
        assert (gpar[0, npar:] == 0).all(), "a slot no shape owns must receive exactly 0"
        check(backend, f"{name} {cell} ({n1},{n2})", gpar[0, :npar], shapes, cell, n1, n2, gnn, left)
        if (n1, n2) == GRIDS[1]:
            assert np.array_equal(call_backward(be, [shapes], cell, n1, n2, gnn[None], pad=2)[1], gpar), "not bit-identical on repetition"
            rc, zero = call_backward(be, [shapes], cell, n1, n2, np.zeros_like(gnn)[None], pad=2)
            assert rc == 0 and (zero == 0).all(), "an all-zero gnn must give an exactly zero gpar"


@pytest.mark.parametrize("backend", BACKENDS)
def test_shape_normal_field_backward_batch_with_per_point_parameters(backend):
    be = get_backend(backend)
    pts = [[(E, [0.17 + 0.02 * b, 0.11, 0.32, 0.27 + 0.01 * b, 0.3]), (R, [0.2 + 0.02 * b, 0.1, 0.95, 0.62, -0.5 + 0.1 * b]), (P, TRIANGLE)]
           for b in range(3)]
    gs = [masked_gradient(pts[b], "oblique", 33, 17, [11, b]) for b in range(3)]
    rc, gpar = call_backward(be, pts, "oblique", 33, 17, np.stack([g for g, _ in gs]))
    assert rc == 0
    for b in range(3):
        check(backend, f"batch[{b}]", gpar[b], pts[b], "oblique", 33, 17, *gs[b])
    assert not np.array_equal(gpar[0], gpar[1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_shape_normal_field_backward_150_gon(backend):
    be = get_backend(backend)
    shapes = [(P, regular(150, 0.52, 0.47, 0.3, lobes=0.15)), (E, [0.05, 0.08, 0.5, 0.5, 0.2])]      # a shape after the passes, too
    gnn, left = masked_gradient(shapes, "square", 16, 16, [13])
    rc, gpar = call_backward(be, [shapes], "square", 16, 16, gnn[None])
    assert rc == 0
    check(backend, "gon150", gpar[0], shapes, "square", 16, 16, gnn, left)


def test_reference_matches_central_differences():
    """The forward-mode reference against central differences of shape_nv_reference.field in long double (no kernel involved): every
    parameter of a rectangle + an ellipse with a nested ellipse + a triangle on the oblique cell (no Rx = Ry: a central difference across
    the tie of min(Rx, Ry) averages its two one-sided derivatives, the contract picks one).  The truncation of the difference falls as h^2
    down to h = 1e-8; the agreement there is recorded in the reference's docstring."""
    LD = np.longdouble
    shapes = STRUCTURES["rectangle"] + [(E, [0.30, 0.20, 0.52, 0.48, 0.3]), (E, [0.10, 0.08, 0.50, 0.50, 0.1]), (P, [0.05, 0.08, 0.3, 0.1, 0.12, 0.33])]
    a1, a2 = CELLS["oblique"]
    n1, n2 = 33, 17
    h = LD(1e-8)
    nom = nvr.field(shapes, a1, a2, n1, n2)
    keep = ~nvr.excluded(shapes, a1, a2, n1, n2, nom["coh"])
    tans = list(ngr.tangents(shapes, a1, a2, n1, n2))
    k, worst = 0, 0.0
    for s, (kind, par) in enumerate(shapes):
        for j in range(len(par)):
            f = []
            for sign in (1, -1):
                q = [LD(v) for v in par]
                q[j] = q[j] + sign * h
                f.append(nvr.field(shapes[:s] + [(kind, q)] + shapes[s + 1:], a1, a2, n1, n2))
            same = keep & ((f[0]["nn"] == 0).all(axis=0) == (f[1]["nn"] == 0).all(axis=0))
            fd = (f[0]["nn"] - f[1]["nn"]) / (2 * h)
            err = float(np.abs(tans[k] - fd)[:, same].max() / np.abs(tans[k])[:, same].max())
            worst = max(worst, err)
            print(f"parameter {k} (shape {s}, {j}): |tangent - FD| / max |tangent| = {err:.1e}")
            assert same.mean() > 0.99 and err <= 1e-9
            k += 1
    print(f"worst {worst:.1e}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_error_codes(backend):
    be = get_backend(backend)
    ok = [[(E, [0.3, 0.2, 0.5, 0.5, 0.0])]]
    g = np.ones((1, 3, 8, 8))
    call = lambda pts=ok, ws_short=0, **kw: call_backward(be, pts, "square", 8, 8, g, ws_short=ws_short, over=kw)[0]
    assert call() == 0
    assert call([[(3, [0.3, 0.2, 0.5, 0.5, 0.0])]]) == ARG                       # unknown kind
    assert call([[(P, [0.1, 0.1, 0.5, 0.1])]]) == ARG                            # K < 3
    assert call([[(E, [0.3, 0.2, 0.5, 0.5])]]) == ARG                            # an ellipse has five parameters
    assert call(lattice=(ctypes.c_double * 4)(1.0, 0.0, 2.0, 0.0)) == ARG        # a cell without area
    assert call(lattice=(ctypes.c_double * 4)(1.0, 0.0, 0.0, np.inf)) == ARG
    assert call(lattice=None) == ARG
    for kw in (dict(S=0), dict(npar=0), dict(batch=0), dict(batch=65536), dict(n1=0), dict(n2=-1)):
        assert call(**kw) == ARG, kw
    for name in ("kind", "voff", "par", "gnn", "gpar", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(n1=2049) == UNSUPPORTED and call(n2=2049) == UNSUPPORTED
    assert call(ws_short=8) == WS
    assert be.lib.shape_normal_field_backward_ws_bytes(1, 5, 0, 8, 8) == 0


# Worst err / floor over all the cases a backend runs, rounded up (the bound is 16).
WORST_EMU = 1.1
WORST_MI355X = 1.5
