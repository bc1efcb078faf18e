"""Mirror-symmetry folding of the layer eigenproblem: the host side (plan, validation) of include/trx.h trx_sym_fold / trx_sym_unfold.

A layer that is invariant under x -> -x about a plane, lit with kx0 = 0, has A = P Q commuting with R_x = diag(-J_x, +J_x) on [Ex; Ey]
(R_y = diag(+J_y, -J_y) for the y mirror, ky0 = 0).  J_x sends the unit vector of harmonic (m, n) to exp(+2 pi i m c / nx) times that of (-m, n),
where c is the integer with grid[i, j] == grid[(c - i) mod nx, j]: c = nx - 1 for a grid sampled at (i + 1/2) h (torcwa_amd.geometry), c = 0 for
a grid that is symmetric about sample 0.  In the basis T of joint eigenvectors of the mirrors A splits into two (one mirror) or four (two)
independent blocks; the eigenvectors come back in the original basis (W = T blockdiag(W_k)), so nothing downstream changes.
"""
import numpy as np
import torch

SYMMETRIES = ("x", "y", "xy")
# class (eigenvalue of R_x, of R_y) -> block; one mirror: +1 -> 0, -1 -> 1
_CLASS = {(1, 1): 0, (1, -1): 1, (-1, 1): 2, (-1, -1): 3}


def check_symmetry(symmetry):
    if symmetry is not None and symmetry not in SYMMETRIES:
        raise ValueError(f"symmetry must be None or one of {SYMMETRIES}, got {symmetry!r}")


def check_orders_closed(mn, symmetry):
    """ValueError unless the order set holds (-m, n) with every (m, n) for an x mirror, (m, -n) for a y mirror."""
    have = {(int(p), int(q)) for p, q in mn}
    for ax, name in ((0, "x"), (1, "y")):
        if name not in symmetry:
            continue
        for p, q in have:
            r = (-p, q) if ax == 0 else (p, -q)
            if r not in have:
                raise ValueError(f'symmetry="{symmetry}": the order set is not closed under the {name} mirror: it holds ({p}, {q}) but not {r}')


class SymPlan:
    """The sparse unitary T as trx_sym_fold reads it: idx [n,4] int32, wt [n,4] complex128 (numpy), off [nblk+1]; groups: [(size, [blocks])] in
    the packing order of include/trx.h (blocks of equal size together, groups by first block).  Device copies are made per dtype on demand."""

    def __init__(self, idx, wt, off):
        self.idx, self.wt, self.off = idx, wt, off
        self.n = int(idx.shape[0])
        self.nblk = len(off) - 1
        self.sizes = [int(off[k + 1] - off[k]) for k in range(self.nblk)]
        self.groups = []
        for k, s in enumerate(self.sizes):
            for g in self.groups:
                if g[0] == s:
                    g[1].append(k)
                    break
            else:
                self.groups.append((s, [k]))
        self._dev = {}
        self._rows, self._rows_dev = None, {}

    def device(self, device, dtype):
        """(idx, wt, off) tensors on `device`, wt in `dtype`."""
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = (torch.as_tensor(self.idx, device=device).contiguous(), torch.as_tensor(self.wt, device=device).to(dtype).contiguous(),
                              torch.as_tensor(np.asarray(self.off, dtype=np.int32), device=device).contiguous())
        return self._dev[key]

    def rows(self, device=None, dtype=None):
        """The row plan trx_sym_fold_backward reads: (ridx [n,4] int32, rwt [n,4]); slot k of row r names the column of block k whose support
        holds r and T's entry there (weight 0, index off[k], if block k has none).  Without arguments the numpy arrays (rwt complex128), else
        tensors on `device` with rwt in `dtype`, cached like device()."""
        if self._rows is None:
            ridx = np.repeat(np.asarray(self.off[:-1], dtype=np.int32)[None, :], self.n, axis=0)
            ridx = np.concatenate([ridx, np.zeros((self.n, 4 - self.nblk), dtype=np.int32)], axis=1)
            rwt = np.zeros((self.n, 4), dtype=np.complex128)
            for k in range(self.nblk):
                for j in range(self.off[k], self.off[k + 1]):
                    for q in range(4):
                        if self.wt[j, q] != 0:
                            r = self.idx[j, q]
                            if rwt[r, k] != 0:
                                raise ValueError(f"SymPlan: row {r} lies in two columns of block {k}; the supports inside a block must be disjoint")
                            ridx[r, k], rwt[r, k] = j, self.wt[j, q]
            self._rows = (np.ascontiguousarray(ridx), rwt)
        if device is None:
            return self._rows
        key = (str(device), dtype)
        if key not in self._rows_dev:
            self._rows_dev[key] = (torch.as_tensor(self._rows[0], device=device).contiguous(),
                                   torch.as_tensor(self._rows[1], device=device).to(dtype).contiguous())
        return self._rows_dev[key]

    def expansion(self, k, device, dtype):
        """(rows, src, w) of x = T_k y as plain indexing, x[rows] += w * y[src]: the non-zeros of block k's columns (rows int64 in [0, n), src
        int64 local to the block, w in `dtype`).  The rows of one block are distinct (disjoint supports).  Tensors on `device`, cached."""
        key = ("expand", k, str(device), dtype)
        if key not in self._dev:
            J, q = np.nonzero(self.wt[self.off[k]:self.off[k + 1]] != 0)
            rows = self.idx[self.off[k] + J, q].astype(np.int64)
            self._dev[key] = (torch.as_tensor(rows, device=device), torch.as_tensor(J.astype(np.int64), device=device),
                              torch.as_tensor(self.wt[self.off[k] + J, q], device=device).to(dtype))
        return self._dev[key]

    def dense(self, dtype=np.clongdouble):
        """T as a dense [n, n] numpy array (tests, diagnostics)."""
        T = np.zeros((self.n, self.n), dtype=dtype)
        for j in range(self.n):
            for q in range(4):
                if self.wt[j, q] != 0:
                    T[self.idx[j, q], j] += self.wt[j, q]
        return T


def opposite_block(nblk, k):
    """The block k' that an E -> H or H -> E operator (Q, Vf; P, Vf^-1) connects block k with: H is a pseudovector, so its mirror eigenvalues are
    minus those of E.  k' = 3 - k for two mirrors (_CLASS), 1 - k for one; block k' has the size of block k."""
    if nblk not in (2, 4) or not (0 <= k < nblk):
        raise ValueError(f"opposite_block: block {k} of {nblk}")
    return nblk - 1 - k


def sector_coordinates(plan, c):
    """T^H e_c, the unit vector of row c of the original basis in the sectors: [(k, j, w)] with w = conj(T[c, off[k] + j]) for every block k that
    has a column holding row c (at most one per block, SymPlan.rows).  The x / y component of order (0, 0) is one entry of weight 1."""
    ridx, rwt = plan.rows()
    if not (0 <= int(c) < plan.n):
        raise ValueError(f"sector_coordinates: column {c} outside [0, {plan.n})")
    return [(k, int(ridx[c, k] - plan.off[k]), complex(np.conj(rwt[c, k]))) for k in range(plan.nblk) if rwt[c, k] != 0]


def build_plan(mn, symmetry, cx=0, nx=1, cy=0, ny=1):
    """SymPlan of the order list mn [N,2] (matrix order) for symmetry "x" | "y" | "xy" and the grid centres cx, cy (see the module docstring).
    The weights carry the exact phases in float64; a column's entries are [(m, n), (-m, n), (m, -n), (-m, -n)] as far as they are distinct."""
    check_symmetry(symmetry)
    mn = np.asarray(mn, dtype=np.int64)
    check_orders_closed(mn, symmetry)
    N = len(mn)
    pos = {(int(p), int(q)): i for i, (p, q) in enumerate(mn)}
    use_x, use_y = "x" in symmetry, "y" in symmetry
    phx = lambda m: np.exp(2j * np.pi * ((m * cx) % nx) / nx) if cx else 1.0 + 0.0j
    phy = lambda q: np.exp(2j * np.pi * ((q * cy) % ny) / ny) if cy else 1.0 + 0.0j
    cols = []                                           # (block, [(row, weight)])
    for comp in (0, 1):                                 # Ex: R_x = -J_x, R_y = +J_y;  Ey: R_x = +J_x, R_y = -J_y
        sx, sy = (-1, 1) if comp == 0 else (1, -1)
        for (m, q) in ((int(p), int(r)) for p, r in mn):
            if (use_x and m < 0) or (use_y and q < 0):
                continue                                # one representative per orbit
            a_s = (1, -1) if (use_x and m > 0) else (1,)
            b_s = (1, -1) if (use_y and q > 0) else (1,)
            for a in a_s:
                for b in b_s:
                    ent = [(comp * N + pos[(m, q)], 1.0 + 0.0j)]
                    if use_x and m > 0:
                        ent.append((comp * N + pos[(-m, q)], a * phx(m)))
                    if use_y and q > 0:
                        ent.append((comp * N + pos[(m, -q)], b * phy(q)))
                    if use_x and m > 0 and use_y and q > 0:
                        ent.append((comp * N + pos[(-m, -q)], a * b * phx(m) * phy(q)))
                    rx, ry = (sx * a if use_x else 1), (sy * b if use_y else 1)
                    blk = _CLASS[(rx, ry)] if (use_x and use_y) else (0 if (rx if use_x else ry) == 1 else 1)
                    cols.append((blk, [(r, w / np.sqrt(len(ent))) for r, w in ent]))
    nblk = 4 if (use_x and use_y) else 2
    cols.sort(key=lambda c: c[0])                       # stable: generation order inside a block
    n = 2 * N
    assert len(cols) == n
    idx = np.zeros((n, 4), dtype=np.int32)
    wt = np.zeros((n, 4), dtype=np.complex128)
    off = np.zeros(nblk + 1, dtype=np.int32)
    for j, (blk, ent) in enumerate(cols):
        off[blk + 1:] += 1
        idx[j, :] = ent[0][0]
        for q, (r, w) in enumerate(ent):
            idx[j, q], wt[j, q] = r, w
    return SymPlan(idx, wt, off)


def grid_centres(grids, symmetry, tol):
    """(cx, nx, cy, ny) of the patterned grids ([B,nx,ny] or [nx,ny] tensors on one device) of a layer: per claimed axis the c with
    max |g[i] - g[(c - i) mod nx]| <= tol max |g| for EVERY grid, c = nx - 1 tried before c = 0; an axis that is not claimed, or c = 0, gives
    (0, 1).  ValueError when a claimed mirror fits neither.  One device reduction (all figures in one tensor, one transfer)."""
    figs = []
    for g in grids:
        g = g if g.dim() == 3 else g[None]
        a = torch.abs(g).amax().to(torch.float64)
        row = [a]
        for ax, name in ((1, "x"), (2, "y")):
            if name in symmetry:
                f = torch.flip(g, dims=(ax,))
                row += [torch.abs(g - f).amax().to(torch.float64), torch.abs(g - torch.roll(f, 1, dims=ax)).amax().to(torch.float64)]
        figs.append(torch.stack(row))
    figs = torch.stack(figs).cpu().numpy()              # [grids, 1 + 2 axes]
    out = []
    col = 1
    for ax, name in ((1, "x"), (2, "y")):
        if name not in symmetry:
            out += [0, 1]
            continue
        sizes = {int(g.shape[ax - 3]) for g in grids}
        ok_half = bool((figs[:, col] <= tol * figs[:, 0]).all())
        ok_zero = bool((figs[:, col + 1] <= tol * figs[:, 0]).all())
        if ok_half and len(sizes) == 1:
            nn = sizes.pop()
            out += [nn - 1, nn]
        elif ok_zero:
            out += [0, 1]
        elif ok_half:
            raise ValueError(f'symmetry="{symmetry}": the eps and mu grids of a layer mirror about their half-cell centre along {name} but differ '
                             f"in size along it ({sorted(sizes)}): their Fourier phases differ, give them one size")
        else:
            worst = float((np.minimum(figs[:, col], figs[:, col + 1]) / np.maximum(figs[:, 0], 1e-300)).max())
            raise ValueError(f'symmetry="{symmetry}": a grid of this layer is not mirror-symmetric along {name}: max |g[i] - g[(c - i) mod n]| / max |g| '
                             f"= {worst:.3g} for the better of c = n - 1 and c = 0, above symmetry_tol = {tol:g}")
        col += 2
    return tuple(out)
