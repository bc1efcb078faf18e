"""Thin, batched Python face of the C ABI in include/trx.h.

`Engine` owns nothing but a library handle and a device: every call allocates its outputs/workspaces as torch
tensors on that device (PyTorch is used only for device memory and streams) and passes raw pointers plus the current
HIP stream to libtrx.  There is no CPU fallback: the default engine binds torcwa_amd/libtrx.so (gfx950) and requires
a CUDA/ROCm device.  (The test-suite can inject the kernel-logic emulator build with host tensors; see tests/.)
"""
import ctypes
import os
import threading

import torch

from . import _lib

_CODE = {torch.complex64: _lib.C64, torch.complex128: _lib.C128}
_REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}


class NumericalError(RuntimeError):
    pass


def _phase(name):
    """Wall-clock bracket of an Engine method for the per-phase table of bench.py: when `engine.profile_phases` is on, a pair of HIP events
    is recorded on the current stream around the call (no synchronisation; Engine.phase_report() reads them after the timed region)."""
    def deco(fn):
        def wrapped(self, *a, **kw):
            if not self.profile_phases or self.device.type != "cuda":
                return fn(self, *a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
            try:
                return fn(self, *a, **kw)
            finally:
                e1.record(torch.cuda.current_stream(self.device))
                self._phase_events.append((name, e0, e1))
        wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
        return wrapped
    return deco


class Engine:
    def __init__(self, lib=None, device=None):
        if lib is None:
            lib = _lib.lib()                       # raises TrxError if libtrx.so has not been built
            if device is None:
                device = torch.device("cuda")
            device = torch.device(device)
            if device.type != "cuda" or not torch.cuda.is_available():
                raise _lib.TrxError("torcwa_amd runs on an MI355X (ROCm) device only; no CPU path exists. "
                                    f"Requested device: {device}, torch.cuda.is_available()={torch.cuda.is_available()}")
        self.lib = lib
        self.device = torch.device(device if device is not None else "cpu")
        self.check_info = True
        self._fail_acc = {}            # per host thread: device-side count of non-zero info entries seen while check_info is False
        self.last_eig_fallback = 0
        self._tls = threading.local()
        self.profile_phases = False    # bench.py: event pairs around the phases of a layer-solve (see _phase)
        self._phase_events = []

    def phase_report(self, reset=True):
        """{phase: summed milliseconds} of the calls bracketed since the last reset (synchronises the device)."""
        out = {}
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for name, e0, e1 in self._phase_events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        if reset:
            self._phase_events = []
        return out

    # -- helpers ---------------------------------------------------------------------------------------
    @property
    def stream(self):
        if self.device.type == "cuda":
            return torch.cuda.current_stream(self.device).cuda_stream
        return None

    def _ws(self, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)

    def _ints(self, n):
        return torch.zeros(int(n), dtype=torch.int32, device=self.device)

    @staticmethod
    def _c(t):
        return t if t.is_contiguous() else t.contiguous()

    def failures(self):
        """Number of batch entries that reported a numerical failure since the last call (one device sync).  The counters are
        kept per host thread (each thread accumulates on its own stream); they are combined here after a device-wide sync."""
        acc, self._fail_acc = self._fail_acc, {}
        if not acc:
            return 0
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return sum(int(c) for c in acc.values())

    def _check(self, *tensors):
        """Raw pointers carry no type information: refuse operands on another device or of mixed / non-complex dtypes here,
        instead of an invalid device access or garbage inside the kernel."""
        dt = tensors[0].dtype
        for t in tensors:
            if t.device != self.device and not (t.device.type == self.device.type and self.device.index is None):
                raise ValueError(f"libtrx operand on {t.device}, engine on {self.device}")
            if t.dtype != dt or dt not in _CODE:
                raise TypeError(f"libtrx operands must share one complex dtype (got {[str(x.dtype) for x in tensors]})")

    def _info(self, info, what):
        if not self.check_info:        # deferred, sync-free accounting (throughput runs); read with failures()
            c = (info != 0).sum()
            tid = threading.get_ident()
            prev = self._fail_acc.get(tid)
            self._fail_acc[tid] = c if prev is None else prev + c
            return
        if self.check_info:
            bad = int((info != 0).sum())
            if bad:
                raise NumericalError(f"{what}: {bad} of {info.numel()} batch entries reported a numerical failure "
                                     f"(info={info[info != 0][:8].tolist()})")

    # -- a5 --------------------------------------------------------------------------------------------
    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat(self, grid, ox, oy, dtype):
        """[B,nx,ny] real/complex grid -> [B,N,N] convolution matrix (torcwa/rcwa.py:1183-1204)."""
        B, nx, ny = grid.shape
        cplx = grid.is_complex()
        grid = self._c(grid.to(dtype if cplx else _REAL[dtype]))
        N = (2 * ox + 1) * (2 * oy + 1)
        out = torch.empty((B, N, N), dtype=dtype, device=self.device)
        nws = self.lib.convmat_ws_bytes(_CODE[dtype], B, nx, ny, ox, oy)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat(_CODE[dtype], int(cplx), grid.data_ptr(), B, nx, ny, ox, oy, out.data_ptr(),
                                        ws.data_ptr(), nws, self.stream))
        return out

    def _orders(self, mn, mmax=None, nmax=None):
        """[N,2] harmonic list -> (contiguous int32 tensor on the device, N, mmax, nmax); the box defaults to the list's largest |m|, |n|."""
        mn = torch.as_tensor(mn)
        if mmax is None or nmax is None:
            mmax, nmax = (int(v) for v in mn.detach().abs().amax(dim=0).cpu())
        return self._c(mn.to(device=self.device, dtype=torch.int32)), int(mn.shape[0]), int(mmax), int(nmax)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_orders(self, grid, mn, dtype, mmax=None, nmax=None):
        """[B,n1,n2] real/complex grid and [N,2] harmonic list (m, n) -> [B,N,N] convolution matrix out[b,i,j] = c[m_i-m_j, n_i-n_j]
        (include/trx.h: trx_convmat_orders).  mmax / nmax: the coefficient box (default: the largest |m| / |n| of the list)."""
        B, n1, n2 = grid.shape
        cplx = grid.is_complex()
        grid = self._c(grid.to(dtype if cplx else _REAL[dtype]))
        mn, N, mmax, nmax = self._orders(mn, mmax, nmax)
        out = torch.empty((B, N, N), dtype=dtype, device=self.device)
        nws = self.lib.convmat_orders_ws_bytes(_CODE[dtype], B, n1, n2, N, mmax, nmax)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_orders(_CODE[dtype], int(cplx), grid.data_ptr(), B, n1, n2, mn.data_ptr(), N, mmax, nmax, out.data_ptr(),
                                               ws.data_ptr(), nws, self.stream))
        return out

    def _shape_args(self, packed):
        """The device operands of a packed shape list (shapes.ShapeLayer.pack): kind [S], voff [S+1] int32, par [B, npar] fp64, val [B, S+1]
        complex128, and the host double[4] of the reciprocal vectors."""
        kind = self._c(packed.kind.to(device=self.device, dtype=torch.int32))
        voff = self._c(packed.voff.to(device=self.device, dtype=torch.int32))
        par = self._c(packed.par.detach().to(device=self.device, dtype=torch.float64))
        val = self._c(packed.val.detach().to(device=self.device, dtype=torch.complex128))
        recip = (ctypes.c_double * 4)(*[float(v) for v in packed.recip])
        return kind, voff, par, val, recip

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_shapes(self, packed, mn, dtype, mmax=None, nmax=None, want_coef=False):
        """Packed vector shapes and an [N,2] harmonic list -> [B,N,N] convolution matrix from the closed-form Fourier coefficients
        (include/trx.h: trx_convmat_shapes).  want_coef: also return the complex128 box [B, 4mmax+1, 4nmax+1]."""
        kind, voff, par, val, recip = self._shape_args(packed)
        B, npar = par.shape
        mn, N, mmax, nmax = self._orders(mn, mmax, nmax)
        out = torch.empty((B, N, N), dtype=dtype, device=self.device)
        coef = torch.empty((B, 4 * mmax + 1, 4 * nmax + 1), dtype=torch.complex128, device=self.device) if want_coef else None
        nws = self.lib.convmat_shapes_ws_bytes(_CODE[dtype], B, N, mmax, nmax)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_shapes(_CODE[dtype], kind.data_ptr(), voff.data_ptr(), int(kind.numel()), par.data_ptr(), npar,
                                               val.data_ptr(), ctypes.addressof(recip), float(packed.cell_area), B, mn.data_ptr(), N, mmax, nmax,
                                               out.data_ptr(), coef.data_ptr() if want_coef else None, ws.data_ptr(), nws, self.stream))
        return (out, coef) if want_coef else out

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def toeplitz_sums(self, gE, mn, mmax=None, nmax=None):
        """Adjoint of the Toeplitz gather: [B,N,N] -> the complex128 box [B, 4mmax+1, 4nmax+1] of diagonal sums (trx_toeplitz_sums)."""
        self._check(gE)
        gE = self._c(gE)
        B = gE.shape[0]
        mn, N, mmax, nmax = self._orders(mn, mmax, nmax)
        gbox = torch.empty((B, 4 * mmax + 1, 4 * nmax + 1), dtype=torch.complex128, device=self.device)
        nws = self.lib.toeplitz_sums_ws_bytes(_CODE[gE.dtype], B, N, mmax, nmax)
        ws = self._ws(nws)
        self.lib.check(self.lib.toeplitz_sums(_CODE[gE.dtype], gE.data_ptr(), B, mn.data_ptr(), N, mmax, nmax, gbox.data_ptr(), ws.data_ptr(), nws,
                                              self.stream))
        return gbox

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_shapes_backward(self, packed, gbox, mmax, nmax):
        """(gpar [B, npar] fp64, gval [B, S+1] complex128) from the gradient of the coefficient box (trx_convmat_shapes_backward)."""
        kind, voff, par, val, recip = self._shape_args(packed)
        B, npar = par.shape
        S = int(kind.numel())
        gbox = self._c(gbox.to(torch.complex128))
        gpar = torch.empty((B, npar), dtype=torch.float64, device=self.device)
        gval = torch.empty((B, S + 1), dtype=torch.complex128, device=self.device)
        self.lib.check(self.lib.convmat_shapes_backward(kind.data_ptr(), voff.data_ptr(), S, par.data_ptr(), npar, val.data_ptr(),
                                                        ctypes.addressof(recip), float(packed.cell_area), B, int(mmax), int(nmax),
                                                        gbox.data_ptr(), gpar.data_ptr(), gval.data_ptr(), self.stream))
        return gpar, gval

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_li(self, grid, ox, oy, dtype, keep_inverses=False):
        """[B,nx,ny] grid -> (Ex, Ey) [B,N,N], Li's inverse-rule convolution matrices of the x and y field components (include/trx.h:
        trx_convmat_li).  keep_inverses: also return the complex128 Toeplitz inverses Ux [B,nx,2oy+1,2oy+1], Uy [B,ny,2ox+1,2ox+1]
        (for the adjoint); otherwise (Ex, Ey, None, None)."""
        B, nx, ny = grid.shape
        cplx = grid.is_complex()
        grid = self._c(grid.to(dtype if cplx else _REAL[dtype]))
        N = (2 * ox + 1) * (2 * oy + 1)
        Ex = torch.empty((B, N, N), dtype=dtype, device=self.device)
        Ey = torch.empty_like(Ex)
        Ux = Uy = None
        if keep_inverses:
            Ux = torch.empty((B, nx, 2 * oy + 1, 2 * oy + 1), dtype=torch.complex128, device=self.device)
            Uy = torch.empty((B, ny, 2 * ox + 1, 2 * ox + 1), dtype=torch.complex128, device=self.device)
        info = self._ints(B)
        nws = self.lib.convmat_li_ws_bytes(_CODE[dtype], B, nx, ny, ox, oy)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_li(_CODE[dtype], int(cplx), grid.data_ptr(), B, nx, ny, ox, oy, Ex.data_ptr(), Ey.data_ptr(),
                                           Ux.data_ptr() if keep_inverses else None, Uy.data_ptr() if keep_inverses else None,
                                           info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "convmat_li (1: zero grid value, 2: singular Toeplitz block)")
        return Ex, Ey, Ux, Uy

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_li_shapes(self, packed, rval, Lx, Ly, ox, oy, dtype, keep=False):
        """Packed axis-aligned rectangles -> (Ex, Ey) [B,N,N], Li's inverse-rule matrices in closed form (include/trx.h:
        trx_convmat_li_shapes).  rval: [B,S+1] reciprocal values (shapes.ShapeLayer.reciprocal_values).  keep: also return what the adjoint
        needs, (Ex, Ey, Ux [B,K,2oy+1,2oy+1], Uy [B,K,2ox+1,2ox+1], brk [B,2,K+1] float64, rec [B,2,3S] int32), K = 2S + 1."""
        kind, voff, par, _, _ = self._shape_args(packed)
        rval = self._c(rval.detach().to(device=self.device, dtype=torch.complex128))
        B, npar = par.shape
        S = int(kind.numel())
        K = 2 * S + 1
        N = (2 * ox + 1) * (2 * oy + 1)
        Ex = torch.empty((B, N, N), dtype=dtype, device=self.device)
        Ey = torch.empty_like(Ex)
        Ux = Uy = brk = rec = None
        if keep:
            Ux = torch.empty((B, K, 2 * oy + 1, 2 * oy + 1), dtype=torch.complex128, device=self.device)
            Uy = torch.empty((B, K, 2 * ox + 1, 2 * ox + 1), dtype=torch.complex128, device=self.device)
            brk = torch.empty((B, 2, K + 1), dtype=torch.float64, device=self.device)
            rec = torch.empty((B, 2, 3 * S), dtype=torch.int32, device=self.device)
        info = self._ints(B)
        nws = self.lib.convmat_li_shapes_ws_bytes(_CODE[dtype], B, S, ox, oy)
        ws = self._ws(nws)
        opt = lambda t: t.data_ptr() if t is not None else None
        self.lib.check(self.lib.convmat_li_shapes(_CODE[dtype], kind.data_ptr(), voff.data_ptr(), S, par.data_ptr(), npar, rval.data_ptr(),
                                                  float(Lx), float(Ly), B, ox, oy, Ex.data_ptr(), Ey.data_ptr(), opt(Ux), opt(Uy), opt(brk),
                                                  opt(rec), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "convmat_li_shapes (1: an rval entry not finite or a zero background value, 2: singular Toeplitz block, 3: a rectangle that is "
                         "rotated, without area or wider than the cell)")
        return (Ex, Ey, Ux, Uy, brk, rec) if keep else (Ex, Ey)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_li_shapes_backward(self, packed, rval, Lx, Ly, ox, oy, brk, rec, ga_x, gw_y, ga_y, gw_x):
        """(gpar [B, npar] fp64, grval [B, S+1] complex128) from the adjoints of the strip tables (trx_convmat_li_shapes_backward)."""
        kind, voff, par, _, _ = self._shape_args(packed)
        rval = self._c(rval.detach().to(device=self.device, dtype=torch.complex128))
        B, npar = par.shape
        S = int(kind.numel())
        tabs = [self._c(t.to(torch.complex128)) for t in (ga_x, gw_y, ga_y, gw_x)]
        gpar = torch.empty((B, npar), dtype=torch.float64, device=self.device)
        grval = torch.empty((B, S + 1), dtype=torch.complex128, device=self.device)
        self.lib.check(self.lib.convmat_li_shapes_backward(kind.data_ptr(), voff.data_ptr(), S, par.data_ptr(), npar, rval.data_ptr(), float(Lx),
                                                           float(Ly), B, ox, oy, self._c(brk).data_ptr(), self._c(rec).data_ptr(),
                                                           *[t.data_ptr() for t in tabs], gpar.data_ptr(), grval.data_ptr(), self.stream))
        return gpar, grval

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def normal_field(self, grid, sigma, hx=1.0, hy=1.0):
        """[B,nx,ny] grid -> [B,3,nx,ny] float64 products (Nx^2, Nx Ny, Ny^2) of the normal-vector field derived from the grid
        (include/trx.h: trx_normal_field; sigma in cells, hx / hy the grid spacings)."""
        B, nx, ny = grid.shape
        cplx = grid.is_complex()
        dt = grid.dtype if grid.dtype in (torch.float32, torch.complex64) else (torch.complex128 if cplx else torch.float64)
        grid = self._c(grid.to(dt))
        code = _lib.C64 if dt in (torch.float32, torch.complex64) else _lib.C128
        nn = torch.empty((B, 3, nx, ny), dtype=torch.float64, device=self.device)
        nws = self.lib.normal_field_ws_bytes(code, B, nx, ny)
        ws = self._ws(nws)
        self.lib.check(self.lib.normal_field(code, int(cplx), grid.data_ptr(), B, nx, ny, float(sigma), float(hx), float(hy), nn.data_ptr(),
                                             ws.data_ptr(), nws, self.stream))
        return nn

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_nv(self, grid, ox, oy, dtype, *, sigma=None, hx=1.0, hy=1.0, nn=None):
        """[B,nx,ny] grid -> (Exx, Exy, Eyy) [B,N,N], the normal-vector tensor of convolution matrices (include/trx.h: trx_convmat_nv).
        nn: [B,3,nx,ny] float64 product grids of a caller-supplied field, or None to derive the field from the grid with blur `sigma`."""
        B, nx, ny = grid.shape
        cplx = grid.is_complex()
        grid = self._c(grid.to(dtype if cplx else _REAL[dtype]))
        N = (2 * ox + 1) * (2 * oy + 1)
        Exx = torch.empty((B, N, N), dtype=dtype, device=self.device)
        Exy, Eyy = torch.empty_like(Exx), torch.empty_like(Exx)
        if nn is not None:
            nn = self._c(nn.to(device=self.device, dtype=torch.float64))
            if tuple(nn.shape) != (B, 3, nx, ny):
                raise ValueError(f"normal-field products must be [{B}, 3, {nx}, {ny}], got {list(nn.shape)}")
        elif sigma is None:
            raise ValueError("convmat_nv needs sigma when no field is supplied")
        info = self._ints(B)
        nws = self.lib.convmat_nv_ws_bytes(_CODE[dtype], B, nx, ny, ox, oy)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_nv(_CODE[dtype], int(cplx), grid.data_ptr(), B, nx, ny, ox, oy, float(sigma or 0.0), float(hx), float(hy),
                                           nn.data_ptr() if nn is not None else None, Exx.data_ptr(), Exy.data_ptr(), Eyy.data_ptr(),
                                           info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "convmat_nv (1: zero grid value, 2: singular [1/eps])")
        return Exx, Exy, Eyy

    @staticmethod
    def _cell(h):
        """host double[4] (row-major 2 x 2 cell matrix) for the C ABI."""
        return (ctypes.c_double * 4)(*torch.as_tensor(h, dtype=torch.float64).reshape(4).tolist())

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def normal_field_lattice(self, grid, sigma, h):
        """normal_field on an oblique cell: h is the 2 x 2 cell matrix, rows a1/n1 and a2/n2 (include/trx.h: trx_normal_field_lattice)."""
        B, n1, n2 = grid.shape
        cplx = grid.is_complex()
        dt = grid.dtype if grid.dtype in (torch.float32, torch.complex64) else (torch.complex128 if cplx else torch.float64)
        grid = self._c(grid.to(dt))
        code = _lib.C64 if dt in (torch.float32, torch.complex64) else _lib.C128
        nn = torch.empty((B, 3, n1, n2), dtype=torch.float64, device=self.device)
        nws = self.lib.normal_field_ws_bytes(code, B, n1, n2)
        ws = self._ws(nws)
        self.lib.check(self.lib.normal_field_lattice(code, int(cplx), grid.data_ptr(), B, n1, n2, float(sigma), self._cell(h), nn.data_ptr(),
                                                     ws.data_ptr(), nws, self.stream))
        return nn

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_nv_orders(self, grid, mn, dtype, *, sigma=None, h=None, nn=None, mmax=None, nmax=None):
        """convmat_nv for an [N,2] harmonic list on an oblique cell (include/trx.h: trx_convmat_nv_orders): (Exx, Exy, Eyy) [B,N,N].
        h: the 2 x 2 cell matrix (rows a1/n1, a2/n2) that orients the derived field; nn: [B,3,n1,n2] float64 products of a supplied field."""
        B, n1, n2 = grid.shape
        cplx = grid.is_complex()
        grid = self._c(grid.to(dtype if cplx else _REAL[dtype]))
        mn, N, mmax, nmax = self._orders(mn, mmax, nmax)
        Exx = torch.empty((B, N, N), dtype=dtype, device=self.device)
        Exy, Eyy = torch.empty_like(Exx), torch.empty_like(Exx)
        if nn is not None:
            nn = self._c(nn.to(device=self.device, dtype=torch.float64))
            if tuple(nn.shape) != (B, 3, n1, n2):
                raise ValueError(f"normal-field products must be [{B}, 3, {n1}, {n2}], got {list(nn.shape)}")
        elif sigma is None or h is None:
            raise ValueError("convmat_nv_orders needs sigma and h when no field is supplied")
        info = self._ints(B)
        nws = self.lib.convmat_nv_orders_ws_bytes(_CODE[dtype], B, n1, n2, N, mmax, nmax)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_nv_orders(_CODE[dtype], int(cplx), grid.data_ptr(), B, n1, n2, mn.data_ptr(), N, mmax, nmax,
                                                  float(sigma or 0.0), self._cell(h) if h is not None else None,
                                                  nn.data_ptr() if nn is not None else None, Exx.data_ptr(), Exy.data_ptr(), Eyy.data_ptr(),
                                                  info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "convmat_nv_orders (1: zero grid value, 2: singular [1/eps])")
        return Exx, Exy, Eyy

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def shape_normal_field(self, packed, lattice, n1, n2):
        """Packed vector shapes and the lattice (rows a1, a2) -> [B,3,n1,n2] float64 products (Nx^2, Nx Ny, Ny^2) of the blended normal field
        of the shape list at the DFT's sample positions (include/trx.h: trx_shape_normal_field)."""
        kind, voff, par, _, _ = self._shape_args(packed)
        B, npar = par.shape
        nn = torch.empty((B, 3, int(n1), int(n2)), dtype=torch.float64, device=self.device)
        self.lib.check(self.lib.shape_normal_field(kind.data_ptr(), voff.data_ptr(), int(kind.numel()), par.data_ptr(), npar, self._cell(lattice),
                                                   B, int(n1), int(n2), nn.data_ptr(), self.stream))
        return nn

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def shape_normal_field_backward(self, packed, lattice, gnn):
        """gpar [B, npar] fp64 from the gradient gnn [B,3,n1,n2] of the field products: the adjoint of shape_normal_field (include/trx.h:
        trx_shape_normal_field_backward)."""
        kind, voff, par, _, _ = self._shape_args(packed)
        B, npar = par.shape
        gnn = self._c(gnn.to(device=self.device, dtype=torch.float64))
        if gnn.dim() != 4 or tuple(gnn.shape[:2]) != (B, 3):
            raise ValueError(f"the gradient of the field products must be [{B}, 3, n1, n2], got {list(gnn.shape)}")
        n1, n2 = int(gnn.shape[2]), int(gnn.shape[3])
        S = int(kind.numel())
        gpar = torch.empty((B, npar), dtype=torch.float64, device=self.device)
        nws = self.lib.shape_normal_field_backward_ws_bytes(S, npar, B, n1, n2)
        ws = self._ws(nws)
        self.lib.check(self.lib.shape_normal_field_backward(kind.data_ptr(), voff.data_ptr(), S, par.data_ptr(), npar, self._cell(lattice), B, n1,
                                                            n2, gnn.data_ptr(), gpar.data_ptr(), ws.data_ptr(), nws, self.stream))
        return gpar

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def convmat_nv_shapes(self, packed, rval, lattice, mn, dtype, n1, n2, *, nn=None, mmax=None, nmax=None):
        """Packed vector shapes -> (Exx, Exy, Eyy) [B,N,N], the normal-vector tensor with closed-form [eps] and [1/eps] (include/trx.h:
        trx_convmat_nv_shapes).  rval: [B,S+1] reciprocal values (shapes.ShapeLayer.reciprocal_values); nn: [B,3,n1,n2] float64 products of a
        supplied field, or None to sample the field of the shape list on n1 x n2."""
        kind, voff, par, val, recip = self._shape_args(packed)
        B, npar = par.shape
        n1, n2 = int(n1), int(n2)
        rval = self._c(rval.detach().to(device=self.device, dtype=torch.complex128))
        if tuple(rval.shape) != tuple(val.shape):
            raise ValueError(f"reciprocal values must be {list(val.shape)} like val, got {list(rval.shape)}")
        mn, N, mmax, nmax = self._orders(mn, mmax, nmax)
        Exx = torch.empty((B, N, N), dtype=dtype, device=self.device)
        Exy, Eyy = torch.empty_like(Exx), torch.empty_like(Exx)
        if nn is not None:
            nn = self._c(nn.to(device=self.device, dtype=torch.float64))
            if tuple(nn.shape) != (B, 3, n1, n2):
                raise ValueError(f"normal-field products must be [{B}, 3, {n1}, {n2}], got {list(nn.shape)}")
        info = self._ints(B)
        nws = self.lib.convmat_nv_shapes_ws_bytes(_CODE[dtype], B, n1, n2, N, mmax, nmax)
        ws = self._ws(nws)
        self.lib.check(self.lib.convmat_nv_shapes(_CODE[dtype], kind.data_ptr(), voff.data_ptr(), int(kind.numel()), par.data_ptr(), npar,
                                                  val.data_ptr(), rval.data_ptr(), ctypes.addressof(recip), float(packed.cell_area),
                                                  self._cell(lattice), B, n1, n2, mn.data_ptr(), N, mmax, nmax,
                                                  nn.data_ptr() if nn is not None else None, Exx.data_ptr(), Exy.data_ptr(), Eyy.data_ptr(),
                                                  info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "convmat_nv_shapes (1: a medium with eps zero or non-finite, 2: singular [1/eps])")
        return Exx, Exy, Eyy

    # -- dense blocks ----------------------------------------------------------------------------------
    def gemm(self, A, Bm, *, opA=0, opB=0, alpha=1.0, beta=0.0, out=None):
        """Batched C = alpha op(A) op(B) + beta C for contiguous [B,*,*] operands."""
        A, Bm = self._c(A), self._c(Bm)
        self._check(A, Bm)
        dt = A.dtype
        Bt = A.shape[0]
        m = A.shape[1] if opA == 0 else A.shape[2]
        k = A.shape[2] if opA == 0 else A.shape[1]
        n = Bm.shape[2] if opB == 0 else Bm.shape[1]
        if out is None:
            out = torch.empty((Bt, m, n), dtype=dt, device=self.device)
        ctype = ctypes.c_double if dt == torch.complex128 else ctypes.c_float
        al = (ctype * 2)(complex(alpha).real, complex(alpha).imag)
        be = (ctype * 2)(complex(beta).real, complex(beta).imag)
        self.lib.check(self.lib.gemm(_CODE[dt], opA, opB, m, n, k, ctypes.addressof(al), A.data_ptr(), A.shape[2],
                                     A.shape[1] * A.shape[2], Bm.data_ptr(), Bm.shape[2], Bm.shape[1] * Bm.shape[2],
                                     ctypes.addressof(be), out.data_ptr(), n, m * n, Bt, self.stream))
        return out

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def inverse(self, A):
        """Returns inv(A) for [B,n,n] (A is not modified)."""
        self._check(A)
        A = A.clone()
        B, n, _ = A.shape
        piv, info = self._ints(B * n), self._ints(B)
        nws = self.lib.inverse_ws_bytes(_CODE[A.dtype], n, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.inverse(_CODE[A.dtype], A.data_ptr(), n, B, piv.data_ptr(), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "inverse")
        return A

    @_phase("other (gemm / solve)")
    def solve(self, A, Bm):
        """Returns X with A X = B ([B,n,n], [B,n,r]); inputs are not modified."""
        self._check(A, Bm)
        A, X = A.clone(), Bm.clone()
        B, n, _ = A.shape
        piv, info = self._ints(B * n), self._ints(B)
        self.lib.check(self.lib.lu_solve(_CODE[A.dtype], A.data_ptr(), n, X.data_ptr(), X.shape[2], B, piv.data_ptr(), info.data_ptr(), self.stream))
        self._info(info, "lu_solve")
        return X

    # -- a7 --------------------------------------------------------------------------------------------
    @_phase("eigendecomposition (trx_eig)")
    def eig(self, A, destroy=False, refine_steps=0, route=0, out=None):
        """(w [B,n], V [B,n,n]) with A V = V diag(w) (torcwa/torch_eig.py:14).

        refine_steps: Newton steps of libtrx's mixed-precision route (complex128 input of at least 256 rows: fp32 eigendecomposition
        refined in fp64, include/trx.h "eig_refine"); 0 = the library default (2: the accuracy class of the all-fp64 pipeline; measured on
        MI355X, one step is NOT enough for the 1e-5 gate of a complex64 problem at order [15,15] -- the fp32 start of this pipeline leaves
        max |E| ~ 2e-2 ... 2e-1 there).
        route: 0 = the library's automatic choice (mixed precision for complex128 input with n >= 256 and batch >= 8), 1 = all-fp64 (all-fp32 for
        complex64 input), 3 = mixed wherever n >= 8 (include/trx.h "eig_vec").  After the call `eig_fallback_of_last_call()` gives the number of
        matrices the mixed route redid in fp64 (per calling thread).
        out: optional (w, V) contiguous tensors of the result's shapes to write into (e.g. slices of the packed buffer of sym_packed)."""
        self._check(A)
        if int(route) not in (0, 1, 3):
            raise ValueError("eig route must be 0 (automatic), 1 (one precision) or 3 (mixed); 2 was the removed inverse-iteration route")
        opts = (int(refine_steps) & 0xF) | ((int(route) & 0xF) << 4)          # per-call option word of trx_eig_opts (no process-global knob is touched: thread-safe)
        # (No route policy lives here any more: matrices the mixed-precision route cannot certify -- clusters of close eigenvalues beyond the
        # refinement's exact treatment -- are redone in fp64 INSIDE the library, as a sub-batch; results do not depend on call history.)
        A = self._c(A) if destroy else A.clone()
        B, n, _ = A.shape
        dt = A.dtype
        if out is None:
            w = torch.empty((B, n), dtype=dt, device=self.device)
            V = torch.empty((B, n, n), dtype=dt, device=self.device)
        else:
            w, V = out
            self._check(A, w, V)
            if tuple(w.shape) != (B, n) or tuple(V.shape) != (B, n, n) or not (w.is_contiguous() and V.is_contiguous()):
                raise ValueError(f"eig: out must be contiguous ([{B}, {n}], [{B}, {n}, {n}]), got {list(w.shape)} and {list(V.shape)}")
        info = self._ints(B)
        nws = self.lib.eig_ws_bytes_opts(_CODE[dt], n, B, opts)
        ws = self._ws(nws)
        self.lib.check(self.lib.eig_opts(_CODE[dt], A.data_ptr(), w.data_ptr(), V.data_ptr(), n, B, info.data_ptr(), ws.data_ptr(), nws, self.stream, opts))
        fb = int(self.lib.eig_last_fallback())        # matrices of THIS call redone in fp64 (thread-local in the library: the calling thread's last trx_eig)
        self._tls.eig_fallback = fb                   # per host thread: the solver that called reads its own call's count (eig_fallback_of_last_call)
        self.last_eig_fallback = fb                   # diagnostic only: shared by every thread of a multi-stream sweep
        self._info(info, "eig")
        return w, V

    def eig_fallback_of_last_call(self):
        """Matrices the calling thread's last `eig` redid in fp64 (0 if this thread has not called it)."""
        return getattr(self._tls, "eig_fallback", 0)

    @_phase("adjoint (eig backward, solves)")
    def eig_backward(self, w, V, gw, gV, broadening):
        """gA of the reference's broadened eig adjoint (torcwa/torch_eig.py:19-44) in one library call."""
        B, n, _ = V.shape
        dt = V.dtype
        gA = torch.empty((B, n, n), dtype=dt, device=self.device)
        piv, info = self._ints(B * n), self._ints(B)
        nws = self.lib.eig_backward_ws_bytes(_CODE[dt], n, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.eig_backward(_CODE[dt], self._c(w).data_ptr(), self._c(V).data_ptr(), self._c(gw.to(dt)).data_ptr(),
                                             self._c(gV.to(dt)).data_ptr(), float(broadening), n, B, gA.data_ptr(), piv.data_ptr(), info.data_ptr(),
                                             ws.data_ptr(), nws, self.stream))
        self._info(info, "eig_backward")
        return gA

    # -- a6 / a8 / a9 ----------------------------------------------------------------------------------
    @_phase("layer S-matrix (V = P^-1 W Kz, trx_layer_smatrix)")
    def hmodes(self, E, mu, kx, ky, W, kz):
        """V = P^-1 W diag(kz) for homogeneous mu [B] via the rank-N structure of P (include/trx.h: trx_hmodes)."""
        B, n, _ = W.shape
        N = n // 2
        dt = W.dtype
        V = torch.empty((B, n, n), dtype=dt, device=self.device)
        piv, info = self._ints(B * N), self._ints(B)
        nws = self.lib.hmodes_ws_bytes(_CODE[dt], N, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.hmodes(_CODE[dt], self._c(E).data_ptr(), self._c(mu.to(dt)).data_ptr(), self._c(kx).data_ptr(), self._c(ky).data_ptr(),
                                       self._c(W).data_ptr(), self._c(kz).data_ptr(), N, B, V.data_ptr(), piv.data_ptr(), info.data_ptr(),
                                       ws.data_ptr(), nws, self.stream))
        self._info(info, "hmodes")
        return V

    @_phase("layer S-matrix (V = P^-1 W Kz, trx_layer_smatrix)")
    def layer_smatrix(self, P, Q, W, kzfac, vfinv, phase, *, use_q=False, want_c=True, V=None):
        """Layer S-matrix (torcwa/rcwa.py:1244-1281).  vfinv: [4,B,N]; returns S11, S21, V, Cplus, Cminus.
        V given (from hmodes): the H-field modes are taken as input (use_q = 2 of the C ABI)."""
        B, n, _ = W.shape
        N = n // 2
        dt = W.dtype
        S = torch.empty((2, B, n, n), dtype=dt, device=self.device)     # S11 | S21 contiguous: without coupling coefficients they double
        S11, S21 = S[0], S[1]                                           # as the kernel's last scratch block (include/trx.h)
        if V is not None:
            V, use_q = self._c(V), 2
        else:
            V = torch.empty_like(S11)
        cp = torch.empty_like(S11) if want_c else None
        cm = torch.empty_like(S11) if want_c else None
        piv, info = self._ints(3 * B * n), self._ints(3 * B)
        nws = (self.lib.layer_smatrix_ws_bytes if want_c else self.lib.layer_smatrix_ws_bytes_lean)(_CODE[dt], N, B)
        ws = self._ws(nws)
        W, kzfac, vfinv, phase = self._c(W), self._c(kzfac), self._c(vfinv), self._c(phase)
        self.lib.check(self.lib.layer_smatrix(
            _CODE[dt], self._c(P).data_ptr() if P is not None else None, self._c(Q).data_ptr() if Q is not None else None,
            W.data_ptr(), kzfac.data_ptr(), vfinv.data_ptr(), phase.data_ptr(), int(use_q), N, B, S11.data_ptr(), S21.data_ptr(),
            V.data_ptr(), cp.data_ptr() if want_c else None, cm.data_ptr() if want_c else None, piv.data_ptr(), info.data_ptr(),
            ws.data_ptr(), nws, self.stream))
        self._info(info, "layer_smatrix")
        return S11, S21, V, cp, cm

    @_phase("Redheffer star products")
    def redheffer(self, Sm, Sn):
        """Star product of two S-matrices given as lists [S11,S21,S12,S22] of [B,n,n] (torcwa/rcwa.py:1283-1306).
        Returns (Sout list, X1, X2, Y1, Y2) with the four C-propagation factors."""
        Sm = [self._c(t) for t in Sm]
        Sn = [self._c(t) for t in Sn]
        B, n, _ = Sm[0].shape
        dt = Sm[0].dtype
        out = [torch.empty((B, n, n), dtype=dt, device=self.device) for _ in range(4)]
        XY = torch.empty((2, B, n, 2 * n), dtype=dt, device=self.device)
        piv, info = self._ints(B * n), self._ints(B)
        nws = self.lib.redheffer_ws_bytes(_CODE[dt], n, B)
        ws = self._ws(nws)
        arr = ctypes.c_void_p * 4
        pm, pn, po = arr(*[t.data_ptr() for t in Sm]), arr(*[t.data_ptr() for t in Sn]), arr(*[t.data_ptr() for t in out])
        self.lib.check(self.lib.redheffer(_CODE[dt], ctypes.addressof(pm), ctypes.addressof(pn), ctypes.addressof(po), XY.data_ptr(), n, B,
                                          piv.data_ptr(), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "redheffer")
        X, Y = XY[0], XY[1]
        return out, X[:, :, :n], X[:, :, n:], Y[:, :, :n], Y[:, :, n:]


    @_phase("Redheffer star products")
    def redheffer_halfspace(self, side, bd, S, want_xy=True):
        """Star product with a block-diagonal half-space S-matrix (side 0: Sin * S, side 1: S * Sout).
        bd: [4,4,B,N] diagonals (see include/trx.h).  want_xy=False (no coupling lists to propagate) lets side 0 use the
        cheaper right-solve algebra; the factor slots of the result are then None."""
        S = [self._c(t) for t in S]
        B, n, _ = S[0].shape
        N = n // 2
        dt = S[0].dtype
        bd = self._c(bd.to(dt))
        out = [torch.empty((B, n, n), dtype=dt, device=self.device) for _ in range(4)]
        lean = (int(side) == 0) and not want_xy
        XY = None if lean else torch.empty((2, B, n, 2 * n), dtype=dt, device=self.device)
        piv, info = self._ints(B * n), self._ints(B)
        nws = self.lib.redheffer_halfspace_ws_bytes(_CODE[dt], N, B, int(side), 0 if lean else 1)
        ws = self._ws(nws)
        arr = ctypes.c_void_p * 4
        ps, po = arr(*[t.data_ptr() for t in S]), arr(*[t.data_ptr() for t in out])
        self.lib.check(self.lib.redheffer_halfspace(_CODE[dt], int(side), bd.data_ptr(), ctypes.addressof(ps), ctypes.addressof(po),
                                                    None if lean else XY.data_ptr(), N, B, piv.data_ptr(), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "redheffer_halfspace")
        if lean:
            return out, None, None, None, None
        X, Y = XY[0], XY[1]
        return out, X[:, :, :n], X[:, :, n:], Y[:, :, :n], Y[:, :, n:]

    @_phase("Redheffer star products")
    def redheffer_halfspace_columns(self, side, bd, S, block, cols):
        """Columns `cols` (1 to 16 indices in [0, n), shared by the batch) of block `block` (0..3 = S11, S21, S12, S22) of the star product with
        a block-diagonal half-space S-matrix (side 0: Sin * S, side 1: S * Sout), as [B, n, len(cols)]: one LU of K and O(n^2) work instead
        of the four n x n blocks of `redheffer_halfspace` (include/trx.h: trx_redheffer_halfspace_columns)."""
        S = [self._c(t) for t in S]
        self._check(*S)
        B, n, _ = S[0].shape
        N = n // 2
        dt = S[0].dtype
        bd = self._c(bd.to(dt))
        cols = [int(c) for c in cols]
        m = len(cols)
        out = torch.empty((B, n, m), dtype=dt, device=self.device)
        piv, info = self._ints(B * n), self._ints(B)
        nws = self.lib.redheffer_halfspace_columns_ws_bytes(_CODE[dt], N, B, m)
        ws = self._ws(nws)
        ps = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in S])
        pc = (ctypes.c_int * max(m, 1))(*cols)
        self.lib.check(self.lib.redheffer_halfspace_columns(_CODE[dt], int(side), bd.data_ptr(), ctypes.addressof(ps), int(block), ctypes.addressof(pc), m,
                                                            out.data_ptr(), N, B, piv.data_ptr(), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "redheffer_halfspace_columns")
        return out

    # -- eigenproblem assembly (csrc/assembly.hip) --------------------------------------------------------
    def _build_pq(self, entry, *ops):
        """P, Q [B,2N,2N] from one of the trx_build_pq* entries; ops: its [B,N,N] matrices, then kx, ky [B,N], in the entry's order."""
        ops = [self._c(t) for t in ops]
        self._check(*ops)
        B, N, _ = ops[0].shape
        P = torch.empty((B, 2 * N, 2 * N), dtype=ops[0].dtype, device=self.device)
        Q = torch.empty_like(P)
        self.lib.check(entry(_CODE[P.dtype], *[t.data_ptr() for t in ops], N, B, P.data_ptr(), Q.data_ptr(), self.stream))
        return P, Q

    def _build_a(self, entry, ws_bytes, mats, mu, kx, ky):
        """A = P Q [B,2N,2N] for homogeneous mu [B] from one of the trx_build_a* entries (workspace: its ws_bytes); mats: its [B,N,N] matrices."""
        B, N, _ = mats[0].shape
        dt = mats[0].dtype
        A = torch.empty((B, 2 * N, 2 * N), dtype=dt, device=self.device)
        nws = ws_bytes(_CODE[dt], N, B)
        ws = self._ws(nws)
        ops = [self._c(t) for t in (*mats, mu.to(dt), kx, ky)]
        self._check(*ops)
        self.lib.check(entry(_CODE[dt], *[t.data_ptr() for t in ops], N, B, A.data_ptr(), ws.data_ptr(), nws, self.stream))
        return A

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_pq(self, E, Einv, M, Minv, kx, ky):
        """P, Q of torcwa/rcwa.py:1226-1232 (Laurent's rule; include/trx.h: trx_build_pq)."""
        return self._build_pq(self.lib.build_pq, E, Einv, M, Minv, kx, ky)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_a(self, E, Einv, mu, kx, ky):
        """A = P Q for homogeneous mu [B] via the block structure (two N^3 GEMMs)."""
        return self._build_a(self.lib.build_a, self.lib.build_a_ws_bytes, (E, Einv), mu, kx, ky)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_pq_aniso(self, Ex, Ey, Einv, Mx, My, Minv, kx, ky):
        """P, Q with per-component convolution matrices (Li's rule; include/trx.h: trx_build_pq_aniso)."""
        return self._build_pq(self.lib.build_pq_aniso, Ex, Ey, Einv, Mx, My, Minv, kx, ky)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_a_aniso(self, Ex, Ey, Einv, mu, kx, ky):
        """A = P Q for homogeneous mu [B] with per-component Ex, Ey (two N^3 GEMMs; include/trx.h: trx_build_a_aniso)."""
        return self._build_a(self.lib.build_a_aniso, self.lib.build_a_aniso_ws_bytes, (Ex, Ey, Einv), mu, kx, ky)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_pq_tensor(self, Exx, Exy, Eyy, Einv, M, Minv, kx, ky):
        """P, Q with the in-plane permittivity tensor (normal-vector rule; include/trx.h: trx_build_pq_tensor)."""
        return self._build_pq(self.lib.build_pq_tensor, Exx, Exy, Eyy, Einv, M, Minv, kx, ky)

    @_phase("assembly (convolution matrices, E^-1, A = PQ)")
    def build_a_tensor(self, Exx, Exy, Eyy, Einv, mu, kx, ky):
        """A = P Q for homogeneous mu [B] with the in-plane tensor (one N x 2N GEMM; include/trx.h: trx_build_a_tensor)."""
        return self._build_a(self.lib.build_a_tensor, self.lib.build_a_tensor_ws_bytes, (Exx, Exy, Eyy, Einv), mu, kx, ky)

    # -- power flux ------------------------------------------------------------------------------------
    @_phase("power flux (trx_matvec, trx_layer_flux)")
    def matvec(self, A, X):
        """Y[b] = A[b] X[b] for A [B,m,k] and a skinny X [B,k,c] or [k,c] (shared by the batch), 1 <= c <= 16 (include/trx.h: trx_matvec)."""
        A, X = self._c(A), self._c(X)
        self._check(A, X)
        B, m, k = A.shape
        shared = X.dim() == 2
        c = X.shape[-1]
        if X.shape[-2] != k or (not shared and X.shape[0] != B) or not (1 <= c <= 16):
            raise ValueError(f"matvec: A {list(A.shape)} against X {list(X.shape)} (X is [B,k,c] or [k,c] with 1 <= c <= 16)")
        Y = torch.empty((B, m, c), dtype=A.dtype, device=self.device)
        self.lib.check(self.lib.matvec(_CODE[A.dtype], A.data_ptr(), X.data_ptr(), 0 if shared else k * c, Y.data_ptr(), m, k, c, B, self.stream))
        return Y

    @_phase("power flux (trx_matvec, trx_layer_flux)")
    def layer_flux(self, W, V, cplus, cminus, kz, omega, d, z, *, z_is_fraction=False):
        """[B,nz] float64 un-normalised power flux through the planes z [B,nz] of a layer (include/trx.h: trx_layer_flux).  W, V [B,n,n];
        cplus, cminus, kz [B,n]; omega, d [B] real."""
        W, V, cplus, cminus, kz = (self._c(t) for t in (W, V, cplus, cminus, kz))
        self._check(W, V, cplus, cminus, kz)
        B, n, _ = W.shape
        f64 = lambda t: self._c(t.to(device=self.device, dtype=torch.float64))
        omega, d, z = f64(omega), f64(d), f64(z)
        nz = z.shape[1]
        if tuple(V.shape) != (B, n, n) or any(tuple(t.shape) != (B, n) for t in (cplus, cminus, kz)) or omega.shape != (B,) or d.shape != (B,) \
                or z.shape[0] != B or n % 2:
            raise ValueError("layer_flux: W, V [B,n,n]; cplus, cminus, kz [B,n]; omega, d [B]; z [B,nz]")
        flux = torch.empty((B, nz), dtype=torch.float64, device=self.device)
        nws = self.lib.layer_flux_ws_bytes(_CODE[W.dtype], n // 2, nz, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.layer_flux(_CODE[W.dtype], W.data_ptr(), V.data_ptr(), cplus.data_ptr(), cminus.data_ptr(), kz.data_ptr(),
                                           omega.data_ptr(), d.data_ptr(), z.data_ptr(), int(bool(z_is_fraction)), n // 2, nz, B, flux.data_ptr(),
                                           ws.data_ptr(), nws, self.stream))
        return flux

    # -- field maps -----------------------------------------------------------------------------------
    @_phase("field maps (trx_layer_field, trx_field_synth)")
    def layer_field(self, W, V, cplus, cminus, kz, omega, d, z, kx, ky, *, z_is_fraction=False):
        """[B,6,N,nz] Fourier coefficients (ex, ey, hx, hy, ky hx - kx hy, kx ey - ky ex) at the depths z [B,nz] of a layer (include/trx.h:
        trx_layer_field).  W, V [B,n,n]; cplus, cminus, kz [B,n]; omega, d [B] and kx, ky [B,N] real."""
        W, V, cplus, cminus, kz = (self._c(t) for t in (W, V, cplus, cminus, kz))
        self._check(W, V, cplus, cminus, kz)
        B, n, _ = W.shape
        f64 = lambda t: self._c(t.to(device=self.device, dtype=torch.float64))
        omega, d, z, kx, ky = f64(omega), f64(d), f64(z), f64(kx), f64(ky)
        if tuple(V.shape) != (B, n, n) or any(tuple(t.shape) != (B, n) for t in (cplus, cminus, kz)) or omega.shape != (B,) or d.shape != (B,) \
                or z.dim() != 2 or z.shape[0] != B or n % 2 or any(tuple(t.shape) != (B, n // 2) for t in (kx, ky)):
            raise ValueError("layer_field: W, V [B,n,n]; cplus, cminus, kz [B,n]; omega, d [B]; z [B,nz]; kx, ky [B,n/2]")
        nz = z.shape[1]
        out = torch.empty((B, 6, n // 2, nz), dtype=W.dtype, device=self.device)
        self.lib.check(self.lib.layer_field(_CODE[W.dtype], W.data_ptr(), V.data_ptr(), cplus.data_ptr(), cminus.data_ptr(), kz.data_ptr(),
                                            omega.data_ptr(), d.data_ptr(), z.data_ptr(), int(bool(z_is_fraction)), kx.data_ptr(), ky.data_ptr(),
                                            n // 2, nz, B, out.data_ptr(), self.stream))
        return out

    @_phase("field maps (trx_layer_field, trx_field_synth)")
    def field_synth(self, coef, kx, ky, omega, u, v):
        """[B,ncomp,nu,nv,T] = sum_m coef[B,ncomp,m,T] exp(i omega (kx_m u + ky_m v)) for coef [B,ncomp,N,T], kx, ky [B,N], omega [B], u [nu],
        v [nv] (real); nv = 1 or T = 1 (include/trx.h: trx_field_synth)."""
        coef = self._c(coef)
        self._check(coef)
        B, ncomp, N, T = coef.shape
        f64 = lambda t: self._c(t.to(device=self.device, dtype=torch.float64))
        kx, ky, omega, u, v = f64(kx), f64(ky), f64(omega), f64(u).reshape(-1), f64(v).reshape(-1)
        if tuple(kx.shape) != (B, N) or tuple(ky.shape) != (B, N) or omega.shape != (B,):
            raise ValueError("field_synth: coef [B,ncomp,N,T]; kx, ky [B,N]; omega [B]; u [nu]; v [nv]")
        nu, nv = u.shape[0], v.shape[0]
        out = torch.empty((B, ncomp, nu, nv, T), dtype=coef.dtype, device=self.device)
        self.lib.check(self.lib.field_synth(_CODE[coef.dtype], coef.data_ptr(), kx.data_ptr(), ky.data_ptr(), omega.data_ptr(), u.data_ptr(),
                                            v.data_ptr(), ncomp, N, T, nu, nv, B, out.data_ptr(), self.stream))
        return out

    # -- volume integrals ------------------------------------------------------------------------------
    @_phase("volume integrals (trx_modal_overlap)")
    def modal_overlap(self, M, cplus, cminus, kz, omega, d, zr, s, z_is_fraction=False):
        """[B,nr] complex128 sum_kl M_kl T_kl(z0, z1) over the ranges zr [B,nr,2] of a layer (include/trx.h: trx_modal_overlap).  M [B,n,n];
        cplus, cminus, kz [B,n]; omega, d [B] real; s = +1 / -1."""
        M, cplus, cminus, kz = (self._c(t) for t in (M, cplus, cminus, kz))
        self._check(M, cplus, cminus, kz)
        B, n, _ = M.shape
        f64 = lambda t: self._c(t.to(device=self.device, dtype=torch.float64))
        omega, d, zr = f64(omega), f64(d), f64(zr)
        if M.shape[2] != n or any(tuple(t.shape) != (B, n) for t in (cplus, cminus, kz)) or omega.shape != (B,) or d.shape != (B,) \
                or zr.dim() != 3 or zr.shape[0] != B or zr.shape[2] != 2:
            raise ValueError("modal_overlap: M [B,n,n]; cplus, cminus, kz [B,n]; omega, d [B]; zr [B,nr,2]")
        if int(s) not in (-1, 1):
            raise ValueError(f"modal_overlap: s must be +1 or -1, got {s!r}")
        nr = zr.shape[1]
        out = torch.empty((B, nr), dtype=torch.complex128, device=self.device)
        nws = self.lib.modal_overlap_ws_bytes(_CODE[M.dtype], n, nr, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.modal_overlap(_CODE[M.dtype], M.data_ptr(), cplus.data_ptr(), cminus.data_ptr(), kz.data_ptr(), omega.data_ptr(),
                                              d.data_ptr(), zr.data_ptr(), int(bool(z_is_fraction)), int(s), n, nr, B, out.data_ptr(), ws.data_ptr(),
                                              nws, self.stream))
        return out

    # -- thickness sweeps that reuse a layer's modes -----------------------------------------------------
    def _tk_operand(self, op, dt, B, n):
        """One side of a swept layer for the C ABI: None (nothing there: the identity), a [4,4,B,N] tensor of diagonals (block-diagonal S-matrix,
        as redheffer_halfspace takes it) or a list of four [B,n,n] tensors.  Returns (kind, pointer, objects to keep alive)."""
        if op is None:
            return 0, None, None
        if torch.is_tensor(op):
            bd = self._c(op.to(dt))
            if tuple(bd.shape) != (4, 4, B, n // 2):
                raise ValueError(f"thickness sweep: a block-diagonal operand must be [4, 4, {B}, {n // 2}], got {list(bd.shape)}")
            self._check(bd)
            return 1, bd.data_ptr(), bd
        S = [self._c(t) for t in op]
        self._check(*S)
        if len(S) != 4 or any(tuple(t.shape) != (B, n, n) or t.dtype != dt for t in S):
            raise ValueError(f"thickness sweep: a dense operand is four [{B}, {n}, {n}] tensors of dtype {dt}")
        arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in S])
        return 2, ctypes.addressof(arr), (S, arr)

    @_phase("thickness sweep: prepare (trx_thickness_prepare)")
    def thickness_prepare(self, W, V, vfinv, left, right, direction, cols):
        """The thickness-independent part of a thickness sweep of one layer (include/trx.h: trx_thickness_prepare).  W, V [B,n,n]: the layer's
        modes; vfinv [4,B,N]; left / right: everything on that side of the layer as one S-matrix (see _tk_operand); direction 0 = forward,
        1 = backward incidence; cols: 1 to 16 column indices in [0, n).  Returns the handle Engine.thickness_columns takes."""
        W, V, vfinv = self._c(W), self._c(V), self._c(vfinv)
        self._check(W, V, vfinv)
        B, n, _ = W.shape
        N = n // 2
        dt = W.dtype
        cols = [int(c) for c in cols]
        m = len(cols)
        if int(direction) not in (0, 1):
            raise ValueError(f"thickness_prepare: direction must be 0 (forward) or 1 (backward), got {direction!r}")
        lk, lp, lkeep = self._tk_operand(left, dt, B, n)
        rk, rp, rkeep = self._tk_operand(right, dt, B, n)
        rho = torch.empty((2, B, n, n), dtype=dt, device=self.device)
        src = torch.empty((2, B, n, max(m, 1)), dtype=dt, device=self.device)
        AB = torch.empty((2, B, n, n), dtype=dt, device=self.device)
        piv, info = self._ints(B * n), self._ints(2 * B)
        nws = self.lib.thickness_prepare_ws_bytes(_CODE[dt], N, B)
        ws = self._ws(nws)
        pc = (ctypes.c_int * max(m, 1))(*cols)
        self.lib.check(self.lib.thickness_prepare(_CODE[dt], W.data_ptr(), V.data_ptr(), vfinv.data_ptr(), lk, lp, rk, rp, int(direction),
                                                  ctypes.addressof(pc), m, N, B, rho[0].data_ptr(), rho[1].data_ptr(), src.data_ptr(), AB.data_ptr(),
                                                  piv.data_ptr(), info.data_ptr(), ws.data_ptr(), nws, self.stream))
        self._info(info, "thickness_prepare")
        return dict(rho=rho, src=src, AB=AB, direction=int(direction), m=m, B=B, N=N, dtype=dt, left=(lk, lp, lkeep), right=(rk, rp, rkeep))

    @_phase("thickness sweep: columns (trx_thickness_columns)")
    def thickness_columns(self, prep, phase, port, chunk=None):
        """[B, T, n, m]: for every thickness the columns (those of the prepare call) of the block of the whole stack's S-matrix that
        (direction, port) reads (include/trx.h: trx_thickness_columns).  phase [B, T, n] = exp(i omega kz d_t); port 0 = transmission,
        1 = reflection; chunk: thicknesses per library call (the workspace holds two n x n matrices per point and thickness; default: all T)."""
        B, N, m, dt = prep["B"], prep["N"], prep["m"], prep["dtype"]
        n = 2 * N
        phase = self._c(phase)
        self._check(prep["rho"], phase)
        if phase.dim() != 3 or phase.shape[0] != B or phase.shape[2] != n:
            raise ValueError(f"thickness_columns: phase must be [{B}, T, {n}], got {list(phase.shape)}")
        if int(port) not in (0, 1):
            raise ValueError(f"thickness_columns: port must be 0 (transmission) or 1 (reflection), got {port!r}")
        T = phase.shape[1]
        out = torch.empty((B, T, n, m), dtype=dt, device=self.device)
        info = self._ints(B * T)
        chunk = T if not chunk else max(1, min(int(chunk), T))
        if B > 0:
            chunk = max(1, min(chunk, 65535 // B))
        esz = phase.element_size()
        (lk, lp, _), (rk, rp, _) = prep["left"], prep["right"]
        rho, src, AB = prep["rho"], prep["src"], prep["AB"]
        for t0 in range(0, T, chunk):
            Tc = min(chunk, T - t0)
            nws = self.lib.thickness_columns_ws_bytes(_CODE[dt], N, B, Tc, m)
            ws = self._ws(nws)
            piv = self._ints(B * Tc * (n + 1))
            self.lib.check(self.lib.thickness_columns(_CODE[dt], rho[0].data_ptr(), rho[1].data_ptr(), src.data_ptr(), AB.data_ptr(),
                                                      phase.data_ptr() + t0 * n * esz, T, Tc, prep["direction"], int(port), lk, lp, rk, rp, m, N, B,
                                                      out.data_ptr() + t0 * n * m * esz, piv.data_ptr(), info.data_ptr() + 4 * t0, ws.data_ptr(), nws,
                                                      self.stream))
            del ws, piv
        self._info(info, "thickness_columns")
        return out

    def _tk_out_operand(self, op, direction, port, dt, B, n):
        """The output-side block O of a swept solve -- None, dense [B,n,n] or the four diagonals [4,B,N] of a block-diagonal one -- as the
        (left, right) operands of the C ABI: O sits in the block the forward reads (Rgt11, or Lft22), the other side is absent.  Returns
        ((lk, lp), (rk, rp), objects to keep alive)."""
        on_right = (int(direction) == 0) != (int(port) == 1)
        if op is None:
            return (0, None), (0, None), None
        op = self._c(op)
        self._check(op)
        if tuple(op.shape) == (B, n, n) and op.dtype == dt:
            arr = (ctypes.c_void_p * 4)(*[op.data_ptr()] * 4)
            side, keep = (2, ctypes.addressof(arr)), (op, arr)
        elif tuple(op.shape) == (4, B, n // 2) and op.dtype == dt:
            full = torch.zeros((4, 4, B, n // 2), dtype=dt, device=self.device)
            full[0 if on_right else 3] = op
            side, keep = (1, full.data_ptr()), full
        else:
            raise ValueError(f"thickness sweep: the output operator is [{B}, {n}, {n}] (dense) or [4, {B}, {n // 2}] (block diagonal) of dtype {dt}, "
                             f"got {list(op.shape)} {op.dtype}")
        return ((0, None), side, keep) if on_right else (side, (0, None), keep)

    def _tk_chunk(self, chunk, T, B):
        chunk = T if not chunk else max(1, min(int(chunk), T))
        return max(1, min(chunk, 65535 // B)) if B > 0 else chunk

    @_phase("thickness sweep: columns (trx_thickness_columns)")
    def thickness_columns_keep(self, rho, src, AB, phase, direction, port, op=None, chunk=None):
        """(out, cp), both [B, T, n, m]: thickness_columns from the prepare step's tensors -- rho [2,B,n,n], src [2,B,n,m], AB [2,B,n,n] -- and
        the output-side block `op` (see _tk_out_operand), together with the solved amplitude cp that thickness_columns_backward needs
        (include/trx.h: trx_thickness_columns_keep)."""
        rho, src, AB, phase = self._c(rho), self._c(src), self._c(AB), self._c(phase)
        self._check(rho, src, AB, phase)
        _, B, n, m = src.shape
        N, dt, T = n // 2, rho.dtype, phase.shape[1]
        if tuple(rho.shape) != (2, B, n, n) or tuple(AB.shape) != (2, B, n, n) or tuple(phase.shape) != (B, T, n):
            raise ValueError(f"thickness_columns_keep: rho and AB must be [2, {B}, {n}, {n}] and phase [{B}, T, {n}], got {list(rho.shape)}, "
                             f"{list(AB.shape)}, {list(phase.shape)}")
        (lk, lp), (rk, rp), keep = self._tk_out_operand(op, direction, port, dt, B, n)
        out = torch.empty((B, T, n, m), dtype=dt, device=self.device)
        cp = torch.empty((B, T, n, m), dtype=dt, device=self.device)
        info = self._ints(B * T)
        chunk = self._tk_chunk(chunk, T, B)
        esz = phase.element_size()
        for t0 in range(0, T, chunk):
            Tc = min(chunk, T - t0)
            nws = self.lib.thickness_columns_ws_bytes(_CODE[dt], N, B, Tc, m)
            ws = self._ws(nws)
            piv = self._ints(B * Tc * (n + 1))
            self.lib.check(self.lib.thickness_columns_keep(_CODE[dt], rho[0].data_ptr(), rho[1].data_ptr(), src.data_ptr(), AB.data_ptr(),
                                                           phase.data_ptr() + t0 * n * esz, T, Tc, int(direction), int(port), lk, lp, rk, rp, m, N, B,
                                                           out.data_ptr() + t0 * n * m * esz, cp.data_ptr() + t0 * n * m * esz, piv.data_ptr(),
                                                           info.data_ptr() + 4 * t0, ws.data_ptr(), nws, self.stream))
            del ws, piv
        self._info(info, "thickness_columns")
        return out, cp

    @_phase("thickness sweep: columns backward (trx_thickness_columns_backward)")
    def thickness_columns_backward(self, rho, AB, phase, cp, gout, direction, port, op=None, needs=(True,) * 5, chunk=None):
        """(grho [2,B,n,n], gsrc [2,B,n,m], gAB [2,B,n,n], gphase [B,T,n], gop like op): the adjoint of thickness_columns_keep for the incoming
        gradient gout [B,T,n,m] (include/trx.h: trx_thickness_columns_backward).  needs: which of the five are wanted; the others come back None
        and their work is skipped.  Chunked over T like the forward: the first chunk writes, the later ones accumulate."""
        rho, AB, phase, cp, gout = self._c(rho), self._c(AB), self._c(phase), self._c(cp), self._c(gout)
        self._check(rho, AB, phase, cp, gout)
        B, T, n, m = cp.shape
        N, dt = n // 2, rho.dtype
        if tuple(gout.shape) != (B, T, n, m) or tuple(phase.shape) != (B, T, n) or tuple(rho.shape) != (2, B, n, n) or tuple(AB.shape) != (2, B, n, n):
            raise ValueError(f"thickness_columns_backward: cp and gout must be [{B}, {T}, {n}, {m}], phase [{B}, {T}, {n}], rho and AB "
                             f"[2, {B}, {n}, {n}], got {list(gout.shape)}, {list(phase.shape)}, {list(rho.shape)}, {list(AB.shape)}")
        (lk, lp), (rk, rp), keep = self._tk_out_operand(op, direction, port, dt, B, n)
        new = lambda want, shape: torch.zeros(shape, dtype=dt, device=self.device) if want else None
        grho, gsrc, gAB, gphase = new(needs[0], (2, B, n, n)), new(needs[1], (2, B, n, m)), new(needs[2], (2, B, n, n)), new(needs[3], (B, T, n))
        gop = new(needs[4] and op is not None, tuple(op.shape) if op is not None else ())
        p = lambda t, off=0: None if t is None else t.data_ptr() + off
        info = self._ints(B * T)
        chunk = self._tk_chunk(chunk, T, B)
        esz = phase.element_size()
        for t0 in range(0, T, chunk):
            Tc = min(chunk, T - t0)
            nws = self.lib.thickness_columns_backward_ws_bytes(_CODE[dt], N, B, Tc, m)
            ws = self._ws(nws)
            piv = self._ints(B * Tc * (n + 1))
            self.lib.check(self.lib.thickness_columns_backward(_CODE[dt], rho[0].data_ptr(), rho[1].data_ptr(), AB.data_ptr(),
                                                               phase.data_ptr() + t0 * n * esz, T, Tc, int(direction), int(port), lk, lp, rk, rp, m, N, B,
                                                               cp.data_ptr() + t0 * n * m * esz, gout.data_ptr() + t0 * n * m * esz, p(grho),
                                                               p(grho, B * n * n * esz), p(gsrc), p(gAB), p(gphase, t0 * n * esz), p(gop), int(t0 > 0),
                                                               piv.data_ptr(), info.data_ptr() + 4 * t0, ws.data_ptr(), nws, self.stream))
            del ws, piv
        self._info(info, "thickness_columns_backward")
        return grho, gsrc, gAB, gphase, gop

    # -- mirror-symmetry folding ------------------------------------------------------------------------
    @_phase("symmetry fold (trx_sym_fold)")
    def sym_fold(self, A, plan):
        """Diagonal blocks of T^H A T for A [B,n,n] and a torcwa_amd.symmetry.SymPlan (include/trx.h: trx_sym_fold).  Returns (blocks, resid):
        blocks = one [g * B, s, s] tensor per group of plan.groups (views of one packed buffer; block-major, then batch), resid [B] float64 = the
        largest discarded entry relative to max |A|.  A is not modified."""
        A = self._c(A)
        self._check(A)
        B, n, _ = A.shape
        if n != plan.n:
            raise ValueError(f"sym_fold: A is {n} x {n}, the plan is for n = {plan.n}")
        dt = A.dtype
        idx, wt, off = plan.device(self.device, dt)
        packed = torch.empty(B * sum(s * s for s in plan.sizes), dtype=dt, device=self.device)
        resid = torch.empty(B, dtype=torch.float64, device=self.device)
        nws = self.lib.sym_fold_ws_bytes(_CODE[dt], n, B)
        ws = self._ws(nws)
        self.lib.check(self.lib.sym_fold(_CODE[dt], A.data_ptr(), n, B, idx.data_ptr(), wt.data_ptr(), off.data_ptr(), plan.nblk, packed.data_ptr(),
                                         resid.data_ptr(), ws.data_ptr(), nws, self.stream))
        blocks, at = [], 0
        for s, ks in plan.groups:
            cnt = len(ks) * B * s * s
            blocks.append(packed[at:at + cnt].view(len(ks) * B, s, s))
            at += cnt
        return blocks, resid

    def sym_packed(self, plan, B, dtype):
        """Empty packed buffers for the eigenpairs of the blocks of B matrices: (Wp, lp, Wk, lamk) -- the flat buffers trx_sym_unfold reads and
        their per-group views ([g * B, s, s], [g * B, s]) in the order of plan.groups, to be filled in place (eig(..., out=(lamk[i], Wk[i])))."""
        Wp = torch.empty(B * sum(s * s for s in plan.sizes), dtype=dtype, device=self.device)
        lp = torch.empty(B * plan.n, dtype=dtype, device=self.device)
        Wk, lamk, a2, a1 = [], [], 0, 0
        for s, ks in plan.groups:
            g = len(ks) * B
            Wk.append(Wp[a2:a2 + g * s * s].view(g, s, s))
            lamk.append(lp[a1:a1 + g * s].view(g, s))
            a2, a1 = a2 + g * s * s, a1 + g * s
        return Wp, lp, Wk, lamk

    @_phase("symmetry unfold (trx_sym_unfold)")
    def sym_unfold(self, Wk, lamk, plan):
        """(lam [B,n], W [B,n,n]) in the original basis from the eigenvectors and eigenvalues of the blocks (include/trx.h: trx_sym_unfold):
        W[:, block k] = T_k W_k.  Wk, lamk: the flat packed buffers of sym_packed (read in place, no copy), or lists with one [g * B, s, s] /
        [g * B, s] tensor per group of plan.groups (packed here: one extra copy of sum_k n_k^2 elements)."""
        n = plan.n
        if torch.is_tensor(Wk):
            self._check(Wk, lamk)
            dt = Wk.dtype
            B = lamk.numel() // n
            if Wk.dim() != 1 or lamk.dim() != 1 or lamk.numel() != B * n or Wk.numel() != B * sum(s * s for s in plan.sizes):
                raise ValueError("sym_unfold: packed Wk / lamk must be the flat buffers of sym_packed")
            Wp, lp = self._c(Wk), self._c(lamk)
        else:
            self._check(*Wk, *lamk)
            dt = Wk[0].dtype
            B = Wk[0].shape[0] // len(plan.groups[0][1])
            for (s, ks), w, l in zip(plan.groups, Wk, lamk):
                if tuple(w.shape) != (len(ks) * B, s, s) or tuple(l.shape) != (len(ks) * B, s):
                    raise ValueError(f"sym_unfold: group of {len(ks)} blocks of size {s} needs [{len(ks) * B}, {s}, {s}] and [{len(ks) * B}, {s}], "
                                     f"got {list(w.shape)} and {list(l.shape)}")
            Wp = torch.cat([w.reshape(-1) for w in Wk])
            lp = torch.cat([l.reshape(-1) for l in lamk])
        idx, wt, off = plan.device(self.device, dt)
        W = torch.empty((B, n, n), dtype=dt, device=self.device)
        lam = torch.empty((B, n), dtype=dt, device=self.device)
        self.lib.check(self.lib.sym_unfold(_CODE[dt], Wp.data_ptr(), lp.data_ptr(), n, B, idx.data_ptr(), wt.data_ptr(), off.data_ptr(), plan.nblk,
                                           W.data_ptr(), lam.data_ptr(), self.stream))
        return lam, W

    @_phase("symmetry fold backward (trx_sym_fold_backward)")
    def sym_fold_backward(self, gblocks, plan):
        """gA [B,n,n] = sum_k T_k gB_k T_k^H (include/trx.h: trx_sym_fold_backward), the adjoint of sym_fold.  gblocks: the flat packed buffer,
        or a list with one [g * B, s, s] tensor per group of plan.groups (packed here)."""
        n = plan.n
        if torch.is_tensor(gblocks):
            self._check(gblocks)
            Gp = self._c(gblocks)
            if Gp.dim() != 1:
                raise ValueError("sym_fold_backward: a packed gblocks must be the flat buffer")
        else:
            self._check(*gblocks)
            for (s, ks), g in zip(plan.groups, gblocks):
                if g.dim() != 3 or tuple(g.shape[1:]) != (s, s) or g.shape[0] % len(ks):
                    raise ValueError(f"sym_fold_backward: group of {len(ks)} blocks of size {s} needs [{len(ks)} B, {s}, {s}], got {list(g.shape)}")
            Gp = torch.cat([g.reshape(-1) for g in gblocks])
        tot = sum(s * s for s in plan.sizes)
        B = Gp.numel() // tot
        if Gp.numel() != B * tot:
            raise ValueError(f"sym_fold_backward: {Gp.numel()} elements are no multiple of the plan's {tot} per matrix")
        dt = Gp.dtype
        _, _, off = plan.device(self.device, dt)
        ridx, rwt = plan.rows(self.device, dt)
        gA = torch.empty((B, n, n), dtype=dt, device=self.device)
        self.lib.check(self.lib.sym_fold_backward(_CODE[dt], Gp.data_ptr(), n, B, ridx.data_ptr(), rwt.data_ptr(), off.data_ptr(), plan.nblk,
                                                  gA.data_ptr(), self.stream))
        return gA

    @_phase("symmetry unfold backward (trx_sym_unfold_backward)")
    def sym_unfold_backward(self, gW, glam, plan):
        """(gWk, glamk): the adjoint of sym_unfold (include/trx.h: trx_sym_unfold_backward), gW_k = T_k^H gW[:, block k] and the slices of glam,
        as lists with one [g * B, s, s] / [g * B, s] tensor per group of plan.groups (views of two packed buffers)."""
        gW, glam = self._c(gW), self._c(glam)
        self._check(gW, glam)
        B, n, _ = gW.shape
        if n != plan.n or tuple(glam.shape) != (B, n):
            raise ValueError(f"sym_unfold_backward: gW {list(gW.shape)} / glam {list(glam.shape)} do not fit the plan's n = {plan.n}")
        dt = gW.dtype
        idx, wt, off = plan.device(self.device, dt)
        Wp, lp, Wk, lamk = self.sym_packed(plan, B, dt)
        self.lib.check(self.lib.sym_unfold_backward(_CODE[dt], gW.data_ptr(), glam.data_ptr(), n, B, idx.data_ptr(), wt.data_ptr(), off.data_ptr(),
                                                    plan.nblk, Wp.data_ptr(), lp.data_ptr(), self.stream))
        return Wk, lamk

    # -- sector folds ------------------------------------------------------------------------------------
    @_phase("symmetry sector fold (trx_sym_fold_pair)")
    def sym_fold_pair(self, M, plan, kl, kr):
        """[B, n_kl, n_kr] = T_kl^H M T_kr for M [B,n,n] and one pair of blocks of a SymPlan (include/trx.h: trx_sym_fold_pair).  M is not
        modified and need not commute with the mirrors."""
        M = self._c(M)
        self._check(M)
        B, n, _ = M.shape
        if n != plan.n or M.shape[2] != n:
            raise ValueError(f"sym_fold_pair: M is {list(M.shape[1:])}, the plan is for n = {plan.n}")
        kl, kr = self._pair(plan, kl, kr)
        dt = M.dtype
        idx, wt, off = plan.device(self.device, dt)
        out = torch.empty((B, plan.sizes[kl], plan.sizes[kr]), dtype=dt, device=self.device)
        self.lib.check(self.lib.sym_fold_pair(_CODE[dt], M.data_ptr(), n, B, idx.data_ptr(), wt.data_ptr(), off.data_ptr(), plan.nblk, kl, kr,
                                              out.data_ptr(), self.stream))
        return out

    @_phase("symmetry sector fold (trx_sym_fold_pair)")
    def sym_fold_pair_bd(self, bd, plan, kl, kr):
        """sym_fold_pair of a 2x2-block-diagonal operator given as its four diagonals bd [4,B,N] (BlockDiag2.d stacked): the dense
        [B, n_kl, n_kr] block (include/trx.h: trx_sym_fold_pair_bd)."""
        bd = self._c(bd)
        self._check(bd)
        if bd.dim() != 3 or bd.shape[0] != 4 or 2 * bd.shape[2] != plan.n:
            raise ValueError(f"sym_fold_pair_bd: bd must be [4, B, {plan.n // 2}], got {list(bd.shape)}")
        _, B, N = bd.shape
        kl, kr = self._pair(plan, kl, kr)
        dt = bd.dtype
        idx, wt, off = plan.device(self.device, dt)
        out = torch.empty((B, plan.sizes[kl], plan.sizes[kr]), dtype=dt, device=self.device)
        self.lib.check(self.lib.sym_fold_pair_bd(_CODE[dt], bd.data_ptr(), N, B, idx.data_ptr(), wt.data_ptr(), off.data_ptr(), plan.nblk, kl, kr,
                                                 out.data_ptr(), self.stream))
        return out

    @_phase("symmetry sector fold backward (trx_sym_fold_pairs_backward)")
    def sym_fold_pairs_backward(self, grads, plan, pairs, B=None, dtype=None):
        """gM [B,n,n] = sum_p T_kl_p G_p T_kr_p^H (include/trx.h: trx_sym_fold_pairs_backward), the adjoint of sym_fold_pair over the list
        `pairs` of (kl, kr), at most 16.  grads: one [B, n_kl, n_kr] tensor or None per pair; None is a pair without a gradient.  B, dtype: needed
        only when every gradient is None (the result is then all zeros)."""
        pairs = [self._pair(plan, kl, kr) for kl, kr in pairs]
        if len(grads) != len(pairs) or len(pairs) > 16:
            raise ValueError(f"sym_fold_pairs_backward: {len(grads)} gradients for {len(pairs)} pairs (at most 16)")
        live = [self._c(g) if g is not None else None for g in grads]
        first = next((g for g in live if g is not None), None)
        if first is not None:
            self._check(*[g for g in live if g is not None])
            B, dtype = first.shape[0], first.dtype
        if B is None or dtype is None:
            raise ValueError("sym_fold_pairs_backward: every gradient is None: give B and dtype")
        for g, (kl, kr) in zip(live, pairs):
            if g is not None and (tuple(g.shape) != (B, plan.sizes[kl], plan.sizes[kr]) or g.dtype != dtype):
                raise ValueError(f"sym_fold_pairs_backward: the gradient of pair ({kl}, {kr}) must be [{B}, {plan.sizes[kl]}, {plan.sizes[kr]}] "
                                 f"{dtype}, got {list(g.shape)} {g.dtype}")
        n, m = plan.n, len(pairs)
        _, _, off = plan.device(self.device, dtype)
        ridx, rwt = plan.rows(self.device, dtype)
        gM = torch.empty((B, n, n), dtype=dtype, device=self.device)
        pg = (ctypes.c_void_p * max(m, 1))(*[g.data_ptr() if g is not None and g.numel() else None for g in live])
        pl = (ctypes.c_int * max(m, 1))(*[p[0] for p in pairs])
        pr = (ctypes.c_int * max(m, 1))(*[p[1] for p in pairs])
        self.lib.check(self.lib.sym_fold_pairs_backward(_CODE[dtype], ctypes.addressof(pg), ctypes.addressof(pl), ctypes.addressof(pr), m, n, B,
                                                        ridx.data_ptr(), rwt.data_ptr(), off.data_ptr(), plan.nblk, gM.data_ptr(), self.stream))
        return gM

    @_phase("symmetry sector fold backward (trx_sym_fold_pair_bd_backward)")
    def sym_fold_pair_bd_backward(self, G, plan, kl, kr):
        """gbd [4,B,N]: the four diagonals of T_kl G T_kr^H for G [B, n_kl, n_kr] (include/trx.h: trx_sym_fold_pair_bd_backward), the adjoint of
        sym_fold_pair_bd."""
        G = self._c(G)
        self._check(G)
        kl, kr = self._pair(plan, kl, kr)
        if G.dim() != 3 or tuple(G.shape[1:]) != (plan.sizes[kl], plan.sizes[kr]):
            raise ValueError(f"sym_fold_pair_bd_backward: G must be [B, {plan.sizes[kl]}, {plan.sizes[kr]}], got {list(G.shape)}")
        B, N, dt = G.shape[0], plan.n // 2, G.dtype
        if G.numel() == 0:                                                             # an empty block reaches no diagonal entry
            return torch.zeros((4, B, N), dtype=dt, device=self.device)
        _, _, off = plan.device(self.device, dt)
        ridx, rwt = plan.rows(self.device, dt)
        gbd = torch.empty((4, B, N), dtype=dt, device=self.device)
        self.lib.check(self.lib.sym_fold_pair_bd_backward(_CODE[dt], G.data_ptr(), N, B, ridx.data_ptr(), rwt.data_ptr(), off.data_ptr(), plan.nblk,
                                                          kl, kr, gbd.data_ptr(), self.stream))
        return gbd

    @staticmethod
    def _pair(plan, kl, kr):
        kl, kr = int(kl), int(kr)
        if not (0 <= kl < plan.nblk and 0 <= kr < plan.nblk):
            raise ValueError(f"blocks ({kl}, {kr}) outside the plan's {plan.nblk}")
        return kl, kr


_default = None


def default_engine():
    global _default
    if _default is None:
        _default = Engine()
    return _default
