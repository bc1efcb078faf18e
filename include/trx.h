/* libtrx -- C ABI of the MI355X-native RCWA layer-solve hot path.
 *
 * The reference (kch3782/torcwa 0.1.4.2) has no FFI of its own: the hot path is a chain of torch.* calls inside
 * torcwa/rcwa.py and the single-op seam torcwa/torch_eig.py (`Eig.apply`, used at rcwa.py:1236).  This header is
 * the boundary a maintainer would bind those call sites to (see INTEGRATION.md for the ctypes stub).  Every entry
 * point cites the reference lines it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / HIP types.  `stream` is a hipStream_t passed as void*.
 *  - All matrices are row-major, interleaved complex (re,im), layout-identical to torch.complex64 / complex128;
 *    batched tensors are [batch, rows, cols] contiguous unless a leading dimension / stride is given.
 *  - All pointers are DEVICE pointers (HBM).  The library never allocates device memory and is stream-ordered and
 *    re-entrant: the caller owns every buffer including the workspace, whose size is returned by the matching
 *    *_ws_bytes() function.  Every entry point is asynchronous EXCEPT trx_eig, whose QR iteration is convergence-driven:
 *    per outer iteration (about n / 16 of them per sub-batch) the host reads a 12-byte progress summary from pinned memory, one
 *    iteration after it was produced, and for batch >= 8 it runs the QR phase of 2-4 sub-batches on internal non-blocking streams
 *    (forked from and joined back into `stream` with events) so that their latency-bound steps overlap; on the mixed-precision route it
 *    also reads the per-matrix flag words after the refinement.  Those streams and events come from
 *    a process-wide pool created on first use (nothing is created or destroyed per call), and no environment variable is read per call.
 *  - Return value: 0 = ok, <0 = TRX_ERR_* (bad argument / launch failure).  Numerical failures (singular pivot,
 *    eigensolver non-convergence) are reported LAPACK-style in the device-resident `info[batch]` array.
 */
#ifndef TRX_H_
#define TRX_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { TRX_C64 = 0, TRX_C128 = 1 };          /* dtype */
enum { TRX_OP_N = 0, TRX_OP_T = 1, TRX_OP_C = 2 };
enum {
    TRX_OK = 0,
    TRX_ERR_DTYPE = -1,
    TRX_ERR_ARG = -2,
    TRX_ERR_WORKSPACE = -3,
    TRX_ERR_LAUNCH = -4,
    TRX_ERR_UNSUPPORTED = -5
};

int trx_version(void);                        /* major*10000 + minor*100 + patch */
const char* trx_strerror(int code);

/* ---- Fourier factorisation: torcwa/rcwa.py:1183-1204 (`_material_conv`: fft2 -> Toeplitz gather) --------------
 * out[b,i,j] = c[b, (m_i-m_j) mod nx, (n_i-n_j) mod ny],  c = DFT2(grid[b]) / (nx*ny),
 * i = (m+ox)*(2*oy+1) + (n+oy).  Only the (4ox+1)(4oy+1) needed coefficients are computed (pruned DFT).
 * grid: [batch, nx, ny] real (grid_is_complex=0) or complex, in the real/complex type of `dtype`.
 * Requires nx > 2*ox and ny > 2*oy (same as the reference's negative-index wrap). */
size_t trx_convmat_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy);
int trx_convmat(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy,
                void* out, void* ws, size_t ws_bytes, void* stream);

/* ---- Fourier factorisation for an arbitrary order set (oblique lattices, circular truncation; no reference counterpart) ---------------
 * out[b,i,j] = c[b, m_i-m_j, n_i-n_j],  c = DFT2(grid[b]) / (n1*n2),  (m_i, n_i) = mn[i]: a device int32 [N,2] list of harmonic indices in
 * the lattice basis (grid axis 0 along a1, axis 1 along a2), in the caller's order.  The coefficients are those of trx_convmat over the box
 * |p| <= 2 mmax, |q| <= 2 nmax (same pruned fp64 DFT), so mn = the x-major rectangle of (ox, oy) with mmax = ox, nmax = oy gives trx_convmat's
 * output bit for bit.  Requires n1 > 2*mmax, n2 > 2*nmax and |m_i| <= mmax, |n_i| <= nmax (else TRX_ERR_ARG; the list is checked on the host,
 * one synchronisation of `stream`); max(n1, n2) <= 2048 as trx_convmat. */
size_t trx_convmat_orders_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax);
int trx_convmat_orders(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax, int nmax,
                       void* out, void* ws, size_t ws_bytes, void* stream);

/* ---- Fourier factorisation, Li's inverse rule (no reference counterpart: the reference has Laurent's rule only) ---------------------
 * L. Li, JOSA A 13, 1870 (1996); 14, 2758 (1997).  For each grid[b] ([nx, ny], layout and index map as trx_convmat):
 *   Ex[(m,n),(m',n')] = F[m,m',n-n'],  F[m,m',q] = (1/ny) sum_y Uy[y][m,m'] e^{-2 pi i q y/ny},  Uy[y] = Toeplitz_x(1/grid[:,y])^-1
 *   Ey[(m,n),(m',n')] = G[n,n',m-m'],  G[n,n',p] = (1/nx) sum_x Ux[x][n,n'] e^{-2 pi i p x/nx},  Ux[x] = Toeplitz_y(1/grid[x,:])^-1
 * where Toeplitz_x(f)[m,m'] = fhat[m-m'] of the 1-D DFT along x divided by nx ((2ox+1)^2), Toeplitz_y likewise ((2oy+1)^2).  Ex multiplies the
 * x component of E (inverse rule across the x discontinuities), Ey the y component.  Ex, Ey: [batch,N,N] outputs in `dtype`.
 * Ux [batch,nx,2oy+1,2oy+1], Uy [batch,ny,2ox+1,2ox+1]: optional complex128 outputs of the small inverses (NULL: not kept; the adjoint needs
 * them).  info[batch] (device): 0 ok, 1 a grid value is zero (it stays 1 although the block of that row then fails too), 2 a Toeplitz block
 * is singular.  All arithmetic is fp64 for both dtypes and in the same order: a complex64 call returns the complex128 result, rounded once.
 * Requires nx > 2ox, ny > 2oy and max(nx, ny) <= 2048 (as trx_convmat); 2*max(ox,oy)+1 <= 99, i.e. max(ox,oy) <= 49 (one Toeplitz block of
 * (2o+1)^2 complex128 elements is held in the LDS of one CU, 160 KiB on gfx950), else TRX_ERR_UNSUPPORTED.  The workspace holds the pruned
 * DFTs of 1/grid, the per-direction transforms and, unless Ux / Uy are given, the inverses of a chunk of rows no larger than one complex64 output
 * (the same chunk for both dtypes). */
size_t trx_convmat_li_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy);
int trx_convmat_li(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy, void* Ex, void* Ey,
                   void* Ux, void* Uy, int* info, void* ws, size_t ws_bytes, void* stream);

/* Li's rule for a list of axis-aligned rectangles in closed form (no grid): kind, voff, S, par, npar as trx_convmat_shapes, every shape a
 * rectangle (Wx, Wy, Cx, Cy, theta = 0) on the rectangular cell Lx x Ly with the order box (ox, oy) of trx_convmat_li.  rval [batch, S+1]
 * complex128: rval[b,0] = 1/eps_background, rval[b,s+1] = 1/eps_s - 1/eps_host, so 1/eps = rval_0 + sum_s rval_s chi_s (nesting needs
 * nothing further; other overlap is the caller's error).  1/eps is piecewise constant along y: between 0 and the y-edges of the rectangles,
 * reduced into the cell and sorted, lie K = 2S + 1 strips [t_k, t_k+1] of height h_k and midpoint y_k, and
 *   a_k[p] = rval_0 delta_p0 + sum_{s active in k} rval_s (Wx_s/Lx) sinc(pi p Wx_s/Lx) e^{-2 pi i p Cx_s/Lx},  Uy[k] = Toeplitz(a_k)^-1,
 *   w_k[q] = (h_k/Ly) sinc(pi q h_k/Ly) e^{-2 pi i q y_k/Ly},   F[m,m',q] = sum_k Uy[k][m,m'] w_k[q],   Ex[(m,n),(m',n')] = F[m,m',n-n'];
 * Ey is the mirror image (vertical strips between the x-edges, Ux[k] of size (2oy+1)^2, G[n,n',p]).  The strips stand where the grid rows of
 * trx_convmat_li stand and the weights where its twiddles stand: the inverses, the transform and the scatter are its kernels.
 * Strip states come from the events: per rectangle lo = (C - W/2) reduced into [0, L), hi = lo + W; hi <= L: it opens at lo and closes at hi
 * (an edge exactly on the cell boundary stays at L); hi > L: it is active at 0+, closes at hi - L and opens at lo.  Events sort by position,
 * ties by index (0 the origin, 1 + 2s open, 2 + 2s close); s is active in strip k iff [rank(open) <= k] xor [rank(close) <= k] xor wraps.
 * A strip of zero height has weight 0 and the state of the one-sided limit.
 * Outputs: Ex, Ey [batch,N,N] in `dtype`; optional Ux [batch,K,2oy+1,2oy+1], Uy [batch,K,2ox+1,2ox+1] complex128 (NULL: not kept); optional
 * strip record for the adjoint: brk [batch,2,K+1] fp64 (direction 0: the y-breakpoints t_0 = 0 .. t_K = Ly, direction 1: the x-breakpoints)
 * and rec [batch,2,3S] int32 (per rectangle: rank of its open event, rank of its close event, wraps).  info[batch] (device): 0 ok; 1 an
 * rval entry is not finite or rval[b,0] is zero; 2 a Toeplitz block is singular; 3 a
 * rectangle has theta != 0, a width that is not positive or exceeds the cell, or a centre that is not finite.  All arithmetic is fp64 for both
 * dtypes: a complex64 call returns the complex128 result rounded once.  One workgroup per (point, direction) stages the list in LDS,
 * rank-sorts the events (each thread counts what sorts before its own: no data-dependent loop), and writes a_k and w_k summing the active
 * rectangles in ascending s.  Latency-bound and tiny: K batch Toeplitz blocks where the grid path has (nx + ny) batch.
 * NOT detected: a rectangle whose medium has 1/eps = 0 (rval_0 + the rval of the rectangle and of its hosts sums to zero, e.g. eps = inf).  The
 * entry sees sums of rval only and does not know a rectangle's host; above order 0 the Toeplitz block of a function that vanishes on part of
 * the period is non-singular, so such a layer returns finite numbers with info 0.  The caller keeps eps finite (BatchedRCWA refuses it).
 * TRX_ERR_ARG: a kind that is not a rectangle (and the list errors of trx_convmat_shapes), Lx or Ly not positive, batch > 65535;
 * TRX_ERR_UNSUPPORTED: S > 127 (K = 255: one workgroup sorts a point's events), 2*max(ox,oy)+1 > 99 as trx_convmat_li.
 *
 * trx_convmat_li_shapes_backward: the adjoint of the strip tables, in PyTorch's convention as trx_convmat_shapes_backward.  ga_x [batch,K,4ox+1]
 * and gw_y [batch,K,4oy+1]: the adjoints of a_k and w_k of direction 0; ga_y [batch,K,4oy+1], gw_x [batch,K,4ox+1]: of direction 1 (all
 * complex128).  gpar [batch,npar] fp64 (theta slots and unowned slots 0), grval [batch,S+1] complex128.  d w_(r-1) / d t_r = -d w_r / d t_r =
 * e^{-2 pi i q t_r/L} / L at the breakpoint of rank r; d t / d C = 1, d t / d W = -+1/2 for the lower / upper edge; d a_k[p] / d Wx = rval_s
 * cos(pi p Wx/Lx) e^{..} / Lx, d a_k[p] / d Cx = (-2 pi i p/Lx) term.  One workgroup of 256 threads per (point, parameter) and per (point,
 * value); each thread sums its terms in ascending order, then a fixed tree: no atomics, bit-identical on repetition. */
size_t trx_convmat_li_shapes_ws_bytes(int dtype, int batch, int S, int ox, int oy);
int trx_convmat_li_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* rval, double Lx, double Ly,
                          int batch, int ox, int oy, void* Ex, void* Ey, void* Ux, void* Uy, double* brk, int* rec, int* info, void* ws,
                          size_t ws_bytes, void* stream);
int trx_convmat_li_shapes_backward(const int* kind, const int* voff, int S, const double* par, int npar, const void* rval, double Lx, double Ly,
                                   int batch, int ox, int oy, const double* brk, const int* rec, const void* ga_x, const void* gw_y,
                                   const void* ga_y, const void* gw_x, double* gpar, void* grval, void* stream);

/* ---- Fourier factorisation, normal-vector method (no reference counterpart) -----------------------------------------------------------
 * Schuster et al., JOSA A 24, 2880 (2007); Goetz et al., Opt. Express 16, 17295 (2008).  For each grid[b] ([nx, ny], layout and index map as
 * trx_convmat) and an in-plane unit field N normal to the material interfaces:
 *   D = [eps] - [1/eps]^-1,   Exx = [eps] - {D, [Nx Nx]},   Exy (= Eyx) = -{D, [Nx Ny]},   Eyy = [eps] - {D, [Ny Ny]}
 * ([f]: the Laurent convolution matrix of trx_convmat; {D, C} = (D C + C D)/2, the symmetrised product, which keeps the tensor Hermitian
 * for a lossless grid -- with the plain product D C a lossless layer does not conserve energy at finite order).  Exx, Exy, Eyy: [batch,N,N] outputs in `dtype`; E_z keeps Laurent's [eps].
 *
 * trx_normal_field: the products nn[b] = (Nx^2, Nx Ny, Ny^2) ([batch,3,nx,ny] fp64) of the field derived from the grid.  J = Re(grad g grad g^H)
 * from periodic central differences with grid spacings hx, hy (only their ratio matters: pass Lx/nx, Ly/ny), blurred along y and then x by
 * the periodic Gaussian w[k] = exp(-k^2/(2 sigma^2)) / sum_k, |k| <= ceil(3 sigma) cells (sigma = 0: no blur); N = principal eigenvector of
 * the blurred J:  with d = Jxx - Jyy, o = 2 Jxy, r = hypot(d, o):  Nx^2 = (1 + d/r)/2, Nx Ny = o/(2r), Ny^2 = (1 - d/r)/2 where
 * r > 1e-3 (Jxx + Jyy) (a unit field); elsewhere 0, i.e. Laurent's rule.  grid in the real / complex type of `dtype`; 0 <= sigma <= 256,
 * nx, ny <= 2048, else TRX_ERR_UNSUPPORTED.
 * trx_convmat_nv: the tensor.  nn: optional [batch,3,nx,ny] fp64 product grids supplied by the caller (an analytic field); NULL = derive them
 * from the grid (sigma, hx, hy as trx_normal_field; ignored otherwise).  info[batch] (device): 0 ok, 1 a grid value is zero, 2 [1/eps] is
 * singular.  All arithmetic is fp64 for both dtypes ([1/eps]^-1 by trx_inverse in complex128).  Requires nx > 2ox, ny > 2oy, max(nx, ny) <= 2048. */
size_t trx_normal_field_ws_bytes(int dtype, int batch, int nx, int ny);
int trx_normal_field(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, double sigma, double hx, double hy, double* nn,
                     void* ws, size_t ws_bytes, void* stream);
size_t trx_convmat_nv_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy);
int trx_convmat_nv(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy, double sigma, double hx, double hy,
                   const double* nn, void* Exx, void* Exy, void* Eyy, int* info, void* ws, size_t ws_bytes, void* stream);
/* On an oblique lattice with an arbitrary order set.  h: HOST double[4], the row-major cell matrix whose rows are a1/n1 and a2/n2 (grid axis 0
 * along a1, axis 1 along a2).  The physical gradient is h^-1 (du g, dv g) of the periodic central differences du, dv in index units; the blur
 * stays in index space (on a skewed cell it is anisotropic in physical units).  A diagonal h with positive entries is trx_normal_field with
 * hx = h[0], hy = h[3], bit for bit.  trx_normal_field_lattice takes the workspace of trx_normal_field_ws_bytes.
 * trx_convmat_nv_orders: trx_convmat_nv with the [eps], [1/eps] and product matrices of trx_convmat_orders (mn, N, mmax, nmax as there) and
 * the field of trx_normal_field_lattice (h is ignored when nn is given).  Same outputs, info and arithmetic; N x N outputs. */
int trx_normal_field_lattice(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, double sigma, const double* h, double* nn,
                             void* ws, size_t ws_bytes, void* stream);
size_t trx_convmat_nv_orders_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax);
int trx_convmat_nv_orders(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax, int nmax,
                          double sigma, const double* h, const double* nn, void* Exx, void* Exy, void* Eyy, int* info, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- Fourier factorisation of vector shapes in closed form (no reference counterpart; what S4 and other design codes offer) ----------------------
 * eps(r) = sum_G c(G) e^{+iG.r}, G = p b1 + q b2, b_i . a_j = 2 pi delta_ij, r in the coordinates of the field axes (origin at the cell corner):
 *   c(G) = val[b,0] delta_G0 + sum_s val[b,s+1] chi_s(G),   chi_s(G) = (1 / cell_area) int_shape e^{-iG.r} d2r
 * val[b,0] is the background and val[b,s+1] the contrast of shape s against the medium it sits in ([batch, S+1] complex128).
 *   kind 0, ellipse   (Rx, Ry, Cx, Cy, theta): chi = (pi Rx Ry / A) 2 J1(rho) / rho e^{-iG.c}, rho = hypot(Rx G'x, Ry G'y), 1 at rho = 0
 *   kind 1, rectangle (Wx, Wy, Cx, Cy, theta): chi = (Wx Wy / A) sinc(G'x Wx / 2) sinc(G'y Wy / 2) e^{-iG.c}, sinc t = sin t / t
 *   kind 2, simple polygon (x0, y0, ... x_{K-1}, y_{K-1}, counter-clockwise; a clockwise list gives the negative), e_k = v_{k+1} - v_k, m_k the midpoint:
 *           chi = (i / (A |G|^2)) sum_k (Gx e_ky - Gy e_kx) e^{-iG.m_k} sinc(G.e_k / 2) for G != 0, the shoelace area / A at G = 0
 * with G' = (cos theta Gx + sin theta Gy, -sin theta Gx + cos theta Gy).  kind [S] and voff [S+1] are device int32: shape s owns
 * par[b, voff[s] .. voff[s+1]-1] of the fp64 rows par [batch, npar] (5 values, or 2K for a polygon: K comes from the offsets).  recip: HOST
 * double[4] = b1, b2.  The box coef[b, p + 2mmax, q + 2nmax] (|p| <= 2 mmax, |q| <= 2 nmax; complex128) is gathered into out [batch,N,N] by the
 * kernel of trx_convmat_orders (mn, N, mmax, nmax and their check as there); coef = NULL keeps the box in the workspace (ws is not read when
 * coef is given).  All arithmetic is fp64 for both dtypes: a complex64 call returns the complex128 result rounded once.  Every sinc, jinc and
 * hat integral has a series branch for small arguments.  One thread per (b, p, q) loops over shapes and edges; a shape's parameters are staged
 * in LDS in passes of 256 doubles.  No atomics.  Work model: one sincos per (coefficient, edge) and one j1 per (coefficient, ellipse):
 * latency- and transcendental-bound; traffic is the box (16 B per coefficient) and the gather's output.
 * TRX_ERR_ARG: an unknown kind, an ellipse / rectangle without exactly 5 values, a polygon with fewer than 3 vertices or an odd number of
 * values, offsets that decrease or leave the row, cell_area <= 0, batch > 65535 (kind and voff are checked on the host: one more
 * synchronisation of `stream`). */
size_t trx_convmat_shapes_ws_bytes(int dtype, int batch, int N, int mmax, int nmax);
int trx_convmat_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* val, const double* recip,
                       double cell_area, int batch, const int* mn, int N, int mmax, int nmax, void* out, void* coef, void* ws, size_t ws_bytes,
                       void* stream);
/* Adjoint of the gather of trx_convmat_orders / trx_convmat_shapes: gbox[b, p + 2mmax, q + 2nmax] = the sum of gE[b,i,j] over the pairs with
 * m_i - m_j = p, n_i - n_j = q (0 where the list has no such pair); gE [batch,N,N] in `dtype`, gbox complex128, sums in fp64.  A gather: a table
 * (m, n) -> index or -1 is built on the device in ws (trx_toeplitz_sums_ws_bytes = (2mmax+1)(2nmax+1) int32), one wave per (p, q, b) reads
 * gE[b, i(j), j] over j and ends with a fixed tree: bit-identical on repetition, every element of gE read once by the grid (each wave's reads are
 * a diagonal: 16 B of every 64 B line, so about 4 N^2 x 16 B of traffic).  The list is checked on the host as in trx_convmat_orders and
 * must not repeat a harmonic (TRX_ERR_ARG). */
size_t trx_toeplitz_sums_ws_bytes(int dtype, int batch, int N, int mmax, int nmax);
int trx_toeplitz_sums(int dtype, const void* gE, int batch, const int* mn, int N, int mmax, int nmax, void* gbox, void* ws, size_t ws_bytes,
                      void* stream);
/* Adjoint of the closed forms, in PyTorch's convention: gpar[b,i] = Re sum_pq conj(gbox) dc/dpar[b,i] (fp64 [batch, npar]; 0 for a slot no shape
 * owns), gval[b,0] = gbox[b, G = 0], gval[b,s+1] = sum_pq conj(chi_s) gbox (complex128 [batch, S+1]).  A polygon vertex takes the
 * boundary-velocity form: d(A chi)/dv_k = the sum over the two edges at v_k of n_e l_e int_0^1 t e^{-iG.(a + t (v_k - a))} dt, a the other end,
 * n_e l_e = (e_y, -e_x); the hat integral e^{-i alpha}(e^{-i beta}(1 + i beta) - 1) / beta^2 by its series below |beta| = 1.  d/drho of
 * 2 J1 / rho is -2 J2 / rho.  One workgroup of 256 threads per (b, parameter) and per (b, value); each thread sums its coefficients in ascending
 * order, then a fixed tree: bit-identical on repetition, no atomics, no workspace.  Arguments and TRX_ERR_ARG as trx_convmat_shapes. */
int trx_convmat_shapes_backward(const int* kind, const int* voff, int S, const double* par, int npar, const void* val, const double* recip,
                                double cell_area, int batch, int mmax, int nmax, const void* gbox, double* gpar, void* gval, void* stream);

/* ---- the normal-vector rule on vector shapes -------------------------------------------------------------------------------------------------
 * trx_shape_normal_field: nn[b] = (Nx^2, Nx Ny, Ny^2) ([batch,3,n1,n2] fp64) of the normal field of a shape list, sampled at
 * r = (i/n1) a1 + (j/n2) a2 (the DFT's positions, no half-pixel shift).  kind, voff, S, par, npar as trx_convmat_shapes (same host check and
 * TRX_ERR_ARG cases); lattice: HOST double[4] = a1, a2 (finite, non-zero area).  Every primitive -- an ellipse, or one edge of a polygon (a
 * rectangle (Wx, Wy, C, theta) is its 4-gon C + R(theta)(-+Wx/2, -+Wy/2), counter-clockwise from (-,-)) -- contributes in each of the nine
 * images r' = r - p a1 - q a2, p, q in {-1, 0, 1}:
 *   ellipse (Rx, Ry, c, theta): (u, w) = R(-theta)(r' - c), f = hypot(u/Rx, w/Ry), delta = |f - 1| min(Rx, Ry), g = R(theta)(u/Rx^2, w/Ry^2),
 *           n = g/|g|; no contribution when |g| = 0
 *   edge a -> b, e = b - a, tau = (r' - a).e/|e|^2:  0 < tau < 1: n = (e_y, -e_x)/|e|, delta = |(r' - a).n|;  otherwise v = a (tau <= 0) or b:
 *           delta = |r' - v|, n = (r' - v)/delta; no contribution when delta = 0 (the two branches are continuous across tau = 0 and 1)
 *   J = sum n n^T / (delta^2 + eta^2)^2, eta^2 = 1e-12 |a1 x a2|, over all primitives and images, nested shapes included
 * and the direction is trx_normal_field's: d = Jxx - Jyy, o = 2 Jxy, r = hypot(d, o); where r > 1e-3 (Jxx + Jyy): (1 + d/r)/2, o/(2r),
 * (1 - d/r)/2; elsewhere 0 (Laurent's rule locally: a disk's centre, exact mirror lines far from any boundary).  A blend, not a
 * nearest-boundary choice: no tie lines, and on a mirror-symmetric structure the images cancel in Jxy.  One thread per sample, lanes along
 * n2, grid (ceil(n1 n2 / 256), batch); parameters staged in LDS in passes of 256 doubles; the sum runs shapes ascending, images p outer and q
 * inner, edges ascending: bit-identical on repetition.  No workspace, no atomics, all fp64.  Work model: 9 (ellipses + edges) short
 * evaluations per sample, latency- and divide-bound; 24 B written per sample.  n1, n2 <= 2048 (else TRX_ERR_UNSUPPORTED), batch <= 65535.
 *
 * trx_convmat_nv_shapes: the tensor of trx_convmat_nv_orders for a shape list.  [eps] and [1/eps] are the closed-form box of
 * trx_convmat_shapes gathered by trx_convmat_orders' kernel, once with val and once with rval ([batch, S+1] complex128, the reciprocal values:
 * rval[b,0] = 1/eps_background, rval[b,s+1] = 1/eps_s - 1/eps_host); only the three smooth products are sampled: nn ([batch,3,n1,n2] fp64,
 * the caller's) or NULL = trx_shape_normal_field on n1 x n2 into the workspace (lattice is read only then); their matrices come from the
 * pruned DFT and gather of trx_convmat_orders.  Then the tail of trx_convmat_nv_orders: [1/eps]^-1 by trx_inverse in complex128, D, the six
 * GEMMs.  recip, cell_area, mn, N, mmax, nmax as trx_convmat_shapes.  info[batch] (device): 0 ok; 1 a val / rval entry is not finite or a
 * background entry is zero (a medium with eps zero or non-finite); 2 [1/eps] is singular.  An all-zero nn returns Exx = Eyy = the out of
 * trx_convmat_shapes bit for bit and Exy = 0.  Requires n1 > 2 mmax, n2 > 2 nmax (the bound of trx_convmat_orders; the box of the products
 * reaches +-2 mmax, so a grid with n1 <= 4 mmax aliases its outer coefficients -- the Python layer asks for n1 > 4 mmax), n1, n2 <= 2048
 * (TRX_ERR_UNSUPPORTED) and 3 batch <= 65535 (TRX_ERR_ARG).  All arithmetic is fp64 for both dtypes.
 *
 * trx_shape_normal_field_backward: the adjoint of trx_shape_normal_field, gpar[b,k] = sum_{c,i,j} gnn[b,c,i,j] d nn[b,c,i,j] / d par[b,k]
 * (gnn [batch,3,n1,n2] fp64, gpar [batch,npar] fp64, every element written), with the forward's primitives, nine images, eta^2 and coherence
 * floor.  The forward is piecewise smooth and the derivative is that of the current piece.  Branch conventions (part of the contract):
 *   - a sample whose forward products are 0 contributes nothing (coherence <= 1e-3; |g| = 0; a vertex hit with delta = 0 adds no term);
 *   - the derivative of |.| at 0 is 0 (it is multiplied by delta in dw/ddelta = -4 delta w / (delta^2 + eta^2) anyway);
 *   - the derivative of min(Rx, Ry) goes to Rx when Rx <= Ry, else to Ry (a circle, whose R is packed into both, gets the right total);
 *   - on the vertex branch of an edge (tau < 0 or tau > 1) the derivative goes to the vertex that was selected; a sample on a branch line
 *     (tau = 0 or 1 -- round coordinates on a regular grid do hit them) sits on a C0 kink of the field and takes the mean of the two pieces'
 *     derivatives: the symmetric derivative, what a central difference sees, as sign(0) = 0 is for |.|.  On the line means to within rounding:
 *     |(r' - a).e - t| <= 16 eps (|(r' - a)_x e_x| + |(r' - a)_y e_y| + t) for t = 0 or |e|^2, about 1e-14 of the cell in distance;
 *   - a rectangle's (Wx, Wy, Cx, Cy, theta) receive the chain rule through its four vertices; a slot of the row no shape owns receives 0.
 * Per sample J is recomputed as the forward does, in the same order, and the direction step is differentiated in the scaled form
 * k = (a o/r - beta d/r) / r, a = (g_xx - g_yy)/2, beta = g_xy/2: g_d = (o/r) k on d(Jxx - Jyy), g_o = -(d/r) k on d(2 Jxy) -- the unit vector and a
 * single 1/r.  G = [[g_d, g_o], [g_o, -g_d]] is trace-free and orthogonal to J; each term w n n^T, w = 1/(delta^2 + eta^2)^2, contributes
 * dw (n^T G n) + 2 w (t^T G n)(t . dn), t = (-n_y, n_x), formed from the term's own unit normal.  Three launches, no atomics: (1) the forward's
 * kernel with the direction adjoint as its epilogue writes G [batch,2,n1,n2]; (2) grid (chunk, slot, batch), 256 threads: a workgroup is live
 * on the first slot of an ellipse / rectangle and on the x slot of a polygon vertex (the edge that starts there); it accumulates the <= 5
 * partials of that primitive over its chunk of samples x 9 images in registers (samples with G = 0 are skipped) and reduces them by the
 * fixed wave_sum tree and an ascending sum over its four waves; chunks: min(ceil(n1 n2 / 256), 256), so one disk at 256 x 256 is 256
 * workgroups; (3) one thread per (b, slot) sums the chunks in ascending order, for a polygon vertex the edge that ends there and then the edge
 * that starts there.  Bit-identical on repetition.  Work model: the forward again plus one derivative pass of the same 9 (ellipses + edges)
 * evaluations per sample (about three times the divides of the forward's); traffic 24 + 2 x 16 B per sample.  TRX_ERR_ARG as the forward
 * entry (and for gnn, gpar or ws NULL), TRX_ERR_WORKSPACE below trx_shape_normal_field_backward_ws_bytes, TRX_ERR_UNSUPPORTED for n1 or
 * n2 > 2048 or npar > 65535; a refused call writes nothing. */
int trx_shape_normal_field(const int* kind, const int* voff, int S, const double* par, int npar, const double* lattice, int batch, int n1, int n2,
                           double* nn, void* stream);
size_t trx_shape_normal_field_backward_ws_bytes(int S, int npar, int batch, int n1, int n2);
int trx_shape_normal_field_backward(const int* kind, const int* voff, int S, const double* par, int npar, const double* lattice, int batch, int n1,
                                    int n2, const double* gnn, double* gpar, void* ws, size_t ws_bytes, void* stream);
size_t trx_convmat_nv_shapes_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax);
int trx_convmat_nv_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* val, const void* rval,
                          const double* recip, double cell_area, const double* lattice, int batch, int n1, int n2, const int* mn, int N, int mmax,
                          int nmax, const double* nn, void* Exx, void* Exy, void* Eyy, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- dense complex building blocks (the torch.matmul / torch.linalg.inv call sites, rcwa.py:1157-1304) -------- */
/* C = alpha*op(A)*op(B) + beta*C, batched with element strides; alpha/beta point to HOST complex scalars.  lda / ldb / ldc >= the row length of
 * the stored operand; strideA or strideB may be 0 (one operand shared by the batch).  Only the m x n elements of each C are written: columns
 * between n and ldc keep their contents.  beta = 0 does not read C (BLAS semantics: a NaN in C does not propagate). */
int trx_gemm(int dtype, int opA, int opB, int m, int n, int k, const void* alpha, const void* A, int lda,
             long strideA, const void* B, int ldb, long strideB, const void* beta, void* C, int ldc, long strideC,
             int batch, void* stream);
/* Solve A X = B in place (partial-pivot LU; A is overwritten by its factors, B by X).
 * piv: int[batch*n] device scratch; info: int[batch] device (0 ok, k>0: zero pivot at column k). */
int trx_lu_solve(int dtype, void* A, int n, void* B, int nrhs, int batch, int* piv, int* info, void* stream);
/* A <- inverse(A) (LU + solve against the identity); ws: batch*n*n elements. */
size_t trx_inverse_ws_bytes(int dtype, int n, int batch);
int trx_inverse(int dtype, void* A, int n, int batch, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- eigendecomposition: torcwa/torch_eig.py:12-17 (`Eig.forward` -> torch.linalg.eig), rcwa.py:1236/1238 -----
 * A [batch,n,n] general complex, DESTROYED.  w [batch,n] eigenvalues, V [batch,n,n] right eigenvectors in the
 * COLUMNS of V (A V = V diag(w)), each column scaled to unit 2-norm (LAPACK geev convention).  Order of the
 * eigenpairs is unspecified (as in LAPACK).  info[b] = 0 ok, >0: number of eigenvalues that failed to converge.
 * Size limit: n*n*sizeof(element) < 4 GiB (n < 16384 for complex128), else TRX_ERR_ARG. */
size_t trx_eig_ws_bytes(int dtype, int n, int batch);
int trx_eig(int dtype, void* A, void* w, void* V, int n, int batch, int* info, void* ws, size_t ws_bytes,
            void* stream);
/* The same with PER-CALL options instead of the process-global knobs "eig_refine" / "eig_vec" (which remain the defaults of trx_eig):
 *   opts bits 0-3: Newton steps of the mixed-precision route, 1-4 (0 = the knob's value);  bits 4-7: eigenvector route, 1-3 as knob "eig_vec"
 *   (0 = the knob's value); other bits must be 0.  The options live only on the calling thread for the duration of the call, so solvers on
 *   different host threads -- or a complex64 and a complex128 solver of one process -- cannot change each other's route or step count
 *   (torcwa_amd.Engine.eig uses these entry points; tests/test_eig.py::test_eig_opts_two_threads).  The workspace size depends on the route:
 *   size it with trx_eig_ws_bytes_opts and the SAME opts. */
/* Number of matrices of the calling thread's last trx_eig / trx_eig_opts that the mixed-precision route could not certify and redid with the
 * all-fp64 pipeline (a cluster of close eigenvalues beyond the refinement's exact treatment: symmetric meta-atoms, dense spectra of large
 * orders; an fp32 result too far off; a singular eigenvector matrix).  Up to a third of the batch is redone as a compact sub-batch inside
 * the same workspace, beyond that the whole batch (the count is then `batch`); 0 = nothing was redone.  Diagnostic only: results do not
 * depend on it, and the library keeps no state between calls. */
int trx_eig_last_fallback(void);
size_t trx_eig_ws_bytes_opts(int dtype, int n, int batch, unsigned opts);
int trx_eig_opts(int dtype, void* A, void* w, void* V, int n, int batch, int* info, void* ws, size_t ws_bytes, void* stream, unsigned opts);

/* Tuning knobs of libtrx (no reference counterpart).  Results do not depend on any of them (tests/test_eig.py, tests/test_blocks.py); they
 * select code paths.  Knobs are process-global and unsynchronised: trx_tuning must not race with a running trx_eig / trx_lu_solve
 * (per-call alternative for the eigensolver's route and refinement depth: trx_eig_opts).  The
 * environment variables named below are read ONCE per process as initial values.  Returns TRX_OK, or TRX_ERR_ARG for an unknown key or a
 * value out of range.  Unless stated otherwise value 0 = automatic (chosen from n and the batch size).
 *   QR phase of trx_eig
 *   "qr_groups"   1-8   iteration groups on their own streams (TRX_QR_GROUPS)        auto: 4 (batch >= 64), 2 (batch >= 8), 1
 *   "qr_aed"      16-64 aggressive-early-deflation window (TRX_QR_AED)                auto: 64; 48 for one chain per sweep below batch 64
 *   "qr_chains"   1-3   bulge chains per sweep (TRX_QR_CHAINS)                        auto: 3 for batch <= 2, 2 up to batch 48, 1 above (one chain =
 *                       the form with super-steps and fused launches, which pays when the batch fills the chip)
 *   "qr_nibble"   0-100 LITERAL percentage, default 100 (TRX_QR_NIBBLE): an AED that deflated less than this share of its window is
 *                       followed by a sweep in the same outer iteration; 0 switches that sweep off.  No automatic value.
 *   "qr_moves"    0-64  LITERAL bound, default 12 (TRX_QR_MOVES): undeflatable eigenvalues an AED moves out of the way; 0 = no reordering.
 *   "qr_rotb"     1 = the in-LDS Schur solver of the AED broadcasts each rotation with ds_bpermute (round-3 code); default: v_readlane (TRX_QR_ROTB)
 *   "qr_super"    1-8   window steps per launch of the chase kernel (one chain per sweep: TRX_QR_SUPER)     auto: 4 (fp32), 8 (fp64).  The workgroup applies each
 *                       window's unitary itself to the band of columns the next windows slide over; the left update beyond the band is one
 *                       launch per super-step, the right update of H and the update of Z one launch per sweep (link log of the sweep)
 *   "qr_defer"    1 = right update of H and update of Z after every super-step instead of once per sweep (TRX_QR_DEFER)   auto: once per sweep
 *                       when the sweep has one chain; with 2-3 chains the following chain reads the rows, so it is per step
 *   "qr_fuse"     1 = every update of a launch's links as its own launch, as in round 5 (TRX_QR_FUSE)
 *                       auto: one chain per sweep -- the NEXT chase launch carries far workgroups that apply the left update beyond the columns the
 *                       chase reaches; several chains -- the NEXT step's chase launch carries the right / Z update of the step (two strips per
 *                       rider wave: TRX_QR_RSPW, environment only)
 *   "slab_spw"    1, 2, 4  strips per wave of the left update (TRX_SLAB_SPW)           auto: 1
 *   "slab_band"   1 = dense window unitary always (TRX_SLAB_BAND)                     auto: skip the structurally zero blocks of a chase unitary
 *   Eigenvector route of trx_eig
 *   "eig_vec"     1 = all-fp64 pipeline (all-fp32 for complex64 input) with Schur vectors, 3 = mixed precision wherever n >= 8: fp32
 *                       eigendecomposition refined to fp64 by Newton steps (TRX_EIG_VEC)
 *                       auto: mixed precision for complex128 input of n >= 256 AND batch >= 8, else Schur vectors; trx_eig_ws_bytes depends on
 *                       this knob (per call and race-free: trx_eig_opts).  (2, inverse iteration on the Hessenberg matrix, was removed in round 5.)
 *   "eig_refine"  1-4   Newton steps of the mixed-precision route; 0 = default (2: eigen-residual ~1e-11 ||A||, what a complex64 caller's
 *                       1e-5 needs with five digits to spare; 3 reach the all-fp64 pipeline's 1e-13 -- torcwa_amd.Engine asks for 3 per call
 *                       (trx_eig_opts) whenever the caller's own dtype is complex128)
 *   GEMM (trx_gemm and every product inside the library)
 *   "gemm_big"    4 = large-tile complex128 kernel (128 x 96 on 8 waves; outputs of at least 2 x 2 tiles, k >= 64) OFF: the 64 x 64 tile everywhere
 *                       (TRX_GEMM_BIG)                                                                              auto: on
 *   LU (trx_lu_solve, trx_inverse and everything built on them)
 *   "lu_split"    rows: a panel is factored by several workgroups per matrix while at least this many rows remain (TRX_LU_SPLIT); 1 = never;
 *                       0 = automatic: only panels too tall for the LDS-resident one-workgroup kernel (fp64: above 1971 rows, fp32: 3942)
 *   "lu_split_batch"  largest batch that uses the row-split panel (TRX_LU_SPLIT_BATCH); 0 = any batch
 *   "lu_sub"      1 = panels column by column as in rounds 1 - 5, 2 = sub-blocks of 4 columns everywhere (TRX_LU_SUB)
 *                       auto: sub-blocks of 8 columns, of 4 for panels too tall for 8 (same pivots)
 *   Hessenberg reduction
 *   "hess_group"  1-4   panels whose right updates of Z and of the rows above the panel are merged into one block reflector and applied
 *                       together (TRX_HESS_GROUP); 1 = every panel on its own as in rounds 1 - 5                      auto: 4
 *   TRX_HESS_RPW=2 (environment only) streams two rows per wave and pass in the BLAS-2 kernel instead of four. */
int trx_tuning(const char* key, int value);

/* Adjoint of the eigendecomposition: torcwa/torch_eig.py:19-44 (`Eig.backward`, the Lorentzian-broadened formula)
 *   gA = (V^H)^-1 (diag(gw) + conj(F) o (V^H gV)) V^H,   F_ij = conj(w_j - w_i) / (|w_j - w_i|^2 + broadening), F_ii = 0.
 * w [batch,n], V [batch,n,n] as returned by trx_eig; gw [batch,n], gV [batch,n,n] incoming gradients; gA [batch,n,n] output.
 * broadening: `Eig.broadening_parameter` (1e-10 by default); pass the smallest positive number of the dtype to reproduce the
 * reference's un-broadened branch (torch_eig.py:27-31).  piv: int[batch*n], info: int[batch] (LU of V^H). */
size_t trx_eig_backward_ws_bytes(int dtype, int n, int batch);
int trx_eig_backward(int dtype, const void* w, const void* V, const void* gw, const void* gV, double broadening, int n, int batch,
                     void* gA, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- layer eigenproblem assembly: torcwa/rcwa.py:1224-1232 (`_eigen_decomposition`, P and Q) -------------------
 * P = [[Kx Ei Ky, M - Kx Ei Kx],[Ky Ei Ky - M, -Ky Ei Kx]],  Q = [[-Kx Mi Ky, Kx Mi Kx - E],[E - Ky Mi Ky, Ky Mi Kx]]
 * E, Einv, Mu, Muinv: [batch,N,N] (Einv = inverse of the permittivity convolution matrix, etc.);
 * kx, ky: [batch,N] complex (the diagonals of Kx_norm, Ky_norm, rcwa.py:1138-1141); P, Q: [batch,2N,2N].
 * One implementation (csrc/assembly.hip) serves this entry, trx_build_pq_aniso and trx_build_pq_tensor, and likewise the three trx_build_a*. */
int trx_build_pq(int dtype, const void* E, const void* Einv, const void* Mu, const void* Muinv, const void* kx,
                 const void* ky, int N, int batch, void* P, void* Q, void* stream);

/* ---- layer scattering matrix: torcwa/rcwa.py:1244-1281 (`_solve_layer_smatrix`) --------------------------------
 * Inputs  W [batch,n,n] eigenvectors (E_eigvec), n = 2N;
 *         kzfac [batch,n]: kz (use_q=0: V = P^-1 W diag(kz), rcwa.py:1264) or 1/kz (use_q=1: V = Q W diag(1/kz), :1262);
 *         use_q=2: V is an INPUT (already computed, e.g. by trx_hmodes); P, Q and kzfac are not read;
 *         vfinv [4,batch,N]: the four diagonals (p11,p12,p21,p22) of Vf^-1 = [[p11,p12],[p21,p22]] (Vf: rcwa.py:1143-1147);
 *         phase [batch,n] = exp(i*omega*kz*thickness) (rcwa.py:1246).
 * Outputs S11, S21 [batch,n,n] (the layer's S22 == S11 and S12 == S21 identically), V [batch,n,n] (H_eigvec),
 *         optional Cplus, Cminus [batch,n,n]: Cf = [Cplus; Cminus], Cb = [Cminus; Cplus] (rcwa.py:1271-1274).
 * piv: int[3*batch*n], info: int[3*batch] (slot 0..B-1: P factorisation; B..3B-1: the two n x n inverses).
 * Accuracy: S11 is formed as M+ - M-, M+- = W (I +- X) T+-^-1 (two n x n solves instead of the reference's 2n x 2n inverse), with an error of
 *         eps cond(T+-) |M+-|.  When every mode of a layer is strongly evanescent (max |phase| << 1) S11 itself is much smaller than M+-, and
 *         its error RELATIVE TO max |S11| grows by max |M+-| / max |S11| (measured: 62 x LAPACK's at max |phase| = 6.5e-3, n = 70); relative to
 *         the layer's S21 it does not (tests/test_smatrix_blocks.py::test_layer_smatrix).
 * Workspace: trx_layer_smatrix_ws_bytes (6 matrices per point); when Cplus == NULL and S11 | S21 are ONE contiguous
 * [2*batch,n,n] block (S21 == S11 + batch*n*n) the outputs double as scratch and trx_layer_smatrix_ws_bytes_lean (4) suffices. */
size_t trx_layer_smatrix_ws_bytes(int dtype, int N, int batch);
size_t trx_layer_smatrix_ws_bytes_lean(int dtype, int N, int batch);
/* H-field modes V = P^-1 W diag(kz) (rcwa.py:1248, 1264) of a layer with HOMOGENEOUS mu, from the rank-N structure
 * P = mu J + [Kx; Ky] E^-1 [Ky, -Kx] (rcwa.py:1226-1228): one N x N factorisation of E - (Kx^2 + Ky^2)/mu and a 2N-column
 * solve replace the LU of the 2N x 2N matrix P (0.29 n^3 instead of 1.33 n^3 complex MACs).  E [batch,N,N] permittivity
 * convolution matrix (NOT its inverse), mu [batch], kx, ky [batch,N], W [batch,n,n], kz [batch,n]; V [batch,n,n] output.
 * piv: int[batch*N], info: int[batch]; ws: trx_hmodes_ws_bytes. */
size_t trx_hmodes_ws_bytes(int dtype, int N, int batch);
int trx_hmodes(int dtype, const void* E, const void* mu, const void* kx, const void* ky, const void* W, const void* kz, int N, int batch,
               void* V, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);
int trx_layer_smatrix(int dtype, const void* P, const void* Q, const void* W, const void* kzfac, const void* vfinv,
                      const void* phase, int use_q, int N, int batch, void* S11, void* S21, void* V, void* Cplus,
                      void* Cminus, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- Redheffer star product: torcwa/rcwa.py:1283-1306 (`_RS_prod`) -----------------------------------------------
 * Sm, Sn, Sout: HOST arrays of 4 device pointers in the reference's order [S11, S21, S12, S22], each [batch,n,n];
 * outputs must not alias inputs.  XY [batch,n,2n] x 2 receives X = [t1 Sm11 | t1 Sm12 Sn22] and
 * Y = [t2 Sn21 Sm11 | t2 Sn22] -- exactly the four products the reference needs to propagate the mode-coupling
 * coefficients C (rcwa.py:1297-1304), so the caller can do that lazily.  piv: int[batch*n], info: int[batch].  Any n >= 1, odd n included
 * (element alignment of every buffer suffices). */
size_t trx_redheffer_ws_bytes(int dtype, int n, int batch);
int trx_redheffer(int dtype, const void* const* Sm, const void* const* Sn, void* const* Sout, void* XY, int n, int batch,
                  int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* Star product with a HALF-SPACE operand (the Sin / Sout coupling steps of solve_global_smatrix, rcwa.py:198-208).
 * The four blocks of Sin / Sout are 2x2-block-diagonal (rcwa.py:1157-1181), so they are passed as diagonals
 * bd[4 blocks S11,S21,S12,S22][4 diagonals d11,d12,d21,d22][batch][N] and every product with them is O(n^2).
 * side = 0: half-space on the left (Sin * S);  side = 1: on the right (S * Sout).  Other arguments as trx_redheffer.
 * XY may be NULL for side = 0 when the coupling factors are not needed (no C lists to propagate): the product is then
 * formed with right-solves (4.33 n^3 instead of 6.33 n^3 complex MACs) and needs the larger workspace reported by
 * trx_redheffer_halfspace_ws_bytes(dtype, N, batch, side, want_xy = 0). */
size_t trx_redheffer_halfspace_ws_bytes(int dtype, int N, int batch, int side, int want_xy);
int trx_redheffer_halfspace(int dtype, int side, const void* bd, const void* const* S, void* const* Sout, void* XY, int N, int batch,
                            int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* PROBED half-space star product: m columns of ONE block of the product instead of its four n x n blocks -- what a sweep reads (S_parameters
 * takes a few rows of one or two columns of one block, rcwa.py:300-524).  side, bd, S as trx_redheffer_halfspace; block = 0..3 in the order
 * [S11, S21, S12, S22]; cols: HOST array of m column indices in [0, 2N), shared by the batch, 1 <= m <= 16; out [batch,n,m] receives
 * out[b, :, q] = (block of Sin * S or S * Sout)[b, :, cols[q]].  With Sm * Sn, K = I - Sm12 Sn21 and e_c the unit vector of column c:
 *   v = Sm11 e_c (blocks 0, 1)  or  Sm12 (Sn22 e_c) (blocks 2, 3);   u = K^-1 v;
 *   block 0: Sn11 u;  block 1: Sm21 e_c + Sm22 (Sn21 u);  block 2: Sn12 e_c + Sn11 u;  block 3: Sm22 (Sn22 e_c + Sn21 u).
 * K is an O(n^2) row (side 0) or column (side 1) combination, so the call costs one LU of K (n^3/3 complex MACs), one m-column solve and at
 * most one dense mat-vec: 0.33 n^3 instead of 4.33 n^3.  The inputs are not modified and out must not alias them.  piv: int[batch*n];
 * info: int[batch], set by the LU of K exactly as in trx_redheffer_halfspace (non-zero: singular K, that point's columns are not finite).
 * ws: trx_redheffer_halfspace_columns_ws_bytes = one [batch,n,n] matrix for K and three [batch,n,m] column blocks.  batch <= 65535;
 * TRX_ERR_ARG for a block, a column index or m out of range. */
size_t trx_redheffer_halfspace_columns_ws_bytes(int dtype, int N, int batch, int m);
int trx_redheffer_halfspace_columns(int dtype, int side, const void* bd, const void* const* S, int block, const int* cols, int m, void* out,
                                    int N, int batch, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* A = P Q (rcwa.py:1236) for a layer with homogeneous mu[batch], from its block structure (two N^3 GEMMs instead of
 * one (2N)^3): A = [[mu E - Ky^2 - Kx Gx, KxKy - Kx Gy],[KxKy - Ky Gx, mu E - Kx^2 - Ky Gy]], G* = Einv (K* E). */
size_t trx_build_a_ws_bytes(int dtype, int N, int batch);
int trx_build_a(int dtype, const void* E, const void* Einv, const void* mu, const void* kx, const void* ky, int N, int batch, void* A,
                void* ws, size_t ws_bytes, void* stream);

/* P, Q (as trx_build_pq) with a convolution matrix per field component (Li's rule; the full in-plane tensor: trx_build_pq_tensor):
 *   P = [[Kx Ei Ky, My - Kx Ei Kx],[Ky Ei Ky - Mx, -Ky Ei Kx]],  Q = [[-Kx Mi Ky, Kx Mi Kx - Ey],[Ex - Ky Mi Ky, Ky Mi Kx]]
 * Einv / Minv: inverses of the LAURENT matrices (they act on Ez / Hz).  Ex = Ey = E, Mx = My = M gives trx_build_pq
 * (the same code: bit-identical results). */
int trx_build_pq_aniso(int dtype, const void* Ex, const void* Ey, const void* Einv, const void* Mx, const void* My, const void* Minv,
                       const void* kx, const void* ky, int N, int batch, void* P, void* Q, void* stream);
/* A = P Q for homogeneous mu[batch] with per-component Ex, Ey (two N^3 GEMMs, as trx_build_a):
 *   A = [[mu Ex - Ky^2 - Kx Gx, KxKy - Kx Gy],[KxKy - Ky Gx, mu Ey - Kx^2 - Ky Gy]],  Gx = Einv (Kx Ex), Gy = Einv (Ky Ey). */
size_t trx_build_a_aniso_ws_bytes(int dtype, int N, int batch);
int trx_build_a_aniso(int dtype, const void* Ex, const void* Ey, const void* Einv, const void* mu, const void* kx, const void* ky, int N, int batch,
                      void* A, void* ws, size_t ws_bytes, void* stream);

/* P, Q (as trx_build_pq) with the in-plane permittivity tensor of trx_convmat_nv (Eyx = Exy):
 *   P = [[Kx Ei Ky, M - Kx Ei Kx],[Ky Ei Ky - M, -Ky Ei Kx]],  Q = [[-Kx Mi Ky - Exy, Kx Mi Kx - Eyy],[Exx - Ky Mi Ky, Ky Mi Kx + Exy]]
 * Einv: inverse of the LAURENT [eps] (it acts on Ez); Mu / Muinv as trx_build_pq.  Exx = Eyy = E, Exy = 0 gives trx_build_pq (the same
 * code with the Exy terms added: equal results). */
int trx_build_pq_tensor(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Einv, const void* Mu, const void* Muinv,
                        const void* kx, const void* ky, int N, int batch, void* P, void* Q, void* stream);
/* A = P Q for homogeneous mu[batch] with the tensor (one N x 2N GEMM, the cost of trx_build_a_aniso's two N^3 products):
 *   A = [[mu Exx - Ky^2 - Kx Gx, mu Exy + KxKy - Kx Gy],[mu Exy + KxKy - Ky Gx, mu Eyy - Kx^2 - Ky Gy]],
 *   [Gx, Gy] = Einv [Kx Exx + Ky Exy, Kx Exy + Ky Eyy]. */
size_t trx_build_a_tensor_ws_bytes(int dtype, int N, int batch);
int trx_build_a_tensor(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Einv, const void* mu, const void* kx, const void* ky,
                       int N, int batch, void* A, void* ws, size_t ws_bytes, void* stream);

/* ---- power flux through the planes of a stack (no reference counterpart; the formulas are those of the reference's field maps,
 *      torcwa/rcwa.py:708-755, reduced over the unit cell by Parseval) ------------------------------------------------------------------
 * trx_matvec: Y[b] = A[b] X[b] for a skinny right-hand side.  A [batch,m,k]; X [batch,k,c] with element stride strideX between points
 * (strideX = 0: one X shared by the batch); Y [batch,m,c]; 1 <= c <= 16, batch <= 65535.  One wave per row of A, fp64 accumulation for both
 * dtypes, a fixed reduction tree (bitwise reproducible).  Used for [c+; c-] = C_layer E_i and for S_block E_i in the half-spaces.  No workspace. */
int trx_matvec(int dtype, const void* A, const void* X, long strideX, void* Y, int m, int k, int c, int batch, void* stream);
/* trx_layer_flux: the cell-averaged z component of Re(E x H*) at nz planes inside a layer, un-normalised,
 *   flux[b,t] = Re sum_{j<N} ( e_j conj(h_{j+N}) - e_{j+N} conj(h_j) ),   e = W (a + b),  h = V (a - b)          (n = 2N rows: x then y)
 *   a_k = cplus_k exp(i omega kz_k z),   b_k = cminus_k exp(i omega kz_k (d - z)),   z = z[b,t]  (z_is_fraction: z[b,t] d[b])
 * W, V [batch,n,n] (E_eigvec, H_eigvec; 16-byte aligned), cplus, cminus, kz [batch,n] in `dtype` (element alignment suffices); omega, d [batch],
 * z [batch,nz] and the output flux [batch,nz] are float64.  nz = 0 or batch = 0 returns TRX_OK without touching any buffer (ws may be NULL).  The phase factors are formed in the kernel; neither the [n,nz] right-hand sides nor the products W(a+b), V(a-b)
 * are written to memory.  Traffic model: W and V are read once per tile of up to 16 planes (2 n^2 elements per point and tile; 118 MB at
 * n = 1922 in complex128), everything else is O(n nz).  Dot products and the sum over j are accumulated in fp64 for both dtypes.  Deterministic:
 * each workgroup (32 harmonics j, i.e. the four row blocks the sum pairs) writes one partial per plane to the workspace and a second kernel adds
 * them in a fixed order; no floating-point atomics.  ws: trx_layer_flux_ws_bytes (ceil(N/32) nz batch doubles), 16-byte aligned. */
size_t trx_layer_flux_ws_bytes(int dtype, int N, int nz, int batch);
int trx_layer_flux(int dtype, const void* W, const void* V, const void* cplus, const void* cminus, const void* kz, const double* omega,
                   const double* d, const double* z, int z_is_fraction, int N, int nz, int batch, double* flux, void* ws, size_t ws_bytes,
                   void* stream);

/* ---- field maps for a batch (the formulas of the reference's field_xy / field_xz / field_yz, torcwa/rcwa.py:598-1112) -----------------------
 * trx_layer_field: the Fourier coefficients of the fields inside one internal layer at nz depths, with the mode amplitudes of trx_layer_flux,
 *   a_k = cplus_k exp(i omega kz_k z),  b_k = cminus_k exp(i omega kz_k (d - z)),  e = W (a + b),  h = V (a - b)       (n = 2N rows: x then y)
 *   out[b,0..3,j,t] = ex_j, ey_j, hx_j, hy_j   (= e_j, e_{j+N}, h_j, h_{j+N})
 *   out[b,4,j,t]    = ky_j hx_j - kx_j hy_j    (E_z before [eps]^-1)
 *   out[b,5,j,t]    = kx_j ey_j - ky_j ex_j    (H_z before [mu]^-1)                                 z = z[b,t]  (z_is_fraction: z[b,t] d[b])
 * W, V [batch,n,n] (16-byte aligned), cplus, cminus, kz [batch,n] and out [batch,6,N,nz] in `dtype` (element alignment suffices); omega, d
 * [batch], z [batch,nz] and kx, ky [batch,N] are float64.  nz = 0 or batch = 0 returns TRX_OK without touching any buffer; batch <= 65535.
 * Exponents, dot products and rows 4, 5 are fp64 for both dtypes; the result is rounded once, to `dtype`.  The right-hand sides are formed in
 * LDS and never written to memory.  Traffic model: W and V are read once per tile of up to 16 depths (2 n^2 elements per point and tile; 118 MB
 * at n = 1922 in complex128) and 6 N nz elements are written; everything else is O(n nz).  No workspace and no atomics: each output element
 * is owned by one thread of one workgroup (32 harmonics j, i.e. rows j and j + N of W and of V), so two calls give the same bits. */
int trx_layer_field(int dtype, const void* W, const void* V, const void* cplus, const void* cminus, const void* kz, const double* omega,
                    const double* d, const double* z, int z_is_fraction, const double* kx, const double* ky, int N, int nz, int batch, void* out,
                    void* stream);
/* trx_field_synth: Fourier coefficients to space, the Bloch phases formed in the kernel,
 *   out[b,c,iu,iv,t] = sum_m coef[b,c,m,t] exp(i omega_b (kx[b,m] u_iu + ky[b,m] v_iv))
 * coef [batch,ncomp,N,T] and out [batch,ncomp,nu,nv T] in `dtype` (element alignment suffices); kx, ky [batch,N] and omega [batch] float64;
 * u [nu], v [nv] float64, shared by the batch.  1 <= ncomp <= 6; either nv = 1 (a vertical cut with T depths) or T = 1 (a horizontal map), else
 * TRX_ERR_ARG.  For a yz cut the caller swaps the roles: (ky, kx) and (y_axis, [x0]).  kx, ky are arbitrary per harmonic: any order set, any
 * lattice.  nu = 0, nv = 0 or batch = 0 returns TRX_OK without touching any buffer; batch <= 65535, nu <= 16 * 65535.
 * Phases and sums are fp64 for both dtypes.  All ncomp components of a point share one phase.  A map takes the phase as the product of a u table
 * [16, 16] and a v table [16, 64] staged in LDS per chunk of 16 harmonics -- 0.08 sincos per (point, harmonic) -- and a cut stages one table
 * [16, 8] of the whole phase; neither the [nu,N] and [N,nv] phase matrices nor (phase x coef) reach memory.  Work model: 4 real multiply-adds
 * per (point, harmonic) for the phase product and 4 per component, 28 for six, in vector fp64; traffic: coef is read once per tile of 16 x 64
 * points (from cache after the first) and out is written once.  Deterministic: each output element is owned by one thread, summed over m in
 * ascending order; no workspace, no atomics. */
int trx_field_synth(int dtype, const void* coef, const double* kx, const double* ky, const double* omega, const double* u, const double* v,
                    int ncomp, int N, int T, int nu, int nv, int batch, void* out, void* stream);

/* ---- volume integrals inside a layer (no reference counterpart; the closed form other RCWA codes offer as a layer volume integral) -------
 * trx_modal_overlap: out[b,r] = sum_{k,l} M[b,k,l] T_kl(z0, z1), (z0, z1) = zr[b,r] (z_is_fraction: times d[b]), the z integral over [z0, z1] of
 * sum_kl M_kl conj(a_k + s b_k)(a_l + s b_l) with the mode amplitudes of trx_layer_flux,
 *   a_k(z) = cplus_k e_k(z),   b_k(z) = cminus_k e_k(d - z),   e_k(z) = exp(i omega kz_k z),   Im kz >= 0   (|e_k| <= 1 on [0, d]):
 *   T_kl = conj(c+_k) c+_l G++_kl + s conj(c+_k) c-_l G+-_kl + s conj(c-_k) c+_l G-+_kl + conj(c-_k) c-_l G--_kl
 *   G++ = int conj(e_k(z)) e_l(z) dz       G+- = int conj(e_k(z)) e_l(d - z) dz
 *   G-+ = int conj(e_k(d - z)) e_l(z) dz   G-- = int conj(e_k(d - z)) e_l(d - z) dz
 * With M = Phi^H Gamma Phi this is (1 / cell) int int int w |F|^2 for the field F = Phi (a + s b) and the weight w whose convolution matrix is
 * Gamma: Phi = W, s = +1 for [ex; ey]; V, s = -1 for [hx; hy]; [eps]^-1 (Ky V_x - Kx V_y), s = -1 for ez; [mu]^-1 (Kx W_y - Ky W_x), s = +1 for hz.
 * End-point rule: every integrand is g(z) = exp(alpha z + beta) with |g| <= 1 on [0, d], and int_{z0}^{z1} g = g(z_e) D phi(x), D = z1 - z0,
 * phi(x) = (e^x - 1) / x, with z_e = z0, x = alpha D where Re alpha <= 0 and z_e = z1, x = -alpha D otherwise: Re x <= 0, so nothing overflows
 * and no 0 * inf appears however evanescent the modes.  phi is evaluated by its series for |x| < 1/2 and phi(0) = 1 exactly (the diagonal terms
 * of a lossless propagating mode).  Ranges need not be ordered: z1 < z0 gives the negated integral of (z1, z0), bit for bit.
 * M [batch,n,n] (16-byte aligned), cplus, cminus, kz [batch,n] in `dtype`; omega, d [batch] and zr [batch,nr,2] float64; s = +1 or -1; any n >= 1;
 * out [batch,nr] complex128 for both dtypes (16-byte aligned).  nr = 0 or batch = 0 returns TRX_OK without touching any buffer (ws may be NULL);
 * batch <= 65535; TRX_ERR_ARG for another s or nr < 0.  Exponents, phi and the sums are fp64 for both dtypes.  Traffic model: M is read once per
 * tile of up to 16 ranges (n^2 elements per point and tile; 59 MB at n = 1922 in complex128), the end-point factors are O(n nr) and stay in LDS
 * and registers; neither the G matrices nor T are written to memory.  Deterministic: each workgroup (16 rows of M) writes one partial per range
 * to the workspace and a second kernel adds them in a fixed order; no floating-point atomics.
 * ws: trx_modal_overlap_ws_bytes = 16 ceil(n/16) nr batch bytes, 16-byte aligned. */
size_t trx_modal_overlap_ws_bytes(int dtype, int n, int nr, int batch);
int trx_modal_overlap(int dtype, const void* M, const void* cplus, const void* cminus, const void* kz, const double* omega, const double* d,
                      const double* zr, int z_is_fraction, int s, int n, int nr, int batch, void* out, void* ws, size_t ws_bytes, void* stream);

/* ---- mirror-symmetry folding of a layer eigenproblem (no reference counterpart; the reduction S4, RETICOLO and others offer) ---------------
 * A layer that is invariant under x -> -x about a plane (and / or y -> -y), lit with kx0 = 0 (ky0 = 0), has A = P Q commuting with the mirror
 * R_x = diag(-J_x, +J_x) on [Ex; Ey] (R_y = diag(+J_y, -J_y)), where J_x sends the unit vector of harmonic (m, n) to exp(+2 pi i m c / nx) times
 * that of (-m, n); c is the integer with grid[i, j] == grid[(c - i) mod nx, j] (c = nx - 1 for samples at (i + 1/2) h, c = 0 for a grid that is
 * symmetric about sample 0).  In the basis T of joint eigenvectors of the mirrors A is block diagonal: two blocks of n / 2 for one mirror, four
 * of about n / 4 for two.  T is unitary and sparse and is handed over as a PLAN in device memory, built once by the caller (never by the kernels):
 *   idx [n,4] int32   rows of the non-zeros of column j of T (unused slots: any row in [0, n) with weight 0)
 *   wt  [n,4] `dtype` their values (modulus 1/sqrt(2) or 1/2 or 1)
 *   off [nblk+1] int32  the columns of T are sorted by block: block k is columns off[k] .. off[k+1]-1, off[0] = 0, off[nblk] = n, 1 <= nblk <= 4
 * Inside one block the columns of T have disjoint supports (true of any basis built orbit by orbit); trx_sym_unfold relies on it.
 * Packing of per-block arrays ("packed"): blocks of equal size n_k form a group, groups ordered by their first block; a group of g blocks is one
 * contiguous [g * batch, n_k, n_k] array (block-major, then batch), ready for ONE trx_eig call per distinct size; eigenvalues likewise as
 * [g * batch, n_k].  The groups follow each other without padding: sum_k batch n_k^2 (sum_k batch n_k = batch n) elements in all.
 *
 * trx_sym_fold: blocks (packed) = the diagonal blocks B_k = T_k^H A T_k of A [batch,n,n] (not modified); resid[batch] (double) = the largest
 * modulus among the entries of T^H A T OUTSIDE the diagonal blocks, divided by max |A| (0 for A = 0): rounding level when A commutes with the
 * mirrors, O(1) when it does not.  Separable: C = T^H A along the rows, then C T along the columns, 2 - 4 reads per element and pass.
 * Traffic model (elements per matrix): 2 n^2 (one mirror) or 4 n^2 (two) read of A, n^2 written and read back for C, sum_k n_k^2 written:
 * (nblk + 2 + 1 / nblk) n^2 = 4.5 n^2 / 6.25 n^2, i.e. 266 MB / 369 MB per complex128 matrix at n = 1922; no arithmetic to speak of.  Deterministic (exact maxima, combined in a
 * fixed order; no atomics).  A malformed off (not monotone from 0 to n) writes no block and sets resid to NaN; idx is clamped into [0, n).
 * ws: trx_sym_fold_ws_bytes = one [batch,n,n] matrix for C and 16 ceil(n/8) batch bytes of partial maxima, 16-byte aligned.
 * trx_sym_unfold: W [batch,n,n] and lam [batch,n] from the packed eigenvectors Wk and eigenvalues lamk of the blocks (as trx_eig returns them
 * per group): W[:, off[k]:off[k+1]] = T_k W_k, lam = the block eigenvalues in block order.  T is unitary, so the columns of W keep the unit
 * 2-norm of trx_eig's geev convention and A W = W diag(lam) holds in the original basis.  W is zero-filled first (rows a block does not reach),
 * then every element has one writer: 2 n^2 written, sum_k n_k^2 read.  No workspace.
 * Adjoints, in PyTorch's complex convention (a linear map Y = L(X) has gX = L^H(gY)); they make the folded eigenproblem differentiable:
 * trx_sym_fold_backward: gA [batch,n,n] = sum_k T_k gB_k T_k^H from the packed block gradients gblocks (the packing of trx_sym_fold's output).
 * resid carries no gradient.  Only the diagonal blocks of T^H A T reach the output of trx_sym_fold, so gA is the gradient of the
 * mirror-constrained problem: it commutes with the mirrors whatever gblocks holds.  The kernel reads the ROW plan, built by the caller like
 * the plan itself:
 *   ridx [n,4] int32   slot k: the column of block k (a column index of T, in off[k] .. off[k+1]-1) whose support holds row r
 *   rwt  [n,4] `dtype` T's entry there, 0 if block k has no such column (and for slots k >= nblk); ridx of such a slot: any value
 * (a row lies in at most one column per block because the supports inside a block are disjoint), so that
 *   gA[r,c] = sum_k rwt[r,k] gB_k[ridx[r,k] - off[k], ridx[c,k] - off[k]] conj(rwt[c,k]):
 * a gather with one writer per element; no zero fill, no workspace, no atomics.  Indices are clamped into their block.  A malformed off fills
 * gA with NaN.  Traffic model (elements per matrix): n^2 written, at most one element of gB_k read per element and block: (1 + nblk) n^2.
 * trx_sym_unfold_backward: gWk (packed) and glamk (packed) from gW [batch,n,n] and glam [batch,n]: gW_k = T_k^H gW[:, off[k]:off[k+1]] (row j a
 * combination of the at most four rows idx[off[k]+j][q] of gW with conj(wt)), glam_k = glam[off[k]:off[k+1]]; the layout trx_sym_unfold reads.
 * Every element of gWk and glamk is written, the inputs are not modified.  A malformed off leaves gWk alone (its packing is not defined) and
 * fills glamk, batch n elements whatever the blocks, with NaN.  Traffic model: n^2 read, sum_k n_k^2 written: (1 + 1 / nblk) n^2.  No workspace.
 * Sector folds: one pair of blocks of T^H M T for any M, not only one that commutes with the mirrors.  E -> E operators (A, the blocks of a
 * layer S-matrix, of Sin / Sout) are block diagonal in T; E -> H and H -> E operators (Q, Vf; P, Vf^-1) connect block k with the opposite
 * block only (H is a pseudovector), k' = nblk - 1 - k, which has the size of block k.
 * trx_sym_fold_pair: out [batch,n_kl,n_kr] = T_kl^H M T_kr for M [batch,n,n] (not modified), 0 <= kl, kr < nblk, n_k = off[k+1] - off[k];
 * rectangular when the sizes differ.  One pass, no n x n intermediate: an output element combines the at most 16 elements
 * M[idx[I][p], idx[J][q]] of column I = off[kl] + i and J = off[kr] + j of T with conj(wt[I][p]) wt[J][q].  Every element of out is written,
 * one writer each; a block of size 0 is legal and writes nothing.  A malformed off (not monotone from 0 to n) fills out -- n_kl x n_kr as off
 * states them, each held inside [0, n] -- with NaN; idx is clamped into [0, n).  Traffic model (elements per matrix): at most 16 n_kl n_kr
 * read, n_kl n_kr written: 17 (n / nblk)^2, about n^2 per pair for two mirrors (59 MB per complex128 matrix at n = 1922).  No workspace.
 * trx_sym_fold_pair_bd: the same for a 2x2-block-diagonal M given as its four diagonals bd [4][batch][N] (d11, d12, d21, d22; n = 2 N; the
 * layout of one block of trx_redheffer_halfspace's bd): the dense out [batch,n_kl,n_kr], zeros included.  Serves Vf^-1 (pair k, k'), the blocks
 * of Sin / Sout and of a homogeneous layer's S-matrix (pair k, k).  Traffic model: the 4 N diagonal entries read, n_kl n_kr written.
 * N <= 16384.
 * Adjoints of the sector folds, in PyTorch's complex convention; they make a sector solve differentiable.  Both read the ROW plan ridx / rwt of
 * trx_sym_fold_backward: a gather with one writer per element, no zero fill, no workspace, no atomics; indices are clamped into their block.
 * trx_sym_fold_pairs_backward: the adjoint of npairs trx_sym_fold_pair calls on the same M, in one pass:
 *   gM[r,c] = sum_p rwt[r,kl_p] G_p[ridx[r,kl_p] - off[kl_p], ridx[c,kr_p] - off[kr_p]] conj(rwt[c,kr_p])      (gM = sum_p T_kl_p G_p T_kr_p^H)
 * G: HOST array of npairs device pointers, G_p [batch,n_kl_p,n_kr_p]; kl, kr: HOST arrays of npairs block indices; 0 <= npairs <= 16.  The table
 * travels to the kernel by value: no device-side pointer array.  A null G_p is a pair whose output took no gradient: it is skipped (its kl, kr are
 * still checked).  Every element of gM [batch,n,n] is written: 0 where no pair reaches, all zeros when every pointer is null or npairs = 0.  A pair
 * may occur more than once.  A malformed off fills gM with NaN.  A layer folds P on the pairs (k, k') and Q on (k', k) of every block k: one call
 * per matrix writes n^2 once, where nblk calls would each write n^2 and leave nblk - 1 full-size additions to the caller.  Traffic model (elements
 * per matrix): n^2 written, at most one element of G_p read per element and pair whose two weights are non-zero: at most (1 + npairs) n^2, and
 * (1 + 1 / nblk) n^2 distinct (the pairs (k, k') of all k hold n^2 / nblk elements; an orbit re-reads its element in the same rows).
 * trx_sym_fold_pair_bd_backward: the adjoint of ONE trx_sym_fold_pair_bd: the four diagonals gbd [4][batch][N] of T_kl G T_kr^H,
 *   gbd[2p+q][b][m] = rwt[pN+m,kl] G[b][ridx[pN+m,kl] - off[kl], ridx[qN+m,kr] - off[kr]] conj(rwt[qN+m,kr]),   p, q in {0, 1},
 * from G [batch,n_kl,n_kr].  All 4 batch N entries are written, 0 where a weight is 0; a malformed off fills them with NaN.  O(N) work: at most
 * 4 N elements of G read and 4 N written per matrix; the caller sums over pairs.  N <= 16384.
 * All eight: stream-ordered, no host synchronisation, deterministic, no atomics; complex64 and complex128; n^2 < 2^31, batch <= 65535,
 * 1 <= nblk <= 4, else TRX_ERR_ARG (also for kl or kr outside [0, nblk)); batch = 0 returns TRX_OK without touching any buffer.  Element
 * alignment suffices for every buffer but ws. */
size_t trx_sym_fold_ws_bytes(int dtype, int n, int batch);
int trx_sym_fold(int dtype, const void* A, int n, int batch, const int* idx, const void* wt, const int* off, int nblk, void* blocks, double* resid,
                 void* ws, size_t ws_bytes, void* stream);
int trx_sym_unfold(int dtype, const void* Wk, const void* lamk, int n, int batch, const int* idx, const void* wt, const int* off, int nblk, void* W,
                   void* lam, void* stream);
int trx_sym_fold_backward(int dtype, const void* gblocks, int n, int batch, const int* ridx, const void* rwt, const int* off, int nblk, void* gA,
                          void* stream);
int trx_sym_unfold_backward(int dtype, const void* gW, const void* glam, int n, int batch, const int* idx, const void* wt, const int* off, int nblk,
                            void* gWk, void* glamk, void* stream);
int trx_sym_fold_pair(int dtype, const void* M, int n, int batch, const int* idx, const void* wt, const int* off, int nblk, int kl, int kr,
                      void* out, void* stream);
int trx_sym_fold_pair_bd(int dtype, const void* bd, int N, int batch, const int* idx, const void* wt, const int* off, int nblk, int kl, int kr,
                         void* out, void* stream);
int trx_sym_fold_pairs_backward(int dtype, const void* const* G, const int* kl, const int* kr, int npairs, int n, int batch, const int* ridx,
                                const void* rwt, const int* off, int nblk, void* gM, void* stream);
int trx_sym_fold_pair_bd_backward(int dtype, const void* G, int N, int batch, const int* ridx, const void* rwt, const int* off, int nblk, int kl,
                                  int kr, void* gbd, void* stream);

/* ---- thickness sweeps that reuse a layer's modes (no reference counterpart; what modal solvers offer as a layer-thickness scan) ----------------
 * The modes W, kz, V of a layer do not depend on its thickness d, only the diagonal phase X = exp(i omega kz d) does.  With F = Vf^-1 V (the
 * 2x2-block-diagonal Vf^-1 of trx_layer_smatrix), A = W + F, B = W - F, mode amplitudes c+ referenced to the layer's left interface and c- to
 * its right one, the amplitudes in the free-space gaps next to the layer are
 *   left:  f = (A c+ + B X c-)/2,  r = (B c+ + A X c-)/2        right:  f' = (A X c+ + B c-)/2,  r' = (B X c+ + A c-)/2.
 * Lft = the cascade of everything left of the layer (input half-space * earlier layers), Rgt = everything right of it, blocks in the order
 * [S11, S21, S12, S22] as everywhere in this header; R_L = Lft12, R_R = Rgt21.
 * Operands.  Each side is given as (kind, pointer): kind 0 = absent (the identity S-matrix; pointer ignored), 1 = block diagonal: a device
 * array bd [4,4,batch,N] as trx_redheffer_halfspace takes it, 2 = dense: a HOST array of 4 device pointers, each [batch,n,n].
 *
 * trx_thickness_prepare (once per point; nothing in it depends on the thickness):
 *   AB [2,batch,n,n] = A | B;   P_L = A - R_L B,  rhoL = P_L^-1 (R_L A - B);   P_R = A - R_R B,  rhoR = P_R^-1 (R_R A - B)      [batch,n,n]
 *   (the products with R are O(n^2) row combinations for kind 1, one GEMM each for kind 2, absent for kind 0), one LU and an n-column solve per
 *   side; and for the m requested columns e_c, cols: HOST array of m indices in [0, 2N), 1 <= m <= 16, shared by the batch:
 *   src [2,batch,n,m]:  src[0] = P_L^-1 2 Lft11 e_c,  src[1] = Lft21 e_c   (direction 0, forward incidence)
 *                       src[0] = P_R^-1 2 Rgt22 e_c,  src[1] = Rgt12 e_c   (direction 1, backward incidence)
 *   W, V [batch,n,n] (E_eigvec, H_eigvec), vfinv [4,batch,N] as trx_layer_smatrix.  piv: int[batch*n]; info: int[2*batch], slots 0..batch-1 the
 *   LU of P_L, batch..2 batch-1 that of P_R (non-zero: singular, that point's outputs are not finite).  ws: trx_thickness_prepare_ws_bytes = one
 *   [batch,n,n] matrix.  Cost: 2.67 n^3 complex MACs per point (+ 2 n^3 per dense side).  Traffic of the new kernels, elements per point:
 *   A | B: 2 n^2 read (W, V), 2 n^2 written; P and the right-hand side of one side: 2 n^2 read, 2 n^2 written; the columns O(n m).
 *
 * trx_thickness_columns (per chunk of T thicknesses): out[b,t,:,q] = column cols[q] of the block of Lft * layer(d_t) * Rgt that
 *   (direction, port) reads -- port 0 = transmission, 1 = reflection: blocks S11, S21 for direction 0 and S22, S12 for direction 1 -- i.e. what
 *   trx_redheffer_halfspace_columns returns for a stack rebuilt at each thickness.  phase [batch,ldt,n] = exp(i omega kz d_t), |phase| <= 1.
 *   direction 0:  K = I - (rhoL X)(rhoR X),  c+ = K^-1 src[0],  c- = rhoR X c+;   direction 1:  K = I - (rhoR X)(rhoL X),  c- = K^-1 src[0],
 *   c+ = rhoL X c-;   transmission = Rgt11 f' (direction 0) / Lft22 r (1);   reflection = src[1] + Lft22 r (0) / src[1] + Rgt11 f' (1).
 *   Per (point, thickness): X rho X and K = I in one elementwise pass (rho read once per point for all T), one GEMM with the other rho shared
 *   over t (batch stride 0), one LU of K, an m-column solve, skinny products: 1.33 n^3 complex MACs.  direction, m and the operands must be
 *   those of the prepare call.  ldt >= T: the leading dimension of the thickness axis of phase, out [batch,ldt,n,m] and info [batch,ldt], so a
 *   caller that chunks T passes pointers offset by t0 (phase + t0 n, out + t0 n m, info + t0) and the arrays' full T as ldt.
 *   info[b,t]: the LU of K (non-zero: singular K, that entry's columns are not finite).  piv: int[batch*T*(n+1)] scratch.
 *   ws: trx_thickness_columns_ws_bytes = batch T (2 n^2 + 5 n m) elements; it scales with T: the caller chunks T.  batch * T <= 65535.
 *   Traffic of the new kernels, elements: K assembly n^2 read per point, 2 n^2 written per (point, thickness); the skinny products read their
 *   one or two n x n matrices ceil(T m / 8) times per point; everything else is O(n m) per (point, thickness).
 * trx_thickness_columns_keep: trx_thickness_columns, same arguments, results and bits, that also stores the solved amplitude (c+ for direction 0,
 *   c- for direction 1) in cp [batch,ldt,n,m], laid out like out.  It is the one forward intermediate the adjoint needs.
 *
 * trx_thickness_columns_backward (per chunk of T thicknesses): the adjoint of trx_thickness_columns in PyTorch's convention for holomorphic
 *   functions (for C = A B: gA = G B^H, gB = A^H G), no atomics: every gradient element has one writer and a fixed summation order, so a
 *   repeated call gives the same bits.  gout [batch,ldt,n,m]: the incoming gradient of out; cp: as trx_thickness_columns_keep stored it.
 *   Outputs, each optional (null: not wanted, its work is skipped; all null: nothing at all is written):
 *     grhoL, grhoR [batch,n,n];  gsrc [2,batch,n,m] (of src[0] and src[1]; src[1] takes a gradient from the reflection port only, zero otherwise);
 *     gAB [2,batch,n,n];  gphase [batch,ldt,n] (written, never accumulated: a thickness belongs to one chunk);  gop: the gradient of the ONE
 *     block of the output-side operand that the forward multiplies with (Rgt11 or Lft22): [batch,n,n] for a dense operand, its four diagonals
 *     [4,batch,N] for a block-diagonal one, ignored for an absent one.
 *   accumulate = 1 adds to grhoL, grhoR, gsrc, gAB and gop instead of overwriting them (the second and later chunks of the thickness axis).
 *   With X = diag(phase_t), rho_A / rho_B = rhoL / rhoR (direction 0) or rhoR / rhoL (1), O the output block, per thickness (recomputed:
 *   u = X cp, cs = rho_B u, w = X cs):
 *     g~ = O^H gout (gout without O);  gO += gout g^H, g the forward's column before O;  reflection: gsrc[1] += gout
 *     transmission: u~ = A^H g~/2, cs~ = B^H g~/2, gA += g~ u^H/2, gB += g~ cs^H/2, cp~ = 0
 *     reflection:   cp~ = B^H g~/2, w~ = A^H g~/2, gB += g~ cp^H/2, gA += g~ w^H/2, cs~ = conj(x) w~, gx += sum_q w~ conj(cs), u~ = 0
 *     grho_B += cs~ u^H;  u~ += rho_B^H cs~;  gx += sum_q u~ conj(cp);  cp~ += conj(x) u~
 *     lambda = K^-H cp~ (K^H = I - (X rho_B X)^H rho_A^H: one GEMM and one LU, the forward's 1.33 n^3 again);  gsrc[0] += lambda
 *     grho_A += lambda w^H;  mu = rho_A^H lambda;  grho_B += (conj(x) mu) u^H;  gx += sum_q mu conj(cs) + conj(cp) (rho_B^H (conj(x) mu))
 *   info[b,t] (leading dimension ldt): the LU of K^H, written when a gradient that needs the solve is wanted (grhoL, grhoR, gsrc, gphase).
 *   piv: int[batch*T*(n+1)] scratch.  ws: trx_thickness_columns_backward_ws_bytes = batch T (2 n^2 + 15 n m) elements.  Validation as
 *   trx_thickness_columns; accumulate must be 0 or 1.
 * All: stream-ordered, no host synchronisation; complex64 and complex128; batch <= 65535; batch = 0 (and T = 0) returns TRX_OK without touching
 * any buffer; TRX_ERR_ARG for a kind, direction, port, column index or m out of range or a missing pointer, TRX_ERR_WORKSPACE for a short ws. */
size_t trx_thickness_prepare_ws_bytes(int dtype, int N, int batch);
int trx_thickness_prepare(int dtype, const void* W, const void* V, const void* vfinv, int left_kind, const void* left, int right_kind,
                          const void* right, int direction, const int* cols, int m, int N, int batch, void* rhoL, void* rhoR, void* src, void* AB,
                          int* piv, int* info, void* ws, size_t ws_bytes, void* stream);
size_t trx_thickness_columns_ws_bytes(int dtype, int N, int batch, int T, int m);
int trx_thickness_columns(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T,
                          int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch,
                          void* out, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);
int trx_thickness_columns_keep(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T,
                               int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch,
                               void* out, void* cp, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);
size_t trx_thickness_columns_backward_ws_bytes(int dtype, int N, int batch, int T, int m);
int trx_thickness_columns_backward(int dtype, const void* rhoL, const void* rhoR, const void* AB, const void* phase, int ldt, int T, int direction,
                                   int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch,
                                   const void* cp, const void* gout, void* grhoL, void* grhoR, void* gsrc, void* gAB, void* gphase, void* gop,
                                   int accumulate, int* piv, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- measurement aid (no reference counterpart): HIP-event timing of the dominant kernels --------------------
 * trx_prof_enable(1) makes the instrumented launch sites record hipEvents on the launch stream.  Sampling is systematic and
 * uniform over the run: every stride-th launch of a tag is timed; when the pool (2048 event pairs per tag) is full every
 * other sample is dropped and the stride doubles.  trx_prof_get(tag, out[7]) waits for those events and returns
 * {launches, timed_launches, algorithmic flops of the timed launches, algorithmic bytes of the timed launches,
 * milliseconds of the timed launches, flops of ALL launches, bytes of ALL launches} (the last two are exact sums, not samples).  Tags: 0 gemm N,N; 1 gemm other ops; 2 QR prepare (AED);
 * 3 QR off-window update; 4 QR window chase; 5 Hessenberg gemv; 6 Hessenberg reflector column; 7 LU panel; 8 - 15 see trx_prof_tag_name;
 * 16 trx_sym_fold (both passes); 17 trx_sym_unfold (zero fill and scatter); 18 trx_thickness_prepare (whole call); 19 - 21 the stages of
 * trx_thickness_columns, one event pair per call each: 19 K assembly and its GEMMs, 20 LU of K and the column solve, 21 amplitudes and read-out;
 * 22 trx_sym_fold_backward; 23 trx_sym_unfold_backward; 24 trx_sym_fold_pair; 25 trx_sym_fold_pair_bd; 26 trx_sym_fold_pairs_backward;
 * 27 trx_sym_fold_pair_bd_backward; 28 trx_thickness_columns_backward (whole call). */
int trx_prof_enable(int on);
int trx_prof_reset(void);
int trx_prof_get(int tag, double* out);
const char* trx_prof_tag_name(int tag);

#ifdef __cplusplus
}
#endif
#endif /* TRX_H_ */
