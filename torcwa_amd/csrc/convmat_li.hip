// Fourier factorisation (Li's inverse rule, L. Li, JOSA A 13, 1870 (1996); 14, 2758 (1997)): permittivity grid -> the two
// convolution matrices E_x (multiplies Ex) and E_y (multiplies Ey) of a patterned layer with axis-aligned discontinuities.
//
//   E_x: inverse rule along x, Laurent along y.  Per grid row y:  a_y[p] = (1/nx) sum_x g[x,y]^-1 e^{-2 pi i p x / nx},  p in [-2ox, 2ox];
//        T_y[m,m'] = a_y[m-m'],  U_y = T_y^-1 ((2ox+1)^2);  F[m,m',q] = (1/ny) sum_y U_y[m,m'] e^{-2 pi i q y / ny};
//        E_x[(m,n),(m',n')] = F[m,m',n-n'].
//   E_y: the mirror image (y-DFT of 1/g per x, (2oy+1)^2 inverses V_x, x-DFT of V_x):  E_y[(m,n),(m',n')] = G[n,n',m-m'].
//
// Pipeline (all arithmetic in fp64 for both dtypes, as convmat.hip; exact integer phase reduction of every twiddle):
//   1. pruned DFTs of 1/g: along y per x (contiguous rows through LDS) and along x per y (lanes over y: coalesced rows of the grid);
//      a zero grid value sets info[b] = 1;
//   2. batched small Toeplitz inverses: one workgroup per matrix, in-place Gauss-Jordan with partial pivoting, the matrix held in LDS
//      (w^2 x 16 B: 105 KB at w = 81, the large-LDS opt-in of common.hpp); a zero pivot sets info[b] = 2;
//   3. the transform of U along the other axis as the library's batched GEMM  F_b = U_b^T W  ([w^2, ny] x [ny, 4o'+1]), accumulated
//      over chunks of rows when the caller does not keep U (the chunk bounds the workspace);
//   4. scatter of F, G into E_x, E_y [B,N,N] in the compute dtype.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace trx {
namespace {

typedef cx<double> zc;

constexpr size_t LI_LDS_MAX = 160 * 1024;         // gfx950: 160 KiB of LDS per CU

// LDS of one Toeplitz inverse of size w: the matrix, its pivot column, the pivot record and the pivot of the current step
static inline size_t toeplitz_lds_bytes(int w) { return sizeof(cx<double>) * (size_t)(w * w + w) + sizeof(int) * (size_t)(w + 1); }

template <class T, bool CPLX>
__device__ __forceinline__ zc recip_at(const T* g, long e, int* info_b) {
    const zc v = CPLX ? zc((double)g[2 * e], (double)g[2 * e + 1]) : zc((double)g[e], 0.0);
    if (v.x == 0.0 && v.y == 0.0) *info_b = 1;
    return crecip(v);
}

// ax[b, x, q] = (1/ny) sum_y g[b,x,y]^-1 exp(-2 pi i (q-2oy) y / ny)      (one workgroup per grid row x: contiguous reads)
template <class T, bool CPLX>
__global__ __launch_bounds__(128) void recip_dft_y_kernel(const T* __restrict__ grid, int nx, int ny, int oy, zc* __restrict__ ax,
                                                          int* __restrict__ info) {
    TRX_DYN_SMEM(smem);
    zc* tw = reinterpret_cast<zc*>(smem);          // [ny]
    zc* row = tw + ny;                             // [ny]
    const int x = blockIdx.x, b = blockIdx.y;
    const int nq = 4 * oy + 1;
    const T* g = grid + ((long)b * nx + x) * (long)ny * (CPLX ? 2 : 1);
    for (int y = threadIdx.x; y < ny; y += blockDim.x) {
        double s, c;
        sincospi(-2.0 * (double)y / (double)ny, &s, &c);
        tw[y] = zc(c, s);
        row[y] = recip_at<T, CPLX>(g, y, info + b);
    }
    __syncthreads();
    const double scale = 1.0 / (double)ny;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        int step = (q - 2 * oy) % ny;
        if (step < 0) step += ny;
        zc acc(0.0, 0.0);
        int idx = 0;
        for (int y = 0; y < ny; ++y) {
            cfma(acc, row[y], tw[idx]);
            idx += step;
            if (idx >= ny) idx -= ny;
        }
        ax[((long)b * nx + x) * nq + q] = scale * acc;
    }
}

// ay[b, y, p] = (1/nx) sum_x g[b,x,y]^-1 exp(-2 pi i (p-2ox) x / nx).  256 threads = 4 waves; lane = y (64 consecutive grid columns, so
// every load of the x loop is one coalesced row segment), wave = one of 4 consecutive p.
template <class T, bool CPLX>
__global__ __launch_bounds__(256) void recip_dft_x_kernel(const T* __restrict__ grid, int nx, int ny, int ox, zc* __restrict__ ay) {
    TRX_DYN_SMEM(smem);
    zc* tw = reinterpret_cast<zc*>(smem);          // [nx]
    const int b = blockIdx.z;
    const int np = 4 * ox + 1;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        double s, c;
        sincospi(-2.0 * (double)x / (double)nx, &s, &c);
        tw[x] = zc(c, s);
    }
    __syncthreads();
    const int y = blockIdx.x * 64 + (threadIdx.x & 63);
    const int p = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= ny || p >= np) return;
    const T* g = grid + (long)b * nx * (long)ny * (CPLX ? 2 : 1);
    int step = (p - 2 * ox) % nx;
    if (step < 0) step += nx;
    int dummy = 0;                                 // zero values are reported by recip_dft_y_kernel, which visits every element once
    zc acc(0.0, 0.0);
    int idx = 0;
    for (int x = 0; x < nx; ++x) {
        cfma(acc, recip_at<T, CPLX>(g, (long)x * ny + y, &dummy), tw[idx]);
        idx += step;
        if (idx >= nx) idx -= nx;
    }
    ay[((long)b * ny + y) * np + p] = (1.0 / (double)nx) * acc;
}

// U[b, r-r0] = inverse of the w x w Toeplitz matrix T[m,m'] = coef[b, r, m-m'+w-1] (w = 2o+1, coef has 2w-1 = 4o+1 entries per row).
// One workgroup per matrix; in-place Gauss-Jordan with row interchanges (partial pivoting on |re|+|im|), undone as column interchanges
// in reverse order at the end.  LDS: the matrix, its pivot column and the pivot record.
__global__ __launch_bounds__(256) void toeplitz_inv_kernel(const zc* __restrict__ coef, int nrows, int r0, int w, zc* __restrict__ U,
                                                           long u_bstride, int* __restrict__ info) {
    TRX_DYN_SMEM(smem);
    zc* A = reinterpret_cast<zc*>(smem);           // [w*w]
    zc* colk = A + w * w;                          // [w]
    int* piv = reinterpret_cast<int*>(colk + w);   // [w]
    int& s_p = piv[w];
    const int r = r0 + blockIdx.x, b = blockIdx.y;
    const int ww = w * w, nc = 2 * w - 1, tid = threadIdx.x, nt = blockDim.x;
    const zc* c = coef + ((long)b * nrows + r) * nc;
    for (int e = tid; e < ww; e += nt) {
        const int i = e / w, j = e - i * w;
        A[e] = c[i - j + w - 1];
    }
    __syncthreads();
    bool singular = false;
    for (int k = 0; k < w; ++k) {
        if (tid < 64) {                            // pivot search: wave 0, lanes over rows k..w-1
            double best = -1.0;
            int bi = k;
            for (int i = k + tid; i < w; i += 64) {
                const double v = abs1(A[i * w + k]);
                if (v > best) { best = v; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (tid == 0) {
                s_p = best > 0.0 ? bi : -1;
                piv[k] = best > 0.0 ? bi : k;
            }
        }
        __syncthreads();
        const int p = s_p;
        if (p < 0) { singular = true; break; }     // uniform: every thread reads the same s_p
        if (p != k)
            for (int j = tid; j < w; j += nt) { const zc t = A[k * w + j]; A[k * w + j] = A[p * w + j]; A[p * w + j] = t; }
        __syncthreads();
        const zc d = crecip(A[k * w + k]);
        for (int i = tid; i < w; i += nt) colk[i] = A[i * w + k];
        __syncthreads();
        for (int j = tid; j < w; j += nt) A[k * w + j] = (j == k ? zc(1.0, 0.0) : A[k * w + j]) * d;
        __syncthreads();
        for (int e = tid; e < ww; e += nt) {
            const int i = e / w, j = e - i * w;
            if (i == k) continue;
            zc v = j == k ? zc(0.0, 0.0) : A[e];
            v -= colk[i] * A[k * w + j];
            A[e] = v;
        }
        __syncthreads();
    }
    if (singular) {                                // a zero grid value (info 1, set by recip_dft_y_kernel before) makes its row's block NaN,
        if (tid == 0 && info[b] == 0) info[b] = 2; // which ends here too: the cause stays on record.  Benign race: the workgroups of
                                                   // one b all store the same 2, and only over 0
        return;
    }
    for (int k = w - 1; k >= 0; --k) {             // A^-1 = (P A)^-1 P: the row interchanges become column interchanges
        const int p = piv[k];
        if (p != k)
            for (int i = tid; i < w; i += nt) { const zc t = A[i * w + k]; A[i * w + k] = A[i * w + p]; A[i * w + p] = t; }
        __syncthreads();
    }
    zc* u = U + (long)b * u_bstride + (long)blockIdx.x * ww;
    for (int e = tid; e < ww; e += nt) u[e] = A[e];
}

// W[r, q] = (1/n) exp(-2 pi i (q-2o) r / n),  r in [0,n), q in [0, 4o+1)
__global__ __launch_bounds__(256) void twiddle_kernel(int n, int o, zc* __restrict__ W) {
    const int nq = 4 * o + 1;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)n * nq) return;
    const int r = (int)(e / nq), q = (int)(e - (long)r * nq);
    long idx = ((long)(q - 2 * o) * r) % n;
    if (idx < 0) idx += n;
    double s, c;
    sincospi(-2.0 * (double)idx / (double)n, &s, &c);
    W[e] = zc(c / n, s / n);
}

// Ex[b,i,j] = F[b, m_i, m_j, n_i-n_j+2oy],  Ey[b,i,j] = G[b, n_i, n_j, m_i-m_j+2ox],  i = (m+ox)(2oy+1) + (n+oy)
template <class T>
__global__ __launch_bounds__(256) void li_scatter_kernel(const zc* __restrict__ F, const zc* __restrict__ G, int ox, int oy,
                                                         cx<T>* __restrict__ Ex, cx<T>* __restrict__ Ey) {
    const int b = blockIdx.z;
    const int wx = 2 * ox + 1, wy = 2 * oy + 1, N = wx * wy;
    const int nq = 4 * oy + 1, np = 4 * ox + 1;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= N) return;
    const int mi = i / wy, ni = i - mi * wy;
    const int mj = j / wy, nj = j - mj * wy;
    const zc f = F[(((long)b * wx + mi) * wx + mj) * nq + (ni - nj + 2 * oy)];
    const zc g = G[(((long)b * wy + ni) * wy + nj) * np + (mi - mj + 2 * ox)];
    const long o = ((long)b * N + i) * N + j;
    Ex[o] = cx<T>((T)f.x, (T)f.y);
    Ey[o] = cx<T>((T)g.x, (T)g.y);
}

struct LiLayout {                    // workspace carving of trx_convmat_li (element counts of zc)
    long ay, ax, wy_tw, wx_tw, F, G, U;
    int rc_y, rc_x;                  // rows per chunk of the Toeplitz inverses when U is not an output
};

LiLayout li_layout(int batch, int nx, int ny, int ox, int oy) {
    LiLayout L;
    const long wx = 2 * ox + 1, wy = 2 * oy + 1, np = 4 * ox + 1, nq = 4 * oy + 1, N = wx * wy;
    L.ay = (long)batch * ny * np;
    L.ax = (long)batch * nx * nq;
    L.wy_tw = (long)ny * nq;
    L.wx_tw = (long)nx * np;
    L.F = (long)batch * wx * wx * nq;
    L.G = (long)batch * wy * wy * np;
    // chunk of rows whose inverses are held at once: at most one complex64 output's size (B N^2 x 8 B), at least one row.  The same for
    // both dtypes: the chunks fix the order of the fp64 accumulation, and a complex64 call must return the rounded complex128 result.
    const long cap = N * N / 2;
    L.rc_y = (int)std::max(1L, std::min((long)ny, cap / (wx * wx)));
    L.rc_x = (int)std::max(1L, std::min((long)nx, cap / (wy * wy)));
    L.U = (long)batch * std::max((long)L.rc_y * wx * wx, (long)L.rc_x * wy * wy);
    return L;
}

// One direction: coef [B, nrows, 4o+1] -> Toeplitz inverses (w = 2o+1) per row -> Out[b] = sum_r U_r^T Wtw[r, :]  ([w^2, 4o'+1]).
// Wtw: [nrows, nq2] shared by the batch (w_bstride = 0: the twiddles of a grid) or one table per point (the strip weights of a shape list).
int li_direction(hipStream_t s, const zc* coef, int nrows, int w, const zc* Wtw, long w_bstride, int nq2, int batch, zc* Ukeep, zc* Uws, int rc,
                 zc* Out, int* info) {
    const long ww = (long)w * w;
    const size_t lds = toeplitz_lds_bytes(w);
    if (set_max_dyn_smem((const void*)toeplitz_inv_kernel, lds)) return TRX_ERR_LAUNCH;
    const zc one(1.0, 0.0), zero(0.0, 0.0);
    if (Ukeep) {                     // the caller keeps every inverse (adjoint): one pass, U in place
        TRX_LAUNCH(toeplitz_inv_kernel, dim3(nrows, batch), dim3(256), lds, s, coef, nrows, 0, w, Ukeep, (long)nrows * ww, info);
        TRX_CHECK_LAUNCH();
        return gemm<double>(s, TRX_OP_T, TRX_OP_N, (int)ww, nq2, nrows, one, Ukeep, (int)ww, (long)nrows * ww, Wtw, nq2, w_bstride, zero, Out,
                            nq2, ww * nq2, batch);
    }
    for (int r0 = 0; r0 < nrows; r0 += rc) {
        const int rn = std::min(rc, nrows - r0);
        TRX_LAUNCH(toeplitz_inv_kernel, dim3(rn, batch), dim3(256), lds, s, coef, nrows, r0, w, Uws, (long)rn * ww, info);
        TRX_CHECK_LAUNCH();
        int rc2 = gemm<double>(s, TRX_OP_T, TRX_OP_N, (int)ww, nq2, rn, one, Uws, (int)ww, (long)rn * ww, Wtw + (long)r0 * nq2, nq2,
                               w_bstride, r0 == 0 ? zero : one, Out, nq2, ww * nq2, batch);
        if (rc2) return rc2;
    }
    return TRX_OK;
}

template <class T>
int convmat_li_t(int cplx, const void* grid, int batch, int nx, int ny, int ox, int oy, void* Ex, void* Ey, void* Ux, void* Uy, int* info,
                 void* ws, hipStream_t s) {
    const LiLayout L = li_layout(batch, nx, ny, ox, oy);
    zc* ay = reinterpret_cast<zc*>(ws);
    zc* ax = ay + L.ay;
    zc* twy = ax + L.ax;
    zc* twx = twy + L.wy_tw;
    zc* F = twx + L.wx_tw;
    zc* G = F + L.F;
    zc* Uw = G + L.G;
    const int wx = 2 * ox + 1, wy = 2 * oy + 1, np = 4 * ox + 1, nq = 4 * oy + 1, N = wx * wy;
    if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s) != hipSuccess) return TRX_ERR_LAUNCH;
    const size_t sm1 = sizeof(zc) * 2 * (size_t)ny, sm2 = sizeof(zc) * (size_t)nx;
    if (cplx) {
        TRX_LAUNCH((recip_dft_y_kernel<T, true>), dim3(nx, batch), dim3(128), sm1, s, (const T*)grid, nx, ny, oy, ax, info);
        TRX_LAUNCH((recip_dft_x_kernel<T, true>), dim3(cdiv_i(ny, 64), cdiv_i(np, 4), batch), dim3(256), sm2, s, (const T*)grid, nx, ny, ox, ay);
    } else {
        TRX_LAUNCH((recip_dft_y_kernel<T, false>), dim3(nx, batch), dim3(128), sm1, s, (const T*)grid, nx, ny, oy, ax, info);
        TRX_LAUNCH((recip_dft_x_kernel<T, false>), dim3(cdiv_i(ny, 64), cdiv_i(np, 4), batch), dim3(256), sm2, s, (const T*)grid, nx, ny, ox, ay);
    }
    TRX_LAUNCH(twiddle_kernel, dim3(cdiv_i((long)ny * nq, 256)), dim3(256), 0, s, ny, oy, twy);
    TRX_LAUNCH(twiddle_kernel, dim3(cdiv_i((long)nx * np, 256)), dim3(256), 0, s, nx, ox, twx);
    TRX_CHECK_LAUNCH();
    // E_x: inverses of the x-Toeplitz blocks per grid row y, transformed along y
    int rc = li_direction(s, ay, ny, wx, twy, 0, nq, batch, (zc*)Uy, Uw, L.rc_y, F, info);
    if (rc) return rc;
    // E_y: inverses of the y-Toeplitz blocks per grid row x, transformed along x
    rc = li_direction(s, ax, nx, wy, twx, 0, np, batch, (zc*)Ux, Uw, L.rc_x, G, info);
    if (rc) return rc;
    TRX_LAUNCH((li_scatter_kernel<T>), dim3(cdiv_i(N, 256), N, batch), dim3(256), 0, s, (const zc*)F, (const zc*)G, ox, oy, (cx<T>*)Ex,
               (cx<T>*)Ey);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// ---- Li's rule for a list of axis-aligned rectangles, in closed form ---------------------------------------------------------------------
// 1/eps = rval[0] + sum_s rval[s+1] chi_s is piecewise constant along y: the cell splits into K = 2S + 1 horizontal strips between 0 and the
// y-edges of the rectangles.  In strip k the x-coefficients of 1/eps are a_k[p] = rval[0] delta_p0 + sum_{s active in k} rval[s+1] (Wx/Lx)
// sinc(pi p Wx/Lx) e^{-2 pi i p Cx/Lx}, and the y-transform of the strip's indicator is w_k[q] = (h_k/Ly) sinc(pi q h_k/Ly) e^{-2 pi i q y_k/Ly}:
// the strips stand where the grid rows of trx_convmat_li stand and the weights where its twiddles stand.  E_y: the same with x and y exchanged.
// Direction d = 0: strips along y, coefficients along x (E_x);  d = 1: the mirror image (E_y).
//
// Events of one direction: index 0 the origin, 1 + 2s the lower edge of rectangle s (it opens), 2 + 2s its upper edge (it closes), each
// reduced into the cell; a rectangle that crosses the cell boundary is active at 0+ (wraps = 1) and closes before it opens.  Each thread
// counts the events that sort before its own (ties by index): a rank sort without a data-dependent loop.  Rectangle s is active in strip k
// iff [rank(open) <= k] xor [rank(close) <= k] xor wraps: a strip of zero height carries weight 0 and the state of the one-sided limit.
constexpr int LS_BLOCK = 256;
constexpr int LS_SMAX = 127;                       // K = 2S + 1 <= 255 events: one workgroup sorts a point's events

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ double sincpi_f(double x) {           // sin(pi x) / (pi x)
    if (x == 0.0) return 1.0;
    double s, c;
    sincospi(x, &s, &c);
    return s / (M_PI * x);
}
__device__ __forceinline__ zc expm2pi(double x) {                // e^{-2 pi i x}
    double s, c;
    sincospi(-2.0 * x, &s, &c);
    return zc(c, s);
}
__device__ __forceinline__ bool strip_active(const int* rk, int s, int k) { return ((rk[3 * s] <= k) != (rk[3 * s + 1] <= k)) != (rk[3 * s + 2] != 0); }

// grid (2, batch).  coef[d]: [B, K, 4 o_c + 1] (the rows of toeplitz_inv_kernel), wgt[d]: [B, K, 4 o_s + 1] with o_c / o_s the order along the
// coefficient / strip axis of direction d.  brk [B, 2, K + 1] and rec [B, 2, 3 S] (rank of open, rank of close, wraps) may be NULL.
__global__ __launch_bounds__(LS_BLOCK) void li_strips_kernel(const int* __restrict__ voff, int S, const double* __restrict__ par, int npar,
                                                             const zc* __restrict__ rval, double Lx, double Ly, int ox, int oy,
                                                             zc* __restrict__ coef0, zc* __restrict__ coef1, zc* __restrict__ wgt0,
                                                             zc* __restrict__ wgt1, double* __restrict__ brk, int* __restrict__ rec,
                                                             int* __restrict__ info) {
    __shared__ double pos[2 * LS_SMAX + 2], srt[2 * LS_SMAX + 2], cw[LS_SMAX], cc[LS_SMAX];
    __shared__ zc rv[LS_SMAX];
    __shared__ int rk[3 * LS_SMAX], flag[2];
    const int d = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = 2 * S + 1;
    const double Ls = d == 0 ? Ly : Lx, Lc = d == 0 ? Lx : Ly;   // period along the strip axis / the coefficient axis
    const int oc = d == 0 ? ox : oy, os = d == 0 ? oy : ox;
    const int nc = 4 * oc + 1, nw = 4 * os + 1;
    const double* pr = par + (long)b * npar;
    const zc* rvb = rval + (long)b * (S + 1);
    if (tid == 0) { flag[0] = 0; flag[1] = 0; pos[0] = 0.0; }
    if (tid <= K) srt[tid] = tid == K ? Ls : 0.0;
    __syncthreads();
    if (tid < S) {
        const double* q = pr + voff[tid];
        const double ws = q[d == 0 ? 1 : 0], cs = q[d == 0 ? 3 : 2];
        cw[tid] = q[d == 0 ? 0 : 1];
        cc[tid] = q[d == 0 ? 2 : 3];
        const zc r = rvb[tid + 1];
        rv[tid] = r;
        double lo = cs - 0.5 * ws;
        lo -= floor(lo / Ls) * Ls;
        if (lo >= Ls) lo -= Ls;                    // a tiny negative edge rounds to the period itself
        if (lo < 0.0) lo = 0.0;
        const double hi = lo + ws;
        const int wraps = hi > Ls;                 // an edge exactly on the cell boundary stays at Ls
        pos[1 + 2 * tid] = lo;
        pos[2 + 2 * tid] = wraps ? hi - Ls : hi;
        rk[3 * tid + 2] = wraps;
        if (!finite_d(r.x) || !finite_d(r.y)) flag[0] = 1;        // benign race: every writer stores the same 1
        if (!(q[4] == 0.0) || !(q[0] > 0.0) || !(q[1] > 0.0) || !(q[0] <= Lx) || !(q[1] <= Ly) || !finite_d(q[2]) || !finite_d(q[3])) flag[1] = 1;
    }
    if (tid == S) {
        const zc r = rvb[0];
        if (!finite_d(r.x) || !finite_d(r.y) || (r.x == 0.0 && r.y == 0.0)) flag[0] = 1;
    }
    __syncthreads();
    if (tid < K) {
        const double mine = pos[tid];
        int r = 0;
        for (int e = 0; e < K; ++e) {
            const double o = pos[e];
            r += (o < mine || (o == mine && e < tid)) ? 1 : 0;
        }
        srt[r] = mine;
        if (tid > 0) rk[3 * ((tid - 1) >> 1) + ((tid - 1) & 1)] = r;
    }
    __syncthreads();
    zc* a = (d == 0 ? coef0 : coef1) + (long)b * K * nc;
    for (int e = tid; e < K * nc; e += LS_BLOCK) {
        const int k = e / nc, p = e - k * nc - 2 * oc;
        zc acc = p == 0 ? rvb[0] : zc(0.0, 0.0);
        for (int s = 0; s < S; ++s) {
            if (!strip_active(rk, s, k)) continue;
            const double f = cw[s] / Lc;
            cfma(acc, rv[s], (f * sincpi_f(p * f)) * expm2pi(p * cc[s] / Lc));
        }
        a[e] = acc;
    }
    zc* wg = (d == 0 ? wgt0 : wgt1) + (long)b * K * nw;
    for (int e = tid; e < K * nw; e += LS_BLOCK) {
        const int k = e / nw, q = e - k * nw - 2 * os;
        const double f = (srt[k + 1] - srt[k]) / Ls, mid = 0.5 * (srt[k] + srt[k + 1]);
        wg[e] = (f * sincpi_f(q * f)) * expm2pi(q * mid / Ls);
    }
    if (brk && tid <= K) brk[((long)b * 2 + d) * (K + 1) + tid] = srt[tid];
    if (rec)
        for (int e = tid; e < 3 * S; e += LS_BLOCK) rec[((long)b * 2 + d) * 3 * S + e] = rk[e];
    if (d == 0 && tid == 0) {                      // both directions see the same list: one of them reports
        const int code = flag[1] ? 3 : flag[0] ? 1 : 0;
        if (code) info[b] = code;
    }
}

__device__ __forceinline__ zc ls_block_sum(zc v, zc* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = LS_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

// Adjoint of li_strips_kernel.  grid (npar + S + 1, batch): item w < npar is par[b, w], w = npar is rval[b, 0], w = npar + 1 + s is
// rval[b, s + 1].  ga[d] / gw[d]: the adjoints of coef[d] / wgt[d].  A width or centre along axis c gets the coefficient part from the
// direction whose coefficients run along c (d = c) and the breakpoint part from the other one: with w_k[q] = (1/L) int_strip e^{-2 pi i q t/L} dt,
// d w_{r-1} / d t_r = -d w_r / d t_r = e^{-2 pi i q t_r / L} / L at the breakpoint of rank r.
__global__ __launch_bounds__(LS_BLOCK) void li_strips_backward_kernel(const int* __restrict__ voff, int S, const double* __restrict__ par, int npar,
                                                                      const zc* __restrict__ rval, double Lx, double Ly, int ox, int oy,
                                                                      const double* __restrict__ brk, const int* __restrict__ rec,
                                                                      const zc* __restrict__ ga0, const zc* __restrict__ gw0,
                                                                      const zc* __restrict__ ga1, const zc* __restrict__ gw1,
                                                                      double* __restrict__ gpar, zc* __restrict__ grval) {
    __shared__ zc red[LS_BLOCK];
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = 2 * S + 1;
    const double* pr = par + (long)b * npar;
    zc acc(0.0, 0.0);
    if (w >= npar) {                               // a value: grval = sum conj(d a / d rval) ga over both directions
        const int s = w - npar - 1;
        for (int d = 0; d < 2; ++d) {
            const int oc = d == 0 ? ox : oy, nc = 4 * oc + 1;
            const zc* ga = (d == 0 ? ga0 : ga1) + (long)b * K * nc;
            const int* rk = rec + ((long)b * 2 + d) * 3 * S;
            if (s < 0) {
                for (int k = tid; k < K; k += LS_BLOCK) acc += ga[k * nc + 2 * oc];
                continue;
            }
            const double* q = pr + voff[s];
            const double Lc = d == 0 ? Lx : Ly, f = q[d] / Lc, c = q[2 + d];
            for (int e = tid; e < K * nc; e += LS_BLOCK) {
                const int k = e / nc, p = e - k * nc - 2 * oc;
                if (!strip_active(rk, s, k)) continue;
                cfma_conj(acc, (f * sincpi_f(p * f)) * expm2pi(p * c / Lc), ga[e]);
            }
        }
        const zc tot = ls_block_sum(acc, red);
        if (tid == 0) grval[(long)b * (S + 1) + s + 1] = tot;
        return;
    }
    int s = -1;
    for (int t = 0; t < S; ++t)
        if (w >= voff[t] && w < voff[t + 1]) s = t;
    const int j = s < 0 ? 4 : w - voff[s];
    if (j >= 4) {                                  // theta, or a slot of the row that belongs to no shape
        if (tid == 0) gpar[(long)b * npar + w] = 0.0;
        return;
    }
    const int c = j & 1;                           // the axis the parameter lies along; j < 2: a width, else a centre
    const bool width = j < 2;
    const int o = c == 0 ? ox : oy, n = 4 * o + 1;
    const double L = c == 0 ? Lx : Ly;
    const double* q = pr + voff[s];
    const zc delta = rval[(long)b * (S + 1) + s + 1];
    {                                              // coefficients along c: direction c
        const zc* ga = (c == 0 ? ga0 : ga1) + (long)b * K * n;
        const int* rk = rec + ((long)b * 2 + c) * 3 * S;
        const double f = q[c] / L, ctr = q[2 + c];
        for (int e = tid; e < K * n; e += LS_BLOCK) {
            const int k = e / n, p = e - k * n - 2 * o;
            if (!strip_active(rk, s, k)) continue;
            const zc ph = expm2pi(p * ctr / L);
            zc dv;
            if (width) {
                double sn, cs;
                sincospi(p * f, &sn, &cs);
                dv = (cs / L) * ph;                // d(W/L sinc(pi p W/L)) / dW = cos(pi p W/L) / L
            } else {
                const zc v = (f * sincpi_f(p * f)) * ph;
                const double g = 2.0 * M_PI * p / L;
                dv = zc(g * v.y, -g * v.x);        // -2 pi i p / L times the term
            }
            dv = delta * dv;
            acc.x += ga[e].x * dv.x + ga[e].y * dv.y;            // Re(conj(ga) d a / d par)
        }
    }
    {                                              // breakpoints along c: the other direction
        const int d = 1 - c;
        const zc* gw = (d == 0 ? gw0 : gw1) + (long)b * K * n;
        const int* rk = rec + ((long)b * 2 + d) * 3 * S;
        const double* t = brk + ((long)b * 2 + d) * (K + 1);
        for (int e = tid; e < 2 * n; e += LS_BLOCK) {
            const int edge = e / n, qq = e - edge * n - 2 * o;
            int r = rk[3 * s + edge];              // 1 .. 2S: the strips r - 1 and r meet at this breakpoint
            r = r < 1 ? 1 : r > 2 * S ? 2 * S : r; // (a record of a refused point stays inside the tables)
            const double sign = !width ? 1.0 : edge == 0 ? -0.5 : 0.5;
            const zc ph = expm2pi(qq * t[r] / L);
            const zc g = gw[(r - 1) * n + qq + 2 * o] - gw[r * n + qq + 2 * o];
            acc.x += sign / L * (g.x * ph.x + g.y * ph.y);
        }
    }
    const zc tot = ls_block_sum(acc, red);
    if (tid == 0) gpar[(long)b * npar + w] = tot.x;
}

struct LiShapesLayout {              // workspace carving of trx_convmat_li_shapes (element counts of zc)
    long coef0, coef1, wgt0, wgt1, F, G, U;
    int rc0, rc1;                    // strips per chunk of the Toeplitz inverses when U is not an output
};

LiShapesLayout li_shapes_layout(int batch, int S, int ox, int oy) {
    LiShapesLayout L;
    const long K = 2 * S + 1, wx = 2 * ox + 1, wy = 2 * oy + 1, np = 4 * ox + 1, nq = 4 * oy + 1, N = wx * wy;
    L.coef0 = L.wgt1 = (long)batch * K * np;
    L.coef1 = L.wgt0 = (long)batch * K * nq;
    L.F = (long)batch * wx * wx * nq;
    L.G = (long)batch * wy * wy * np;
    const long cap = N * N / 2;      // as li_layout: the same chunks for both dtypes
    L.rc0 = (int)std::max(1L, std::min(K, cap / (wx * wx)));
    L.rc1 = (int)std::max(1L, std::min(K, cap / (wy * wy)));
    L.U = (long)batch * std::max((long)L.rc0 * wx * wx, (long)L.rc1 * wy * wy);
    return L;
}

// kind / voff of a list of rectangles, checked on the host (one copy and one synchronisation of s): the check of trx_convmat_shapes, and
// nothing but rectangles
int rectangles_check(hipStream_t s, const int* kind, const int* voff, int S, int npar) {
    std::vector<int> h((size_t)2 * S + 1);
    if (hipMemcpyAsync(h.data(), kind, sizeof(int) * S, hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipMemcpyAsync(h.data() + S, voff, sizeof(int) * (S + 1), hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return TRX_ERR_LAUNCH;
    const int* vo = h.data() + S;
    if (vo[0] < 0 || vo[S] > npar) return TRX_ERR_ARG;
    for (int i = 0; i < S; ++i)
        if (h[i] != 1 || vo[i + 1] - vo[i] != 5) return TRX_ERR_ARG;
    return TRX_OK;
}

inline bool good_period(double L) { return L > 0.0 && std::isfinite(L); }

template <class T>
int convmat_li_shapes_t(const int* voff, int S, const double* par, int npar, const void* rval, double Lx, double Ly, int batch, int ox, int oy,
                        void* Ex, void* Ey, void* Ux, void* Uy, double* brk, int* rec, int* info, void* ws, hipStream_t s) {
    const LiShapesLayout L = li_shapes_layout(batch, S, ox, oy);
    zc* coef0 = reinterpret_cast<zc*>(ws);
    zc* coef1 = coef0 + L.coef0;
    zc* wgt0 = coef1 + L.coef1;
    zc* wgt1 = wgt0 + L.wgt0;
    zc* F = wgt1 + L.wgt1;
    zc* G = F + L.F;
    zc* Uw = G + L.G;
    const int K = 2 * S + 1, wx = 2 * ox + 1, wy = 2 * oy + 1, np = 4 * ox + 1, nq = 4 * oy + 1, N = wx * wy;
    if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s) != hipSuccess) return TRX_ERR_LAUNCH;
    TRX_LAUNCH(li_strips_kernel, dim3(2, batch), dim3(LS_BLOCK), 0, s, voff, S, par, npar, (const zc*)rval, Lx, Ly, ox, oy, coef0, coef1, wgt0, wgt1,
               brk, rec, info);
    TRX_CHECK_LAUNCH();
    // E_x: inverses of the x-Toeplitz blocks per horizontal strip, weighted along y;  E_y: the mirror image
    int rc = li_direction(s, coef0, K, wx, wgt0, (long)K * nq, nq, batch, (zc*)Uy, Uw, L.rc0, F, info);
    if (rc) return rc;
    rc = li_direction(s, coef1, K, wy, wgt1, (long)K * np, np, batch, (zc*)Ux, Uw, L.rc1, G, info);
    if (rc) return rc;
    TRX_LAUNCH((li_scatter_kernel<T>), dim3(cdiv_i(N, 256), N, batch), dim3(256), 0, s, (const zc*)F, (const zc*)G, ox, oy, (cx<T>*)Ex,
               (cx<T>*)Ey);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace
}  // namespace trx

using namespace trx;

extern "C" size_t trx_convmat_li_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy) {
    (void)dtype;                     // every buffer is complex128 and the row chunk is the same for both dtypes
    if (batch <= 0 || ox < 0 || oy < 0 || nx <= 0 || ny <= 0) return 0;
    const LiLayout L = li_layout(batch, nx, ny, ox, oy);
    return sizeof(zc) * (size_t)(L.ay + L.ax + L.wy_tw + L.wx_tw + L.F + L.G + L.U);
}

extern "C" int trx_convmat_li(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy, void* Ex, void* Ey,
                              void* Ux, void* Uy, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (!grid || !Ex || !Ey || !info || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || ox < 0 || oy < 0 || nx <= 2 * ox || ny <= 2 * oy) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_convmat_li_ws_bytes(dtype, batch, nx, ny, ox, oy)) return TRX_ERR_WORKSPACE;
    if ((size_t)16 * 2 * (size_t)(nx > ny ? nx : ny) > 64 * 1024) return TRX_ERR_UNSUPPORTED;
    if (toeplitz_lds_bytes(2 * (ox > oy ? ox : oy) + 1) > LI_LDS_MAX) return TRX_ERR_UNSUPPORTED;      // 2o+1 <= 99
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64) return convmat_li_t<float>(grid_is_complex, grid, batch, nx, ny, ox, oy, Ex, Ey, Ux, Uy, info, ws, s);
    return convmat_li_t<double>(grid_is_complex, grid, batch, nx, ny, ox, oy, Ex, Ey, Ux, Uy, info, ws, s);
}

extern "C" size_t trx_convmat_li_shapes_ws_bytes(int dtype, int batch, int S, int ox, int oy) {
    (void)dtype;                     // every buffer is complex128 and the strip chunk is the same for both dtypes
    if (batch <= 0 || S <= 0 || ox < 0 || oy < 0) return 0;
    const LiShapesLayout L = li_shapes_layout(batch, S, ox, oy);
    return sizeof(zc) * (size_t)(L.coef0 + L.coef1 + L.wgt0 + L.wgt1 + L.F + L.G + L.U);
}

extern "C" int trx_convmat_li_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* rval, double Lx,
                                     double Ly, int batch, int ox, int oy, void* Ex, void* Ey, void* Ux, void* Uy, double* brk, int* rec, int* info,
                                     void* ws, size_t ws_bytes, void* stream) {
    if (!kind || !voff || !par || !rval || !Ex || !Ey || !info || !ws) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || ox < 0 || oy < 0 || !good_period(Lx) || !good_period(Ly)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (S > LS_SMAX) return TRX_ERR_UNSUPPORTED;
    if (toeplitz_lds_bytes(2 * (ox > oy ? ox : oy) + 1) > LI_LDS_MAX) return TRX_ERR_UNSUPPORTED;      // 2o+1 <= 99, as trx_convmat_li
    if (ws_bytes < trx_convmat_li_shapes_ws_bytes(dtype, batch, S, ox, oy)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    const int rc = rectangles_check(s, kind, voff, S, npar);
    if (rc) return rc;
    if (dtype == TRX_C64)
        return convmat_li_shapes_t<float>(voff, S, par, npar, rval, Lx, Ly, batch, ox, oy, Ex, Ey, Ux, Uy, brk, rec, info, ws, s);
    return convmat_li_shapes_t<double>(voff, S, par, npar, rval, Lx, Ly, batch, ox, oy, Ex, Ey, Ux, Uy, brk, rec, info, ws, s);
}

extern "C" int trx_convmat_li_shapes_backward(const int* kind, const int* voff, int S, const double* par, int npar, const void* rval, double Lx,
                                              double Ly, int batch, int ox, int oy, const double* brk, const int* rec, const void* ga_x,
                                              const void* gw_y, const void* ga_y, const void* gw_x, double* gpar, void* grval, void* stream) {
    if (!kind || !voff || !par || !rval || !brk || !rec || !ga_x || !gw_y || !ga_y || !gw_x || !gpar || !grval) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || ox < 0 || oy < 0 || !good_period(Lx) || !good_period(Ly)) return TRX_ERR_ARG;
    if (S > LS_SMAX || npar + S + 1 > 65535) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    const int rc = rectangles_check(s, kind, voff, S, npar);
    if (rc) return rc;
    TRX_LAUNCH(li_strips_backward_kernel, dim3(npar + S + 1, batch), dim3(LS_BLOCK), 0, s, voff, S, par, npar, (const zc*)rval, Lx, Ly, ox, oy, brk,
               rec, (const zc*)ga_x, (const zc*)gw_y, (const zc*)ga_y, (const zc*)gw_x, gpar, (zc*)grval);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
