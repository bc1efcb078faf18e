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
int li_direction(hipStream_t s, const zc* coef, int nrows, int w, const zc* Wtw, int nq2, int batch, zc* Ukeep, zc* Uws, int rc, zc* Out,
                 int* info) {
    const long ww = (long)w * w;
    const size_t lds = toeplitz_lds_bytes(w);
    if (set_max_dyn_smem((const void*)toeplitz_inv_kernel, lds)) return TRX_ERR_LAUNCH;
    const zc one(1.0, 0.0), zero(0.0, 0.0);
    if (Ukeep) {                     // the caller keeps every inverse (adjoint): one pass, U in place
        TRX_LAUNCH(toeplitz_inv_kernel, dim3(nrows, batch), dim3(256), lds, s, coef, nrows, 0, w, Ukeep, (long)nrows * ww, info);
        TRX_CHECK_LAUNCH();
        return gemm<double>(s, TRX_OP_T, TRX_OP_N, (int)ww, nq2, nrows, one, Ukeep, (int)ww, (long)nrows * ww, Wtw, nq2, 0, zero, Out, nq2,
                            ww * nq2, batch);
    }
    for (int r0 = 0; r0 < nrows; r0 += rc) {
        const int rn = std::min(rc, nrows - r0);
        TRX_LAUNCH(toeplitz_inv_kernel, dim3(rn, batch), dim3(256), lds, s, coef, nrows, r0, w, Uws, (long)rn * ww, info);
        TRX_CHECK_LAUNCH();
        int rc2 = gemm<double>(s, TRX_OP_T, TRX_OP_N, (int)ww, nq2, rn, one, Uws, (int)ww, (long)rn * ww, Wtw + (long)r0 * nq2, nq2, 0,
                               r0 == 0 ? zero : one, Out, nq2, ww * nq2, batch);
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
    int rc = li_direction(s, ay, ny, wx, twy, nq, batch, (zc*)Uy, Uw, L.rc_y, F, info);
    if (rc) return rc;
    // E_y: inverses of the y-Toeplitz blocks per grid row x, transformed along x
    rc = li_direction(s, ax, nx, wy, twx, np, batch, (zc*)Ux, Uw, L.rc_x, G, info);
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
