// Thickness sweeps that reuse a layer's modes (include/trx.h: trx_thickness_prepare, trx_thickness_columns; no reference counterpart).
// The modes W, kz, V of a layer do not depend on its thickness d; only the diagonal phase X = exp(i w kz d) does.  With
//   F = Vf^-1 V,  A = W + F,  B = W - F                      (the layer's modes seen from the free-space gap, as layer_T_kernel forms them)
// and mode amplitudes c+ (referenced to the left interface) and c- (to the right one), the gap amplitudes next to the layer are
//   left :  f  = (A c+ + B X c-)/2,   r  = (B c+ + A X c-)/2        right :  f' = (A X c+ + B c-)/2,   r' = (B X c+ + A c-)/2
// Everything left of the layer is a scattering matrix Lft, everything right of it Rgt (blocks [S11, S21, S12, S22]); their reflections
// R_L = Lft12, R_R = Rgt21 close the two interfaces:  f = Lft11 a + R_L r,  r' = R_R f' + Rgt22 b.  Once per point
//   P_L = A - R_L B,  rho_L = P_L^-1 (R_L A - B),      P_R = A - R_R B,  rho_R = P_R^-1 (R_R A - B)
// turn them into reflection operators in the layer's own mode basis (c+ = s + rho_L X c-, c- = rho_R X c+ for forward incidence), and per
// thickness only  K = I - (rho_L X)(rho_R X)  has to be formed (one GEMM) and factored (one LU): 1.33 n^3 complex MACs instead of a new
// eigendecomposition.  |x| <= 1 for every mode and no W^-1 appears: as stable as the S-matrix cascade it replaces.
// The adjoint (trx_thickness_columns_keep, trx_thickness_columns_backward): everything that depends on the thickness is a solve with m <= 16
// right-hand sides, so one thickness costs one more factorisation (K^H) and O(n^2 m) work, and the gradients of rho_L, rho_R, A, B and the
// output-side operator are sums of rank-m outer products over the thicknesses, each element written by one thread (no atomics).
#include "common.hpp"
#include "prof.hpp"

namespace trx {
namespace {

constexpr int TK_MAX_COLS = 16;            // = the column limit of trx_redheffer_halfspace_columns
constexpr int TK_CT = 8;                   // (thickness, column) pairs per wave of the skinny product
struct TkCols { int c[TK_MAX_COLS]; };
enum { TK_ABSENT = 0, TK_BD = 1, TK_DENSE = 2 };

template <class T>
struct TkOp {                               // one side of the swept layer
    int kind;
    const cx<T>* bd;                        // TK_BD: [4 blocks][4 diagonals][B][N]
    const cx<T>* S[4];                      // TK_DENSE: [B,n,n] each
};

__device__ __forceinline__ cx<double> tk_f64(cx<float> a) { return cx<double>((double)a.x, (double)a.y); }
__device__ __forceinline__ cx<double> tk_f64(cx<double> a) { return a; }

// element (i, j) of the dense form of a block-diagonal operator d[4 diagonals][B][N]
template <class T>
__device__ inline cx<T> tk_bd_elem(const cx<T>* __restrict__ d, long dstride, int b, int N, int i, int j) {
    const int ii = i < N ? i : i - N, jj = j < N ? j : j - N;
    if (ii != jj) return cx<T>(T(0), T(0));
    return d[(long)((i < N ? 0 : 2) + (j < N ? 0 : 1)) * dstride + (long)b * N + ii];
}

// A = W + F, B = W - F,  F = Vf^-1 V (Vf^-1 2x2-block-diagonal: rows i and i+N of V combine).  Reads W and V once, writes A and B once:
// 4 n^2 elements per point, rows contiguous (16-byte accesses in complex128).
template <class T>
__global__ __launch_bounds__(256) void tk_ab_kernel(const cx<T>* __restrict__ W, const cx<T>* __restrict__ V, const cx<T>* __restrict__ p11,
                                                    const cx<T>* __restrict__ p12, const cx<T>* __restrict__ p21, const cx<T>* __restrict__ p22, int N,
                                                    cx<T>* __restrict__ A, cx<T>* __restrict__ B) {
    const int b = blockIdx.z, i = blockIdx.y;           // i in [0, N)
    const int n = 2 * N;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long o0 = ((long)b * n + i) * n + j, o1 = ((long)b * n + i + N) * n + j;
    const cx<T> v0 = V[o0], v1 = V[o1], w0 = W[o0], w1 = W[o1];
    const long d = (long)b * N + i;
    const cx<T> f0 = p11[d] * v0 + p12[d] * v1;
    const cx<T> f1 = p21[d] * v0 + p22[d] * v1;
    A[o0] = w0 + f0; B[o0] = w0 - f0;
    A[o1] = w1 + f1; B[o1] = w1 - f1;
}

// P = A - D B,  Nn = D A - B  for a block-diagonal reflection D (row combination of rows i and i+N); D == nullptr: P = A, Nn = -B (no
// reflection, and the start of the dense case, whose products follow as two GEMMs).  Reads A and B once, writes P and Nn once.
template <class T>
__global__ __launch_bounds__(256) void tk_pn_kernel(const cx<T>* __restrict__ A, const cx<T>* __restrict__ B, const cx<T>* __restrict__ D, long dstride,
                                                    int N, cx<T>* __restrict__ P, cx<T>* __restrict__ Nn) {
    const int b = blockIdx.z, i = blockIdx.y;           // i in [0, N)
    const int n = 2 * N;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long o0 = ((long)b * n + i) * n + j, o1 = ((long)b * n + i + N) * n + j;
    const cx<T> a0 = A[o0], a1 = A[o1], b0 = B[o0], b1 = B[o1];
    cx<T> p0 = a0, p1 = a1, q0 = -b0, q1 = -b1;
    if (D) {
        const long di = (long)b * N + i;
        const cx<T> d0 = D[di], d1 = D[dstride + di], d2 = D[2 * dstride + di], d3 = D[3 * dstride + di];
        p0 -= d0 * b0 + d1 * b1;
        p1 -= d2 * b0 + d3 * b1;
        q0 += d0 * a0 + d1 * a1;
        q1 += d2 * a0 + d3 * a1;
    }
    P[o0] = p0; P[o1] = p1;
    Nn[o0] = q0; Nn[o1] = q1;
}

// out[b, i, q] = scale * (column cols[q] of one block of an operand): block-diagonal, dense, or absent (ident: the identity, else zero)
template <class T>
__global__ __launch_bounds__(256) void tk_col_kernel(int kind, const cx<T>* __restrict__ D, long dstride, const cx<T>* __restrict__ S, int ident,
                                                     TkCols cols, int m, int N, T scale, cx<T>* __restrict__ out) {
    const int b = blockIdx.z, q = blockIdx.y, n = 2 * N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = cols.c[q];
    cx<T> v(T(0), T(0));
    if (kind == TK_BD) v = tk_bd_elem(D, dstride, b, N, i, c);
    else if (kind == TK_DENSE) v = S[((long)b * n + i) * n + c];
    else if (ident && i == c) v.x = T(1);
    out[((long)b * n + i) * m + q] = scale * v;
}

// M[b,t] = X_t rho X_t (row and column scaling by the phase of thickness t) and K[b,t] = I, for every t of the chunk: rho is read ONCE per
// point, 2 T n^2 elements are written.  The product rho' M is then subtracted from K by the GEMM (rho' shared over t: batch stride 0).
template <class T>
__global__ __launch_bounds__(256) void tk_mk_kernel(const cx<T>* __restrict__ rho, const cx<T>* __restrict__ x, int ldt, int Tn, int n,
                                                    cx<T>* __restrict__ M, cx<T>* __restrict__ K) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const cx<T> r = rho[((long)b * n + i) * n + j];
    const cx<T> id((i == j) ? T(1) : T(0), T(0));
    for (int t = 0; t < Tn; ++t) {
        const cx<T>* xt = x + ((long)b * ldt + t) * n;
        const long o = (((long)b * Tn + t) * n + i) * n + j;
        M[o] = xt[i] * r * xt[j];
        K[o] = id;
    }
}

// dst[b, t, :, :] = src[b, :, :]   ([B,n,m] column blocks, one copy per thickness)
template <class T>
__global__ __launch_bounds__(256) void tk_bcast_kernel(const cx<T>* __restrict__ src, long per, int Tn, long total, cx<T>* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long e = idx % per, b = idx / per / Tn;
    dst[idx] = src[b * per + e];
}

// out[b, t, i, q] = x[b, t, i] * in[b, t, i, q]
template <class T>
__global__ __launch_bounds__(256) void tk_scale_kernel(const cx<T>* __restrict__ in, const cx<T>* __restrict__ x, int ldt, int Tn, int n, int m,
                                                       long total, cx<T>* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long row = idx / m;                               // (b * Tn + t) * n + i
    const int i = (int)(row % n);
    const long bt = row / n;
    const long b = bt / Tn, t = bt % Tn;
    out[idx] = x[(b * ldt + t) * n + i] * in[idx];
}

// info[b, t] (leading dimension ldt) = tmp[b * Tn + t]
__global__ __launch_bounds__(256) void tk_info_kernel(const int* __restrict__ tmp, int ldt, int Tn, int total, int* __restrict__ info) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    info[(long)(idx / Tn) * ldt + idx % Tn] = tmp[idx];
}

// out[b, t, :, q] = scale * (A1[b] X1[b, t, :, q] + A2[b] X2[b, t, :, q]) + Y0[b, :, q]      (A2 / X2 and Y0 optional)
// The matrices depend on the point only, the skinny right-hand sides on the thickness too: one wave per row of A, lanes along k, up to TK_CT
// (thickness, column) pairs per wave, fp64 accumulation for both dtypes and a fixed shuffle tree (as trx_matvec).  A1 | A2 are read
// ceil(T m / TK_CT) times per point whatever T; the right-hand sides ([n, T m] elements per point) stay in cache.
// X1, X2: [B, T, n, m] contiguous; out: [t][n][m] inside a point, `so` elements between points.
template <class T>
__global__ __launch_bounds__(256) void tk_matvec_kernel(const cx<T>* __restrict__ A1, const cx<T>* __restrict__ A2, const cx<T>* __restrict__ X1,
                                                        const cx<T>* __restrict__ X2, const cx<T>* __restrict__ Y0, double scale, cx<T>* __restrict__ out,
                                                        long so, int n, int m, int Tn) {
    const int lane = threadIdx.x & 63, b = blockIdx.z;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = row < n;                                   // wave-uniform
    const int c0 = blockIdx.y * TK_CT, ncols = Tn * m;
    const long arow = ((long)b * n + (live ? row : 0)) * n;
    const long xb = (long)b * Tn * n * m;
    long off[TK_CT];
    cx<double> acc[TK_CT];
#pragma unroll
    for (int cc = 0; cc < TK_CT; ++cc) {
        const int col = (c0 + cc < ncols) ? c0 + cc : c0;        // clamped: a dead slot repeats the tile's first pair and is not stored
        off[cc] = xb + (long)(col / m) * n * m + col % m;
        acc[cc] = cx<double>(0.0, 0.0);
    }
    for (int kk = lane; kk < n; kk += 64) {
        const cx<double> a1 = tk_f64(A1[arow + kk]);
#pragma unroll
        for (int cc = 0; cc < TK_CT; ++cc) cfma(acc[cc], a1, tk_f64(X1[off[cc] + (long)kk * m]));
        if (A2) {
            const cx<double> a2 = tk_f64(A2[arow + kk]);
#pragma unroll
            for (int cc = 0; cc < TK_CT; ++cc) cfma(acc[cc], a2, tk_f64(X2[off[cc] + (long)kk * m]));
        }
    }
#pragma unroll
    for (int cc = 0; cc < TK_CT; ++cc) {
        double re = scale * wave_sum(acc[cc].x), im = scale * wave_sum(acc[cc].y);
        const int col = c0 + cc;
        if (live && lane == 0 && col < ncols) {
            const int t = col / m, q = col % m;
            if (Y0) { const cx<T> y = Y0[((long)b * n + row) * m + q]; re += (double)y.x; im += (double)y.y; }
            out[(long)b * so + ((long)t * n + row) * m + q] = cx<T>((T)re, (T)im);
        }
    }
}

// out[b, t, :, q] = (D g[b, t, :, q]  or  g[b, t, :, q]) + Y0[b, :, q]      (D block diagonal or absent, Y0 optional; g: [B, T, n, m] contiguous)
template <class T>
__global__ __launch_bounds__(256) void tk_comb_kernel(const cx<T>* __restrict__ D, long dstride, const cx<T>* __restrict__ g, const cx<T>* __restrict__ Y0,
                                                      int Tn, int N, int m, long total, cx<T>* __restrict__ out, long so) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int n = 2 * N;
    const int q = (int)(idx % m);
    const long row = idx / m;
    const int i = (int)(row % n);
    const long bt = row / n;
    const int b = (int)(bt / Tn), t = (int)(bt % Tn);
    cx<T> v;
    if (D) {
        const int ii = i < N ? i : i - N;
        const long base = bt * n * m + q;
        v = tk_bd_elem(D, dstride, b, N, i, ii) * g[base + (long)ii * m] + tk_bd_elem(D, dstride, b, N, i, ii + N) * g[base + (long)(ii + N) * m];
    } else {
        v = g[idx];
    }
    if (Y0) v += Y0[((long)b * n + i) * m + q];
    out[(long)b * so + ((long)t * n + i) * m + q] = v;
}

// ---- adjoint of trx_thickness_columns (include/trx.h: trx_thickness_columns_backward) --------------------------------------------------------

// dst[b * sd + t * per + e] = src[b * ss + t * per + e]: the thickness axis of a [B, ldt, n, m] array <-> the chunk's contiguous [B, T, n, m]
template <class T>
__global__ __launch_bounds__(256) void tk_copy_kernel(const cx<T>* __restrict__ src, long ss, cx<T>* __restrict__ dst, long sd, long tper, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long b = idx / tper, e = idx % tper;
    dst[b * sd + e] = src[b * ss + e];
}

// out[b, t, i, q] = conj(x[b, t, i]) * in[b, t, i, q] + add[b, t, i, q]      (add optional)
template <class T>
__global__ __launch_bounds__(256) void tk_cscale_kernel(const cx<T>* __restrict__ in, const cx<T>* __restrict__ x, const cx<T>* __restrict__ add, int ldt,
                                                        int Tn, int n, int m, long total, cx<T>* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long row = idx / m;                               // (b * Tn + t) * n + i
    const int i = (int)(row % n);
    const long bt = row / n;
    const long b = bt / Tn, t = bt % Tn;
    cx<T> v = conj(x[(b * ldt + t) * n + i]) * in[idx];
    if (add) v += add[idx];
    out[idx] = v;
}

// Conjugate-transposed skinny product:  out[b, t, :, q] = scale * (A1[b]^H X1[b, t, :, q] + A2[b]^H X2[b, t, :, q]) + Y[b, t, :, q]
// (A2 / X2 and Y optional; all skinny operands [B, T, n, m] contiguous).  One thread per output row i and TK_CT (thickness, column) pairs: the
// lanes of a wave read A[b, k, i .. i+63], a row segment, coalesced; X[.., k, ..] is the same address in every lane.  No cross-lane reduction;
// fp64 accumulation in the fixed order k = 0 .. n-1 for both dtypes.  A1 | A2 are read ceil(T m / TK_CT) times per point.
template <class T>
__global__ __launch_bounds__(256) void tk_matvec_ct_kernel(const cx<T>* __restrict__ A1, const cx<T>* __restrict__ A2, const cx<T>* __restrict__ X1,
                                                           const cx<T>* __restrict__ X2, const cx<T>* __restrict__ Y, double scale,
                                                           cx<T>* __restrict__ out, int n, int m, int Tn) {
    const int b = blockIdx.z, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c0 = blockIdx.y * TK_CT, ncols = Tn * m;
    const long ab = (long)b * n * n + i, xb = (long)b * Tn * n * m;
    long off[TK_CT];
    cx<double> acc[TK_CT];
#pragma unroll
    for (int cc = 0; cc < TK_CT; ++cc) {
        const int col = (c0 + cc < ncols) ? c0 + cc : c0;        // clamped: a dead slot repeats the tile's first pair and is not stored
        off[cc] = xb + (long)(col / m) * n * m + col % m;
        acc[cc] = cx<double>(0.0, 0.0);
    }
    for (int k = 0; k < n; ++k) {
        const cx<double> a1 = conj(tk_f64(A1[ab + (long)k * n]));
#pragma unroll
        for (int cc = 0; cc < TK_CT; ++cc) cfma(acc[cc], a1, tk_f64(X1[off[cc] + (long)k * m]));
        if (A2) {
            const cx<double> a2 = conj(tk_f64(A2[ab + (long)k * n]));
#pragma unroll
            for (int cc = 0; cc < TK_CT; ++cc) cfma(acc[cc], a2, tk_f64(X2[off[cc] + (long)k * m]));
        }
    }
#pragma unroll
    for (int cc = 0; cc < TK_CT; ++cc) {
        if (c0 + cc >= ncols) continue;
        const long o = off[cc] + (long)i * m;
        double re = scale * acc[cc].x, im = scale * acc[cc].y;
        if (Y) { const cx<T> y = Y[o]; re += (double)y.x; im += (double)y.y; }
        out[o] = cx<T>((T)re, (T)im);
    }
}

// out[b, t, :, q] = D^H g[b, t, :, q] for the block-diagonal D [4 diagonals][B][N]: (D^H)[i, j] = conj(D[j, i])
template <class T>
__global__ __launch_bounds__(256) void tk_comb_ct_kernel(const cx<T>* __restrict__ D, long dstride, const cx<T>* __restrict__ g, int Tn, int N, int m,
                                                         long total, cx<T>* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int n = 2 * N;
    const int q = (int)(idx % m);
    const long row = idx / m;
    const int i = (int)(row % n);
    const long bt = row / n;
    const int b = (int)(bt / Tn);
    const int ii = i < N ? i : i - N;
    const long base = bt * n * m + q;
    out[idx] = conj(tk_bd_elem(D, dstride, b, N, ii, i)) * g[base + (long)ii * m] + conj(tk_bd_elem(D, dstride, b, N, ii + N, i)) * g[base + (long)(ii + N) * m];
}

constexpr int TK_MAX_TERMS = 4;
template <class T>
struct TkTerms {                            // G (+)= sum_k scale[k] * sum_{t,q} L[k][b,t,i,q] conj(R[k][b,t,j,q])
    const cx<T>* L[TK_MAX_TERMS];
    const cx<T>* R[TK_MAX_TERMS];
    double scale[TK_MAX_TERMS];
    int nterms;
};

// Outer-product accumulation over the (thickness, column) pairs of a chunk: one thread per element G[b, i, j] (lanes along j: G is written
// along its rows), terms, thicknesses and columns summed in that fixed order in fp64.  Every element has exactly one writer: no atomics, a
// repeated call gives the same bits.  accumulate: add to what G holds (the second and later chunks of the thickness axis).
template <class T>
__global__ __launch_bounds__(256) void tk_outer_kernel(TkTerms<T> tm, int accumulate, int Tn, int n, int m, cx<T>* __restrict__ G) {
    const int b = blockIdx.z, i = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long xb = (long)b * Tn * n * m;
    cx<double> tot(0.0, 0.0);
    for (int k = 0; k < tm.nterms; ++k) {
        const cx<T>*__restrict__ L = tm.L[k], *__restrict__ R = tm.R[k];
        cx<double> acc(0.0, 0.0);
        for (int t = 0; t < Tn; ++t) {
            const long lo = xb + ((long)t * n + i) * m, ro = xb + ((long)t * n + j) * m;
            for (int q = 0; q < m; ++q) cfma(acc, tk_f64(L[lo + q]), conj(tk_f64(R[ro + q])));
        }
        tot.x += tm.scale[k] * acc.x;
        tot.y += tm.scale[k] * acc.y;
    }
    const long o = ((long)b * n + i) * n + j;
    if (accumulate) { const cx<T> g0 = G[o]; tot.x += (double)g0.x; tot.y += (double)g0.y; }
    G[o] = cx<T>((T)tot.x, (T)tot.y);
}

// The gradient of a block-diagonal output operator: only its four diagonals, gD[2 r + c][b][ii] (+)= sum_{t,q} L[b,t,ii + r N,q] conj(R[b,t,ii + c N,q])
template <class T>
__global__ __launch_bounds__(256) void tk_outer_bd_kernel(const cx<T>* __restrict__ L, const cx<T>* __restrict__ R, int accumulate, int Tn, int N, int m,
                                                          long bN, cx<T>* __restrict__ gD) {
    const int b = blockIdx.z, k = blockIdx.y, ii = blockIdx.x * blockDim.x + threadIdx.x;
    if (ii >= N) return;
    const int n = 2 * N, i = ii + (k >> 1) * N, j = ii + (k & 1) * N;
    const long xb = (long)b * Tn * n * m;
    cx<double> acc(0.0, 0.0);
    for (int t = 0; t < Tn; ++t) {
        const long lo = xb + ((long)t * n + i) * m, ro = xb + ((long)t * n + j) * m;
        for (int q = 0; q < m; ++q) cfma(acc, tk_f64(L[lo + q]), conj(tk_f64(R[ro + q])));
    }
    const long o = (long)k * bN + (long)b * N + ii;
    if (accumulate) { const cx<T> g0 = gD[o]; acc.x += (double)g0.x; acc.y += (double)g0.y; }
    gD[o] = cx<T>((T)acc.x, (T)acc.y);
}

// dst[b, e] (+)= sum_t src[b, t, e]   (e over the n m elements of a column block; src == nullptr: zero), in the fixed order t = 0 .. T-1
template <class T>
__global__ __launch_bounds__(256) void tk_tsum_kernel(const cx<T>* __restrict__ src, int accumulate, int Tn, long per, long total, cx<T>* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long b = idx / per, e = idx % per;
    cx<double> acc(0.0, 0.0);
    if (src)
        for (int t = 0; t < Tn; ++t) { const cx<double> v = tk_f64(src[(b * Tn + t) * per + e]); acc.x += v.x; acc.y += v.y; }
    if (accumulate) { const cx<T> g0 = dst[idx]; acc.x += (double)g0.x; acc.y += (double)g0.y; }
    dst[idx] = cx<T>((T)acc.x, (T)acc.y);
}

// The phase gradient, three row reductions in one launch:
//   gx[b, t, i] = sum_q (p1 + mu)[i, q] conj(cs[i, q]) + (ub + rnu)[i, q] conj(cp[i, q])        (p1 optional: the reflection port's w-bar)
template <class T>
__global__ __launch_bounds__(256) void tk_gphase_kernel(const cx<T>* __restrict__ p1, const cx<T>* __restrict__ mu, const cx<T>* __restrict__ cs,
                                                        const cx<T>* __restrict__ ub, const cx<T>* __restrict__ rnu, const cx<T>* __restrict__ cp, int ldt,
                                                        int Tn, int n, int m, long total, cx<T>* __restrict__ gx) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;           // (b * Tn + t) * n + i
    if (row >= total) return;
    const int i = (int)(row % n);
    const long bt = row / n;
    const long b = bt / Tn, t = bt % Tn;
    cx<double> acc(0.0, 0.0);
    for (int q = 0; q < m; ++q) {
        const long o = row * m + q;
        cx<double> a = tk_f64(mu[o]);
        if (p1) { const cx<double> v = tk_f64(p1[o]); a.x += v.x; a.y += v.y; }
        const cx<double> c = tk_f64(ub[o]) + tk_f64(rnu[o]);
        cfma(acc, a, conj(tk_f64(cs[o])));
        cfma(acc, c, conj(tk_f64(cp[o])));
    }
    gx[(b * ldt + t) * n + i] = cx<T>((T)acc.x, (T)acc.y);
}

template <class T>
int thickness_prepare_t(hipStream_t s, const cx<T>* W, const cx<T>* V, const cx<T>* pv, const TkOp<T>& L, const TkOp<T>& R, int direction,
                        const int* cols, int m, int N, int batch, cx<T>* rhoL, cx<T>* rhoR, cx<T>* src, cx<T>* AB, int* piv, int* info, cx<T>* ws) {
    const int n = 2 * N;
    const long nn = (long)n * n, bn = (long)batch * nn, bN = (long)batch * N, bv = (long)batch * n * m;
    const cx<T> one(T(1), T(0)), mone(T(-1), T(0));
    const dim3 blk(256), gN(cdiv_i(n, 256), N, batch), gp(cdiv_i(n, 256), m, batch);
    int dense_sides = (L.kind == TK_DENSE) + (R.kind == TK_DENSE);
    ProfScope prof(PROF_THICK_PREPARE, s, 8.0 * batch * (double)nn * n * (2.0 * (1.0 / 3.0 + 1.0) + 2.0 * dense_sides),
                   (double)sizeof(cx<T>) * batch * nn * (4.0 + 2.0 * (4.0 + 2.0)));
    cx<T>*A = AB, *B = AB + bn, *P = ws;
    TkCols pc;
    for (int q = 0; q < TK_MAX_COLS; ++q) pc.c[q] = q < m ? cols[q] : 0;
    TRX_LAUNCH((tk_ab_kernel<T>), gN, blk, 0, s, W, V, pv, pv + bN, pv + 2 * bN, pv + 3 * bN, N, A, B);
    int rc;
    for (int side = 0; side < 2; ++side) {
        const TkOp<T>& op = side ? R : L;
        const int rblk = side ? 1 : 2;                  // the reflection the layer sees: Lft12 on its left, Rgt21 on its right
        cx<T>* rho = side ? rhoR : rhoL;
        const cx<T>* D = op.kind == TK_BD ? op.bd + (long)rblk * 4 * bN : nullptr;
        TRX_LAUNCH((tk_pn_kernel<T>), gN, blk, 0, s, (const cx<T>*)A, (const cx<T>*)B, D, bN, N, P, rho);
        if (op.kind == TK_DENSE) {
            rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, n, n, n, mone, op.S[rblk], n, nn, B, n, nn, one, P, n, nn, batch); if (rc) return rc;
            rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, n, n, n, one, op.S[rblk], n, nn, A, n, nn, one, rho, n, nn, batch); if (rc) return rc;
        }
        rc = lu_factor<T>(s, P, n, nn, n, piv, batch, info + (long)side * batch); if (rc) return rc;
        rc = lu_solve<T>(s, P, n, nn, n, piv, rho, n, nn, n, batch); if (rc) return rc;
        if (side == direction) {
            // the side the wave comes from: s = P^-1 2 T e_c with T = Lft11 (forward) / Rgt22 (backward), and the part of the reflected
            // column that does not pass through the layer, Lft21 e_c / Rgt12 e_c
            const int tblk = side ? 3 : 0, cblk = side ? 2 : 1;
            TRX_LAUNCH((tk_col_kernel<T>), gp, blk, 0, s, op.kind, op.kind == TK_BD ? op.bd + (long)tblk * 4 * bN : nullptr, bN, op.S[tblk], 1, pc, m, N,
                       T(2), src);
            rc = lu_solve<T>(s, P, n, nn, n, piv, src, m, (long)n * m, m, batch); if (rc) return rc;
            TRX_LAUNCH((tk_col_kernel<T>), gp, blk, 0, s, op.kind, op.kind == TK_BD ? op.bd + (long)cblk * 4 * bN : nullptr, bN, op.S[cblk], 0, pc, m, N,
                       T(1), src + bv);
        }
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int thickness_columns_t(hipStream_t s, const cx<T>* rhoL, const cx<T>* rhoR, const cx<T>* src, const cx<T>* AB, const cx<T>* phase, int ldt, int Tn,
                        int direction, int port, const TkOp<T>& L, const TkOp<T>& R, int m, int N, int batch, cx<T>* out, cx<T>* cp_keep, int* piv, int* info,
                        cx<T>* ws) {
    const int n = 2 * N;
    const long nn = (long)n * n, bn = (long)batch * nn, bN = (long)batch * N, BT = (long)batch * Tn, per = (long)n * m, tv = BT * per;
    const cx<T> one(T(1), T(0)), mone(T(-1), T(0));
    const dim3 blk(256), gn(cdiv_i(n, 256), n, batch), gflat(cdiv_i(tv, 256)), gmv(cdiv_i(n, 4), cdiv_i((long)Tn * m, TK_CT), batch);
    const cx<T>* const nul = nullptr;
    cx<T>*M = ws, *K = ws + BT * nn;
    cx<T>*cp = K + BT * nn, *u = cp + tv, *cs = u + tv, *w = cs + tv, *g = w + tv;
    int* itmp = piv + BT * n;                           // contiguous info of the LU, scattered into info[b, t] afterwards
    // forward: K = I - (rho_L X)(rho_R X), the solved amplitude is c+;  backward: K = I - (rho_R X)(rho_L X), the solved amplitude is c-
    const cx<T>*rhoA = direction ? rhoR : rhoL, *rhoB = direction ? rhoL : rhoR;
    const cx<T>*A = AB, *B = AB + bn;
    int rc;
    {
        ProfScope prof(PROF_THICK_KGEMM, s, 8.0 * BT * (double)nn * n, (double)sizeof(cx<T>) * (bn * 2.0 + BT * nn * 4.0));
        TRX_LAUNCH((tk_mk_kernel<T>), gn, blk, 0, s, rhoB, phase, ldt, Tn, n, M, K);
        for (int b = 0; b < batch; ++b) {               // rho_A[b] is shared by the T products of point b: batch stride 0
            rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, n, n, n, mone, rhoA + (long)b * nn, n, 0L, M + (long)b * Tn * nn, n, nn, one, K + (long)b * Tn * nn, n, nn, Tn);
            if (rc) return rc;
        }
    }
    {
        ProfScope prof(PROF_THICK_LU, s, 8.0 * BT * (double)nn * n / 3.0, (double)sizeof(cx<T>) * BT * nn * 2.0);
        TRX_LAUNCH((tk_bcast_kernel<T>), gflat, blk, 0, s, src, per, Tn, tv, cp);
        rc = lu_factor<T>(s, K, n, nn, n, piv, (int)BT, itmp); if (rc) return rc;
        TRX_LAUNCH(tk_info_kernel, dim3(cdiv_i(BT, 256)), blk, 0, s, (const int*)itmp, ldt, Tn, (int)BT, info);
        rc = lu_solve<T>(s, K, n, nn, n, piv, cp, m, per, m, (int)BT); if (rc) return rc;
        // the solved amplitude is all the adjoint needs of this call: [batch, ldt, n, m] like out
        if (cp_keep) TRX_LAUNCH((tk_copy_kernel<T>), gflat, blk, 0, s, (const cx<T>*)cp, (long)Tn * per, cp_keep, (long)ldt * per, (long)Tn * per, tv);
    }
    ProfScope prof(PROF_THICK_READOUT, s, 8.0 * BT * (double)nn * m * 4.0, (double)sizeof(cx<T>) * bn * 4.0);
    // u = X cp;  the other amplitude cs = rho_B u;  w = X cs
    TRX_LAUNCH((tk_scale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)cp, phase, ldt, Tn, n, m, tv, u);
    TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, rhoB, nul, (const cx<T>*)u, nul, nul, 1.0, cs, (long)Tn * per, n, m, Tn);
    // transmission leaves through the far side:  (A u + B cs)/2 = f' (forward) / r (backward), then Rgt11 / Lft22;
    // reflection through the near side:          (B cp + A w)/2 = r (forward) / f' (backward), then Lft22 / Rgt11, plus Lft21 e_c / Rgt12 e_c
    const bool refl = port == 1;
    const TkOp<T>& op = ((direction == 0) != refl) ? R : L;
    const int oblk = (&op == &R) ? 0 : 3;
    const cx<T>* Y0 = refl ? src + (long)batch * per : nul;
    const bool direct = op.kind == TK_ABSENT;
    cx<T>* gdst = direct ? out : g;
    const long gso = direct ? (long)ldt * per : (long)Tn * per;
    if (!refl) {
        TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, A, B, (const cx<T>*)u, (const cx<T>*)cs, nul, 0.5, gdst, gso, n, m, Tn);
    } else {
        TRX_LAUNCH((tk_scale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)cs, phase, ldt, Tn, n, m, tv, w);
        TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, B, A, (const cx<T>*)cp, (const cx<T>*)w, direct ? Y0 : nul, 0.5, gdst, gso, n, m, Tn);
    }
    if (op.kind == TK_BD)
        TRX_LAUNCH((tk_comb_kernel<T>), gflat, blk, 0, s, op.bd + (long)oblk * 4 * bN, bN, (const cx<T>*)g, Y0, Tn, N, m, tv, out, (long)ldt * per);
    else if (op.kind == TK_DENSE)
        TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, op.S[oblk], nul, (const cx<T>*)g, nul, Y0, 1.0, out, (long)ldt * per, n, m, Tn);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// kind / pointer pair of the C ABI -> TkOp; false for a malformed operand
template <class T>
bool tk_operand(int kind, const void* p, TkOp<T>* op) {
    op->kind = kind;
    op->bd = nullptr;
    for (int k = 0; k < 4; ++k) op->S[k] = nullptr;
    if (kind == TK_ABSENT) return true;
    if (!p) return false;
    if (kind == TK_BD) { op->bd = (const cx<T>*)p; return true; }
    if (kind != TK_DENSE) return false;
    const void* const* S = (const void* const*)p;
    for (int k = 0; k < 4; ++k) {
        if (!S[k]) return false;
        op->S[k] = (const cx<T>*)S[k];
    }
    return true;
}

template <class T>
int thickness_prepare_d(hipStream_t s, const void* W, const void* V, const void* vfinv, int lk, const void* lp, int rk, const void* rp, int direction,
                        const int* cols, int m, int N, int batch, void* rhoL, void* rhoR, void* src, void* AB, int* piv, int* info, void* ws) {
    TkOp<T> L, R;
    if (!tk_operand<T>(lk, lp, &L) || !tk_operand<T>(rk, rp, &R)) return TRX_ERR_ARG;
    return thickness_prepare_t<T>(s, (const cx<T>*)W, (const cx<T>*)V, (const cx<T>*)vfinv, L, R, direction, cols, m, N, batch, (cx<T>*)rhoL, (cx<T>*)rhoR,
                                  (cx<T>*)src, (cx<T>*)AB, piv, info, (cx<T>*)ws);
}

template <class T>
int thickness_columns_d(hipStream_t s, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int Tn, int direction,
                        int port, int lk, const void* lp, int rk, const void* rp, int m, int N, int batch, void* out, void* cp, int* piv, int* info, void* ws) {
    TkOp<T> L, R;
    if (!tk_operand<T>(lk, lp, &L) || !tk_operand<T>(rk, rp, &R)) return TRX_ERR_ARG;
    return thickness_columns_t<T>(s, (const cx<T>*)rhoL, (const cx<T>*)rhoR, (const cx<T>*)src, (const cx<T>*)AB, (const cx<T>*)phase, ldt, Tn, direction, port,
                                  L, R, m, N, batch, (cx<T>*)out, (cx<T>*)cp, piv, info, (cx<T>*)ws);
}

constexpr int TK_BWD_SKINNY = 15;         // [B, T, n, m] buffers of the backward's workspace, after its two n x n matrices per (point, thickness)

// The adjoint of thickness_columns_t for one chunk of thicknesses (include/trx.h has the formulas).  rho_A / rho_B, the output operand and its
// block are chosen exactly as in the forward; u, cs, w are recomputed from the saved amplitude cp.  Every gradient pointer may be null.
template <class T>
int thickness_columns_backward_t(hipStream_t s, const cx<T>* rhoL, const cx<T>* rhoR, const cx<T>* AB, const cx<T>* phase, int ldt, int Tn, int direction,
                                 int port, const TkOp<T>& L, const TkOp<T>& R, int m, int N, int batch, const cx<T>* cpk, const cx<T>* gout, cx<T>* grhoL,
                                 cx<T>* grhoR, cx<T>* gsrc, cx<T>* gAB, cx<T>* gphase, cx<T>* gop, int accumulate, int* piv, int* info, cx<T>* ws) {
    const int n = 2 * N;
    const long nn = (long)n * n, bn = (long)batch * nn, bN = (long)batch * N, BT = (long)batch * Tn, per = (long)n * m, tv = BT * per;
    const cx<T> one(T(1), T(0)), mone(T(-1), T(0));
    const dim3 blk(256), gn(cdiv_i(n, 256), n, batch), gflat(cdiv_i(tv, 256)), gmv(cdiv_i(n, 4), cdiv_i((long)Tn * m, TK_CT), batch);
    const dim3 gct(cdiv_i(n, 256), cdiv_i((long)Tn * m, TK_CT), batch);
    const cx<T>* const nul = nullptr;
    const bool refl = port == 1;
    const TkOp<T>& op = ((direction == 0) != refl) ? R : L;
    const int oblk = (&op == &R) ? 0 : 3;
    if (op.kind == TK_ABSENT) gop = nullptr;
    cx<T>*grhoA = direction ? grhoR : grhoL, *grhoB = direction ? grhoL : grhoR;
    if (!grhoA && !grhoB && !gsrc && !gAB && !gphase && !gop) return TRX_OK;
    const bool need_solve = grhoA || grhoB || gsrc || gphase;
    ProfScope prof(PROF_THICK_BACKWARD, s, need_solve ? 8.0 * BT * (double)nn * (n * (4.0 / 3.0) + 12.0 * m) : 8.0 * BT * (double)nn * 6.0 * m,
                   (double)sizeof(cx<T>) * (bn * 8.0 + (need_solve ? BT * nn * 6.0 : 0.0)));
    cx<T>*M = ws, *K = ws + BT * nn, *sk = K + BT * nn;
    cx<T>*cp = sk, *Gc = cp + tv, *u = Gc + tv, *cs = u + tv, *w = cs + tv, *gbb = w + tv, *gf = gbb + tv, *ha = gf + tv, *hb = ha + tv, *csx = hb + tv,
         *ub = csx + tv, *lam = ub + tv, *mu = lam + tv, *nu = mu + tv, *rnu = nu + tv;
    int* itmp = piv + BT * n;
    const cx<T>*rhoA = direction ? rhoR : rhoL, *rhoB = direction ? rhoL : rhoR;
    const cx<T>*A = AB, *B = AB + bn;
    int rc;
    TRX_LAUNCH((tk_copy_kernel<T>), gflat, blk, 0, s, cpk, (long)ldt * per, cp, (long)Tn * per, (long)Tn * per, tv);
    TRX_LAUNCH((tk_copy_kernel<T>), gflat, blk, 0, s, gout, (long)ldt * per, Gc, (long)Tn * per, (long)Tn * per, tv);
    // recomputed: u = X cp, cs = rho_B u, w = X cs
    TRX_LAUNCH((tk_scale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)cp, phase, ldt, Tn, n, m, tv, u);
    TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, rhoB, nul, (const cx<T>*)u, nul, nul, 1.0, cs, (long)Tn * per, n, m, Tn);
    TRX_LAUNCH((tk_scale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)cs, phase, ldt, Tn, n, m, tv, w);
    // output side: g-bar = O^H G-bar; gO = sum G-bar g^H with g the forward's column before the operator
    const cx<T>* gb = Gc;
    if (op.kind == TK_BD) {
        TRX_LAUNCH((tk_comb_ct_kernel<T>), gflat, blk, 0, s, op.bd + (long)oblk * 4 * bN, bN, (const cx<T>*)Gc, Tn, N, m, tv, gbb);
        gb = gbb;
    } else if (op.kind == TK_DENSE) {
        TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, op.S[oblk], nul, (const cx<T>*)Gc, nul, nul, 1.0, gbb, n, m, Tn);
        gb = gbb;
    }
    if (gop) {
        if (!refl) {
            TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, A, B, (const cx<T>*)u, (const cx<T>*)cs, nul, 0.5, gf, (long)Tn * per, n, m, Tn);
        } else {
            TRX_LAUNCH((tk_matvec_kernel<T>), gmv, blk, 0, s, B, A, (const cx<T>*)cp, (const cx<T>*)w, nul, 0.5, gf, (long)Tn * per, n, m, Tn);
        }
        if (op.kind == TK_BD) {
            TRX_LAUNCH((tk_outer_bd_kernel<T>), dim3(cdiv_i(N, 256), 4, batch), blk, 0, s, (const cx<T>*)Gc, (const cx<T>*)gf, accumulate, Tn, N, m, bN, gop);
        } else {
            TkTerms<T> tm = {{Gc}, {gf}, {1.0}, 1};
            TRX_LAUNCH((tk_outer_kernel<T>), gn, blk, 0, s, tm, accumulate, Tn, n, m, gop);
        }
    }
    const dim3 gcol(cdiv_i(batch * per, 256));
    if (gsrc)       // the reflection port adds src[1] to every thickness' columns
        TRX_LAUNCH((tk_tsum_kernel<T>), gcol, blk, 0, s, refl ? (const cx<T>*)Gc : nul, accumulate, Tn, per, batch * per, gsrc + batch * per);
    if (gAB) {      // g = (A u + B cs) / 2 (transmission), (B cp + A w) / 2 (reflection)
        TkTerms<T> ta = {{gb}, {refl ? w : u}, {0.5}, 1}, tb = {{gb}, {refl ? cp : cs}, {0.5}, 1};
        TRX_LAUNCH((tk_outer_kernel<T>), gn, blk, 0, s, ta, accumulate, Tn, n, m, gAB);
        TRX_LAUNCH((tk_outer_kernel<T>), gn, blk, 0, s, tb, accumulate, Tn, n, m, gAB + bn);
    }
    if (!need_solve) {
        TRX_CHECK_LAUNCH();
        return TRX_OK;
    }
    TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, A, nul, gb, nul, nul, 0.5, ha, n, m, Tn);
    TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, B, nul, gb, nul, nul, 0.5, hb, n, m, Tn);
    const cx<T>* csb;                                   // cs-bar; lam holds cp-bar until the adjoint solve turns it into lambda
    if (!refl) {        // u-bar = A^H g-bar / 2 + rho_B^H cs-bar,  cs-bar = B^H g-bar / 2,  cp-bar = conj(x) u-bar
        csb = hb;
        TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, rhoB, nul, csb, nul, (const cx<T>*)ha, 1.0, ub, n, m, Tn);
        TRX_LAUNCH((tk_cscale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)ub, phase, nul, ldt, Tn, n, m, tv, lam);
    } else {            // w-bar = A^H g-bar / 2,  cs-bar = conj(x) w-bar,  u-bar = rho_B^H cs-bar,  cp-bar = B^H g-bar / 2 + conj(x) u-bar
        TRX_LAUNCH((tk_cscale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)ha, phase, nul, ldt, Tn, n, m, tv, csx);
        csb = csx;
        TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, rhoB, nul, csb, nul, nul, 1.0, ub, n, m, Tn);
        TRX_LAUNCH((tk_cscale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)ub, phase, (const cx<T>*)hb, ldt, Tn, n, m, tv, lam);
    }
    // lambda = K^-H cp-bar:  K^H = I - (X rho_B X)^H rho_A^H, one GEMM and one LU per (point, thickness) as in the forward
    TRX_LAUNCH((tk_mk_kernel<T>), gn, blk, 0, s, rhoB, phase, ldt, Tn, n, M, K);
    for (int b = 0; b < batch; ++b) {
        rc = gemm<T>(s, TRX_OP_C, TRX_OP_C, n, n, n, mone, M + (long)b * Tn * nn, n, nn, rhoA + (long)b * nn, n, 0L, one, K + (long)b * Tn * nn, n, nn, Tn);
        if (rc) return rc;
    }
    rc = lu_factor<T>(s, K, n, nn, n, piv, (int)BT, itmp); if (rc) return rc;
    TRX_LAUNCH(tk_info_kernel, dim3(cdiv_i(BT, 256)), blk, 0, s, (const int*)itmp, ldt, Tn, (int)BT, info);
    rc = lu_solve<T>(s, K, n, nn, n, piv, lam, m, per, m, (int)BT); if (rc) return rc;
    if (gsrc) TRX_LAUNCH((tk_tsum_kernel<T>), gcol, blk, 0, s, (const cx<T>*)lam, accumulate, Tn, per, batch * per, gsrc);
    if (grhoA) {        // K = I - rho_A M and M cp = w
        TkTerms<T> tm = {{lam}, {w}, {1.0}, 1};
        TRX_LAUNCH((tk_outer_kernel<T>), gn, blk, 0, s, tm, accumulate, Tn, n, m, grhoA);
    }
    if (grhoB || gphase) {      // mu = rho_A^H lambda is the gradient of M = X rho_B X applied to cp
        TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, rhoA, nul, (const cx<T>*)lam, nul, nul, 1.0, mu, n, m, Tn);
        TRX_LAUNCH((tk_cscale_kernel<T>), gflat, blk, 0, s, (const cx<T>*)mu, phase, nul, ldt, Tn, n, m, tv, nu);
    }
    if (grhoB) {
        TkTerms<T> tm = {{csb, nu}, {u, u}, {1.0, 1.0}, 2};
        TRX_LAUNCH((tk_outer_kernel<T>), gn, blk, 0, s, tm, accumulate, Tn, n, m, grhoB);
    }
    if (gphase) {
        TRX_LAUNCH((tk_matvec_ct_kernel<T>), gct, blk, 0, s, rhoB, nul, (const cx<T>*)nu, nul, nul, 1.0, rnu, n, m, Tn);
        TRX_LAUNCH((tk_gphase_kernel<T>), dim3(cdiv_i(BT * n, 256)), blk, 0, s, refl ? (const cx<T>*)ha : nul, (const cx<T>*)mu, (const cx<T>*)cs,
                   (const cx<T>*)ub, (const cx<T>*)rnu, (const cx<T>*)cp, ldt, Tn, n, m, BT * n, gphase);
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int thickness_columns_backward_d(hipStream_t s, const void* rhoL, const void* rhoR, const void* AB, const void* phase, int ldt, int Tn, int direction, int port,
                                 int lk, const void* lp, int rk, const void* rp, int m, int N, int batch, const void* cp, const void* gout, void* grhoL,
                                 void* grhoR, void* gsrc, void* gAB, void* gphase, void* gop, int accumulate, int* piv, int* info, void* ws) {
    TkOp<T> L, R;
    if (!tk_operand<T>(lk, lp, &L) || !tk_operand<T>(rk, rp, &R)) return TRX_ERR_ARG;
    return thickness_columns_backward_t<T>(s, (const cx<T>*)rhoL, (const cx<T>*)rhoR, (const cx<T>*)AB, (const cx<T>*)phase, ldt, Tn, direction, port, L, R, m,
                                           N, batch, (const cx<T>*)cp, (const cx<T>*)gout, (cx<T>*)grhoL, (cx<T>*)grhoR, (cx<T>*)gsrc, (cx<T>*)gAB,
                                           (cx<T>*)gphase, (cx<T>*)gop, accumulate, piv, info, (cx<T>*)ws);
}

bool tk_kind_ok(int kind, const void* p) { return kind == TK_ABSENT || ((kind == TK_BD || kind == TK_DENSE) && p); }

}  // namespace
}  // namespace trx

using namespace trx;

extern "C" size_t trx_thickness_prepare_ws_bytes(int dtype, int N, int batch) {
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * (size_t)batch * (2 * (size_t)N) * (2 * (size_t)N);
}

extern "C" int trx_thickness_prepare(int dtype, const void* W, const void* V, const void* vfinv, int left_kind, const void* left, int right_kind,
                                     const void* right, int direction, const int* cols, int m, int N, int batch, void* rhoL, void* rhoR, void* src,
                                     void* AB, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0 || batch < 0 || batch > 65535 || (direction != 0 && direction != 1) || m < 1 || m > TK_MAX_COLS || !cols) return TRX_ERR_ARG;
    if (!tk_kind_ok(left_kind, left) || !tk_kind_ok(right_kind, right)) return TRX_ERR_ARG;
    for (int q = 0; q < m; ++q)
        if (cols[q] < 0 || cols[q] >= 2 * N) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (batch == 0) return TRX_OK;
    if (!W || !V || !vfinv || !rhoL || !rhoR || !src || !AB || !piv || !info || !ws) return TRX_ERR_ARG;
    if (ws_bytes < trx_thickness_prepare_ws_bytes(dtype, N, batch)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return thickness_prepare_d<float>(s, W, V, vfinv, left_kind, left, right_kind, right, direction, cols, m, N, batch, rhoL, rhoR, src, AB, piv, info, ws);
    return thickness_prepare_d<double>(s, W, V, vfinv, left_kind, left, right_kind, right, direction, cols, m, N, batch, rhoL, rhoR, src, AB, piv, info, ws);
}

extern "C" size_t trx_thickness_columns_ws_bytes(int dtype, int N, int batch, int T, int m) {
    const size_t n = 2 * (size_t)N;
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * (size_t)batch * (size_t)T * (2 * n * n + 5 * n * (size_t)m);
}

// trx_thickness_columns and trx_thickness_columns_keep: one validation, one kernel sequence; cp == nullptr stores nothing more
static int tk_columns_entry(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T, int direction,
                            int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch, void* out, void* cp,
                            bool want_cp, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0 || batch < 0 || T < 0 || ldt < T || (long)batch * T > 65535 || (direction != 0 && direction != 1) || (port != 0 && port != 1) || m < 1 ||
        m > TK_MAX_COLS || (long)T * m > 65535L * TK_CT)
        return TRX_ERR_ARG;
    if (!tk_kind_ok(left_kind, left) || !tk_kind_ok(right_kind, right)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (batch == 0 || T == 0) return TRX_OK;
    if (!rhoL || !rhoR || !src || !AB || !phase || !out || !piv || !info || !ws || (want_cp && !cp)) return TRX_ERR_ARG;
    if (ws_bytes < trx_thickness_columns_ws_bytes(dtype, N, batch, T, m)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return thickness_columns_d<float>(s, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, cp, piv,
                                          info, ws);
    return thickness_columns_d<double>(s, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, cp, piv,
                                       info, ws);
}

extern "C" int trx_thickness_columns(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T,
                                     int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch,
                                     void* out, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    return tk_columns_entry(dtype, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, nullptr, false,
                            piv, info, ws, ws_bytes, stream);
}

extern "C" int trx_thickness_columns_keep(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T,
                                          int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N,
                                          int batch, void* out, void* cp, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    return tk_columns_entry(dtype, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, cp, true, piv,
                            info, ws, ws_bytes, stream);
}

extern "C" size_t trx_thickness_columns_backward_ws_bytes(int dtype, int N, int batch, int T, int m) {
    const size_t n = 2 * (size_t)N;
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * (size_t)batch * (size_t)T * (2 * n * n + TK_BWD_SKINNY * n * (size_t)m);
}

extern "C" int trx_thickness_columns_backward(int dtype, const void* rhoL, const void* rhoR, const void* AB, const void* phase, int ldt,
                                              int T, int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m,
                                              int N, int batch, const void* cp, const void* gout, void* grhoL, void* grhoR, void* gsrc, void* gAB,
                                              void* gphase, void* gop, int accumulate, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0 || batch < 0 || T < 0 || ldt < T || (long)batch * T > 65535 || (direction != 0 && direction != 1) || (port != 0 && port != 1) || m < 1 ||
        m > TK_MAX_COLS || (long)T * m > 65535L * TK_CT || (accumulate != 0 && accumulate != 1))
        return TRX_ERR_ARG;
    if (!tk_kind_ok(left_kind, left) || !tk_kind_ok(right_kind, right)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (batch == 0 || T == 0) return TRX_OK;
    if (!rhoL || !rhoR || !AB || !phase || !cp || !gout || !piv || !info || !ws) return TRX_ERR_ARG;
    if (ws_bytes < trx_thickness_columns_backward_ws_bytes(dtype, N, batch, T, m)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return thickness_columns_backward_d<float>(s, rhoL, rhoR, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, cp, gout,
                                                   grhoL, grhoR, gsrc, gAB, gphase, gop, accumulate, piv, info, ws);
    return thickness_columns_backward_d<double>(s, rhoL, rhoR, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, cp, gout,
                                                grhoL, grhoR, gsrc, gAB, gphase, gop, accumulate, piv, info, ws);
}
