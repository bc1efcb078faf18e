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
                        int direction, int port, const TkOp<T>& L, const TkOp<T>& R, int m, int N, int batch, cx<T>* out, int* piv, int* info, cx<T>* ws) {
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
                        int port, int lk, const void* lp, int rk, const void* rp, int m, int N, int batch, void* out, int* piv, int* info, void* ws) {
    TkOp<T> L, R;
    if (!tk_operand<T>(lk, lp, &L) || !tk_operand<T>(rk, rp, &R)) return TRX_ERR_ARG;
    return thickness_columns_t<T>(s, (const cx<T>*)rhoL, (const cx<T>*)rhoR, (const cx<T>*)src, (const cx<T>*)AB, (const cx<T>*)phase, ldt, Tn, direction, port,
                                  L, R, m, N, batch, (cx<T>*)out, piv, info, (cx<T>*)ws);
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

extern "C" int trx_thickness_columns(int dtype, const void* rhoL, const void* rhoR, const void* src, const void* AB, const void* phase, int ldt, int T,
                                     int direction, int port, int left_kind, const void* left, int right_kind, const void* right, int m, int N, int batch,
                                     void* out, int* piv, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0 || batch < 0 || T < 0 || ldt < T || (long)batch * T > 65535 || (direction != 0 && direction != 1) || (port != 0 && port != 1) || m < 1 ||
        m > TK_MAX_COLS || (long)T * m > 65535L * TK_CT)
        return TRX_ERR_ARG;
    if (!tk_kind_ok(left_kind, left) || !tk_kind_ok(right_kind, right)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (batch == 0 || T == 0) return TRX_OK;
    if (!rhoL || !rhoR || !src || !AB || !phase || !out || !piv || !info || !ws) return TRX_ERR_ARG;
    if (ws_bytes < trx_thickness_columns_ws_bytes(dtype, N, batch, T, m)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return thickness_columns_d<float>(s, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, piv, info, ws);
    return thickness_columns_d<double>(s, rhoL, rhoR, src, AB, phase, ldt, T, direction, port, left_kind, left, right_kind, right, m, N, batch, out, piv, info, ws);
}
