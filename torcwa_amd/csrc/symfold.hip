// Mirror-symmetry folding of a layer eigenproblem (include/trx.h: trx_sym_fold, trx_sym_unfold).
//
// T is the unitary symmetry-adapted basis of one or two mirrors: column j has at most four non-zeros wt[j][q] in the rows idx[j][q], and the
// columns are sorted by symmetry class (block k = columns off[k] .. off[k+1]-1).  For A commuting with the mirrors T^H A T is block diagonal.
//
//   fold    C = T^H A  (rows_kernel: row j of C is a combination of at most four rows of A, read and written along the rows: coalesced),
//           D = C T    (cols_kernel: column j of D is a combination of at most four columns of C; the lanes of a wave walk j, so the gathers of
//                       one row stay inside that row's n elements, and the plan entry of a column is loaded once for SF_ROWS rows);
//           the entries of D inside a diagonal block go to the packed output, the largest modulus of all the others is the residual.
//   unfold  W[:, block k] = T_k W_k: row j of W_k, scaled, is written to the at most four rows idx[off[k] + j][q] of W (the supports of the
//           columns of one block are disjoint, so every element of W has one writer); W is zeroed first for the rows a block does not reach.
//
// Traffic model per matrix (elements of `dtype`, the one of include/trx.h, DESIGN.md and the prof tags): fold reads the referenced rows of A once
// per referencing column (nblk n^2: 2 n^2 for one mirror, 4 n^2 for two, the rows of one orbit sit in different workgroups), writes and re-reads
// C (2 n^2) and writes sum_k n_k^2 ~ n^2 / nblk: (nblk + 2 + 1 / nblk) n^2 = 4.5 n^2 / 6.25 n^2; unfold writes W twice (zero fill, n^2 each) and
// reads sum_k n_k^2: (2 + 1 / nblk) n^2.  Both are far below one GEMM of the same size.  Maxima are exact and order-independent;
// per workgroup one partial goes to the workspace and a second kernel combines them: deterministic, no atomics.
//
// Adjoints (trx_sym_fold_backward, trx_sym_unfold_backward; PyTorch's convention: Y = L(X) has gX = L^H(gY)).
//   fold backward    gA = sum_k T_k gB_k T_k^H.  A row r of the original basis lies in at most one column of T per block, so with the ROW plan
//                    (ridx[r][k], rwt[r][k]: that column of block k and T's entry, weight 0 if there is none) this is a gather with one writer
//                    per element: gA[r, c] = sum_k rwt[r][k] gB_k[ridx[r][k] - off[k], ridx[c][k] - off[k]] conj(rwt[c][k]).  The lanes of a wave
//                    walk c: the gathers of one row stay inside one row of gB_k, the writes are coalesced.  No zero fill, workspace or atomics.
//   unfold backward  gW_k = T_k^H gW[:, off[k]:off[k+1]]: row j of gW_k is a combination of the at most four rows idx[off[k] + j][q] of gW with
//                    conj(wt), read and written along the rows; glam_k is the matching slice of glam.
// Traffic model per matrix: fold backward writes n^2, reads one element of gB_k per block whose weights are both non-zero (at most nblk n^2; the
// distinct elements are sum_k n_k^2 ~ n^2 / nblk and the re-reads of an orbit fall in the same rows) and 2 n plan rows per SF_ROWS rows:
// counted as (1 + nblk) n^2.  unfold backward reads every element of gW once (n^2: the supports of the columns of one block are disjoint) and
// writes sum_k n_k^2 ~ n^2 / nblk: (1 + 1 / nblk) n^2.
//
// Sector folds (trx_sym_fold_pair, trx_sym_fold_pair_bd): out = T_kl^H M T_kr for ONE pair of blocks, rectangular when their sizes differ.
//   One pass, no n x n intermediate: out[i, j] = sum_p sum_q conj(wt[I][p]) M[idx[I][p], idx[J][q]] wt[J][q], I = off[kl] + i, J = off[kr] + j:
//   at most 16 elements of M per output element.  A workgroup owns SF_ROWS output rows and stages their plan entries in LDS once; the lanes of a
//   wave walk j, so the gathers of one output row stay inside the at most four rows idx[I][p] of M and the writes are coalesced.  _bd: M is
//   2x2-block-diagonal and given as its four diagonals [4][batch][N]; element (r, c) is d[2 (r >= N) + (c >= N)][r mod N] where r = c mod N,
//   0 elsewhere; the dense n_kl x n_kr result is written, zeros included.  The block sizes live in device memory (off), so the grid covers
//   ceil(n / SF_ROWS) row groups and the groups beyond n_kl leave at once.  No workspace, no atomics: every element has one writer.
// Traffic model per matrix: at most 16 n_kl n_kr elements read and n_kl n_kr written, 17 (n / nblk)^2: about n^2 per pair for two mirrors.  _bd
//   reads the 4 N diagonal entries (the 16 candidates of an element are index tests, not loads) and writes n_kl n_kr.
//
// Adjoints of the sector folds (trx_sym_fold_pairs_backward, trx_sym_fold_pair_bd_backward), from the ROW plan like fold backward.
//   pairs backward   gM = sum_p T_kl_p G_p T_kr_p^H for up to SF_MAXPAIRS pairs in ONE pass (a layer folds P on the pairs (k, k') and Q on (k', k)
//                    of every block): gM[r, c] = sum_p rwt[r][kl_p] G_p[ridx[r][kl_p] - off[kl_p], ridx[c][kr_p] - off[kr_p]] conj(rwt[c][kr_p]).
//                    The lane mapping of fold backward: the lanes of a wave walk c, the writes are coalesced and the gathers of one row stay inside
//                    one row of each G_p.  The pair table (pointers, kl, kr) is a kernel argument passed by value; a null pointer is a pair without
//                    a gradient.  One writer per element, every element written: no zero fill, workspace or atomics.
//   pair_bd backward the four diagonals of T_kl G T_kr^H: one thread per m, the elements (p N + m, q N + m), p, q in {0, 1}.
// Traffic model per matrix: pairs backward writes n^2 and reads one element of G_p per element and pair whose two weights are non-zero: counted
// as (1 + npairs) n^2 at most -- for the pairs (k, k') of all k every (r, c) meets up to nblk pairs, but the distinct elements are
// sum_k n_k n_k' ~ n^2 / nblk and the re-reads of an orbit fall in the same rows; 2 n plan rows per SF_ROWS rows.  HBM-bound.  pair_bd backward
// reads at most 4 N elements of G (scattered: one per diagonal entry) and writes 4 N.
#include "common.hpp"
#include "prof.hpp"

using namespace trx;

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_ROWS = 8;        // rows of the output per workgroup
constexpr int SF_MAXBLK = 4;
constexpr int SF_MAXPAIRS = 16;   // pairs of one trx_sym_fold_pairs_backward call: all nblk^2 of two mirrors

// Block offsets and the packing of the per-block arrays: blocks of equal size form one group, groups in the order of their first block;
// a group of g blocks of size s is one contiguous [g, batch, u] region, u = s * s (matrices) or s (eigenvalues).
struct SymLayout {
    int off[SF_MAXBLK + 1];
    long base2[SF_MAXBLK], base1[SF_MAXBLK];   // element offset of (block k, batch entry 0)
    int ok;
};

__device__ __forceinline__ SymLayout sym_layout(const int* __restrict__ off, int nblk, int n, int batch) {
    SymLayout L;
    L.ok = 1;
#pragma unroll
    for (int k = 0; k <= SF_MAXBLK; ++k) L.off[k] = k <= nblk ? off[k] : n;
    if (L.off[0] != 0 || L.off[nblk] != n) L.ok = 0;
#pragma unroll
    for (int k = 0; k < SF_MAXBLK; ++k)
        if (k < nblk && L.off[k + 1] < L.off[k]) L.ok = 0;
#pragma unroll
    for (int k = 0; k < SF_MAXBLK; ++k) {
        L.base2[k] = L.base1[k] = 0;
        if (k >= nblk || !L.ok) continue;
        const long s = L.off[k + 1] - L.off[k];
        long acc2 = 0, acc1 = 0;
        for (int f = 0; f < nblk; ++f) {
            const long sf = L.off[f + 1] - L.off[f];
            bool first = true;
            for (int e = 0; e < f; ++e) first = first && (L.off[e + 1] - L.off[e] != sf);
            if (!first) continue;
            if (sf == s) {                                   // the group of block k: t blocks of this size come before it
                long t = 0;
                for (int e = 0; e < k; ++e) t += (L.off[e + 1] - L.off[e] == s);
                L.base2[k] = acc2 + t * batch * s * s;
                L.base1[k] = acc1 + t * batch * s;
                break;
            }
            long g = 0;
            for (int e = 0; e < nblk; ++e) g += (L.off[e + 1] - L.off[e] == sf);
            acc2 += g * batch * sf * sf;
            acc1 += g * batch * sf;
        }
    }
    return L;
}

__device__ __forceinline__ int block_of(const SymLayout& L, int nblk, int j) {
    int k = 0;
#pragma unroll
    for (int e = 1; e < SF_MAXBLK; ++e) k += (e < nblk && j >= L.off[e]);
    return k;
}

template <class T> __device__ __forceinline__ bool nonzero(cx<T> w) { return w.x != T(0) || w.y != T(0); }
__device__ __forceinline__ int clamp_row(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// largest value of the workgroup in thread 0
__device__ __forceinline__ double block_max(double v) {
    __shared__ double red[SF_THREADS / 64];
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int w = 1; w < SF_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;
    return m;
}

// C = T^H A.  grid (ceil(n / SF_ROWS), batch); amax2 [batch, gridDim.x]: largest |A|^2 among the elements read.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_rows_kernel(const cx<T>* __restrict__ A, const int* __restrict__ idx, const cx<T>* __restrict__ wt,
                                                              int n, cx<T>* __restrict__ C, double* __restrict__ amax2) {
    const int tid = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * SF_ROWS;
    const cx<T>* Ab = A + (long)b * n * n;
    cx<T>* Cb = C + (long)b * n * n;
    double mx = 0.0;
    for (int rr = 0; rr < SF_ROWS && j0 + rr < n; ++rr) {
        const int j = j0 + rr;
        int s[4];
        cx<T> w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[q] = clamp_row(idx[j * 4 + q], n);
            w[q] = conj(wt[j * 4 + q]);
        }
        for (int col = tid; col < n; col += SF_THREADS) {
            cx<T> acc(T(0), T(0));
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (nonzero(w[q])) {                                                // wave-uniform
                    const cx<T> a = Ab[(long)s[q] * n + col];
                    cfma(acc, w[q], a);
                    const double m = (double)a.x * (double)a.x + (double)a.y * (double)a.y;
                    mx = m > mx ? m : mx;
                }
            Cb[(long)j * n + col] = acc;
        }
    }
    mx = block_max(mx);
    if (tid == 0) amax2[(long)b * gridDim.x + blockIdx.x] = mx;
}

// D = C T: diagonal blocks to `blocks`, the largest |D|^2 outside them to omax2 [batch, gridDim.x] (NaN for a malformed plan).
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_cols_kernel(const cx<T>* __restrict__ C, const int* __restrict__ idx, const cx<T>* __restrict__ wt,
                                                              const int* __restrict__ off, int nblk, int n, int batch, cx<T>* __restrict__ blocks,
                                                              double* __restrict__ omax2) {
    const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * SF_ROWS;
    const SymLayout L = sym_layout(off, nblk, n, batch);
    const cx<T>* Cb = C + (long)b * n * n;
    const int rows = n - r0 < SF_ROWS ? n - r0 : SF_ROWS;
    double mx = 0.0;
    if (L.ok) {
        for (int j = tid; j < n; j += SF_THREADS) {
            int s[4];
            cx<T> w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[q] = clamp_row(idx[j * 4 + q], n);
                w[q] = wt[j * 4 + q];
            }
            const int kj = block_of(L, nblk, j);
            const long sj = L.off[kj + 1] - L.off[kj];
            cx<T>* dst = blocks + L.base2[kj] + (long)b * sj * sj + (j - L.off[kj]);
            for (int rr = 0; rr < rows; ++rr) {
                const int r = r0 + rr;
                const cx<T>* Crow = Cb + (long)r * n;
                cx<T> acc(T(0), T(0));
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (nonzero(w[q])) cfma(acc, Crow[s[q]], w[q]);
                if (block_of(L, nblk, r) == kj) {
                    dst[(long)(r - L.off[kj]) * sj] = acc;
                } else {
                    const double m = (double)acc.x * (double)acc.x + (double)acc.y * (double)acc.y;
                    mx = m > mx ? m : mx;
                }
            }
        }
    }
    mx = block_max(mx);
    if (tid == 0) omax2[(long)b * gridDim.x + blockIdx.x] = L.ok ? mx : __builtin_nan("");
}

// resid[b] = sqrt(max omax2) / sqrt(max amax2)
__global__ __launch_bounds__(64) void sym_resid_kernel(const double* __restrict__ amax2, const double* __restrict__ omax2, int groups, int batch,
                                                       double* __restrict__ resid) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double a = 0.0, o = 0.0;
    bool bad = false;
    for (int g = 0; g < groups; ++g) {
        const double va = amax2[(long)b * groups + g], vo = omax2[(long)b * groups + g];
        bad = bad || va != va || vo != vo;
        a = va > a ? va : a;
        o = vo > o ? vo : o;
    }
    resid[b] = bad ? __builtin_nan("") : (a > 0.0 ? sqrt(o) / sqrt(a) : 0.0);
}

// W[idx[J][q], off[k] + c] = wt[J][q] Wk[j, c] for column J = off[k] + j of T; lam[J] = lamk[j].  grid (ceil(n / SF_ROWS), batch); W zeroed before.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_unfold_kernel(const cx<T>* __restrict__ Wk, const cx<T>* __restrict__ lamk, const int* __restrict__ idx,
                                                                const cx<T>* __restrict__ wt, const int* __restrict__ off, int nblk, int n, int batch,
                                                                cx<T>* __restrict__ W, cx<T>* __restrict__ lam) {
    const int tid = threadIdx.x, b = blockIdx.y, J0 = blockIdx.x * SF_ROWS;
    const SymLayout L = sym_layout(off, nblk, n, batch);
    if (!L.ok) return;
    cx<T>* Wb = W + (long)b * n * n;
    for (int rr = 0; rr < SF_ROWS && J0 + rr < n; ++rr) {
        const int J = J0 + rr;
        const int k = block_of(L, nblk, J);
        const long s = L.off[k + 1] - L.off[k];
        const int j = J - L.off[k];
        const cx<T>* src = Wk + L.base2[k] + (long)b * s * s + (long)j * s;
        int rw[4];
        cx<T> w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rw[q] = clamp_row(idx[J * 4 + q], n);
            w[q] = wt[J * 4 + q];
        }
        for (int c = tid; c < (int)s; c += SF_THREADS) {
            const cx<T> v = src[c];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (nonzero(w[q])) Wb[(long)rw[q] * n + L.off[k] + c] = w[q] * v;
        }
        if (tid == 0) lam[(long)b * n + J] = lamk[L.base1[k] + (long)b * s + j];
    }
}

// gA = sum_k T_k gB_k T_k^H from the row plan.  grid (ceil(n / SF_ROWS), batch); a malformed off fills gA with NaN.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_fold_bwd_kernel(const cx<T>* __restrict__ gB, const int* __restrict__ ridx, const cx<T>* __restrict__ rwt,
                                                                  const int* __restrict__ off, int nblk, int n, int batch, cx<T>* __restrict__ gA) {
    const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * SF_ROWS;
    const SymLayout L = sym_layout(off, nblk, n, batch);
    cx<T>* Ab = gA + (long)b * n * n;
    const int rows = n - r0 < SF_ROWS ? n - r0 : SF_ROWS;
    if (!L.ok) {
        const T bad = (T)__builtin_nan("");
        for (int rr = 0; rr < rows; ++rr)
            for (int c = tid; c < n; c += SF_THREADS) Ab[(long)(r0 + rr) * n + c] = cx<T>(bad, bad);
        return;
    }
    for (int c = tid; c < n; c += SF_THREADS) {
        int lc[SF_MAXBLK];
        cx<T> wc[SF_MAXBLK];
#pragma unroll
        for (int k = 0; k < SF_MAXBLK; ++k) {
            const int s = L.off[k + 1] - L.off[k];
            wc[k] = cx<T>(T(0), T(0));
            lc[k] = 0;
            if (k < nblk && s > 0) {
                wc[k] = conj(rwt[c * 4 + k]);
                lc[k] = clamp_row(ridx[c * 4 + k] - L.off[k], s);
            }
        }
        for (int rr = 0; rr < rows; ++rr) {
            const int r = r0 + rr;
            cx<T> acc(T(0), T(0));
#pragma unroll
            for (int k = 0; k < SF_MAXBLK; ++k) {
                const int s = L.off[k + 1] - L.off[k];
                if (k >= nblk || s <= 0) continue;
                const cx<T> wr = rwt[r * 4 + k];                                        // wave-uniform
                if (nonzero(wr) && nonzero(wc[k])) {
                    const int lr = clamp_row(ridx[r * 4 + k] - L.off[k], s);
                    const cx<T> g = gB[L.base2[k] + (long)b * s * s + (long)lr * s + lc[k]];
                    cfma(acc, wr * g, wc[k]);
                }
            }
            Ab[(long)r * n + c] = acc;
        }
    }
}

// gWk[j, c] = sum_q conj(wt[J][q]) gW[idx[J][q], off[k] + c] for column J = off[k] + j of T; glamk[j] = glam[J].  grid (ceil(n / SF_ROWS), batch).
// A malformed off: the packing of gWk is not defined, so it is left alone and glamk (batch n elements whatever the blocks) is filled with NaN.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_unfold_bwd_kernel(const cx<T>* __restrict__ gW, const cx<T>* __restrict__ glam, const int* __restrict__ idx,
                                                                    const cx<T>* __restrict__ wt, const int* __restrict__ off, int nblk, int n, int batch,
                                                                    cx<T>* __restrict__ gWk, cx<T>* __restrict__ glamk) {
    const int tid = threadIdx.x, b = blockIdx.y, J0 = blockIdx.x * SF_ROWS;
    const SymLayout L = sym_layout(off, nblk, n, batch);
    if (!L.ok) {
        const T bad = (T)__builtin_nan("");
        if (tid < SF_ROWS && J0 + tid < n) glamk[(long)b * n + J0 + tid] = cx<T>(bad, bad);
        return;
    }
    const cx<T>* Gb = gW + (long)b * n * n;
    for (int rr = 0; rr < SF_ROWS && J0 + rr < n; ++rr) {
        const int J = J0 + rr;
        const int k = block_of(L, nblk, J);
        const long s = L.off[k + 1] - L.off[k];
        const int j = J - L.off[k];
        cx<T>* dst = gWk + L.base2[k] + (long)b * s * s + (long)j * s;
        int rw[4];
        cx<T> w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rw[q] = clamp_row(idx[J * 4 + q], n);
            w[q] = conj(wt[J * 4 + q]);
        }
        for (int c = tid; c < (int)s; c += SF_THREADS) {
            cx<T> acc(T(0), T(0));
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (nonzero(w[q])) cfma(acc, w[q], Gb[(long)rw[q] * n + L.off[k] + c]);     // wave-uniform
            dst[c] = acc;
        }
        if (tid == 0) glamk[L.base1[k] + (long)b * s + j] = glam[(long)b * n + J];
    }
}

// The extent of blocks kl (rows) and kr (columns) of a sector fold, from off as given: n_k = off[k+1] - off[k], held inside [0, n] so that a
// malformed off (ok = 0) still names the out array the caller sized from the same numbers.
struct PairExtent {
    int ok, ol, nl, oc, nr;
};

__device__ __forceinline__ PairExtent pair_extent(const int* __restrict__ off, int nblk, int n, int kl, int kr) {
    PairExtent E;
    E.ok = off[0] == 0 && off[nblk] == n;
    for (int k = 0; k < nblk; ++k) E.ok = E.ok && off[k + 1] >= off[k];
    E.ol = off[kl];
    E.oc = off[kr];
    const long dl = (long)off[kl + 1] - E.ol, dr = (long)off[kr + 1] - E.oc;
    E.nl = dl < 0 ? 0 : (dl > n ? n : (int)dl);
    E.nr = dr < 0 ? 0 : (dr > n ? n : (int)dr);
    return E;
}

// out[b] = T_kl^H M[b] T_kr.  grid (ceil(n / SF_ROWS), batch).  BD: src = the four diagonals [4][batch][N] of a 2x2-block-diagonal M, n = 2 N.
template <class T, bool BD>
__global__ __launch_bounds__(SF_THREADS) void sym_fold_pair_kernel(const cx<T>* __restrict__ src, const int* __restrict__ idx,
                                                                   const cx<T>* __restrict__ wt, const int* __restrict__ off, int nblk, int n,
                                                                   int batch, int kl, int kr, cx<T>* __restrict__ out) {
    __shared__ int srow[SF_ROWS * 4];
    __shared__ T swx[SF_ROWS * 4], swy[SF_ROWS * 4];
    const int tid = threadIdx.x, b = blockIdx.y, i0 = blockIdx.x * SF_ROWS;
    const PairExtent E = pair_extent(off, nblk, n, kl, kr);
    if (i0 >= E.nl || E.nr == 0) return;                                                // the whole workgroup: before any barrier
    const int rows = E.nl - i0 < SF_ROWS ? E.nl - i0 : SF_ROWS;
    cx<T>* ob = out + ((long)b * E.nl + i0) * E.nr;
    if (!E.ok) {
        const T bad = (T)__builtin_nan("");
        for (long e = tid; e < (long)rows * E.nr; e += SF_THREADS) ob[e] = cx<T>(bad, bad);
        return;
    }
    if (tid < rows * 4) {                                                               // the plan entries of this group's rows, once
        const int I = E.ol + i0 + (tid >> 2);
        const cx<T> w = conj(wt[I * 4 + (tid & 3)]);
        srow[tid] = clamp_row(idx[I * 4 + (tid & 3)], n);
        swx[tid] = w.x;
        swy[tid] = w.y;
    }
    __syncthreads();
    const int N = n >> 1;
    const cx<T>* Mb = BD ? src + (long)b * N : src + (long)b * n * n;
    for (int j = tid; j < E.nr; j += SF_THREADS) {
        const int J = E.oc + j;
        int c[4];
        cx<T> w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            c[q] = clamp_row(idx[J * 4 + q], n);
            w[q] = wt[J * 4 + q];
        }
        for (int rr = 0; rr < rows; ++rr) {
            cx<T> acc(T(0), T(0));
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const cx<T> wl(swx[rr * 4 + p], swy[rr * 4 + p]);
                if (!nonzero(wl)) continue;                                             // wave-uniform
                const int r = srow[rr * 4 + p];
                cx<T> s(T(0), T(0));
                if (BD) {
                    const int rm = r >= N ? r - N : r;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cm = c[q] >= N ? c[q] - N : c[q];
                        if (nonzero(w[q]) && cm == rm) cfma(s, Mb[(long)(2 * (r >= N) + (c[q] >= N)) * batch * N + rm], w[q]);
                    }
                } else {
                    const cx<T>* Mrow = Mb + (long)r * n;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (nonzero(w[q])) cfma(s, Mrow[c[q]], w[q]);
                }
                cfma(acc, wl, s);
            }
            ob[(long)rr * E.nr + j] = acc;
        }
    }
}

// The pair table of trx_sym_fold_pairs_backward: a kernel argument, passed by value.  g[p] null: a pair whose output took no gradient.
struct PairTable {
    const void* g[SF_MAXPAIRS];
    signed char kl[SF_MAXPAIRS], kr[SF_MAXPAIRS];
    int np;
};

// Offset and size of every block from off as given (sizes held inside [0, n], 0 for k >= nblk), and pair_extent's verdict on off.
struct BlockExtents {
    int ok, o[SF_MAXBLK], s[SF_MAXBLK];
};

__device__ __forceinline__ BlockExtents block_extents(const int* __restrict__ off, int nblk, int n) {
    BlockExtents E;
    E.ok = off[0] == 0 && off[nblk] == n;
#pragma unroll
    for (int k = 0; k < SF_MAXBLK; ++k) {
        E.o[k] = E.s[k] = 0;
        if (k >= nblk) continue;
        E.ok = E.ok && off[k + 1] >= off[k];
        const long d = (long)off[k + 1] - off[k];
        E.o[k] = off[k];
        E.s[k] = d < 0 ? 0 : (d > n ? n : (int)d);
    }
    return E;
}

// a[k] for a wave-uniform k, by selects: the array stays in registers
template <class V> __device__ __forceinline__ V pick(const V (&a)[SF_MAXBLK], int k) {
    V v = a[0];
#pragma unroll
    for (int e = 1; e < SF_MAXBLK; ++e) v = k == e ? a[e] : v;
    return v;
}

// gM = sum_p T_kl_p G_p T_kr_p^H from the row plan.  grid (ceil(n / SF_ROWS), batch); a malformed off fills gM with NaN.  The table reaches LDS
// through thread 0 with static indices (a run-time index into a by-value argument would go through scratch); then one thread per (row, pair)
// stages what the row contributes: T's entry and the row of G_p[b] it reads, null where the pair does not reach the row.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_fold_pairs_bwd_kernel(const PairTable P, const int* __restrict__ ridx, const cx<T>* __restrict__ rwt,
                                                                        const int* __restrict__ off, int nblk, int n, int batch,
                                                                        cx<T>* __restrict__ gM) {
    __shared__ const void* sg[SF_MAXPAIRS];
    __shared__ int skl[SF_MAXPAIRS], skr[SF_MAXPAIRS];
    __shared__ const void* srow[SF_ROWS * SF_MAXPAIRS];
    __shared__ T swx[SF_ROWS * SF_MAXPAIRS], swy[SF_ROWS * SF_MAXPAIRS];
    const int tid = threadIdx.x, b = blockIdx.y, r0 = blockIdx.x * SF_ROWS;
    const BlockExtents E = block_extents(off, nblk, n);
    cx<T>* Mb = gM + (long)b * n * n;
    const int rows = n - r0 < SF_ROWS ? n - r0 : SF_ROWS;
    if (!E.ok) {                                                                        // the whole workgroup: before any barrier
        const T bad = (T)__builtin_nan("");
        for (int rr = 0; rr < rows; ++rr)
            for (int c = tid; c < n; c += SF_THREADS) Mb[(long)(r0 + rr) * n + c] = cx<T>(bad, bad);
        return;
    }
    if (tid == 0) {
#pragma unroll
        for (int p = 0; p < SF_MAXPAIRS; ++p) {
            sg[p] = p < P.np ? P.g[p] : nullptr;
            skl[p] = P.kl[p];
            skr[p] = P.kr[p];
        }
    }
    __syncthreads();
    if (tid < SF_ROWS * SF_MAXPAIRS) {
        const int rr = tid / SF_MAXPAIRS, p = tid % SF_MAXPAIRS;
        const cx<T>* row = nullptr;
        cx<T> wr(T(0), T(0));
        if (rr < rows && sg[p]) {
            const int kl = skl[p], sl = pick(E.s, kl), sr = pick(E.s, skr[p]);
            if (sl > 0 && sr > 0) {
                wr = rwt[(r0 + rr) * 4 + kl];
                if (nonzero(wr)) row = (const cx<T>*)sg[p] + ((long)b * sl + clamp_row(ridx[(r0 + rr) * 4 + kl] - pick(E.o, kl), sl)) * sr;
            }
        }
        srow[tid] = row;
        swx[tid] = wr.x;
        swy[tid] = wr.y;
    }
    __syncthreads();
    for (int c = tid; c < n; c += SF_THREADS) {
        int lc[SF_MAXBLK];
        cx<T> wc[SF_MAXBLK];
#pragma unroll
        for (int k = 0; k < SF_MAXBLK; ++k) {
            wc[k] = cx<T>(T(0), T(0));
            lc[k] = 0;
            if (k < nblk && E.s[k] > 0) {
                wc[k] = conj(rwt[c * 4 + k]);
                lc[k] = clamp_row(ridx[c * 4 + k] - E.o[k], E.s[k]);
            }
        }
        for (int rr = 0; rr < rows; ++rr) {
            cx<T> acc(T(0), T(0));
            for (int p = 0; p < P.np; ++p) {
                const cx<T>* row = (const cx<T>*)srow[rr * SF_MAXPAIRS + p];            // the same for every lane
                if (!row) continue;
                const int kr = skr[p];
                const cx<T> w2 = pick(wc, kr);
                if (nonzero(w2)) cfma(acc, cx<T>(swx[rr * SF_MAXPAIRS + p], swy[rr * SF_MAXPAIRS + p]) * row[pick(lc, kr)], w2);
            }
            Mb[(long)(r0 + rr) * n + c] = acc;
        }
    }
}

// gbd[2 p + q][b][m] = element (p N + m, q N + m) of T_kl G[b] T_kr^H.  grid (ceil(N / SF_THREADS), batch); a malformed off fills gbd with NaN.
template <class T>
__global__ __launch_bounds__(SF_THREADS) void sym_fold_pair_bd_bwd_kernel(const cx<T>* __restrict__ G, const int* __restrict__ ridx,
                                                                          const cx<T>* __restrict__ rwt, const int* __restrict__ off, int nblk, int n,
                                                                          int batch, int kl, int kr, cx<T>* __restrict__ gbd) {
    const int N = n >> 1, m = blockIdx.x * SF_THREADS + threadIdx.x, b = blockIdx.y;
    if (m >= N) return;
    const PairExtent E = pair_extent(off, nblk, n, kl, kr);
    const T bad = (T)__builtin_nan("");
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
        const int r = (pq >> 1) * N + m, c = (pq & 1) * N + m;
        cx<T> v(T(0), T(0));
        if (!E.ok) {
            v = cx<T>(bad, bad);
        } else if (E.nl > 0 && E.nr > 0) {
            const cx<T> wr = rwt[r * 4 + kl], wc = conj(rwt[c * 4 + kr]);
            if (nonzero(wr) && nonzero(wc)) {
                const int lr = clamp_row(ridx[r * 4 + kl] - E.ol, E.nl), lc = clamp_row(ridx[c * 4 + kr] - E.oc, E.nr);
                v = (wr * G[((long)b * E.nl + lr) * E.nr + lc]) * wc;
            }
        }
        gbd[((long)pq * batch + b) * N + m] = v;
    }
}

size_t part_bytes(int n, int batch) { return sizeof(double) * 2 * (size_t)cdiv_i(n, SF_ROWS) * (size_t)batch; }

template <class T>
int sym_fold_t(hipStream_t st, const cx<T>* A, int n, int batch, const int* idx, const cx<T>* wt, const int* off, int nblk, cx<T>* blocks,
               double* resid, char* ws) {
    const int groups = cdiv_i(n, SF_ROWS);
    double* amax2 = (double*)ws;
    double* omax2 = amax2 + (size_t)groups * batch;
    cx<T>* C = (cx<T>*)(ws + ((part_bytes(n, batch) + 15) & ~(size_t)15));
    const double nn = (double)n * n * batch;
    ProfScope prof(PROF_SYM_FOLD, st, 8.0 * 8.0 * nn, sizeof(cx<T>) * (nblk + 2.0 + 1.0 / nblk) * nn);   // A once per referencing column, C out and in, blocks
    const dim3 grid(groups, batch);
    TRX_LAUNCH((sym_rows_kernel<T>), grid, dim3(SF_THREADS), 0, st, A, idx, wt, n, C, amax2);
    TRX_CHECK_LAUNCH();
    TRX_LAUNCH((sym_cols_kernel<T>), grid, dim3(SF_THREADS), 0, st, (const cx<T>*)C, idx, wt, off, nblk, n, batch, blocks, omax2);
    TRX_CHECK_LAUNCH();
    TRX_LAUNCH(sym_resid_kernel, dim3(cdiv_i(batch, 64)), dim3(64), 0, st, (const double*)amax2, (const double*)omax2, groups, batch, resid);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int sym_unfold_t(hipStream_t st, const cx<T>* Wk, const cx<T>* lamk, int n, int batch, const int* idx, const cx<T>* wt, const int* off, int nblk,
                 cx<T>* W, cx<T>* lam) {
    const double nn = (double)n * n * batch;
    ProfScope prof(PROF_SYM_UNFOLD, st, 0.0, sizeof(cx<T>) * (2.0 + 1.0 / (nblk > 0 ? nblk : 1)) * nn);
    if (hipMemsetAsync(W, 0, sizeof(cx<T>) * (size_t)n * n * batch, st) != hipSuccess) return TRX_ERR_LAUNCH;
    TRX_LAUNCH((sym_unfold_kernel<T>), dim3(cdiv_i(n, SF_ROWS), batch), dim3(SF_THREADS), 0, st, Wk, lamk, idx, wt, off, nblk, n, batch, W, lam);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int sym_fold_bwd_t(hipStream_t st, const cx<T>* gB, int n, int batch, const int* ridx, const cx<T>* rwt, const int* off, int nblk, cx<T>* gA) {
    const double nn = (double)n * n * batch;
    ProfScope prof(PROF_SYM_FOLD_BWD, st, 8.0 * 2.0 * nblk * nn, sizeof(cx<T>) * (1.0 + nblk) * nn);
    TRX_LAUNCH((sym_fold_bwd_kernel<T>), dim3(cdiv_i(n, SF_ROWS), batch), dim3(SF_THREADS), 0, st, gB, ridx, rwt, off, nblk, n, batch, gA);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int sym_unfold_bwd_t(hipStream_t st, const cx<T>* gW, const cx<T>* glam, int n, int batch, const int* idx, const cx<T>* wt, const int* off, int nblk,
                     cx<T>* gWk, cx<T>* glamk) {
    const double nn = (double)n * n * batch;
    ProfScope prof(PROF_SYM_UNFOLD_BWD, st, 8.0 * nn, sizeof(cx<T>) * (1.0 + 1.0 / nblk) * nn);
    TRX_LAUNCH((sym_unfold_bwd_kernel<T>), dim3(cdiv_i(n, SF_ROWS), batch), dim3(SF_THREADS), 0, st, gW, glam, idx, wt, off, nblk, n, batch, gWk,
               glamk);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T, bool BD>
int sym_fold_pair_t(hipStream_t st, const cx<T>* src, int n, int batch, const int* idx, const cx<T>* wt, const int* off, int nblk, int kl, int kr,
                    cx<T>* out) {
    const double blk = ((double)n / nblk) * ((double)n / nblk) * batch;                 // n_kl n_kr of the model: the sizes stay on the device
    ProfScope prof(BD ? PROF_SYM_FOLD_PAIR_BD : PROF_SYM_FOLD_PAIR, st, 8.0 * 20.0 * blk,
                   sizeof(cx<T>) * (BD ? 2.0 * n * batch + blk : 17.0 * blk));
    TRX_LAUNCH((sym_fold_pair_kernel<T, BD>), dim3(cdiv_i(n, SF_ROWS), batch), dim3(SF_THREADS), 0, st, src, idx, wt, off, nblk, n, batch, kl, kr,
               out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int sym_fold_pairs_bwd_t(hipStream_t st, const PairTable& P, int n, int batch, const int* ridx, const cx<T>* rwt, const int* off, int nblk, cx<T>* gM) {
    const double nn = (double)n * n * batch;
    int live = 0;
    for (int p = 0; p < P.np; ++p) live += P.g[p] != nullptr;
    ProfScope prof(PROF_SYM_FOLD_PAIRS_BWD, st, 8.0 * 2.0 * live * nn, sizeof(cx<T>) * (1.0 + live) * nn);   // gM out, one element per pair at most
    TRX_LAUNCH((sym_fold_pairs_bwd_kernel<T>), dim3(cdiv_i(n, SF_ROWS), batch), dim3(SF_THREADS), 0, st, P, ridx, rwt, off, nblk, n, batch, gM);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int sym_fold_pair_bd_bwd_t(hipStream_t st, const cx<T>* G, int n, int batch, const int* ridx, const cx<T>* rwt, const int* off, int nblk, int kl,
                           int kr, cx<T>* gbd) {
    const double e = 2.0 * n * batch;                                                  // 4 N batch diagonal entries
    ProfScope prof(PROF_SYM_FOLD_PAIR_BD_BWD, st, 8.0 * 2.0 * e, sizeof(cx<T>) * 2.0 * e);                   // one element of G in, one entry out
    TRX_LAUNCH((sym_fold_pair_bd_bwd_kernel<T>), dim3(cdiv_i(n >> 1, SF_THREADS), batch), dim3(SF_THREADS), 0, st, G, ridx, rwt, off, nblk, n, batch,
               kl, kr, gbd);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

int check_common(int dtype, int n, int batch, int nblk) {
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (n < 1 || batch < 0 || batch > 65535 || nblk < 1 || nblk > SF_MAXBLK) return TRX_ERR_ARG;
    if ((size_t)n * (size_t)n >= ((size_t)1 << 31)) return TRX_ERR_ARG;            // 4 n stays inside int as well
    return TRX_OK;
}

}  // namespace

extern "C" size_t trx_sym_fold_ws_bytes(int dtype, int n, int batch) {
    if (n < 0 || batch < 0 || (dtype != TRX_C64 && dtype != TRX_C128)) return 0;
    const size_t el = dtype == TRX_C128 ? 16 : 8;
    return ((part_bytes(n, batch) + 15) & ~(size_t)15) + el * (size_t)n * (size_t)n * (size_t)batch;
}

extern "C" int trx_sym_fold(int dtype, const void* A, int n, int batch, const int* idx, const void* wt, const int* off, int nblk, void* blocks,
                            double* resid, void* ws, size_t ws_bytes, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (batch == 0) return TRX_OK;
    if (!A || !idx || !wt || !off || !blocks || !resid || !ws) return TRX_ERR_ARG;
    if ((size_t)ws & 15) return TRX_ERR_ARG;
    if (ws_bytes < trx_sym_fold_ws_bytes(dtype, n, batch)) return TRX_ERR_WORKSPACE;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_fold_t<float>(st, (const cx<float>*)A, n, batch, idx, (const cx<float>*)wt, off, nblk, (cx<float>*)blocks, resid, (char*)ws);
    return sym_fold_t<double>(st, (const cx<double>*)A, n, batch, idx, (const cx<double>*)wt, off, nblk, (cx<double>*)blocks, resid, (char*)ws);
}

extern "C" int trx_sym_unfold(int dtype, const void* Wk, const void* lamk, int n, int batch, const int* idx, const void* wt, const int* off, int nblk,
                              void* W, void* lam, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (batch == 0) return TRX_OK;
    if (!Wk || !lamk || !idx || !wt || !off || !W || !lam) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_unfold_t<float>(st, (const cx<float>*)Wk, (const cx<float>*)lamk, n, batch, idx, (const cx<float>*)wt, off, nblk, (cx<float>*)W,
                                   (cx<float>*)lam);
    return sym_unfold_t<double>(st, (const cx<double>*)Wk, (const cx<double>*)lamk, n, batch, idx, (const cx<double>*)wt, off, nblk, (cx<double>*)W,
                                (cx<double>*)lam);
}

extern "C" int trx_sym_fold_backward(int dtype, const void* gblocks, int n, int batch, const int* ridx, const void* rwt, const int* off, int nblk,
                                     void* gA, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (batch == 0) return TRX_OK;
    if (!gblocks || !ridx || !rwt || !off || !gA) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_fold_bwd_t<float>(st, (const cx<float>*)gblocks, n, batch, ridx, (const cx<float>*)rwt, off, nblk, (cx<float>*)gA);
    return sym_fold_bwd_t<double>(st, (const cx<double>*)gblocks, n, batch, ridx, (const cx<double>*)rwt, off, nblk, (cx<double>*)gA);
}

extern "C" int trx_sym_unfold_backward(int dtype, const void* gW, const void* glam, int n, int batch, const int* idx, const void* wt, const int* off,
                                       int nblk, void* gWk, void* glamk, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (batch == 0) return TRX_OK;
    if (!gW || !glam || !idx || !wt || !off || !gWk || !glamk) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_unfold_bwd_t<float>(st, (const cx<float>*)gW, (const cx<float>*)glam, n, batch, idx, (const cx<float>*)wt, off, nblk,
                                       (cx<float>*)gWk, (cx<float>*)glamk);
    return sym_unfold_bwd_t<double>(st, (const cx<double>*)gW, (const cx<double>*)glam, n, batch, idx, (const cx<double>*)wt, off, nblk,
                                    (cx<double>*)gWk, (cx<double>*)glamk);
}

extern "C" int trx_sym_fold_pair(int dtype, const void* M, int n, int batch, const int* idx, const void* wt, const int* off, int nblk, int kl, int kr,
                                 void* out, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (kl < 0 || kl >= nblk || kr < 0 || kr >= nblk) return TRX_ERR_ARG;
    if (batch == 0) return TRX_OK;
    if (!M || !idx || !wt || !off || !out) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_fold_pair_t<float, false>(st, (const cx<float>*)M, n, batch, idx, (const cx<float>*)wt, off, nblk, kl, kr, (cx<float>*)out);
    return sym_fold_pair_t<double, false>(st, (const cx<double>*)M, n, batch, idx, (const cx<double>*)wt, off, nblk, kl, kr, (cx<double>*)out);
}

extern "C" int trx_sym_fold_pair_bd(int dtype, const void* bd, int N, int batch, const int* idx, const void* wt, const int* off, int nblk, int kl,
                                    int kr, void* out, void* stream) {
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (N < 1 || N > (1 << 14)) return TRX_ERR_ARG;
    const int n = 2 * N;
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (kl < 0 || kl >= nblk || kr < 0 || kr >= nblk) return TRX_ERR_ARG;
    if (batch == 0) return TRX_OK;
    if (!bd || !idx || !wt || !off || !out) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_fold_pair_t<float, true>(st, (const cx<float>*)bd, n, batch, idx, (const cx<float>*)wt, off, nblk, kl, kr, (cx<float>*)out);
    return sym_fold_pair_t<double, true>(st, (const cx<double>*)bd, n, batch, idx, (const cx<double>*)wt, off, nblk, kl, kr, (cx<double>*)out);
}

extern "C" int trx_sym_fold_pairs_backward(int dtype, const void* const* G, const int* kl, const int* kr, int npairs, int n, int batch,
                                           const int* ridx, const void* rwt, const int* off, int nblk, void* gM, void* stream) {
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (npairs < 0 || npairs > SF_MAXPAIRS) return TRX_ERR_ARG;
    if (npairs > 0 && kl && kr)
        for (int p = 0; p < npairs; ++p)
            if (kl[p] < 0 || kl[p] >= nblk || kr[p] < 0 || kr[p] >= nblk) return TRX_ERR_ARG;
    if (batch == 0) return TRX_OK;
    if ((npairs > 0 && (!G || !kl || !kr)) || !ridx || !rwt || !off || !gM) return TRX_ERR_ARG;
    PairTable P;
    P.np = npairs;
    for (int p = 0; p < SF_MAXPAIRS; ++p) {
        P.g[p] = p < npairs ? G[p] : nullptr;
        P.kl[p] = (signed char)(p < npairs ? kl[p] : 0);
        P.kr[p] = (signed char)(p < npairs ? kr[p] : 0);
    }
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64) return sym_fold_pairs_bwd_t<float>(st, P, n, batch, ridx, (const cx<float>*)rwt, off, nblk, (cx<float>*)gM);
    return sym_fold_pairs_bwd_t<double>(st, P, n, batch, ridx, (const cx<double>*)rwt, off, nblk, (cx<double>*)gM);
}

extern "C" int trx_sym_fold_pair_bd_backward(int dtype, const void* G, int N, int batch, const int* ridx, const void* rwt, const int* off, int nblk,
                                             int kl, int kr, void* gbd, void* stream) {
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (N < 1 || N > (1 << 14)) return TRX_ERR_ARG;
    const int n = 2 * N;
    const int rc = check_common(dtype, n, batch, nblk);
    if (rc != TRX_OK) return rc;
    if (kl < 0 || kl >= nblk || kr < 0 || kr >= nblk) return TRX_ERR_ARG;
    if (batch == 0) return TRX_OK;
    if (!G || !ridx || !rwt || !off || !gbd) return TRX_ERR_ARG;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return sym_fold_pair_bd_bwd_t<float>(st, (const cx<float>*)G, n, batch, ridx, (const cx<float>*)rwt, off, nblk, kl, kr, (cx<float>*)gbd);
    return sym_fold_pair_bd_bwd_t<double>(st, (const cx<double>*)G, n, batch, ridx, (const cx<double>*)rwt, off, nblk, kl, kr, (cx<double>*)gbd);
}
