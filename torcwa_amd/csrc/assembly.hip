// Layer eigenproblem assembly (torcwa/rcwa.py:1224-1236): P, Q and A = PQ of a layer, for all three Fourier rules.  The one implementation
// takes the in-plane permittivity tensor (Exx, Exy = Eyx, Eyy) and a permeability matrix per field component (Mx, My):
//
//   P = [[Kx Ei Ky, My - Kx Ei Kx], [Ky Ei Ky - Mx, -Ky Ei Kx]],  Q = [[-Kx Mi Ky - Exy, Kx Mi Kx - Eyy], [Exx - Ky Mi Ky, Ky Mi Kx + Exy]]
//   A = PQ for homogeneous mu:
//     [[mu Exx - Ky^2 - Kx Gx, mu Exy + KxKy - Kx Gy], [mu Exy + KxKy - Ky Gx, mu Eyy - Kx^2 - Ky Gy]],  [Gx, Gy] = Ei [Kx Exx + Ky Exy, Kx Exy + Ky Eyy]
//
//   Laurent's rule (trx_build_pq, trx_build_a):                   Exx = Eyy = E, Mx = My = M, no Exy
//   Li's rule (trx_build_pq_aniso, trx_build_a_aniso):            Exx = Ex, Eyy = Ey, no Exy
//   normal-vector rule (trx_build_pq_tensor, trx_build_a_tensor): Mx = My = M
//
// TENSOR = false compiles every Exy term out (the pointer is not read), so the rules without Exy keep their own arithmetic bit for bit.
// Without Exy, Gx and Gy are two N x N products; with it they are one N x 2N product (each rule keeps its own GEMM calls).
#include "common.hpp"

namespace trx {
namespace {

// Laurent's rule hands the same matrix in twice (Exx == Eyy, Mx == My): the inputs are only read, so the aliased __restrict__ is sound.
template <class T, bool TENSOR>
__global__ __launch_bounds__(256) void build_pq_kernel(const cx<T>* __restrict__ Exx, const cx<T>* __restrict__ Exy, const cx<T>* __restrict__ Eyy,
                                                       const cx<T>* __restrict__ Ei, const cx<T>* __restrict__ Mx, const cx<T>* __restrict__ My,
                                                       const cx<T>* __restrict__ Mi, const cx<T>* __restrict__ kx, const cx<T>* __restrict__ ky, int N,
                                                       cx<T>* __restrict__ P, cx<T>* __restrict__ Q) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const long o = ((long)b * N + i) * N + j;
    const cx<T> exx = Exx[o], eyy = Eyy[o], ei = Ei[o], mx = Mx[o], my = My[o], mi = Mi[o];
    const cx<T> kxi = kx[(long)b * N + i], kyi = ky[(long)b * N + i], kxj = kx[(long)b * N + j], kyj = ky[(long)b * N + j];
    const int n = 2 * N;
    cx<T>* Pb = P + (long)b * n * n;
    cx<T>* Qb = Q + (long)b * n * n;
    const long r0 = (long)i * n + j, r1 = (long)(i + N) * n + j;
    Pb[r0] = kxi * ei * kyj;
    Pb[r0 + N] = my - kxi * ei * kxj;
    Pb[r1] = kyi * ei * kyj - mx;
    Pb[r1 + N] = -(kyi * ei * kxj);
    cx<T> q11 = -(kxi * mi * kyj), q22 = kyi * mi * kxj;
    if (TENSOR) {
        const cx<T> exy = Exy[o];
        q11 = q11 - exy;
        q22 = q22 + exy;
    }
    Qb[r0] = q11;
    Qb[r0 + N] = kxi * mi * kxj - eyy;
    Qb[r1] = exx - kyi * mi * kyj;
    Qb[r1 + N] = q22;
}

// The right-hand side of the G product, rows of leading dimension ld.  Without Exy: S = K E (one launch per component, ld = N);
// with it: S = [Kx Exx + Ky Exy | Kx Exy + Ky Eyy] (ld = 2N; E, k are Exx, kx).
template <class T, bool TENSOR>
__global__ __launch_bounds__(256) void build_a_rhs_kernel(const cx<T>* __restrict__ E, const cx<T>* __restrict__ k, const cx<T>* __restrict__ Exy,
                                                          const cx<T>* __restrict__ Eyy, const cx<T>* __restrict__ ky, int N, int ld,
                                                          cx<T>* __restrict__ S) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const long o = ((long)b * N + i) * N + j;
    cx<T>* Sr = S + ((long)b * N + i) * ld;
    if (TENSOR) {
        const cx<T> kxi = k[(long)b * N + i], kyi = ky[(long)b * N + i], exy = Exy[o];
        Sr[j] = kxi * E[o] + kyi * exy;
        Sr[j + N] = kxi * exy + kyi * Eyy[o];
    } else {
        Sr[j] = k[(long)b * N + i] * E[o];
    }
}

// A from Gx, Gy (rows of leading dimension ld: two [B,N,N] matrices, or the halves of one [B,N,2N])
template <class T, bool TENSOR>
__global__ __launch_bounds__(256) void assemble_a_kernel(const cx<T>* __restrict__ Exx, const cx<T>* __restrict__ Exy, const cx<T>* __restrict__ Eyy,
                                                         const cx<T>* __restrict__ Gx, const cx<T>* __restrict__ Gy, int ld,
                                                         const cx<T>* __restrict__ mu, const cx<T>* __restrict__ kx, const cx<T>* __restrict__ ky, int N,
                                                         cx<T>* __restrict__ A) {
    const int b = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const long o = ((long)b * N + i) * N + j, og = ((long)b * N + i) * ld + j;
    const cx<T> kxi = kx[(long)b * N + i], kyi = ky[(long)b * N + i], m = mu[b];
    const cx<T> ex = m * Exx[o], ey = m * Eyy[o], gx = Gx[og], gy = Gy[og];
    const int n = 2 * N;
    cx<T>* Ab = A + (long)b * n * n;
    cx<T> a11 = ex - kxi * gx, a12, a21, a22 = ey - kyi * gy;
    if (TENSOR) {
        const cx<T> mxy = m * Exy[o];
        a12 = mxy - kxi * gy;
        a21 = mxy - kyi * gx;
    } else {
        a12 = -(kxi * gy);
        a21 = -(kyi * gx);
    }
    if (i == j) { a11 -= kyi * kyi; a22 -= kxi * kxi; a12 += kxi * kyi; a21 += kxi * kyi; }
    Ab[(long)i * n + j] = a11;
    Ab[(long)i * n + j + N] = a12;
    Ab[(long)(i + N) * n + j] = a21;
    Ab[(long)(i + N) * n + j + N] = a22;
}

template <class T, bool TENSOR>
int build_pq_t(hipStream_t s, const void* Exx, const void* Exy, const void* Eyy, const void* Ei, const void* Mx, const void* My, const void* Mi,
               const void* kx, const void* ky, int N, int batch, void* P, void* Q) {
    typedef const cx<T>* in;
    TRX_LAUNCH((build_pq_kernel<T, TENSOR>), dim3(cdiv_i(N, 256), N, batch), dim3(256), 0, s, (in)Exx, (in)Exy, (in)Eyy, (in)Ei, (in)Mx, (in)My, (in)Mi,
               (in)kx, (in)ky, N, (cx<T>*)P, (cx<T>*)Q);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// ws: S | Gx | Gy, three [B,N,N] matrices (S holds Kx Exx, then Ky Eyy), or with Exy S | G, two [B,N,2N]
template <class T, bool TENSOR>
int build_a_t(hipStream_t s, const void* Exx_, const void* Exy_, const void* Eyy_, const void* Ei_, const void* mu, const void* kx_, const void* ky_,
              int N, int batch, void* A, void* ws) {
    typedef const cx<T>* in;
    const in Exx = (in)Exx_, Exy = (in)Exy_, Eyy = (in)Eyy_, Ei = (in)Ei_, kx = (in)kx_, ky = (in)ky_;
    const long NN = (long)N * N, bNN = (long)batch * NN;
    const cx<T> one(T(1), T(0)), zero(T(0), T(0));
    const dim3 g(cdiv_i(N, 256), N, batch), blk(256);
    const int ld = TENSOR ? 2 * N : N;
    cx<T>* S = (cx<T>*)ws;
    cx<T>* Gx = S + (TENSOR ? 2 : 1) * bNN;
    cx<T>* Gy = TENSOR ? Gx + N : Gx + bNN;
    int rc;
    if (TENSOR) {
        TRX_LAUNCH((build_a_rhs_kernel<T, true>), g, blk, 0, s, Exx, kx, Exy, Eyy, ky, N, ld, S);
        rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, N, 2 * N, N, one, Ei, N, NN, S, 2 * N, 2 * NN, zero, Gx, 2 * N, 2 * NN, batch); if (rc) return rc;
    } else {
        TRX_LAUNCH((build_a_rhs_kernel<T, false>), g, blk, 0, s, Exx, kx, (in)nullptr, (in)nullptr, (in)nullptr, N, ld, S);
        rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, N, N, N, one, Ei, N, NN, S, N, NN, zero, Gx, N, NN, batch); if (rc) return rc;
        TRX_LAUNCH((build_a_rhs_kernel<T, false>), g, blk, 0, s, Eyy, ky, (in)nullptr, (in)nullptr, (in)nullptr, N, ld, S);
        rc = gemm<T>(s, TRX_OP_N, TRX_OP_N, N, N, N, one, Ei, N, NN, S, N, NN, zero, Gy, N, NN, batch); if (rc) return rc;
    }
    TRX_LAUNCH((assemble_a_kernel<T, TENSOR>), g, blk, 0, s, Exx, Exy, Eyy, (in)Gx, (in)Gy, ld, (in)mu, kx, ky, N, (cx<T>*)A);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// f(float()) for complex64, f(double()) for complex128: the one place where a dtype code becomes a template argument
template <class F>
int by_dtype(int dtype, F f) {
    if (dtype == TRX_C64) return f(float());
    if (dtype == TRX_C128) return f(double());
    return TRX_ERR_DTYPE;
}

template <bool TENSOR>
int build_pq(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Ei, const void* Mx, const void* My, const void* Mi,
             const void* kx, const void* ky, int N, int batch, void* P, void* Q, void* stream) {
    if (!Exx || (TENSOR && !Exy) || !Eyy || !Ei || !Mx || !My || !Mi || !kx || !ky || !P || !Q || N <= 0 || batch <= 0) return TRX_ERR_ARG;
    hipStream_t s = api_stream(stream);
    return by_dtype(dtype, [&](auto t) { return build_pq_t<decltype(t), TENSOR>(s, Exx, Exy, Eyy, Ei, Mx, My, Mi, kx, ky, N, batch, P, Q); });
}

template <bool TENSOR>
int build_a(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Ei, const void* mu, const void* kx, const void* ky, int N,
            int batch, void* A, void* ws, size_t ws_bytes, size_t ws_need, void* stream) {
    if (!Exx || (TENSOR && !Exy) || !Eyy || !Ei || !mu || !kx || !ky || !A || !ws || N <= 0 || batch <= 0) return TRX_ERR_ARG;
    if (ws_bytes < ws_need) return TRX_ERR_WORKSPACE;
    hipStream_t s = api_stream(stream);
    return by_dtype(dtype, [&](auto t) { return build_a_t<decltype(t), TENSOR>(s, Exx, Exy, Eyy, Ei, mu, kx, ky, N, batch, A, ws); });
}

}  // namespace
}  // namespace trx

using namespace trx;

extern "C" int trx_build_pq(int dtype, const void* E, const void* Einv, const void* Mu, const void* Muinv, const void* kx,
                            const void* ky, int N, int batch, void* P, void* Q, void* stream) {
    return build_pq<false>(dtype, E, nullptr, E, Einv, Mu, Mu, Muinv, kx, ky, N, batch, P, Q, stream);
}

extern "C" int trx_build_pq_aniso(int dtype, const void* Ex, const void* Ey, const void* Einv, const void* Mx, const void* My, const void* Minv,
                                  const void* kx, const void* ky, int N, int batch, void* P, void* Q, void* stream) {
    return build_pq<false>(dtype, Ex, nullptr, Ey, Einv, Mx, My, Minv, kx, ky, N, batch, P, Q, stream);
}

extern "C" int trx_build_pq_tensor(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Einv, const void* Mu, const void* Muinv,
                                   const void* kx, const void* ky, int N, int batch, void* P, void* Q, void* stream) {
    return build_pq<true>(dtype, Exx, Exy, Eyy, Einv, Mu, Mu, Muinv, kx, ky, N, batch, P, Q, stream);
}

extern "C" size_t trx_build_a_ws_bytes(int dtype, int N, int batch) {
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * 3 * (size_t)batch * N * N;
}

extern "C" int trx_build_a(int dtype, const void* E, const void* Einv, const void* mu, const void* kx, const void* ky, int N, int batch, void* A,
                           void* ws, size_t ws_bytes, void* stream) {
    return build_a<false>(dtype, E, nullptr, E, Einv, mu, kx, ky, N, batch, A, ws, ws_bytes, trx_build_a_ws_bytes(dtype, N, batch), stream);
}

extern "C" size_t trx_build_a_aniso_ws_bytes(int dtype, int N, int batch) {
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * 3 * (size_t)batch * N * N;
}

extern "C" int trx_build_a_aniso(int dtype, const void* Ex, const void* Ey, const void* Einv, const void* mu, const void* kx, const void* ky, int N,
                                 int batch, void* A, void* ws, size_t ws_bytes, void* stream) {
    return build_a<false>(dtype, Ex, nullptr, Ey, Einv, mu, kx, ky, N, batch, A, ws, ws_bytes, trx_build_a_aniso_ws_bytes(dtype, N, batch), stream);
}

extern "C" size_t trx_build_a_tensor_ws_bytes(int dtype, int N, int batch) {
    return (size_t)(dtype == TRX_C128 ? 16 : 8) * 4 * (size_t)batch * N * N;
}

extern "C" int trx_build_a_tensor(int dtype, const void* Exx, const void* Exy, const void* Eyy, const void* Einv, const void* mu, const void* kx,
                                  const void* ky, int N, int batch, void* A, void* ws, size_t ws_bytes, void* stream) {
    return build_a<true>(dtype, Exx, Exy, Eyy, Einv, mu, kx, ky, N, batch, A, ws, ws_bytes, trx_build_a_tensor_ws_bytes(dtype, N, batch), stream);
}
