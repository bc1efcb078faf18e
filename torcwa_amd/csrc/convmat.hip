// Fourier factorisation (Laurent rule): permittivity grid -> block-Toeplitz convolution matrix.
// Replaces torcwa/rcwa.py:1183-1204 (`_material_conv`: torch.fft.fft2 + advanced-index gather).
//
// Only the (4ox+1) x (4oy+1) Fourier coefficients that the Toeplitz gather can address are needed, so instead of
// a full nx x ny FFT the kernels evaluate a pruned, separable DFT directly (rows then columns), with exact integer
// phase reduction ((dn*y) mod ny) and twiddles/accumulation in fp64 for both dtypes, then scatter the coefficients
// into out[b,i,j] = c[b, m_i-m_j, n_i-n_j], i = (m+ox)(2oy+1)+(n+oy)  -- the same index map as rcwa.py:1187-1200.
// trx_convmat_orders: the same coefficients gathered for an arbitrary list of harmonics (m_i, n_i) (oblique lattices, circular truncation).
#include <vector>

#include "common.hpp"

namespace trx {
namespace {

typedef cx<double> zc;

// T1[b, x, q] = sum_y g[b,x,y] * exp(-2 pi i (q-2oy) y / ny)
template <class T, bool CPLX>
__global__ __launch_bounds__(128) void dft_rows_kernel(const T* __restrict__ grid, int nx, int ny, int oy, zc* __restrict__ T1) {
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
        row[y] = CPLX ? zc((double)g[2 * y], (double)g[2 * y + 1]) : zc((double)g[y], 0.0);
    }
    __syncthreads();
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
        T1[((long)b * nx + x) * nq + q] = acc;
    }
}

// coef[b, p, q] = (1/(nx ny)) sum_x T1[b,x,q] * exp(-2 pi i (p-2ox) x / nx)
__global__ __launch_bounds__(128) void dft_cols_kernel(const zc* __restrict__ T1, int nx, int ny, int ox, int oy, zc* __restrict__ coef) {
    TRX_DYN_SMEM(smem);
    zc* tw = reinterpret_cast<zc*>(smem);          // [nx]
    zc* colv = tw + nx;                            // [nx]
    const int q = blockIdx.x, b = blockIdx.y;
    const int nq = 4 * oy + 1, np = 4 * ox + 1;
    for (int x = threadIdx.x; x < nx; x += blockDim.x) {
        double s, c;
        sincospi(-2.0 * (double)x / (double)nx, &s, &c);
        tw[x] = zc(c, s);
        colv[x] = T1[((long)b * nx + x) * nq + q];
    }
    __syncthreads();
    const double scale = 1.0 / ((double)nx * (double)ny);
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
        int step = (p - 2 * ox) % nx;
        if (step < 0) step += nx;
        zc acc(0.0, 0.0);
        int idx = 0;
        for (int x = 0; x < nx; ++x) {
            cfma(acc, colv[x], tw[idx]);
            idx += step;
            if (idx >= nx) idx -= nx;
        }
        coef[((long)b * np + p) * nq + q] = scale * acc;
    }
}

template <class T>
__global__ __launch_bounds__(256) void toeplitz_kernel(const zc* __restrict__ coef, int ox, int oy, cx<T>* __restrict__ out) {
    const int b = blockIdx.z;
    const int wy = 2 * oy + 1, N = (2 * ox + 1) * wy;
    const int nq = 4 * oy + 1, np = 4 * ox + 1;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= N) return;
    const int mi = i / wy, ni = i - mi * wy;
    const int mj = j / wy, nj = j - mj * wy;
    const zc v = coef[((long)b * np + (mi - mj + 2 * ox)) * nq + (ni - nj + 2 * oy)];
    out[((long)b * N + i) * N + j] = cx<T>((T)v.x, (T)v.y);
}

template <class T>
int convmat_t(int cplx, const void* grid, int batch, int nx, int ny, int ox, int oy, void* out, void* ws, hipStream_t s) {
    const int nq = 4 * oy + 1, np = 4 * ox + 1;
    zc* T1 = reinterpret_cast<zc*>(ws);
    zc* coef = T1 + (long)batch * nx * nq;
    const size_t sm1 = sizeof(zc) * 2 * (size_t)ny, sm2 = sizeof(zc) * 2 * (size_t)nx;
    if (cplx) TRX_LAUNCH((dft_rows_kernel<T, true>), dim3(nx, batch), dim3(128), sm1, s, (const T*)grid, nx, ny, oy, T1);
    else      TRX_LAUNCH((dft_rows_kernel<T, false>), dim3(nx, batch), dim3(128), sm1, s, (const T*)grid, nx, ny, oy, T1);
    TRX_LAUNCH(dft_cols_kernel, dim3(nq, batch), dim3(128), sm2, s, (const zc*)T1, nx, ny, ox, oy, coef);
    const int N = (2 * ox + 1) * (2 * oy + 1);
    TRX_LAUNCH((toeplitz_kernel<T>), dim3(cdiv_i(N, 256), N, batch), dim3(256), 0, s, (const zc*)coef, ox, oy, (cx<T>*)out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// ---- arbitrary order set (oblique lattices, circular truncation) -------------------------------------------------------------------------
// out[b,i,j] = coef[b, m_i-m_j+2mmax, n_i-n_j+2nmax] for the caller's list mn[i] = (m_i, n_i).  One workgroup = ORD_ROWS consecutive rows i
// of one batch entry; lanes run over j, so every store of a row is one coalesced segment.  The (4mmax+1)(4nmax+1) coefficient box of the
// entry (61^2 x 16 B = 60 KB at mmax = nmax = 15) is staged in LDS once per workgroup when it fits (LDS), else read from global (L2-resident).
constexpr int ORD_ROWS = 32;
constexpr size_t ORD_LDS_MAX = 160 * 1024;

template <class T, bool LDS>
__global__ __launch_bounds__(256) void orders_gather_kernel(const zc* __restrict__ coef, const int* __restrict__ mn, int N, int mmax, int nmax,
                                                            cx<T>* __restrict__ out) {
    TRX_DYN_SMEM(smem);
    zc* box = reinterpret_cast<zc*>(smem);
    const int b = blockIdx.y;
    const int np = 4 * mmax + 1, nq = 4 * nmax + 1;
    const zc* cb = coef + (long)b * np * nq;
    if (LDS) {
        for (int e = threadIdx.x; e < np * nq; e += blockDim.x) box[e] = cb[e];
        __syncthreads();
    }
    const int i0 = blockIdx.x * ORD_ROWS;
    const int i1 = i0 + ORD_ROWS < N ? i0 + ORD_ROWS : N;
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        const int cj = (2 * mmax - mn[2 * j]) * nq + (2 * nmax - mn[2 * j + 1]);
        for (int i = i0; i < i1; ++i) {
            const int e = cj + mn[2 * i] * nq + mn[2 * i + 1];       // (m_i - m_j + 2mmax) nq + (n_i - n_j + 2nmax)
            const zc v = LDS ? box[e] : cb[e];
            out[((long)b * N + i) * N + j] = cx<T>((T)v.x, (T)v.y);
        }
    }
}

// the gather of a finished coefficient box [batch, 4mmax+1, 4nmax+1] (trx_convmat_orders after its DFT; trx_convmat_shapes after its closed forms)
template <class T>
int orders_gather_t(hipStream_t s, const zc* coef, const int* mn, int N, int mmax, int nmax, int batch, void* out) {
    const int nq = 4 * nmax + 1, np = 4 * mmax + 1;
    const size_t box = sizeof(zc) * (size_t)np * nq;
    const dim3 g(cdiv_i(N, ORD_ROWS), batch), blk(N >= 256 ? 256 : (N > 64 ? 128 : 64));
    if (box <= ORD_LDS_MAX) {
        if (set_max_dyn_smem((const void*)orders_gather_kernel<T, true>, box)) return TRX_ERR_LAUNCH;
        TRX_LAUNCH((orders_gather_kernel<T, true>), g, blk, box, s, (const zc*)coef, mn, N, mmax, nmax, (cx<T>*)out);
    } else {
        TRX_LAUNCH((orders_gather_kernel<T, false>), g, blk, 0, s, (const zc*)coef, mn, N, mmax, nmax, (cx<T>*)out);
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int convmat_orders_t(int cplx, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax, int nmax, void* out, void* ws,
                     hipStream_t s) {
    const int nq = 4 * nmax + 1;
    zc* T1 = reinterpret_cast<zc*>(ws);
    zc* coef = T1 + (long)batch * n1 * nq;
    const size_t sm1 = sizeof(zc) * 2 * (size_t)n2, sm2 = sizeof(zc) * 2 * (size_t)n1;
    if (cplx) TRX_LAUNCH((dft_rows_kernel<T, true>), dim3(n1, batch), dim3(128), sm1, s, (const T*)grid, n1, n2, nmax, T1);
    else      TRX_LAUNCH((dft_rows_kernel<T, false>), dim3(n1, batch), dim3(128), sm1, s, (const T*)grid, n1, n2, nmax, T1);
    TRX_LAUNCH(dft_cols_kernel, dim3(nq, batch), dim3(128), sm2, s, (const zc*)T1, n1, n2, mmax, nmax, coef);
    return orders_gather_t<T>(s, coef, mn, N, mmax, nmax, batch, out);
}
}  // namespace

int orders_gather(hipStream_t s, int dtype, const cx<double>* coef, const int* mn, int N, int mmax, int nmax, int batch, void* out) {
    if (dtype == TRX_C64) return orders_gather_t<float>(s, coef, mn, N, mmax, nmax, batch, out);
    return orders_gather_t<double>(s, coef, mn, N, mmax, nmax, batch, out);
}

int orders_check(hipStream_t s, const int* mn, int N, int mmax, int nmax) {
    std::vector<int> h((size_t)2 * N);
    if (hipMemcpyAsync(h.data(), mn, sizeof(int) * h.size(), hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return TRX_ERR_LAUNCH;
    for (int i = 0; i < N; ++i)
        if (h[2 * i] < -mmax || h[2 * i] > mmax || h[2 * i + 1] < -nmax || h[2 * i + 1] > nmax) return TRX_ERR_ARG;
    return TRX_OK;
}

int convmat_orders_checked(hipStream_t s, int dtype, int cplx, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax,
                           int nmax, void* out, void* ws) {
    if (dtype == TRX_C64) return convmat_orders_t<float>(cplx, grid, batch, n1, n2, mn, N, mmax, nmax, out, ws, s);
    return convmat_orders_t<double>(cplx, grid, batch, n1, n2, mn, N, mmax, nmax, out, ws, s);
}
}  // namespace trx

extern "C" size_t trx_convmat_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy) {
    (void)dtype; (void)ny;
    return sizeof(trx::zc) * ((size_t)batch * nx * (4 * oy + 1) + (size_t)batch * (4 * ox + 1) * (4 * oy + 1));
}

extern "C" int trx_convmat(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy,
                           void* out, void* ws, size_t ws_bytes, void* stream) {
    if (!grid || !out || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || ox < 0 || oy < 0 || nx <= 2 * ox || ny <= 2 * oy) return TRX_ERR_ARG;
    if (ws_bytes < trx_convmat_ws_bytes(dtype, batch, nx, ny, ox, oy)) return TRX_ERR_WORKSPACE;
    if ((size_t)16 * 2 * (size_t)(nx > ny ? nx : ny) > 64 * 1024) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64) return trx::convmat_t<float>(grid_is_complex, grid, batch, nx, ny, ox, oy, out, ws, s);
    if (dtype == TRX_C128) return trx::convmat_t<double>(grid_is_complex, grid, batch, nx, ny, ox, oy, out, ws, s);
    return TRX_ERR_DTYPE;
}

extern "C" size_t trx_convmat_orders_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax) {
    (void)N;
    return trx_convmat_ws_bytes(dtype, batch, n1, n2, mmax, nmax);
}

extern "C" int trx_convmat_orders(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax,
                                  int nmax, void* out, void* ws, size_t ws_bytes, void* stream) {
    if (!grid || !mn || !out || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || N <= 0 || mmax < 0 || nmax < 0 || n1 <= 2 * mmax || n2 <= 2 * nmax) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_convmat_orders_ws_bytes(dtype, batch, n1, n2, N, mmax, nmax)) return TRX_ERR_WORKSPACE;
    if ((size_t)16 * 2 * (size_t)(n1 > n2 ? n1 : n2) > 64 * 1024) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    // every index must lie in the coefficient box: the list is small (N pairs), so it is checked on the host (one stream sync)
    const int rc = trx::orders_check(s, mn, N, mmax, nmax);
    if (rc) return rc;
    return trx::convmat_orders_checked(s, dtype, grid_is_complex, grid, batch, n1, n2, mn, N, mmax, nmax, out, ws);
}
