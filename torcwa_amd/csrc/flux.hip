// Power flux through the planes of a layer (include/trx.h: trx_matvec, trx_layer_flux).
//
//   Phi(z) = Re sum_{j<N} ( e_j conj(h_{j+N}) - e_{j+N} conj(h_j) ),   e = W (a + b),  h = V (a - b),
//   a_k = c+_k exp(i w kz_k z),  b_k = c-_k exp(i w kz_k (d - z))
//
// The work is HBM-bound: W and V (2 n^2 elements per point) are streamed once per tile of up to 16 z columns.  A workgroup owns 32 harmonics
// j and with them the four row blocks the reduction pairs (rows j and j + N of W and of V): 128 rows, whose products with the [n, nz] right-hand
// sides stay in registers (fp64 for both dtypes).  The right-hand sides are formed per k-chunk in LDS from c+-, kz and z; neither they nor the
// products reach HBM.  Per workgroup one partial sum per z goes to the workspace and a second kernel adds the partials in a fixed order, so the
// result is deterministic (no floating-point atomics).
#include "common.hpp"

using namespace trx;

namespace {

constexpr int FX_THREADS = 128;   // two waves
constexpr int FX_R = 32;          // harmonics j per workgroup
constexpr int FX_ROWS = 4 * FX_R; // tile rows: [W rows j | V rows j | W rows j + N | V rows j + N]
constexpr int FX_UNITS = 16;      // 16-byte units per tile row and k-chunk (256 bytes of a matrix row)
constexpr int FX_LDU = FX_UNITS + 1;   // row pitch in units: one access width of padding (cdna_hip_programming.md Guideline 4)
constexpr int FX_ZT = 16;         // z columns per pass over W and V

struct alignas(16) unit16 { unsigned a, b, c, d; };

template <class T> struct fx_elem {
    static constexpr int VEC = 16 / (int)sizeof(cx<T>);      // elements per 16-byte unit: 1 (complex128), 2 (complex64)
    static constexpr int KC = FX_UNITS * VEC;                // k per chunk: 16 / 32
};

template <class T, int NZT> constexpr size_t fx_smem_bytes() {
    return (size_t)FX_ROWS * FX_LDU * 16 + (size_t)2 * fx_elem<T>::KC * NZT * sizeof(cx<double>);
}

template <class T> __device__ __forceinline__ cx<double> to_f64(cx<T> v) { return cx<double>((double)v.x, (double)v.y); }

// grid (ceil(N / FX_R), batch).  z columns t0 .. t0 + nt - 1 (nt <= NZT) of z [batch, nz]; part [batch, gridDim.x, nz].
template <class T, int NZT>
__global__ __launch_bounds__(FX_THREADS) void layer_flux_kernel(const cx<T>* __restrict__ W, const cx<T>* __restrict__ V,
                                                                const cx<T>* __restrict__ cplus, const cx<T>* __restrict__ cminus,
                                                                const cx<T>* __restrict__ kz, const double* __restrict__ omega,
                                                                const double* __restrict__ thick, const double* __restrict__ z, int z_frac, int N,
                                                                int nz, int t0, int nt, double* __restrict__ part) {
    constexpr int VEC = fx_elem<T>::VEC, KC = fx_elem<T>::KC;
    constexpr int TPT = NZT < 8 ? NZT : 8;            // z columns per thread
    constexpr int NTG = NZT / TPT;                    // threads that share a row
    constexpr int NRG = FX_THREADS / NTG;             // row groups
    constexpr int RPT = FX_ROWS / NRG;                // rows per thread (rg, rg + NRG, ...: the same matrix, see the tile order)
    constexpr int UPT = FX_ROWS * FX_UNITS / FX_THREADS;   // 16-byte units a thread stages per chunk
    static_assert(UPT == 16 && FX_THREADS / FX_UNITS == 8, "staging map");
    TRX_DYN_SMEM(smem);
    unit16* tile = (unit16*)smem;
    cx<double>* rhs = (cx<double>*)(smem + (size_t)FX_ROWS * FX_LDU * 16);     // [2][KC][NZT]: a + b, then a - b
    const int tid = threadIdx.x, b = blockIdx.y, n = 2 * N;
    const int j0 = blockIdx.x * FX_R;
    const cx<T>* Wb = W + (long)b * n * n;
    const cx<T>* Vb = V + (long)b * n * n;
    const cx<T>* cpb = cplus + (long)b * n;
    const cx<T>* cmb = cminus + (long)b * n;
    const cx<T>* kzb = kz + (long)b * n;
    const double om = omega[b], dd = thick[b];

    // staging map: unit i of this thread is tile row 8 i + (tid >> 4), unit column tid & 15
    const int srow = tid >> 4, scol = tid & 15;
    unit16 pf[UPT];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < UPT; ++i) {
            const int blk = i >> 2;                              // 0 W top, 1 V top, 2 W bottom, 3 V bottom
            const int j = j0 + 8 * (i & 3) + srow;
            const int k = k0 + scol * VEC;
            const cx<T>* M = (blk & 1) ? Vb : Wb;
            unit16 v = {0u, 0u, 0u, 0u};
            if (j < N && k < n) v = *(const unit16*)(M + (long)(j + (blk >> 1) * N) * n + k);      // n is even: a complex64 pair never straddles the row end
            pf[i] = v;
        }
    };

    const int tg = tid % NTG, rg = tid / NTG;
    const cx<double>* myrhs = rhs + (size_t)((rg >> 5) & 1) * KC * NZT + tg * TPT;      // rows of V take a - b
    cx<double> acc[RPT][TPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int t = 0; t < TPT; ++t) acc[i][t] = cx<double>(0.0, 0.0);

    fetch(0);
    for (int k0 = 0; k0 < n; k0 += KC) {
        __syncthreads();                                         // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < UPT; ++i) tile[(8 * i + srow) * FX_LDU + scol] = pf[i];
        for (int idx = tid; idx < KC * NZT; idx += FX_THREADS) {
            const int kk = idx / NZT, t = idx % NZT, k = k0 + kk;
            cx<double> s(0.0, 0.0), df(0.0, 0.0);
            if (k < n && t < nt) {
                double zt = z[(long)b * nz + t0 + t];
                if (z_frac) zt *= dd;
                const cx<double> q = to_f64(kzb[k]);
                const double wz = om * zt, wr = om * (dd - zt);
                const cx<double> a = to_f64(cpb[k]) * cexp(cx<double>(-wz * q.y, wz * q.x));     // c+ exp(i w kz z)
                const cx<double> bb = to_f64(cmb[k]) * cexp(cx<double>(-wr * q.y, wr * q.x));    // c- exp(i w kz (d - z))
                s = a + bb;
                df = a - bb;
            }
            rhs[idx] = s;
            rhs[KC * NZT + idx] = df;
        }
        __syncthreads();
        if (k0 + KC < n) fetch(k0 + KC);                         // in flight while this chunk is multiplied
        const cx<T>* te = (const cx<T>*)tile;
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            cx<double> w[RPT];
#pragma unroll
            for (int i = 0; i < RPT; ++i) w[i] = to_f64(te[(rg + i * NRG) * (FX_LDU * VEC) + kk]);
#pragma unroll
            for (int t = 0; t < TPT; ++t) {
                const cx<double> r = myrhs[kk * NZT + t];
#pragma unroll
                for (int i = 0; i < RPT; ++i) cfma(acc[i][t], w[i], r);
            }
        }
    }
    __syncthreads();
    cx<double>* res = (cx<double>*)smem;                         // [FX_ROWS][NZT] over the tile (128 * 16 * 16 <= 128 * 17 * 16 bytes)
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int t = 0; t < TPT; ++t) res[(rg + i * NRG) * NZT + tg * TPT + t] = acc[i][t];
    __syncthreads();
    if (tid < nt) {                                              // rows of j >= N hold zeros
        double sum = 0.0;
        for (int jj = 0; jj < FX_R; ++jj) {
            const cx<double> et = res[jj * NZT + tid], ht = res[(FX_R + jj) * NZT + tid];
            const cx<double> eb = res[(2 * FX_R + jj) * NZT + tid], hb = res[(3 * FX_R + jj) * NZT + tid];
            sum += (et.x * hb.x + et.y * hb.y) - (eb.x * ht.x + eb.y * ht.y);
        }
        part[((long)b * gridDim.x + blockIdx.x) * nz + t0 + tid] = sum;
    }
}

__global__ __launch_bounds__(256) void flux_finish_kernel(const double* __restrict__ part, int groups, int nz, int batch, double* __restrict__ flux) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)batch * nz) return;
    const int b = (int)(i / nz), t = (int)(i % nz);
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += part[((long)b * groups + g) * nz + t];
    flux[i] = s;
}

// Y[b] = A[b] X[b]: one wave per row of A, lanes along k, c <= CM fp64 accumulators per lane, a fixed shuffle tree per column.
template <class T, int CM>
__global__ __launch_bounds__(256) void matvec_kernel(const cx<T>* __restrict__ A, const cx<T>* __restrict__ X, long strideX, cx<T>* __restrict__ Y,
                                                     int m, int k, int c) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = row < m;                                   // wave-uniform
    const cx<T>* a = A + ((long)b * m + (live ? row : 0)) * k;
    const cx<T>* x = X + (long)b * strideX;
    cx<double> acc[CM];
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) acc[cc] = cx<double>(0.0, 0.0);
    for (int kk = lane; kk < k; kk += 64) {
        const cx<double> av = to_f64(a[kk]);
#pragma unroll
        for (int cc = 0; cc < CM; ++cc)
            if (cc < c) cfma(acc[cc], av, to_f64(x[(long)kk * c + cc]));
    }
#pragma unroll
    for (int cc = 0; cc < CM; ++cc) {
        const double re = wave_sum(acc[cc].x), im = wave_sum(acc[cc].y);
        if (live && lane == 0 && cc < c) Y[((long)b * m + row) * c + cc] = cx<T>((T)re, (T)im);
    }
}

template <class T>
int matvec_t(hipStream_t s, const cx<T>* A, const cx<T>* X, long strideX, cx<T>* Y, int m, int k, int c, int batch) {
    if (m == 0 || batch == 0) return TRX_OK;
    const dim3 grid(cdiv_i(m, 4), batch), block(256);
    if (c <= 1) TRX_LAUNCH((matvec_kernel<T, 1>), grid, block, 0, s, A, X, strideX, Y, m, k, c);
    else if (c <= 4) TRX_LAUNCH((matvec_kernel<T, 4>), grid, block, 0, s, A, X, strideX, Y, m, k, c);
    else TRX_LAUNCH((matvec_kernel<T, 16>), grid, block, 0, s, A, X, strideX, Y, m, k, c);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T, int NZT>
int flux_pass(hipStream_t s, dim3 grid, const cx<T>* W, const cx<T>* V, const cx<T>* cp, const cx<T>* cm, const cx<T>* kz, const double* omega,
              const double* d, const double* z, int z_frac, int N, int nz, int t0, int nt, double* part) {
    constexpr size_t smem = fx_smem_bytes<T, NZT>();
    if (set_max_dyn_smem((const void*)layer_flux_kernel<T, NZT>, smem)) return TRX_ERR_LAUNCH;
    TRX_LAUNCH((layer_flux_kernel<T, NZT>), grid, dim3(FX_THREADS), smem, s, W, V, cp, cm, kz, omega, d, z, z_frac, N, nz, t0, nt, part);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int layer_flux_t(hipStream_t s, const cx<T>* W, const cx<T>* V, const cx<T>* cp, const cx<T>* cm, const cx<T>* kz, const double* omega,
                 const double* d, const double* z, int z_frac, int N, int nz, int batch, double* flux, double* part) {
    if (batch == 0 || nz == 0) return TRX_OK;
    const int groups = cdiv_i(N, FX_R);
    const dim3 grid(groups, batch);
    for (int t0 = 0; t0 < nz; t0 += FX_ZT) {                     // W and V are streamed once per tile of up to 16 z columns
        const int nt = nz - t0 < FX_ZT ? nz - t0 : FX_ZT;
        const int rc = nt <= 2 ? flux_pass<T, 2>(s, grid, W, V, cp, cm, kz, omega, d, z, z_frac, N, nz, t0, nt, part)
                               : flux_pass<T, FX_ZT>(s, grid, W, V, cp, cm, kz, omega, d, z, z_frac, N, nz, t0, nt, part);
        if (rc) return rc;
    }
    TRX_LAUNCH(flux_finish_kernel, dim3(cdiv_i((long)batch * nz, 256)), dim3(256), 0, s, part, groups, nz, batch, flux);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace

extern "C" int trx_matvec(int dtype, const void* A, const void* X, long strideX, void* Y, int m, int k, int c, int batch, void* stream) {
    if (!A || !X || !Y || m < 0 || k < 0 || batch < 0 || batch > 65535 || c < 1 || c > 16 || strideX < 0) return TRX_ERR_ARG;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64) return matvec_t<float>(s, (const cx<float>*)A, (const cx<float>*)X, strideX, (cx<float>*)Y, m, k, c, batch);
    if (dtype == TRX_C128) return matvec_t<double>(s, (const cx<double>*)A, (const cx<double>*)X, strideX, (cx<double>*)Y, m, k, c, batch);
    return TRX_ERR_DTYPE;
}

extern "C" size_t trx_layer_flux_ws_bytes(int dtype, int N, int nz, int batch) {
    (void)dtype;
    if (N < 0 || nz < 0 || batch < 0) return 0;
    return sizeof(double) * (size_t)cdiv_i(N, FX_R) * (size_t)nz * (size_t)batch;
}

extern "C" int trx_layer_flux(int dtype, const void* W, const void* V, const void* cplus, const void* cminus, const void* kz, const double* omega,
                              const double* d, const double* z, int z_is_fraction, int N, int nz, int batch, double* flux, void* ws,
                              size_t ws_bytes, void* stream) {
    if (N < 1 || nz < 0 || batch < 0 || batch > 65535) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (nz == 0 || batch == 0) return TRX_OK;                                   // nothing to compute: no buffer is touched, none is required
    if (!W || !V || !cplus || !cminus || !kz || !omega || !d || !z || !flux || !ws) return TRX_ERR_ARG;
    if (((size_t)W | (size_t)V | (size_t)ws) & 15) return TRX_ERR_ARG;          // rows are read in 16-byte units
    if (ws_bytes < trx_layer_flux_ws_bytes(dtype, N, nz, batch)) return TRX_ERR_WORKSPACE;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return layer_flux_t<float>(s, (const cx<float>*)W, (const cx<float>*)V, (const cx<float>*)cplus, (const cx<float>*)cminus,
                                   (const cx<float>*)kz, omega, d, z, z_is_fraction, N, nz, batch, flux, (double*)ws);
    return layer_flux_t<double>(s, (const cx<double>*)W, (const cx<double>*)V, (const cx<double>*)cplus, (const cx<double>*)cminus,
                                (const cx<double>*)kz, omega, d, z, z_is_fraction, N, nz, batch, flux, (double*)ws);
}
