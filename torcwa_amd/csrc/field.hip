// Field maps (include/trx.h: trx_layer_field, trx_field_synth).
//
//   trx_layer_field   Fourier coefficients of (Ex, Ey, Hx, Hy) and of the z components before [eps]^-1 / [mu]^-1 at nz depths of one layer:
//                     e = W (a + b),  h = V (a - b),  a_k = c+_k exp(i w kz_k z),  b_k = c-_k exp(i w kz_k (d - z)),
//                     rows 4, 5:  ky_j hx_j - kx_j hy_j,   kx_j ey_j - ky_j ex_j.
//   trx_field_synth   out[c, iu, iv, t] = sum_m coef[c, m, t] exp(i w (kx_m u_iu + ky_m v_iv)): the Bloch sum, phases formed in the kernel.
//
// layer_field_kernel is layer_flux_kernel (flux.hip) with another epilogue: the same workgroup shape (32 harmonics j and with them rows j and
// j + N of W and of V), the same staging and the same k loop, so W and V are streamed once per tile of up to 16 depths and the right-hand sides
// live in LDS only.  It is a SECOND COPY of that loop on purpose: trx_layer_flux has to stay bit for bit what it is, and a shared body would
// leave that to the compiler's contraction choices in two instantiation contexts.
#include "common.hpp"

using namespace trx;

namespace {

// ---- trx_layer_field ----------------------------------------------------------------------------------------------------------------------
constexpr int FL_THREADS = 128;   // two waves
constexpr int FL_R = 32;          // harmonics j per workgroup
constexpr int FL_ROWS = 4 * FL_R; // tile rows: [W rows j | V rows j | W rows j + N | V rows j + N]
constexpr int FL_UNITS = 16;      // 16-byte units per tile row and k-chunk (256 bytes of a matrix row)
constexpr int FL_LDU = FL_UNITS + 1;   // row pitch in units: one access width of padding (cdna_hip_programming.md Guideline 4)
constexpr int FL_ZT = 16;         // depths per pass over W and V

struct alignas(16) unit16 { unsigned a, b, c, d; };

template <class T> struct fl_elem {
    static constexpr int VEC = 16 / (int)sizeof(cx<T>);      // elements per 16-byte unit: 1 (complex128), 2 (complex64)
    static constexpr int KC = FL_UNITS * VEC;                // k per chunk: 16 / 32
};

template <class T, int NZT> constexpr size_t fl_smem_bytes() {
    return (size_t)FL_ROWS * FL_LDU * 16 + (size_t)2 * fl_elem<T>::KC * NZT * sizeof(cx<double>);
}

template <class T> __device__ __forceinline__ cx<double> to_f64(cx<T> v) { return cx<double>((double)v.x, (double)v.y); }
template <class T> __device__ __forceinline__ cx<T> from_f64(cx<double> v) { return cx<T>((T)v.x, (T)v.y); }

// grid (ceil(N / FL_R), batch).  Depths t0 .. t0 + nt - 1 (nt <= NZT) of z [batch, nz]; out [batch, 6, N, nz].
template <class T, int NZT>
__global__ __launch_bounds__(FL_THREADS) void layer_field_kernel(const cx<T>* __restrict__ W, const cx<T>* __restrict__ V,
                                                                 const cx<T>* __restrict__ cplus, const cx<T>* __restrict__ cminus,
                                                                 const cx<T>* __restrict__ kz, const double* __restrict__ omega,
                                                                 const double* __restrict__ thick, const double* __restrict__ z, int z_frac,
                                                                 const double* __restrict__ kx, const double* __restrict__ ky, int N, int nz, int t0,
                                                                 int nt, cx<T>* __restrict__ out) {
    constexpr int VEC = fl_elem<T>::VEC, KC = fl_elem<T>::KC;
    constexpr int TPT = NZT < 8 ? NZT : 8;            // depths per thread
    constexpr int NTG = NZT / TPT;                    // threads that share a row
    constexpr int NRG = FL_THREADS / NTG;             // row groups
    constexpr int RPT = FL_ROWS / NRG;                // rows per thread (rg, rg + NRG, ...: the same matrix, see the tile order)
    constexpr int UPT = FL_ROWS * FL_UNITS / FL_THREADS;   // 16-byte units a thread stages per chunk
    static_assert(UPT == 16 && FL_THREADS / FL_UNITS == 8, "staging map");
    TRX_DYN_SMEM(smem);
    unit16* tile = (unit16*)smem;
    cx<double>* rhs = (cx<double>*)(smem + (size_t)FL_ROWS * FL_LDU * 16);     // [2][KC][NZT]: a + b, then a - b
    const int tid = threadIdx.x, b = blockIdx.y, n = 2 * N;
    const int j0 = blockIdx.x * FL_R;
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
        for (int i = 0; i < UPT; ++i) tile[(8 * i + srow) * FL_LDU + scol] = pf[i];
        for (int idx = tid; idx < KC * NZT; idx += FL_THREADS) {
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
            for (int i = 0; i < RPT; ++i) w[i] = to_f64(te[(rg + i * NRG) * (FL_LDU * VEC) + kk]);
#pragma unroll
            for (int t = 0; t < TPT; ++t) {
                const cx<double> r = myrhs[kk * NZT + t];
#pragma unroll
                for (int i = 0; i < RPT; ++i) cfma(acc[i][t], w[i], r);
            }
        }
    }
    __syncthreads();
    cx<double>* res = (cx<double>*)smem;                         // [FL_ROWS][NZT] over the tile (128 * 16 * 16 <= 128 * 17 * 16 bytes)
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int t = 0; t < TPT; ++t) res[(rg + i * NRG) * NZT + tg * TPT + t] = acc[i][t];
    __syncthreads();
    // epilogue: every (j, t) of the tile is owned by one thread; t runs fastest in out, so a row of depths is one contiguous store
    cx<T>* ob = out + (long)b * 6 * N * nz;
    for (int idx = tid; idx < FL_R * NZT; idx += FL_THREADS) {
        const int jj = idx / NZT, t = idx % NZT, j = j0 + jj;
        if (j >= N || t >= nt) continue;
        const cx<double> ex = res[jj * NZT + t], hx = res[(FL_R + jj) * NZT + t];
        const cx<double> ey = res[(2 * FL_R + jj) * NZT + t], hy = res[(3 * FL_R + jj) * NZT + t];
        const double kxj = kx[(long)b * N + j], kyj = ky[(long)b * N + j];
        const long o = (long)j * nz + t0 + t, cs = (long)N * nz;
        ob[o] = from_f64<T>(ex);
        ob[cs + o] = from_f64<T>(ey);
        ob[2 * cs + o] = from_f64<T>(hx);
        ob[3 * cs + o] = from_f64<T>(hy);
        ob[4 * cs + o] = from_f64<T>(kyj * hx - kxj * hy);
        ob[5 * cs + o] = from_f64<T>(kxj * ey - kyj * ex);
    }
}

template <class T, int NZT>
int field_pass(hipStream_t s, dim3 grid, const cx<T>* W, const cx<T>* V, const cx<T>* cp, const cx<T>* cm, const cx<T>* kz, const double* omega,
               const double* d, const double* z, int z_frac, const double* kx, const double* ky, int N, int nz, int t0, int nt, cx<T>* out) {
    constexpr size_t smem = fl_smem_bytes<T, NZT>();
    if (set_max_dyn_smem((const void*)layer_field_kernel<T, NZT>, smem)) return TRX_ERR_LAUNCH;
    TRX_LAUNCH((layer_field_kernel<T, NZT>), grid, dim3(FL_THREADS), smem, s, W, V, cp, cm, kz, omega, d, z, z_frac, kx, ky, N, nz, t0, nt, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int layer_field_t(hipStream_t s, const cx<T>* W, const cx<T>* V, const cx<T>* cp, const cx<T>* cm, const cx<T>* kz, const double* omega,
                  const double* d, const double* z, int z_frac, const double* kx, const double* ky, int N, int nz, int batch, cx<T>* out) {
    const dim3 grid(cdiv_i(N, FL_R), batch);
    for (int t0 = 0; t0 < nz; t0 += FL_ZT) {                     // W and V are streamed once per tile of up to 16 depths
        const int nt = nz - t0 < FL_ZT ? nz - t0 : FL_ZT;
        const int rc = nt <= 2 ? field_pass<T, 2>(s, grid, W, V, cp, cm, kz, omega, d, z, z_frac, kx, ky, N, nz, t0, nt, out)
                               : field_pass<T, FL_ZT>(s, grid, W, V, cp, cm, kz, omega, d, z, z_frac, kx, ky, N, nz, t0, nt, out);
        if (rc) return rc;
    }
    return TRX_OK;
}

// ---- trx_field_synth ----------------------------------------------------------------------------------------------------------------------
// A workgroup owns FS_TU x FS_TQ output points of one sweep point and all ncomp components of them: 4 waves, a lane per column q (a sample iv
// of a horizontal map, a depth t of a cut), FS_RU rows iu per thread, 6 x FS_RU complex fp64 accumulators.  Per chunk of harmonics the tables
// exp(i w kx_m u) [FS_TU, MC] and exp(i w ky_m v) [MC, FS_TQ] and the coefficients are staged in LDS as complex fp64; the phase of a point is
// the product of two table entries (4 real multiply-adds) and is shared by the components (4 each): 28 for six.  The sincos count is
// (FS_TU + FS_TQ) / (FS_TU FS_TQ) = 0.08 per (point, harmonic) for a map and 1 / FS_TQ for a cut, whose one table holds the whole phase.
constexpr int FS_THREADS = 256;
constexpr int FS_RU = 4;                               // rows iu per thread
constexpr int FS_TU = FS_RU * (FS_THREADS / 64);       // 16 rows iu per workgroup: wave w owns rows 4 w .. 4 w + 3
constexpr int FS_TQ = 64;                              // columns per workgroup
constexpr int FS_MAXC = 6;
constexpr int FS_MC_MAP = 16, FS_MC_CUT = 8;           // harmonics per chunk

template <bool CUT> constexpr size_t fs_smem_bytes() {
    return CUT ? sizeof(cx<double>) * (size_t)(FS_TU * FS_MC_CUT + FS_MAXC * FS_MC_CUT * FS_TQ)                        // 2 + 48 KiB
               : sizeof(cx<double>) * (size_t)(FS_TU * FS_MC_MAP + FS_MC_MAP * FS_TQ + FS_MAXC * FS_MC_MAP);           // 4 + 16 + 1.5 KiB
}

__device__ __forceinline__ cx<double> cis(double th) {
    double s, c;
    sincos(th, &s, &c);
    return cx<double>(c, s);
}

// grid (ceil(nq / FS_TQ), ceil(nu / FS_TU), batch), nq = nv (CUT false: T == 1) or T (CUT true: nv == 1).
// coef [batch, ncomp, N, T]; out [batch, ncomp, nu, nq].
template <class T, bool CUT>
__global__ __launch_bounds__(FS_THREADS) void field_synth_kernel(const cx<T>* __restrict__ coef, const double* __restrict__ kx,
                                                                 const double* __restrict__ ky, const double* __restrict__ omega,
                                                                 const double* __restrict__ u, const double* __restrict__ v, int ncomp, int N,
                                                                 int nu, int nq, cx<T>* __restrict__ out) {
    constexpr int MC = CUT ? FS_MC_CUT : FS_MC_MAP;
    constexpr int CQ = CUT ? FS_TQ : 1;                          // columns of a coefficient row in LDS
    TRX_DYN_SMEM(smem);
    cx<double>* pu = (cx<double>*)smem;                          // [FS_TU][MC]
    cx<double>* pv = pu + FS_TU * MC;                            // [MC][FS_TQ]            (maps only)
    cx<double>* cf = CUT ? pv : pv + MC * FS_TQ;                 // [FS_MAXC][MC][CQ]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.z;
    const int q0 = blockIdx.x * FS_TQ, u0 = blockIdx.y * FS_TU;
    const double om = omega[b];
    const double* kxb = kx + (long)b * N;
    const double* kyb = ky + (long)b * N;
    const cx<T>* cb = coef + (long)b * ncomp * N * (CUT ? nq : 1);
    const double v0 = CUT ? v[0] : 0.0;

    cx<double> acc[FS_MAXC][FS_RU];
#pragma unroll
    for (int c = 0; c < FS_MAXC; ++c)
#pragma unroll
        for (int i = 0; i < FS_RU; ++i) acc[c][i] = cx<double>(0.0, 0.0);

    for (int k0 = 0; k0 < N; k0 += MC) {
        __syncthreads();                                         // the previous chunk has been consumed
        for (int idx = tid; idx < FS_TU * MC; idx += FS_THREADS) {
            const int iu = idx / MC, m = k0 + idx % MC;
            cx<double> p(0.0, 0.0);                              // zero past the last harmonic / row: those terms add nothing
            if (m < N && u0 + iu < nu) p = cis(om * (CUT ? kxb[m] * u[u0 + iu] + kyb[m] * v0 : kxb[m] * u[u0 + iu]));
            pu[idx] = p;
        }
        if constexpr (!CUT) {
            for (int idx = tid; idx < MC * FS_TQ; idx += FS_THREADS) {
                const int m = k0 + idx / FS_TQ, q = q0 + idx % FS_TQ;
                cx<double> p(0.0, 0.0);
                if (m < N && q < nq) p = cis(om * (kyb[m] * v[q]));
                pv[idx] = p;
            }
        }
        for (int idx = tid; idx < ncomp * MC * CQ; idx += FS_THREADS) {
            const int c = idx / (MC * CQ), r = idx % (MC * CQ), m = k0 + r / CQ, q = q0 + r % CQ;
            cx<double> x(0.0, 0.0);
            if (m < N && (!CUT || q < nq)) x = to_f64(cb[CUT ? ((long)c * N + m) * nq + q : (long)c * N + m]);
            cf[idx] = x;
        }
        __syncthreads();
#pragma unroll 2
        for (int mm = 0; mm < MC; ++mm) {
            cx<double> w[FS_RU];
#pragma unroll
            for (int i = 0; i < FS_RU; ++i) w[i] = pu[(wv * FS_RU + i) * MC + mm];
            if constexpr (!CUT) {
                const cx<double> pq = pv[mm * FS_TQ + lane];
#pragma unroll
                for (int i = 0; i < FS_RU; ++i) w[i] = w[i] * pq;
            }
#pragma unroll
            for (int c = 0; c < FS_MAXC; ++c) {
                if (c < ncomp) {                                 // uniform
                    const cx<double> x = cf[(c * MC + mm) * CQ + (CUT ? lane : 0)];
#pragma unroll
                    for (int i = 0; i < FS_RU; ++i) cfma(acc[c][i], x, w[i]);
                }
            }
        }
    }
    const int q = q0 + lane;
    if (q >= nq) return;
    cx<T>* ob = out + (long)b * ncomp * nu * nq;
#pragma unroll
    for (int c = 0; c < FS_MAXC; ++c) {
        if (c < ncomp) {
#pragma unroll
            for (int i = 0; i < FS_RU; ++i) {
                const int iu = u0 + wv * FS_RU + i;
                if (iu < nu) ob[((long)c * nu + iu) * nq + q] = from_f64<T>(acc[c][i]);
            }
        }
    }
}

template <class T, bool CUT>
int field_synth_launch(hipStream_t s, const cx<T>* coef, const double* kx, const double* ky, const double* omega, const double* u, const double* v,
                       int ncomp, int N, int nu, int nq, int batch, cx<T>* out) {
    constexpr size_t smem = fs_smem_bytes<CUT>();
    if (set_max_dyn_smem((const void*)field_synth_kernel<T, CUT>, smem)) return TRX_ERR_LAUNCH;
    const dim3 grid(cdiv_i(nq, FS_TQ), cdiv_i(nu, FS_TU), batch);
    TRX_LAUNCH((field_synth_kernel<T, CUT>), grid, dim3(FS_THREADS), smem, s, coef, kx, ky, omega, u, v, ncomp, N, nu, nq, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int field_synth_t(hipStream_t s, const void* coef, const double* kx, const double* ky, const double* omega, const double* u, const double* v,
                  int ncomp, int N, int T_, int nu, int nv, int batch, void* out) {
    if (T_ > 1) return field_synth_launch<T, true>(s, (const cx<T>*)coef, kx, ky, omega, u, v, ncomp, N, nu, T_, batch, (cx<T>*)out);
    return field_synth_launch<T, false>(s, (const cx<T>*)coef, kx, ky, omega, u, v, ncomp, N, nu, nv, batch, (cx<T>*)out);
}

}  // namespace

extern "C" int trx_layer_field(int dtype, const void* W, const void* V, const void* cplus, const void* cminus, const void* kz, const double* omega,
                               const double* d, const double* z, int z_is_fraction, const double* kx, const double* ky, int N, int nz, int batch,
                               void* out, void* stream) {
    if (N < 1 || nz < 0 || batch < 0 || batch > 65535) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (nz == 0 || batch == 0) return TRX_OK;                                   // nothing to compute: no buffer is touched, none is required
    if (!W || !V || !cplus || !cminus || !kz || !omega || !d || !z || !kx || !ky || !out) return TRX_ERR_ARG;
    if (((size_t)W | (size_t)V) & 15) return TRX_ERR_ARG;                       // rows are read in 16-byte units
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return layer_field_t<float>(s, (const cx<float>*)W, (const cx<float>*)V, (const cx<float>*)cplus, (const cx<float>*)cminus,
                                    (const cx<float>*)kz, omega, d, z, z_is_fraction, kx, ky, N, nz, batch, (cx<float>*)out);
    return layer_field_t<double>(s, (const cx<double>*)W, (const cx<double>*)V, (const cx<double>*)cplus, (const cx<double>*)cminus,
                                 (const cx<double>*)kz, omega, d, z, z_is_fraction, kx, ky, N, nz, batch, (cx<double>*)out);
}

extern "C" int trx_field_synth(int dtype, const void* coef, const double* kx, const double* ky, const double* omega, const double* u,
                               const double* v, int ncomp, int N, int T, int nu, int nv, int batch, void* out, void* stream) {
    if (ncomp < 1 || ncomp > FS_MAXC || N < 1 || T < 1 || nu < 0 || nv < 0 || batch < 0 || batch > 65535) return TRX_ERR_ARG;
    if (nv > 1 && T > 1) return TRX_ERR_ARG;                                    // a horizontal map (T = 1) or a vertical cut (nv = 1)
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (nu == 0 || nv == 0 || batch == 0) return TRX_OK;                        // nothing to compute: no buffer is touched, none is required
    if (cdiv_i(nu, FS_TU) > 65535) return TRX_ERR_ARG;
    if (!coef || !kx || !ky || !omega || !u || !v || !out) return TRX_ERR_ARG;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64) return field_synth_t<float>(s, coef, kx, ky, omega, u, v, ncomp, N, T, nu, nv, batch, out);
    return field_synth_t<double>(s, coef, kx, ky, omega, u, v, ncomp, N, T, nu, nv, batch, out);
}
