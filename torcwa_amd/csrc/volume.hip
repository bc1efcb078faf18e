// Closed-form z integrals of modal products inside a layer (include/trx.h: trx_modal_overlap).
//
//   out[b,r] = sum_{k,l} M[b,k,l] T_kl(z0, z1),   (z0, z1) = zr[b,r]
//   T_kl = conj(c+_k) c+_l G++_kl + s conj(c+_k) c-_l G+-_kl + s conj(c-_k) c+_l G-+_kl + conj(c-_k) c-_l G--_kl
//   G++ = int conj(e_k(z)) e_l(z) dz,  G+- = int conj(e_k(z)) e_l(d - z) dz,  G-+ = int conj(e_k(d - z)) e_l(z) dz,
//   G-- = int conj(e_k(d - z)) e_l(d - z) dz,   e_k(z) = exp(i w kz_k z),  Im kz >= 0
//
// Every integrand is g(z) = exp(alpha z + beta) with |g| <= 1 on [0, d], so int_{lo}^{hi} g = g(z_e) D phi(x), D = hi - lo, phi(x) = (e^x - 1) / x,
// with the end point z_e = lo, x = alpha D where Re alpha <= 0 and z_e = hi, x = -alpha D otherwise: Re x <= 0, nothing overflows and no 0 * inf
// appears.  g(z_e) is a product of per-mode end-point amplitudes a_k(z) = c+_k e_k(z), b_k(z) = c-_k e_k(d - z) at lo and hi, and the four
// integrals share two arguments:  x1 = (-(wi_k + wi_l), wr_l - wr_k) for G++ and G--, x2 = -(|wi_l - wi_k|, +-(wr_k + wr_l)) for G+- and G-+,
// (wr, wi) = w D (Re kz, Im kz).  e^{x1} is a product of per-mode factors; e^{x2} costs one real exp.  phi is its series for |x| < 1/2
// (phi(0) = 1 exactly: every diagonal term of a lossless propagating mode) and (e^x - 1) / x otherwise.  A reversed range is integrated as
// (min, max) and negated.
//
// A workgroup owns 16 rows k of M; its four waves walk the columns l in chunks of 64 (lane = column), each thread holding its 16 elements of
// M in registers for all ranges of the pass.  The end-point factors of the 16 rows live in LDS (wave-uniform broadcast reads), those of a
// lane's column in registers (formed once per range, used for 16 rows).  Neither the G matrices nor T exist in memory.  Traffic model: n^2
// elements of M per point and tile of up to 16 ranges, everything else O(n nr).  All arithmetic is fp64 for both dtypes.  Per workgroup one
// partial sum per range goes to the workspace (waves are combined in a fixed order) and a second kernel adds the partials in a fixed order:
// deterministic, no floating-point atomics.
#include "common.hpp"

using namespace trx;

namespace {

constexpr int VO_THREADS = 256;   // four waves
constexpr int VO_WAVES = VO_THREADS / 64;
constexpr int VO_KB = 16;         // rows k per workgroup
constexpr int VO_RT = 16;         // ranges per pass over M

// end-point factors of one mode for one range [lo, hi]
struct alignas(16) modef {
    cx<double> alo, ahi, blo, bhi;   // c+ e(lo), c+ e(hi), c- e(d - lo), c- e(d - hi)
    cx<double> u;                    // exp(i wr)
    double r, wr, wi;                // exp(-wi);  (wr, wi) = w (hi - lo) (Re kz, Im kz)
    double pad;
};

constexpr size_t vo_smem_bytes() { return sizeof(modef) * VO_KB * VO_RT + sizeof(cx<double>) * VO_WAVES * VO_RT + sizeof(double) * 4 * VO_RT; }

template <class T> __device__ __forceinline__ cx<double> vo_f64(cx<T> v) { return cx<double>((double)v.x, (double)v.y); }

__device__ __forceinline__ modef mode_factors(cx<double> cp, cx<double> cm, cx<double> q, double om, double dd, double lo, double hi) {
    modef f;
    auto e = [&](double z) { const double w = om * z; return cexp(cx<double>(-w * q.y, w * q.x)); };
    f.alo = cp * e(lo);
    f.ahi = cp * e(hi);
    f.blo = cm * e(dd - lo);
    f.bhi = cm * e(dd - hi);
    f.wr = om * q.x * (hi - lo);
    f.wi = om * q.y * (hi - lo);
    f.u = cx<double>(cos(f.wr), sin(f.wr));
    f.r = exp(-f.wi);
    f.pad = 0.0;
    return f;
}

// phi(x) = (e^x - 1) / x for Re x <= 0, ex = e^x
__device__ __forceinline__ cx<double> phi(cx<double> x, cx<double> ex) {
    if (x.x * x.x + x.y * x.y < 0.25) {             // 1 + x/2 (1 + x/3 (... (1 + x/16))): truncation below |x|^16 / 17! < 5e-20
        cx<double> p(1.0, 0.0);
#pragma unroll
        for (int j = 16; j >= 2; --j) {
            const cx<double> t = x * p;
            p = cx<double>(1.0 + t.x * (1.0 / j), t.y * (1.0 / j));
        }
        return p;
    }
    return cdiv(ex - cx<double>(1.0, 0.0), x);
}

// T_kl / (hi - lo)
__device__ __forceinline__ cx<double> pair_term(const modef& fk, const modef& fl, double sd) {
    const cx<double> x1(-(fk.wi + fl.wi), fl.wr - fk.wr);
    const cx<double> p1 = phi(x1, (fk.r * fl.r) * (conj(fk.u) * fl.u));
    const cx<double> t1 = conj(fk.alo) * fl.alo + conj(fk.bhi) * fl.bhi;          // G++ from lo, G-- from hi
    const double re2 = fl.wi - fk.wi, im2 = -(fk.wr + fl.wr);
    const cx<double> us = fk.u * fl.u;
    cx<double> p2, t2;
    if (re2 <= 0.0) {                                                               // G+- from lo, G-+ from hi
        p2 = phi(cx<double>(re2, im2), exp(re2) * conj(us));
        t2 = conj(fk.alo) * fl.blo + conj(fk.bhi) * fl.ahi;
    } else {                                                                        // G+- from hi, G-+ from lo
        p2 = phi(cx<double>(-re2, -im2), exp(-re2) * us);
        t2 = conj(fk.ahi) * fl.bhi + conj(fk.blo) * fl.alo;
    }
    return p1 * t1 + sd * (p2 * t2);
}

// grid (ceil(n / VO_KB), batch).  Ranges t0 .. t0 + nt - 1 (nt <= VO_RT) of zr [batch, nr, 2]; part [batch, gridDim.x, nr].
template <class T>
__global__ __launch_bounds__(VO_THREADS) void modal_overlap_kernel(const cx<T>* __restrict__ M, const cx<T>* __restrict__ cplus,
                                                                   const cx<T>* __restrict__ cminus, const cx<T>* __restrict__ kz,
                                                                   const double* __restrict__ omega, const double* __restrict__ thick,
                                                                   const double* __restrict__ zr, int z_frac, int s, int n, int nr, int t0, int nt,
                                                                   cx<double>* __restrict__ part) {
    TRX_DYN_SMEM(smem);
    modef* kf = (modef*)smem;                                                       // [VO_KB][VO_RT]
    cx<double>* wsum = (cx<double>*)(smem + sizeof(modef) * VO_KB * VO_RT);         // [VO_WAVES][VO_RT]
    double* rng = (double*)(wsum + VO_WAVES * VO_RT);                               // [VO_RT][4]: lo, hi, signed length
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int k0 = blockIdx.x * VO_KB;
    const cx<T>* Mb = M + (long)b * n * n;
    const cx<T>* cpb = cplus + (long)b * n;
    const cx<T>* cmb = cminus + (long)b * n;
    const cx<T>* kzb = kz + (long)b * n;
    const double om = omega[b], dd = thick[b], sd = (double)s;

    if (tid < VO_RT) {
        double lo = 0.0, hi = 0.0, sg = 0.0;
        if (tid < nt) {
            double z0 = zr[((long)b * nr + t0 + tid) * 2], z1 = zr[((long)b * nr + t0 + tid) * 2 + 1];
            if (z_frac) { z0 *= dd; z1 *= dd; }
            lo = z1 < z0 ? z1 : z0;
            hi = z1 < z0 ? z0 : z1;
            sg = z1 < z0 ? -1.0 : 1.0;
        }
        rng[tid * 4] = lo;
        rng[tid * 4 + 1] = hi;
        rng[tid * 4 + 2] = sg * (hi - lo);
    }
    if (tid < VO_WAVES * VO_RT) wsum[tid] = cx<double>(0.0, 0.0);
    __syncthreads();
    {                                                                               // VO_KB * VO_RT == VO_THREADS: one entry per thread
        static_assert(VO_KB * VO_RT == VO_THREADS, "factor map");
        const int kk = tid / VO_RT, r = tid % VO_RT, k = k0 + kk;
        const bool on = k < n && r < nt;
        const cx<double> zero(0.0, 0.0);
        kf[tid] = mode_factors(on ? vo_f64(cpb[k]) : zero, on ? vo_f64(cmb[k]) : zero, on ? vo_f64(kzb[k]) : zero, om, dd, rng[r * 4], rng[r * 4 + 1]);
    }
    __syncthreads();

    const int kcount = n - k0 < VO_KB ? n - k0 : VO_KB;
    for (int c = wave; c * 64 < n; c += VO_WAVES) {                                 // wave-uniform
        const int l = c * 64 + lane;
        const bool live = l < n;
        cx<double> m[VO_KB];
#pragma unroll
        for (int kk = 0; kk < VO_KB; ++kk)
            m[kk] = (live && kk < kcount) ? vo_f64(Mb[(long)(k0 + kk) * n + l]) : cx<double>(0.0, 0.0);
        const cx<double> cpl = live ? vo_f64(cpb[l]) : cx<double>(0.0, 0.0);
        const cx<double> cml = live ? vo_f64(cmb[l]) : cx<double>(0.0, 0.0);
        const cx<double> ql = live ? vo_f64(kzb[l]) : cx<double>(0.0, 0.0);
        for (int r = 0; r < nt; ++r) {
            cx<double> acc(0.0, 0.0);
            if (live) {
                const modef fl = mode_factors(cpl, cml, ql, om, dd, rng[r * 4], rng[r * 4 + 1]);
#pragma unroll
                for (int kk = 0; kk < VO_KB; ++kk)
                    if (kk < kcount) cfma(acc, m[kk], pair_term(kf[kk * VO_RT + r], fl, sd));
            }
            const double re = wave_sum(acc.x), im = wave_sum(acc.y);
            if (lane == 0) wsum[wave * VO_RT + r] += cx<double>(re, im);            // this wave's own slot, chunks in order
        }
    }
    __syncthreads();
    if (tid < nt) {
        cx<double> v = wsum[tid];
#pragma unroll
        for (int w = 1; w < VO_WAVES; ++w) v += wsum[w * VO_RT + tid];
        part[((long)b * gridDim.x + blockIdx.x) * nr + t0 + tid] = rng[tid * 4 + 2] * v;
    }
}

__global__ __launch_bounds__(256) void overlap_finish_kernel(const cx<double>* __restrict__ part, int groups, int nr, int batch,
                                                             cx<double>* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)batch * nr) return;
    const int b = (int)(i / nr), t = (int)(i % nr);
    cx<double> s(0.0, 0.0);
    for (int g = 0; g < groups; ++g) s += part[((long)b * groups + g) * nr + t];
    out[i] = s;
}

template <class T>
int modal_overlap_t(hipStream_t st, const cx<T>* M, const cx<T>* cp, const cx<T>* cm, const cx<T>* kz, const double* omega, const double* d,
                    const double* zr, int z_frac, int s, int n, int nr, int batch, cx<double>* out, cx<double>* part) {
    const int groups = cdiv_i(n, VO_KB);
    const dim3 grid(groups, batch);
    for (int t0 = 0; t0 < nr; t0 += VO_RT) {                                        // M is streamed once per tile of up to 16 ranges
        const int nt = nr - t0 < VO_RT ? nr - t0 : VO_RT;
        TRX_LAUNCH((modal_overlap_kernel<T>), grid, dim3(VO_THREADS), vo_smem_bytes(), st, M, cp, cm, kz, omega, d, zr, z_frac, s, n, nr, t0, nt,
                   part);
        TRX_CHECK_LAUNCH();
    }
    TRX_LAUNCH(overlap_finish_kernel, dim3(cdiv_i((long)batch * nr, 256)), dim3(256), 0, st, part, groups, nr, batch, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace

extern "C" size_t trx_modal_overlap_ws_bytes(int dtype, int n, int nr, int batch) {
    (void)dtype;
    if (n < 0 || nr < 0 || batch < 0) return 0;
    return sizeof(cx<double>) * (size_t)cdiv_i(n, VO_KB) * (size_t)nr * (size_t)batch;
}

extern "C" int trx_modal_overlap(int dtype, const void* M, const void* cplus, const void* cminus, const void* kz, const double* omega,
                                 const double* d, const double* zr, int z_is_fraction, int s, int n, int nr, int batch, void* out, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (n < 1 || nr < 0 || batch < 0 || batch > 65535 || (s != 1 && s != -1)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (nr == 0 || batch == 0) return TRX_OK;                                       // nothing to compute: no buffer is touched, none is required
    if (!M || !cplus || !cminus || !kz || !omega || !d || !zr || !out || !ws) return TRX_ERR_ARG;
    if (((size_t)M | (size_t)out | (size_t)ws) & 15) return TRX_ERR_ARG;
    if (ws_bytes < trx_modal_overlap_ws_bytes(dtype, n, nr, batch)) return TRX_ERR_WORKSPACE;
    hipStream_t st = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return modal_overlap_t<float>(st, (const cx<float>*)M, (const cx<float>*)cplus, (const cx<float>*)cminus, (const cx<float>*)kz, omega, d,
                                      zr, z_is_fraction, s, n, nr, batch, (cx<double>*)out, (cx<double>*)ws);
    return modal_overlap_t<double>(st, (const cx<double>*)M, (const cx<double>*)cplus, (const cx<double>*)cminus, (const cx<double>*)kz, omega,
                                   d, zr, z_is_fraction, s, n, nr, batch, (cx<double>*)out, (cx<double>*)ws);
}
