// Vector-shape layers: the Fourier coefficients of ellipses, rectangles and simple polygons in closed form (no grid), their adjoint, and the
// adjoint of the Toeplitz gather.  No reference counterpart (the reference rasterises everything); the closed forms are the ones S4 and other
// design-oriented RCWA codes use.
//
//   eps(r) = sum_G c(G) e^{+iG.r},  G = p b1 + q b2,  c(G) = val[0] delta_G0 + sum_s val[s+1] chi_s(G),  chi_s(G) = (1/A) int_shape e^{-iG.r} d2r
//   ellipse   chi = (pi Rx Ry / A) jinc(rho) e^{-iG.c},  rho = hypot(Rx G'x, Ry G'y),  jinc(t) = 2 J1(t)/t
//   rectangle chi = (Wx Wy / A) sinc(G'x Wx/2) sinc(G'y Wy/2) e^{-iG.c}                   G' = (cos th Gx + sin th Gy, -sin th Gx + cos th Gy)
//   polygon   chi = (i / (A |G|^2)) sum_k (Gx e_ky - Gy e_kx) e^{-iG.m_k} sinc(G.e_k/2)   (G != 0; the shoelace area / A at G = 0)
// Every sinc, jinc and hat integral has a series branch: an axis-aligned edge makes G.e exactly 0 for whole rows of the box.
// All arithmetic is fp64 for both dtypes.  These kernels are latency- and transcendental-bound (one sincos / j1 per thread, shape and edge;
// a box of 61 x 61 coefficients is 60 KB): the memory traffic is the box written once and, in the gather, read once per 32 rows of `out`.
#include <cmath>
#include <vector>

#include "common.hpp"

namespace trx {
namespace {

typedef cx<double> zc;

enum { SHAPE_ELLIPSE = 0, SHAPE_RECTANGLE = 1, SHAPE_POLYGON = 2 };
constexpr int SH_BLOCK = 256;          // threads per workgroup and doubles of a parameter row per staging pass (128 vertices)

struct Recip { double b1x, b1y, b2x, b2y; };

// ---- scalar functions with their small-argument branches ---------------------------------------------------------------------------------
__device__ __forceinline__ double sinc_f(double t) {             // sin t / t
    if (fabs(t) < 1e-3) { const double u = t * t; return 1.0 - u / 6.0 * (1.0 - u / 20.0 * (1.0 - u / 42.0)); }
    return sin(t) / t;
}
__device__ __forceinline__ double dsinc_f(double t) {            // (cos t - sinc t) / t = sum_n (-1)^n 2n t^(2n-1) / (2n+1)!
    if (fabs(t) < 1.0) {
        const double u = t * t;
        double term = -t / 3.0, acc = term;                      // n = 1
        for (int n = 2; n <= 11; ++n) {
            term *= -u * (double)n / ((double)(n - 1) * (2.0 * n) * (2.0 * n + 1.0));
            acc += term;
        }
        return acc;
    }
    return (cos(t) - sin(t) / t) / t;
}
__device__ __forceinline__ double jinc_f(double t) {             // 2 J1(t) / t
    if (t < 1e-3) { const double u = t * t; return 1.0 - u / 8.0 * (1.0 - u / 24.0 * (1.0 - u / 48.0)); }
    return 2.0 * j1(t) / t;
}
__device__ __forceinline__ double jinc2_f(double t) {            // 2 J2(t) / t^2 = -jinc'(t) / t
    if (t < 1e-2) { const double u = t * t; return 0.25 * (1.0 - u / 12.0 * (1.0 - u / 32.0 * (1.0 - u / 60.0))); }
    return 2.0 * jn(2, t) / (t * t);
}
// hat integral int_0^1 t e^{-i beta t} dt = (e^{-i beta}(1 + i beta) - 1) / beta^2 = sum_n (-i beta)^n / (n! (n + 2))
__device__ __forceinline__ zc hat_f(double beta) {
    if (fabs(beta) < 1.0) {
        zc pw(1.0, 0.0), acc(0.5, 0.0);
        for (int n = 1; n <= 22; ++n) {
            pw = zc(pw.y * beta / n, -pw.x * beta / n);          // pw *= -i beta / n
            acc += (1.0 / (n + 2.0)) * pw;
        }
        return acc;
    }
    double s, c;
    sincos(beta, &s, &c);
    const zc e(c, -s);
    const zc num = e * zc(1.0, beta) - zc(1.0, 0.0);
    return (1.0 / (beta * beta)) * num;
}
__device__ __forceinline__ zc expmi(double phi) {                // e^{-i phi}
    double s, c;
    sincos(phi, &s, &c);
    return zc(c, -s);
}

// ---- chi of one shape at one G ------------------------------------------------------------------------------------------------------------
// q: Rx, Ry, Cx, Cy, theta (ellipse) or Wx, Wy, Cx, Cy, theta (rectangle)
__device__ __forceinline__ void rotated(const double* q, double Gx, double Gy, double* gx, double* gy) {
    double s, c;
    sincos(q[4], &s, &c);
    *gx = c * Gx + s * Gy;
    *gy = -s * Gx + c * Gy;
}
__device__ __forceinline__ zc ellipse_chi(const double* q, double Gx, double Gy, double inv_area) {
    double gx, gy;
    rotated(q, Gx, Gy, &gx, &gy);
    const double rho = hypot(q[0] * gx, q[1] * gy);
    return (M_PI * q[0] * q[1] * inv_area * jinc_f(rho)) * expmi(Gx * q[2] + Gy * q[3]);
}
__device__ __forceinline__ zc rectangle_chi(const double* q, double Gx, double Gy, double inv_area) {
    double gx, gy;
    rotated(q, Gx, Gy, &gx, &gy);
    return (q[0] * q[1] * inv_area * sinc_f(0.5 * gx * q[0]) * sinc_f(0.5 * gy * q[1])) * expmi(Gx * q[2] + Gy * q[3]);
}
// one edge a -> b of a polygon: its term of the edge sum (G != 0) or of the shoelace sum (G = 0, in the real part)
__device__ __forceinline__ zc edge_term(double ax, double ay, double bx, double by, double Gx, double Gy, bool zero) {
    if (zero) return zc(ax * by - bx * ay, 0.0);
    const double ex = bx - ax, ey = by - ay;
    const double w = (Gx * ey - Gy * ex) * sinc_f(0.5 * (Gx * ex + Gy * ey));
    return w * expmi(0.5 * (Gx * (ax + bx) + Gy * (ay + by)));
}
__device__ __forceinline__ zc polygon_finish(zc sum, double Gx, double Gy, double inv_area, bool zero) {
    if (zero) return zc(0.5 * inv_area * sum.x, 0.0);
    const double f = inv_area / (Gx * Gx + Gy * Gy);
    return zc(-f * sum.y, f * sum.x);                            // i f sum
}

// d chi / d q[j] of an ellipse or a rectangle
__device__ __forceinline__ zc ellipse_dchi(const double* q, int j, double Gx, double Gy, double inv_area) {
    double gx, gy;
    rotated(q, Gx, Gy, &gx, &gy);
    const double rho = hypot(q[0] * gx, q[1] * gy);
    const double amp = M_PI * q[0] * q[1] * inv_area;
    const zc ph = expmi(Gx * q[2] + Gy * q[3]);
    switch (j) {
    case 0: return (M_PI * q[1] * inv_area * jinc_f(rho) - amp * jinc2_f(rho) * q[0] * gx * gx) * ph;
    case 1: return (M_PI * q[0] * inv_area * jinc_f(rho) - amp * jinc2_f(rho) * q[1] * gy * gy) * ph;
    case 2: { const zc v = (amp * jinc_f(rho)) * ph; return zc(Gx * v.y, -Gx * v.x); }          // -i Gx chi
    case 3: { const zc v = (amp * jinc_f(rho)) * ph; return zc(Gy * v.y, -Gy * v.x); }
    default: return (-amp * jinc2_f(rho) * (q[0] * q[0] - q[1] * q[1]) * gx * gy) * ph;
    }
}
__device__ __forceinline__ zc rectangle_dchi(const double* q, int j, double Gx, double Gy, double inv_area) {
    double gx, gy;
    rotated(q, Gx, Gy, &gx, &gy);
    const double tx = 0.5 * gx * q[0], ty = 0.5 * gy * q[1];
    const zc ph = expmi(Gx * q[2] + Gy * q[3]);
    switch (j) {
    case 0: return (q[1] * inv_area * cos(tx) * sinc_f(ty)) * ph;                               // d(W sinc(g W / 2)) / dW = cos(g W / 2)
    case 1: return (q[0] * inv_area * sinc_f(tx) * cos(ty)) * ph;
    case 2: { const zc v = (q[0] * q[1] * inv_area * sinc_f(tx) * sinc_f(ty)) * ph; return zc(Gx * v.y, -Gx * v.x); }
    case 3: { const zc v = (q[0] * q[1] * inv_area * sinc_f(tx) * sinc_f(ty)) * ph; return zc(Gy * v.y, -Gy * v.x); }
    default:                                                                                    // dG'x/dth = G'y, dG'y/dth = -G'x
        return (q[0] * q[1] * inv_area * (dsinc_f(tx) * 0.5 * q[0] * gy * sinc_f(ty) - sinc_f(tx) * dsinc_f(ty) * 0.5 * q[1] * gx)) * ph;
    }
}
// d(A chi) / d(component comp of vertex v) in boundary-velocity form: the two edges at v, each n_e l_e int_0^1 t e^{-iG.(a + t (v - a))} dt
// with a the other end.  (px, py) is the vertex before v, (nx, ny) the one after (counter-clockwise).
__device__ __forceinline__ zc vertex_dchi(double px, double py, double vx, double vy, double nx, double ny, int comp, double Gx, double Gy) {
    const double n1 = comp == 0 ? (vy - py) : -(vx - px);        // edge p -> v: (e_y, -e_x)
    const double n2 = comp == 0 ? (ny - vy) : -(nx - vx);        // edge v -> n
    const zc t1 = expmi(Gx * px + Gy * py) * hat_f(Gx * (vx - px) + Gy * (vy - py));
    const zc t2 = expmi(Gx * nx + Gy * ny) * hat_f(Gx * (vx - nx) + Gy * (vy - ny));
    return n1 * t1 + n2 * t2;
}

__device__ __forceinline__ void box_index(int e, int mmax, int nmax, const Recip& r, int* p, int* q, double* Gx, double* Gy) {
    const int nq = 4 * nmax + 1;
    *p = e / nq - 2 * mmax;
    *q = e - (e / nq) * nq - 2 * nmax;
    *Gx = *p * r.b1x + *q * r.b2x;
    *Gy = *p * r.b1y + *q * r.b2y;
}

// ---- forward: one thread per (b, p, q); the thread loops over shapes and edges -------------------------------------------------------------
// A shape's parameters are staged in LDS in passes of SH_BLOCK doubles (plus the vertex that closes the pass's last edge): an ellipse or a
// rectangle takes one pass of 5, a polygon of more than 128 vertices several.  kind / voff / val are wave-uniform reads.
__global__ __launch_bounds__(SH_BLOCK) void shapes_coef_kernel(const int* __restrict__ kind, const int* __restrict__ voff, int S,
                                                               const double* __restrict__ par, int npar, const zc* __restrict__ val, Recip r,
                                                               double inv_area, int mmax, int nmax, zc* __restrict__ coef) {
    TRX_DYN_SMEM(smem);
    double* stage = reinterpret_cast<double*>(smem);             // [SH_BLOCK + 2]
    const int b = blockIdx.y;
    const int nbox = (4 * mmax + 1) * (4 * nmax + 1);
    const int e = blockIdx.x * SH_BLOCK + threadIdx.x;
    const bool active = e < nbox;
    int p, q;
    double Gx, Gy;
    box_index(active ? e : 0, mmax, nmax, r, &p, &q, &Gx, &Gy);
    const bool zero = p == 0 && q == 0;
    const double* pr = par + (long)b * npar;
    const zc* vl = val + (long)b * (S + 1);
    zc acc = zero ? vl[0] : zc(0.0, 0.0);
    for (int s = 0; s < S; ++s) {
        const int k = kind[s], o = voff[s], len = voff[s + 1] - o;
        zc chi(0.0, 0.0);
        if (k != SHAPE_POLYGON) {
            __syncthreads();                                     // the previous shape's parameters have been read
            if (threadIdx.x < 5) stage[threadIdx.x] = pr[o + threadIdx.x];
            __syncthreads();
            chi = k == SHAPE_ELLIPSE ? ellipse_chi(stage, Gx, Gy, inv_area) : rectangle_chi(stage, Gx, Gy, inv_area);
        } else {
            for (int c0 = 0; c0 < len; c0 += SH_BLOCK) {
                const int cnt = len - c0 < SH_BLOCK ? len - c0 : SH_BLOCK;
                __syncthreads();
                for (int t = threadIdx.x; t < cnt + 2; t += SH_BLOCK) {
                    int idx = c0 + t;
                    if (idx >= len) idx -= len;                  // the last edge closes on vertex 0
                    stage[t] = pr[o + idx];
                }
                __syncthreads();
                for (int v = 0; v < cnt; v += 2) chi += edge_term(stage[v], stage[v + 1], stage[v + 2], stage[v + 3], Gx, Gy, zero);
            }
            chi = polygon_finish(chi, Gx, Gy, inv_area, zero);
        }
        cfma(acc, vl[s + 1], chi);
    }
    if (active) coef[(long)b * nbox + e] = acc;
}

// ---- adjoint of the coefficients ------------------------------------------------------------------------------------------------------------
// One workgroup per (b, item): item w < npar is the parameter par[b, w] (gpar = Re sum_pq conj(gbox) dc/dpar), w = npar is val[b, 0] and
// w = npar + 1 + s is val[b, s + 1] (gval = sum_pq conj(chi_s) gbox, torch's convention for c linear in val).  Each thread sums its box entries
// in ascending order, then a fixed LDS tree: two runs give the same bits.
// One workgroup per PARAMETER, not per shape or vertex: the five parameters of an ellipse or rectangle each redo its sincos / j1 / jn over the
// box and the two coordinates of a vertex the same two hat integrals -- a 2 - 5 x saving left for the day the backward matters (it is a few
// ms next to an eigen-adjoint).  jn(2, t) just above the 1e-2 series threshold of jinc2_f loses relative accuracy (forward recurrence, about
// 1e-11 there) on a term that is itself O(rho^2): harmless in absolute terms.
__device__ __forceinline__ zc block_sum(zc v, zc* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = SH_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ zc polygon_chi_global(const double* v, int K, double Gx, double Gy, double inv_area, bool zero) {
    zc sum(0.0, 0.0);
    for (int k = 0; k < K; ++k) {
        const int k1 = k + 1 < K ? k + 1 : 0;
        sum += edge_term(v[2 * k], v[2 * k + 1], v[2 * k1], v[2 * k1 + 1], Gx, Gy, zero);
    }
    return polygon_finish(sum, Gx, Gy, inv_area, zero);
}

__global__ __launch_bounds__(SH_BLOCK) void shapes_backward_kernel(const int* __restrict__ kind, const int* __restrict__ voff, int S,
                                                                   const double* __restrict__ par, int npar, const zc* __restrict__ val,
                                                                   Recip r, double inv_area, int mmax, int nmax, const zc* __restrict__ gbox,
                                                                   double* __restrict__ gpar, zc* __restrict__ gval) {
    TRX_DYN_SMEM(smem);
    zc* red = reinterpret_cast<zc*>(smem);                       // [SH_BLOCK]
    const int w = blockIdx.x, b = blockIdx.y;
    const int nbox = (4 * mmax + 1) * (4 * nmax + 1);
    const double* pr = par + (long)b * npar;
    const zc* g = gbox + (long)b * nbox;
    if (w == npar) {                                             // the background multiplies delta_G0
        if (threadIdx.x == 0) gval[(long)b * (S + 1)] = g[2 * mmax * (4 * nmax + 1) + 2 * nmax];
        return;
    }
    int s;
    if (w < npar) {
        s = -1;
        for (int t = 0; t < S; ++t)
            if (w >= voff[t] && w < voff[t + 1]) s = t;
        if (s < 0) {                                             // a slot of the row that belongs to no shape
            if (threadIdx.x == 0) gpar[(long)b * npar + w] = 0.0;
            return;
        }
    } else {
        s = w - npar - 1;
    }
    const int k = kind[s], o = voff[s], K = (voff[s + 1] - o) / 2;
    const double* q = pr + o;
    zc acc(0.0, 0.0);
    if (w > npar) {
        for (int e = threadIdx.x; e < nbox; e += SH_BLOCK) {
            int p, qq;
            double Gx, Gy;
            box_index(e, mmax, nmax, r, &p, &qq, &Gx, &Gy);
            const bool zero = p == 0 && qq == 0;
            const zc chi = k == SHAPE_ELLIPSE ? ellipse_chi(q, Gx, Gy, inv_area)
                         : k == SHAPE_RECTANGLE ? rectangle_chi(q, Gx, Gy, inv_area) : polygon_chi_global(q, K, Gx, Gy, inv_area, zero);
            cfma_conj(acc, chi, g[e]);
        }
        const zc tot = block_sum(acc, red);
        if (threadIdx.x == 0) gval[(long)b * (S + 1) + s + 1] = tot;
        return;
    }
    const int j = w - o;
    const zc delta = val[(long)b * (S + 1) + s + 1];
    double px = 0, py = 0, vx = 0, vy = 0, nx = 0, ny = 0;
    if (k == SHAPE_POLYGON) {
        const int kv = j / 2, kp = kv > 0 ? kv - 1 : K - 1, kn = kv + 1 < K ? kv + 1 : 0;
        px = q[2 * kp]; py = q[2 * kp + 1]; vx = q[2 * kv]; vy = q[2 * kv + 1]; nx = q[2 * kn]; ny = q[2 * kn + 1];
    }
    for (int e = threadIdx.x; e < nbox; e += SH_BLOCK) {
        int p, qq;
        double Gx, Gy;
        box_index(e, mmax, nmax, r, &p, &qq, &Gx, &Gy);
        zc d;
        if (k == SHAPE_ELLIPSE) d = ellipse_dchi(q, j, Gx, Gy, inv_area);
        else if (k == SHAPE_RECTANGLE) d = rectangle_dchi(q, j, Gx, Gy, inv_area);
        else d = inv_area * vertex_dchi(px, py, vx, vy, nx, ny, j & 1, Gx, Gy);
        d = delta * d;
        acc.x += g[e].x * d.x + g[e].y * d.y;                    // Re(conj(gbox) dc/dpar)
    }
    const zc tot = block_sum(acc, red);
    if (threadIdx.x == 0) gpar[(long)b * npar + w] = tot.x;
}

// ---- adjoint of the Toeplitz gather ----------------------------------------------------------------------------------------------------------
// gbox[b,p,q] = sum over the pairs (i, j) with m_i - m_j = p, n_i - n_j = q of gE[b,i,j].  A gather: inv[(m + mmax)(2 nmax + 1) + n + nmax] = the
// index of harmonic (m, n) in the list or -1, built on the device; one wave per (p, q, b) runs over j, looks up i, sums in fp64 in ascending j
// and ends with the fixed xor tree of wave_sum.  Every element of gE is read exactly once by the whole grid; no atomics.
__global__ void inverse_fill_kernel(int* __restrict__ inv, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) inv[t] = -1;
}
__global__ void inverse_table_kernel(const int* __restrict__ mn, int N, int mmax, int nmax, int* __restrict__ inv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) inv[(mn[2 * i] + mmax) * (2 * nmax + 1) + mn[2 * i + 1] + nmax] = i;
}
template <class T>
__global__ __launch_bounds__(64) void toeplitz_sums_kernel(const cx<T>* __restrict__ gE, const int* __restrict__ mn, const int* __restrict__ inv,
                                                           int N, int mmax, int nmax, zc* __restrict__ gbox) {
    const int q = (int)blockIdx.x - 2 * nmax, p = (int)blockIdx.y - 2 * mmax, b = blockIdx.z;
    const int wn = 2 * nmax + 1;
    const cx<T>* g = gE + (long)b * N * N;
    double re = 0.0, im = 0.0;
    for (int j = threadIdx.x; j < N; j += 64) {
        const int m = mn[2 * j] + p, n = mn[2 * j + 1] + q;
        if (m < -mmax || m > mmax || n < -nmax || n > nmax) continue;
        const int i = inv[(m + mmax) * wn + n + nmax];
        if (i < 0) continue;
        const cx<T> v = g[(long)i * N + j];
        re += (double)v.x;
        im += (double)v.y;
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if (threadIdx.x == 0) gbox[((long)b * (4 * mmax + 1) + blockIdx.y) * (4 * nmax + 1) + blockIdx.x] = zc(re, im);
}

// kind / voff of a shape list, checked on the host (one copy and one synchronisation of s, as orders_check)
int shapes_check(hipStream_t s, const int* kind, const int* voff, int S, int npar) {
    std::vector<int> h((size_t)2 * S + 1);
    if (hipMemcpyAsync(h.data(), kind, sizeof(int) * S, hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipMemcpyAsync(h.data() + S, voff, sizeof(int) * (S + 1), hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return TRX_ERR_LAUNCH;
    const int* kd = h.data();
    const int* vo = h.data() + S;
    if (vo[0] < 0 || vo[S] > npar) return TRX_ERR_ARG;
    for (int i = 0; i < S; ++i) {
        const int len = vo[i + 1] - vo[i];
        if (kd[i] == SHAPE_ELLIPSE || kd[i] == SHAPE_RECTANGLE) {
            if (len != 5) return TRX_ERR_ARG;
        } else if (kd[i] == SHAPE_POLYGON) {
            if (len < 6 || (len & 1)) return TRX_ERR_ARG;          // K >= 3 vertices, two coordinates each
        } else {
            return TRX_ERR_ARG;
        }
    }
    return TRX_OK;
}

// an order list for the inverse table: inside the box and without repeats (a repeated harmonic would make the table ambiguous)
int orders_unique_check(hipStream_t s, const int* mn, int N, int mmax, int nmax) {
    std::vector<int> h((size_t)2 * N);
    if (hipMemcpyAsync(h.data(), mn, sizeof(int) * h.size(), hipMemcpyDeviceToHost, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return TRX_ERR_LAUNCH;
    std::vector<char> seen((size_t)(2 * mmax + 1) * (2 * nmax + 1), 0);
    for (int i = 0; i < N; ++i) {
        const int m = h[2 * i], n = h[2 * i + 1];
        if (m < -mmax || m > mmax || n < -nmax || n > nmax) return TRX_ERR_ARG;
        char& f = seen[(size_t)(m + mmax) * (2 * nmax + 1) + n + nmax];
        if (f) return TRX_ERR_ARG;
        f = 1;
    }
    return TRX_OK;
}

inline bool good_area(double a) { return a > 0.0 && std::isfinite(a); }
inline size_t box_bytes(int batch, int mmax, int nmax) { return sizeof(zc) * (size_t)batch * (4 * mmax + 1) * (4 * nmax + 1); }

}  // namespace

// the coefficient box alone (arguments validated by the caller): the one launch of shapes_coef_kernel, shared with trx_convmat_nv_shapes
int shapes_coef_box(hipStream_t s, const int* kind, const int* voff, int S, const double* par, int npar, const void* val, const double* recip,
                    double cell_area, int batch, int mmax, int nmax, cx<double>* box) {
    const int nbox = (4 * mmax + 1) * (4 * nmax + 1);
    const Recip r{recip[0], recip[1], recip[2], recip[3]};
    TRX_LAUNCH(shapes_coef_kernel, dim3(cdiv_i(nbox, SH_BLOCK), batch), dim3(SH_BLOCK), sizeof(double) * (SH_BLOCK + 2), s, kind, voff, S, par,
               npar, (const zc*)val, r, 1.0 / cell_area, mmax, nmax, box);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

int shapes_list_check(hipStream_t s, const int* kind, const int* voff, int S, int npar) { return shapes_check(s, kind, voff, S, npar); }

}  // namespace trx

extern "C" size_t trx_convmat_shapes_ws_bytes(int dtype, int batch, int N, int mmax, int nmax) {
    (void)dtype; (void)N;
    return trx::box_bytes(batch, mmax, nmax);
}

extern "C" int trx_convmat_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* val,
                                  const double* recip, double cell_area, int batch, const int* mn, int N, int mmax, int nmax, void* out,
                                  void* coef, void* ws, size_t ws_bytes, void* stream) {
    using namespace trx;
    if (!kind || !voff || !par || !val || !recip || !mn || !out) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || N <= 0 || mmax < 0 || nmax < 0 || !good_area(cell_area)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (!coef) {                                                 // the box then lives in the workspace
        if (!ws) return TRX_ERR_ARG;
        if (ws_bytes < trx_convmat_shapes_ws_bytes(dtype, batch, N, mmax, nmax)) return TRX_ERR_WORKSPACE;
    }
    hipStream_t s = api_stream(stream);
    int rc = orders_check(s, mn, N, mmax, nmax);
    if (rc) return rc;
    rc = shapes_check(s, kind, voff, S, npar);
    if (rc) return rc;
    zc* box = reinterpret_cast<zc*>(coef ? coef : ws);
    rc = shapes_coef_box(s, kind, voff, S, par, npar, val, recip, cell_area, batch, mmax, nmax, box);
    if (rc) return rc;
    return orders_gather(s, dtype, box, mn, N, mmax, nmax, batch, out);
}

extern "C" int trx_convmat_shapes_backward(const int* kind, const int* voff, int S, const double* par, int npar, const void* val,
                                           const double* recip, double cell_area, int batch, int mmax, int nmax, const void* gbox, double* gpar,
                                           void* gval, void* stream) {
    using namespace trx;
    if (!kind || !voff || !par || !val || !recip || !gbox || !gpar || !gval) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || mmax < 0 || nmax < 0 || !good_area(cell_area)) return TRX_ERR_ARG;
    hipStream_t s = api_stream(stream);
    const int rc = shapes_check(s, kind, voff, S, npar);
    if (rc) return rc;
    const Recip r{recip[0], recip[1], recip[2], recip[3]};
    TRX_LAUNCH(shapes_backward_kernel, dim3(npar + S + 1, batch), dim3(SH_BLOCK), sizeof(zc) * SH_BLOCK, s, kind, voff, S, par, npar,
               (const zc*)val, r, 1.0 / cell_area, mmax, nmax, (const zc*)gbox, gpar, (zc*)gval);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" size_t trx_toeplitz_sums_ws_bytes(int dtype, int batch, int N, int mmax, int nmax) {
    (void)dtype; (void)batch; (void)N;
    return sizeof(int) * (size_t)(2 * mmax + 1) * (2 * nmax + 1);
}

extern "C" int trx_toeplitz_sums(int dtype, const void* gE, int batch, const int* mn, int N, int mmax, int nmax, void* gbox, void* ws,
                                 size_t ws_bytes, void* stream) {
    using namespace trx;
    if (!gE || !mn || !gbox || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || batch > 65535 || N <= 0 || mmax < 0 || nmax < 0 || 4 * mmax + 1 > 65535) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_toeplitz_sums_ws_bytes(dtype, batch, N, mmax, nmax)) return TRX_ERR_WORKSPACE;
    hipStream_t s = api_stream(stream);
    const int rc = orders_unique_check(s, mn, N, mmax, nmax);
    if (rc) return rc;
    int* inv = reinterpret_cast<int*>(ws);
    const int nt = (2 * mmax + 1) * (2 * nmax + 1);
    TRX_LAUNCH(inverse_fill_kernel, dim3(cdiv_i(nt, 256)), dim3(256), 0, s, inv, nt);
    TRX_LAUNCH(inverse_table_kernel, dim3(cdiv_i(N, 256)), dim3(256), 0, s, mn, N, mmax, nmax, inv);
    const dim3 g(4 * nmax + 1, 4 * mmax + 1, batch);
    if (dtype == TRX_C64) TRX_LAUNCH((toeplitz_sums_kernel<float>), g, dim3(64), 0, s, (const cx<float>*)gE, mn, (const int*)inv, N, mmax, nmax, (zc*)gbox);
    else                  TRX_LAUNCH((toeplitz_sums_kernel<double>), g, dim3(64), 0, s, (const cx<double>*)gE, mn, (const int*)inv, N, mmax, nmax, (zc*)gbox);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
