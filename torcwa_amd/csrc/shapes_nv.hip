// Normal-vector Fourier factorisation of vector-shape layers: the normal field of a shape list (trx_shape_normal_field) and the tensor
// Exx, Exy, Eyy built from closed-form [eps], [1/eps] and the sampled products of that field (trx_convmat_nv_shapes).
//
// The field is a blend, not a nearest-boundary choice.  Sample r = (i / n1) a1 + (j / n2) a2 (the DFT's positions).  Every primitive -- an
// ellipse, or one edge of a polygon (a rectangle is its 4-gon) -- contributes in each of the nine images r' = r - p a1 - q a2, p, q in -1..1:
//   ellipse (Rx, Ry, c, th):  (u, w) = R(-th)(r' - c),  f = hypot(u / Rx, w / Ry),  delta = |f - 1| min(Rx, Ry),
//                             g = R(th)(u / Rx^2, w / Ry^2),  n = g / |g|  (nothing when |g| = 0)
//   edge a -> b, e = b - a:   tau = (r' - a).e / |e|^2;  0 < tau < 1: n = (e_y, -e_x) / |e|, delta = |(r' - a).n|;
//                             else v = a (tau <= 0) or b: delta = |r' - v|, n = (r' - v) / delta  (nothing when delta = 0)
//   J += n n^T / (delta^2 + eta^2)^2,  eta^2 = 1e-12 cell_area
// and the direction is trx_normal_field's: d = Jxx - Jyy, o = 2 Jxy, r = hypot(d, o); where r > 1e-3 (Jxx + Jyy) the products are
// (1 + d/r)/2, o/(2r), (1 - d/r)/2, elsewhere 0 (Laurent's rule locally: a disk's centre, mirror lines far from any boundary).
// One thread per sample, lanes along n2; the sum runs shapes ascending, images p outer and q inner, edges ascending: two calls give the same
// bits.  9 (ellipses + edges) short fp64 evaluations per sample (a divide or two and a square root each): latency- and divide-bound; the
// output is 24 B per sample.  The eps jump never touches a pixel: the three products are smooth, so their DFT is a quadrature.
#include <cmath>

#include "common.hpp"

namespace trx {
namespace {

typedef cx<double> zc;

enum { SHAPE_ELLIPSE = 0, SHAPE_RECTANGLE = 1, SHAPE_POLYGON = 2 };
constexpr int NVS_BLOCK = 256;           // threads per workgroup and doubles of a parameter row per staging pass (128 vertices)
constexpr double NVS_TAU = 1e-3;         // coherence floor, NV_TAU of convmat_nv.hip
constexpr double NVS_ETA2 = 1e-12;       // eta^2 / cell_area
constexpr double NVS_TIE = 16 * 2.220446049250313e-16;      // a sample counts as on a branch line of an edge within 16 eps of its numerator's size

struct Cell { double a1x, a1y, a2x, a2y; };
struct Tensor { double xx, xy, yy; };

__device__ __forceinline__ void add_normal(Tensor& J, double nx, double ny, double delta, double eta2) {
    const double t = delta * delta + eta2;
    const double w = 1.0 / (t * t);
    J.xx += w * (nx * nx);
    J.xy += w * (nx * ny);
    J.yy += w * (ny * ny);
}

// q: Rx, Ry, Cx, Cy and (s, c) = sincos(theta)
__device__ __forceinline__ void ellipse_normal(Tensor& J, const double* q, double s, double c, double x, double y, double eta2) {
    const double dx = x - q[2], dy = y - q[3];
    const double u = c * dx + s * dy, w = -s * dx + c * dy;
    const double f = hypot(u / q[0], w / q[1]);
    const double delta = fabs(f - 1.0) * fmin(q[0], q[1]);
    const double gu = u / (q[0] * q[0]), gw = w / (q[1] * q[1]);
    const double gx = c * gu - s * gw, gy = s * gu + c * gw;
    const double g = hypot(gx, gy);
    if (g == 0.0) return;
    add_normal(J, gx / g, gy / g, delta, eta2);
}

__device__ __forceinline__ void edge_normal(Tensor& J, double ax, double ay, double bx, double by, double x, double y, double eta2) {
    const double ex = bx - ax, ey = by - ay;
    const double dx = x - ax, dy = y - ay;
    const double l2 = ex * ex + ey * ey;
    const double tau = (dx * ex + dy * ey) / l2;
    if (tau > 0.0 && tau < 1.0) {
        const double l = sqrt(l2);
        const double nx = ey / l, ny = -ex / l;
        add_normal(J, nx, ny, fabs(dx * nx + dy * ny), eta2);
    } else {
        const bool first = tau <= 0.0;
        const double vx = x - (first ? ax : bx), vy = y - (first ? ay : by);
        const double delta = hypot(vx, vy);
        if (delta == 0.0) return;
        add_normal(J, vx / delta, vy / delta, delta, eta2);
    }
}

// Parameters are staged in LDS in passes of NVS_BLOCK doubles (plus the vertex that closes a pass's last edge), as in shapes_coef_kernel: an
// ellipse or a rectangle takes one pass of 5, a polygon of up to 128 vertices one pass for all nine images, a longer one its passes inside the
// image loop (so that edges stay the innermost index of the sum).  kind / voff are wave-uniform reads.
// ADJ (trx_shape_normal_field_backward, first pass): the same sum, then the adjoint of the direction step in place of the products -- gnn
// [B,3,n1,n2] in, G = (g_d, g_o) [B,2,n1,n2] out (nn is not written), dL = g_d d(Jxx - Jyy) + g_o d(2 Jxy).
template <bool ADJ>
__global__ __launch_bounds__(NVS_BLOCK) void shape_normal_field_kernel(const int* __restrict__ kind, const int* __restrict__ voff, int S,
                                                                       const double* __restrict__ par, int npar, Cell a, double eta2, int n1,
                                                                       int n2, double* __restrict__ nn, const double* __restrict__ gnn,
                                                                       double* __restrict__ G) {
    TRX_DYN_SMEM(smem);
    double* stage = reinterpret_cast<double*>(smem);             // [NVS_BLOCK + 2]
    const int b = blockIdx.y;
    const long per = (long)n1 * n2;
    const long e = (long)blockIdx.x * NVS_BLOCK + threadIdx.x;
    const bool active = e < per;
    const int i = active ? (int)(e / n2) : 0, j = active ? (int)(e - (long)i * n2) : 0;
    const double fu = (double)i / (double)n1, fv = (double)j / (double)n2;
    const double x0 = fu * a.a1x + fv * a.a2x, y0 = fu * a.a1y + fv * a.a2y;
    const double* pr = par + (long)b * npar;
    Tensor J{0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
        const int k = kind[s], o = voff[s], len = voff[s + 1] - o;
        if (k != SHAPE_POLYGON) {
            __syncthreads();                                     // the previous shape's parameters have been read
            if (threadIdx.x < 5) stage[threadIdx.x] = pr[o + threadIdx.x];
            __syncthreads();
            double sn, cs;
            sincos(stage[4], &sn, &cs);
            double vx[5], vy[5];                                 // the rectangle's 4-gon, closed
            if (k == SHAPE_RECTANGLE) {
                const double hx = 0.5 * stage[0], hy = 0.5 * stage[1];
                const double ux[4] = {-hx, hx, hx, -hx}, uy[4] = {-hy, -hy, hy, hy};
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    vx[v] = stage[2] + cs * ux[v] - sn * uy[v];
                    vy[v] = stage[3] + sn * ux[v] + cs * uy[v];
                }
                vx[4] = vx[0];
                vy[4] = vy[0];
            }
            for (int p = -1; p <= 1; ++p)
                for (int q = -1; q <= 1; ++q) {
                    const double x = x0 - p * a.a1x - q * a.a2x, y = y0 - p * a.a1y - q * a.a2y;
                    if (k == SHAPE_ELLIPSE) {
                        ellipse_normal(J, stage, sn, cs, x, y, eta2);
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v) edge_normal(J, vx[v], vy[v], vx[v + 1], vy[v + 1], x, y, eta2);
                    }
                }
        } else {
            const bool one_pass = len <= NVS_BLOCK;
            for (int p = -1; p <= 1; ++p)
                for (int q = -1; q <= 1; ++q) {
                    const double x = x0 - p * a.a1x - q * a.a2x, y = y0 - p * a.a1y - q * a.a2y;
                    for (int c0 = 0; c0 < len; c0 += NVS_BLOCK) {
                        const int cnt = len - c0 < NVS_BLOCK ? len - c0 : NVS_BLOCK;
                        if (!one_pass || (p == -1 && q == -1)) {     // (uniform over the workgroup)
                            __syncthreads();
                            for (int t = threadIdx.x; t < cnt + 2; t += NVS_BLOCK) {
                                int idx = c0 + t;
                                if (idx >= len) idx -= len;      // the last edge closes on vertex 0
                                stage[t] = pr[o + idx];
                            }
                            __syncthreads();
                        }
                        for (int v = 0; v < cnt; v += 2) edge_normal(J, stage[v], stage[v + 1], stage[v + 2], stage[v + 3], x, y, eta2);
                    }
                }
        }
    }
    if (!active) return;
    const double d = J.xx - J.yy, od = 2.0 * J.xy;
    const double r = hypot(d, od);
    if (ADJ) {
        // with (c, sn) = (d, o) / r the products are (1 + c) / 2, sn / 2, (1 - c) / 2 and dc = (sn / r)(sn dd - c do), dsn = (c / r)(c do - sn dd):
        // dL = k (sn dd - c do), k = (a sn - beta c) / r -- unit vector and one 1 / r, nothing of size J^2 is formed.  Zero products: zero adjoint.
        double gd = 0.0, go = 0.0;
        if (r > NVS_TAU * (J.xx + J.yy)) {
            const double* gi = gnn + (long)b * 3 * per + e;
            const double c = d / r, sn = od / r;
            const double k = (0.5 * (gi[0] - gi[2 * per]) * sn - 0.5 * gi[per] * c) / r;
            gd = sn * k;
            go = -c * k;
        }
        double* out = G + (long)b * 2 * per + e;
        out[0] = gd;
        out[per] = go;
        return;
    }
    double pxx = 0.0, pxy = 0.0, pyy = 0.0;                      // fallback: N N^T = 0 (Laurent's rule where no direction is resolvable)
    if (r > NVS_TAU * (J.xx + J.yy)) {
        const double c = d / r;
        pxx = 0.5 * (1.0 + c);
        pxy = 0.5 * (od / r);
        pyy = 0.5 * (1.0 - c);
    }
    double* out = nn + (long)b * 3 * per + e;
    out[0] = pxx;
    out[per] = pxy;
    out[2 * per] = pyy;
}

// ---- adjoint of the field: the parameter pass ---------------------------------------------------------------------------------------------------
// One term w n n^T of J, w = 1 / (delta^2 + eta^2)^2, under dL = G : dJ with G = [[g_d, g_o], [g_o, -g_d]] (trace-free):
//   dL = dw (n^T G n) + 2 w (n^T G dn) = A ddelta + 2 w P (t . dn),   Q = n^T G n,  P = t^T G n,  t = (-n_y, n_x),  A = -4 delta w Q / (delta^2 + eta^2)
// G is orthogonal to J, so where one primitive dominates J its own Q is a small difference: it is formed from the unit normal (n^T G n), never
// from J, and the direction part from t^T G n -- the 1 / delta^5 terms of that primitive then cancel to rounding of a quantity of the size of
// the result, not of its parts.  The derivative of |.| at 0 is 0 (sign 0), min(Rx, Ry) goes to Rx when Rx <= Ry, a vertex branch to its vertex.
struct Weight { double w, A, P; };

__device__ __forceinline__ Weight term_adjoint(double nx, double ny, double delta, double eta2, double gd, double go) {
    const double t = delta * delta + eta2;
    const double w = 1.0 / (t * t);
    const double c2 = nx * nx - ny * ny, s2 = 2.0 * (nx * ny);
    return Weight{w, -4.0 * delta * (w / t) * (gd * c2 + go * s2), go * c2 - gd * s2};
}

__device__ __forceinline__ double sign_of(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// gp[5] += dL / d(Rx, Ry, Cx, Cy, theta) of one ellipse image
__device__ __forceinline__ void ellipse_normal_adjoint(double* gp, const double* q, double s, double c, double x, double y, double eta2, double gd,
                                                       double go) {
    const double dx = x - q[2], dy = y - q[3];
    const double u = c * dx + s * dy, w = -s * dx + c * dy;
    const double U = u / q[0], W = w / q[1];
    const double f = hypot(U, W);
    const double m = fmin(q[0], q[1]);
    const double delta = fabs(f - 1.0) * m;
    const double gu = u / (q[0] * q[0]), gw = w / (q[1] * q[1]);
    const double gx = c * gu - s * gw, gy = s * gu + c * gw;
    const double g = hypot(gx, gy);
    if (g == 0.0) return;
    const double nx = gx / g, ny = gy / g;
    const Weight k = term_adjoint(nx, ny, delta, eta2, gd, go);
    const double B = 2.0 * k.w * k.P / g;                        // on t . dg: dn = t (t . dg) / |g|
    const double al = k.A * sign_of(f - 1.0) * m / f;            // on U dU + W dW (f > 0 where g != 0)
    const double am = k.A * fabs(f - 1.0);                       // on d min(Rx, Ry)
    const double tbx = s * nx - c * ny, tby = c * nx + s * ny;   // t in the ellipse's frame: t . dg = tb . d(gu, gw) + |g| dtheta
    const double cu = al * U / q[0] + B * tbx / (q[0] * q[0]);   // on du
    const double cw = al * W / q[1] + B * tby / (q[1] * q[1]);   // on dw
    const bool rx = q[0] <= q[1];
    gp[0] += (rx ? am : 0.0) - al * U * U / q[0] - 2.0 * B * tbx * gu / q[0];
    gp[1] += (rx ? 0.0 : am) - al * W * W / q[1] - 2.0 * B * tby * gw / q[1];
    gp[2] += s * cw - c * cu;                                    // du = -c dCx - s dCy + w dtheta,  dw = s dCx - c dCy - u dtheta
    gp[3] += -s * cu - c * cw;
    // cu w - cw u + B |g| with |g| = tby gu - tbx gw, collected: exactly 0 for Rx = Ry, whose field does not depend on theta
    gp[4] += (1.0 / (q[0] * q[0]) - 1.0 / (q[1] * q[1])) * (al * u * w + B * (tby * u + tbx * w));
}

// ga[2], gb[2] += dL / d(a, b) of one edge image
__device__ __forceinline__ void edge_normal_adjoint(double* ga, double* gb, double ax, double ay, double bx, double by, double x, double y,
                                                    double eta2, double gd, double go) {
    const double ex = bx - ax, ey = by - ay;
    const double dx = x - ax, dy = y - ay;
    const double l2 = ex * ex + ey * ey;
    const double tau = (dx * ex + dy * ey) / l2;
    // A sample on a branch line (tau = 0 or 1: structures with round coordinates on a regular grid do hit them) sits on a C0 kink of the
    // field; it takes the mean of the two pieces' derivatives, the symmetric derivative, which is what a central difference sees.  "On the
    // line" is to within the rounding of the numerator, NVS_TIE of the size of its two products (a contracted multiply-add moves an exact
    // 0 or |e|^2 by an ulp): some 1e-14 of the cell in distance.
    const double num = dx * ex + dy * ey, mag = fabs(dx * ex) + fabs(dy * ey);
    const bool tie0 = fabs(num) <= NVS_TIE * mag, tie1 = fabs(num - l2) <= NVS_TIE * (mag + l2);
    const bool tie = tie0 || tie1, inner = !tie && tau > 0.0 && tau < 1.0;
    const double share = tie ? 0.5 : 1.0;
    const bool first = tie ? tie0 : tau <= 0.0;
    const double vx = x - (first ? ax : bx), vy = y - (first ? ay : by);
    const double dv = hypot(vx, vy);
    if (!inner && dv == 0.0) return;                             // a vertex hit: no term in the forward
    if (inner || tie) {
        const double l = sqrt(l2);
        const double nx = ey / l, ny = -ex / l;
        const double sd = dx * nx + dy * ny;
        const Weight k = term_adjoint(nx, ny, fabs(sd), eta2, share * gd, share * go);
        // ddelta = -sign n . ((1 - tau) da + tau db),  t . dn = -n . (db - da) / l
        const double As = k.A * sign_of(sd), B = 2.0 * k.w * k.P / l;
        const double ca = B - As * (1.0 - tau), cb = -B - As * tau;
        ga[0] += ca * nx;
        ga[1] += ca * ny;
        gb[0] += cb * nx;
        gb[1] += cb * ny;
    }
    if (!inner) {
        const double nx = vx / dv, ny = vy / dv;
        const Weight k = term_adjoint(nx, ny, dv, eta2, share * gd, share * go);
        const double B = 2.0 * k.w * k.P / dv;                   // ddelta = -n . dv,  dn = -t (t . dv) / delta
        double* gv = first ? ga : gb;
        gv[0] += B * ny - k.A * nx;
        gv[1] += -B * nx - k.A * ny;
    }
}

constexpr int NVS_PART = 5;              // partials of one primitive: an ellipse's or rectangle's five parameters, or (a_x, a_y, b_x, b_y) of an edge
constexpr int NVS_MAX_CHUNKS = 256;

struct Chunks { int n; long len; };      // n chunks of len samples (a multiple of NVS_BLOCK) cover n1 n2
inline Chunks chunks_of(long per) {
    const long blocks = (per + NVS_BLOCK - 1) / NVS_BLOCK;
    const int n = (int)(blocks < NVS_MAX_CHUNKS ? blocks : NVS_MAX_CHUNKS);
    return Chunks{n, (blocks + n - 1) / n * NVS_BLOCK};
}

// Grid (chunk, w, b): w is a slot of the parameter row, and the workgroup is live where a primitive starts there -- the first slot of an
// ellipse or a rectangle, the x slot of a polygon vertex (the edge from that vertex to the next).  It runs over its chunk of samples x nine
// images with the primitive's partials in registers (a rectangle: its four vertices, then the chain rule to Wx, Wy, C, theta per thread), and
// reduces them by wave_sum and a fixed sum over the four waves into part[b, w, chunk, 0..4].  Samples with G = 0 (zero products) are skipped.
__global__ __launch_bounds__(NVS_BLOCK) void shape_normal_field_param_kernel(const int* __restrict__ kind, const int* __restrict__ voff, int S,
                                                                             const double* __restrict__ par, int npar, Cell a, double eta2, int n1,
                                                                             int n2, long chunk_len, const double* __restrict__ G,
                                                                             double* __restrict__ part) {
    TRX_DYN_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);               // [NVS_BLOCK / 64][NVS_PART]
    const int chunk = blockIdx.x, w = blockIdx.y, b = blockIdx.z;
    int s = -1;
    for (int t = 0; t < S; ++t)
        if (w >= voff[t] && w < voff[t + 1]) s = t;
    if (s < 0) return;                                           // (uniform over the workgroup, as every return before the reduction)
    const int k = kind[s], o = voff[s], len = voff[s + 1] - o, j = w - o;
    if (k == SHAPE_POLYGON ? (j & 1) : j != 0) return;
    const double* q = par + (long)b * npar + o;
    const long per = (long)n1 * n2;
    const double* Gb = G + (long)b * 2 * per;
    double sn = 0.0, cs = 1.0;
    double vx[5], vy[5];                                         // the rectangle's 4-gon, closed, or one polygon edge in [0], [1]
    if (k != SHAPE_POLYGON) sincos(q[4], &sn, &cs);
    if (k == SHAPE_RECTANGLE) {
        const double hx = 0.5 * q[0], hy = 0.5 * q[1];
        const double ux[4] = {-hx, hx, hx, -hx}, uy[4] = {-hy, -hy, hy, hy};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            vx[v] = q[2] + cs * ux[v] - sn * uy[v];
            vy[v] = q[3] + sn * ux[v] + cs * uy[v];
        }
        vx[4] = vx[0];
        vy[4] = vy[0];
    } else if (k == SHAPE_POLYGON) {
        const int j1 = j + 2 < len ? j + 2 : 0;                  // the last edge closes on vertex 0
        vx[0] = q[j]; vy[0] = q[j + 1]; vx[1] = q[j1]; vy[1] = q[j1 + 1];
    }
    double gp[NVS_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double gv[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    const long e0 = (long)chunk * chunk_len;
    const long e1 = e0 + chunk_len < per ? e0 + chunk_len : per;
    for (long e = e0 + threadIdx.x; e < e1; e += NVS_BLOCK) {
        const double gd = Gb[e], go = Gb[per + e];
        if (gd == 0.0 && go == 0.0) continue;
        const int i = (int)(e / n2), jj = (int)(e - (long)i * n2);
        const double fu = (double)i / (double)n1, fv = (double)jj / (double)n2;
        const double x0 = fu * a.a1x + fv * a.a2x, y0 = fu * a.a1y + fv * a.a2y;
        for (int p = -1; p <= 1; ++p)
            for (int r = -1; r <= 1; ++r) {
                const double x = x0 - p * a.a1x - r * a.a2x, y = y0 - p * a.a1y - r * a.a2y;
                if (k == SHAPE_ELLIPSE) {
                    ellipse_normal_adjoint(gp, q, sn, cs, x, y, eta2, gd, go);
                } else if (k == SHAPE_POLYGON) {
                    edge_normal_adjoint(gp, gp + 2, vx[0], vy[0], vx[1], vy[1], x, y, eta2, gd, go);
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) edge_normal_adjoint(gv[v], gv[(v + 1) & 3], vx[v], vy[v], vx[v + 1], vy[v + 1], x, y, eta2, gd, go);
                }
            }
    }
    if (k == SHAPE_RECTANGLE) {                                  // v = C + R(theta)(sx Wx / 2, sy Wy / 2), (sx, sy) = (-,-), (+,-), (+,+), (-,+)
        const double sx[4] = {-0.5, 0.5, 0.5, -0.5}, sy[4] = {-0.5, -0.5, 0.5, 0.5};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            gp[0] += sx[v] * (cs * gv[v][0] + sn * gv[v][1]);
            gp[1] += sy[v] * (cs * gv[v][1] - sn * gv[v][0]);
            gp[2] += gv[v][0];
            gp[3] += gv[v][1];
            gp[4] += gv[v][1] * (vx[v] - q[2]) - gv[v][0] * (vy[v] - q[3]);
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < NVS_PART; ++t) {
        const double v = wave_sum(gp[t]);
        if ((threadIdx.x & 63) == 0) red[wave * NVS_PART + t] = v;
    }
    __syncthreads();
    if (threadIdx.x < NVS_PART) {
        double v = red[threadIdx.x];
        for (int t = 1; t < NVS_BLOCK / 64; ++t) v += red[t * NVS_PART + threadIdx.x];
        part[(((long)b * npar + w) * gridDim.x + chunk) * NVS_PART + threadIdx.x] = v;
    }
}

// gpar[b, i]: the chunks of the primitive that owns slot i in ascending order; a polygon vertex sums the edge that ends there (its b part),
// then the edge that starts there (its a part).  0 for a slot no shape owns.  One thread per (b, i).
__global__ __launch_bounds__(NVS_BLOCK) void shape_normal_field_sum_kernel(const int* __restrict__ kind, const int* __restrict__ voff, int S, int npar,
                                                                           int batch, int nch, const double* __restrict__ part,
                                                                           double* __restrict__ gpar) {
    const long t = (long)blockIdx.x * NVS_BLOCK + threadIdx.x;
    if (t >= (long)batch * npar) return;
    const int b = (int)(t / npar), i = (int)(t - (long)b * npar);
    int s = -1;
    for (int u = 0; u < S; ++u)
        if (i >= voff[u] && i < voff[u + 1]) s = u;
    double acc = 0.0;
    if (s >= 0) {
        const int o = voff[s], len = voff[s + 1] - o, j = i - o;
        const double* pb = part + (long)b * npar * nch * NVS_PART;
        if (kind[s] != SHAPE_POLYGON) {
            for (int c = 0; c < nch; ++c) acc += pb[((long)o * nch + c) * NVS_PART + j];
        } else {
            const int xy = j & 1, v = j - xy, pv = v > 0 ? v - 2 : len - 2;      // the x slots of this vertex and of the one before it
            for (int c = 0; c < nch; ++c) acc += pb[((long)(o + pv) * nch + c) * NVS_PART + 2 + xy];
            for (int c = 0; c < nch; ++c) acc += pb[((long)(o + v) * nch + c) * NVS_PART + xy];
        }
    }
    gpar[t] = acc;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN and inf

// info[b] = 1 where a value or a reciprocal value is not finite, or a background entry is zero: a medium whose eps is zero or non-finite
__global__ __launch_bounds__(256) void nvs_values_kernel(const zc* __restrict__ val, const zc* __restrict__ rval, int S, int batch,
                                                         int* __restrict__ info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    bool bad = false;
    for (int s = 0; s <= S; ++s) {
        const zc v = val[(long)b * (S + 1) + s], r = rval[(long)b * (S + 1) + s];
        bad = bad || !(finite_d(v.x) && finite_d(v.y) && finite_d(r.x) && finite_d(r.y));
        if (s == 0) bad = bad || (v.x == 0.0 && v.y == 0.0) || (r.x == 0.0 && r.y == 0.0);
    }
    info[b] = bad ? 1 : 0;
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

bool cell_of(const double* lattice, Cell* a, double* area) {
    if (!lattice) return false;
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(lattice[k])) return false;
    *a = Cell{lattice[0], lattice[1], lattice[2], lattice[3]};
    *area = std::fabs(lattice[0] * lattice[3] - lattice[1] * lattice[2]);
    return *area > 0.0 && std::isfinite(*area);
}

int field_launch(hipStream_t s, const int* kind, const int* voff, int S, const double* par, int npar, const Cell& a, double area, int batch,
                 int n1, int n2, double* nn) {
    TRX_LAUNCH(shape_normal_field_kernel<false>, dim3(cdiv_i((long)n1 * n2, NVS_BLOCK), batch), dim3(NVS_BLOCK), sizeof(double) * (NVS_BLOCK + 2),
               s, kind, voff, S, par, npar, a, NVS_ETA2 * area, n1, n2, nn, (const double*)nullptr, (double*)nullptr);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

struct NvsBackLayout { size_t G, part, total; };     // byte offsets into the workspace of trx_shape_normal_field_backward

NvsBackLayout nvs_back_layout(int npar, int batch, int n1, int n2) {
    NvsBackLayout L;
    const size_t per = (size_t)n1 * n2;
    L.G = 0;
    L.part = al256(sizeof(double) * 2 * (size_t)batch * per);
    L.total = L.part + al256(sizeof(double) * NVS_PART * (size_t)batch * npar * chunks_of((long)per).n);
    return L;
}

struct NvsLayout {                  // byte offsets into the workspace of trx_convmat_nv_shapes
    size_t box, nn, cws, R, C, inv, piv, iinfo, tmp, total;
    size_t inv_bytes;
};

NvsLayout nvs_layout(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax) {
    NvsLayout L;
    const size_t per = (size_t)n1 * n2, NN = (size_t)N * N, B = (size_t)batch;
    size_t o = 0;
    L.box = o;  o += al256(sizeof(zc) * B * (4 * mmax + 1) * (4 * nmax + 1));     // the box of [eps], then of [1/eps]
    L.nn = o;   o += al256(sizeof(double) * 3 * B * per);                          // the field, when the caller supplies none
    L.cws = o;  o += al256(trx_convmat_orders_ws_bytes(TRX_C128, 3 * batch, n1, n2, N, mmax, nmax));
    L.R = o;    o += al256(sizeof(zc) * B * NN);                                   // [1/eps], then its inverse, then D
    L.C = o;    o += al256(sizeof(zc) * 3 * B * NN);                               // [Nx^2], [Nx Ny], [Ny^2]
    L.inv_bytes = trx_inverse_ws_bytes(TRX_C128, N, batch);
    L.inv = o;  o += al256(L.inv_bytes);
    L.piv = o;  o += al256(sizeof(int) * B * N);
    L.iinfo = o; o += al256(sizeof(int) * B);
    L.tmp = o;  o += dtype == TRX_C64 ? al256(sizeof(zc) * 3 * B * NN) : 0;        // complex128 results of a complex64 call
    L.total = o;
    return L;
}

}  // namespace
}  // namespace trx

using namespace trx;

extern "C" int trx_shape_normal_field(const int* kind, const int* voff, int S, const double* par, int npar, const double* lattice, int batch, int n1,
                                      int n2, double* nn, void* stream) {
    Cell a;
    double area;
    if (!kind || !voff || !par || !nn || !cell_of(lattice, &a, &area)) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || n1 <= 0 || n2 <= 0) return TRX_ERR_ARG;
    if (n1 > 2048 || n2 > 2048) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = api_stream(stream);
    if (int rc = shapes_list_check(s, kind, voff, S, npar)) return rc;
    return field_launch(s, kind, voff, S, par, npar, a, area, batch, n1, n2, nn);
}

extern "C" size_t trx_shape_normal_field_backward_ws_bytes(int S, int npar, int batch, int n1, int n2) {
    if (S <= 0 || npar <= 0 || batch <= 0 || n1 <= 0 || n2 <= 0) return 0;
    return nvs_back_layout(npar, batch, n1, n2).total;
}

extern "C" int trx_shape_normal_field_backward(const int* kind, const int* voff, int S, const double* par, int npar, const double* lattice, int batch,
                                               int n1, int n2, const double* gnn, double* gpar, void* ws, size_t ws_bytes, void* stream) {
    Cell a;
    double area;
    if (!kind || !voff || !par || !gnn || !gpar || !ws || !cell_of(lattice, &a, &area)) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || batch > 65535 || n1 <= 0 || n2 <= 0) return TRX_ERR_ARG;
    if (n1 > 2048 || n2 > 2048 || npar > 65535) return TRX_ERR_UNSUPPORTED;      // npar is a grid dimension of the parameter pass
    if (ws_bytes < trx_shape_normal_field_backward_ws_bytes(S, npar, batch, n1, n2)) return TRX_ERR_WORKSPACE;
    hipStream_t s = api_stream(stream);
    if (int rc = shapes_list_check(s, kind, voff, S, npar)) return rc;
    const NvsBackLayout L = nvs_back_layout(npar, batch, n1, n2);
    const long per = (long)n1 * n2;
    const Chunks ch = chunks_of(per);
    const double eta2 = NVS_ETA2 * area;
    double* G = (double*)((char*)ws + L.G);
    double* part = (double*)((char*)ws + L.part);
    TRX_LAUNCH(shape_normal_field_kernel<true>, dim3(cdiv_i(per, NVS_BLOCK), batch), dim3(NVS_BLOCK), sizeof(double) * (NVS_BLOCK + 2), s, kind,
               voff, S, par, npar, a, eta2, n1, n2, (double*)nullptr, gnn, G);
    TRX_LAUNCH(shape_normal_field_param_kernel, dim3(ch.n, npar, batch), dim3(NVS_BLOCK), sizeof(double) * NVS_PART * (NVS_BLOCK / 64), s, kind,
               voff, S, par, npar, a, eta2, n1, n2, ch.len, (const double*)G, part);
    TRX_LAUNCH(shape_normal_field_sum_kernel, dim3(cdiv_i((long)batch * npar, NVS_BLOCK)), dim3(NVS_BLOCK), 0, s, kind, voff, S, npar, batch, ch.n,
               (const double*)part, gpar);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" size_t trx_convmat_nv_shapes_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax) {
    if (batch <= 0 || N <= 0 || mmax < 0 || nmax < 0 || n1 <= 0 || n2 <= 0) return 0;
    return nvs_layout(dtype, batch, n1, n2, N, mmax, nmax).total;
}

extern "C" int trx_convmat_nv_shapes(int dtype, const int* kind, const int* voff, int S, const double* par, int npar, const void* val,
                                     const void* rval, const double* recip, double cell_area, const double* lattice, int batch, int n1, int n2,
                                     const int* mn, int N, int mmax, int nmax, const double* nn, void* Exx, void* Exy, void* Eyy, int* info,
                                     void* ws, size_t ws_bytes, void* stream) {
    Cell a{1.0, 0.0, 0.0, 1.0};
    double area = 1.0;
    if (!kind || !voff || !par || !val || !rval || !recip || !mn || !Exx || !Exy || !Eyy || !info || !ws) return TRX_ERR_ARG;
    if (S <= 0 || npar <= 0 || batch <= 0 || 3 * (long)batch > 65535 || N <= 0 || mmax < 0 || nmax < 0) return TRX_ERR_ARG;
    if (!(cell_area > 0.0) || !std::isfinite(cell_area) || n1 <= 2 * mmax || n2 <= 2 * nmax) return TRX_ERR_ARG;
    if (!nn && !cell_of(lattice, &a, &area)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_convmat_nv_shapes_ws_bytes(dtype, batch, n1, n2, N, mmax, nmax)) return TRX_ERR_WORKSPACE;
    if (n1 > 2048 || n2 > 2048) return TRX_ERR_UNSUPPORTED;      // also the DFT rows of trx_convmat_orders (32 B per cell of a line in 64 KiB)
    hipStream_t s = api_stream(stream);
    int rc = orders_check(s, mn, N, mmax, nmax);
    if (rc) return rc;
    if ((rc = shapes_list_check(s, kind, voff, S, npar))) return rc;
    const NvsLayout L = nvs_layout(dtype, batch, n1, n2, N, mmax, nmax);
    char* w = (char*)ws;
    const long bNN = (long)batch * N * N;
    zc* box = (zc*)(w + L.box);
    zc* R = (zc*)(w + L.R);
    zc* C = (zc*)(w + L.C);
    zc *oxx, *oxy, *oyy;
    if (dtype == TRX_C128) {
        oxx = (zc*)Exx; oxy = (zc*)Exy; oyy = (zc*)Eyy;
    } else {
        oxx = (zc*)(w + L.tmp); oxy = oxx + bNN; oyy = oxy + bNN;
    }
    TRX_LAUNCH(nvs_values_kernel, dim3(cdiv_i(batch, 256)), dim3(256), 0, s, (const zc*)val, (const zc*)rval, S, batch, info);
    TRX_CHECK_LAUNCH();
    if (!nn) {
        double* nw = (double*)(w + L.nn);
        if ((rc = field_launch(s, kind, voff, S, par, npar, a, area, batch, n1, n2, nw))) return rc;
        nn = nw;
    }
    // [eps] -> oxx and [1/eps] -> R from the same coefficient kernel and gather (complex128), [N_c] -> C[b*3 + c] from the pruned DFT
    if ((rc = shapes_coef_box(s, kind, voff, S, par, npar, val, recip, cell_area, batch, mmax, nmax, box))) return rc;
    if ((rc = orders_gather(s, TRX_C128, box, mn, N, mmax, nmax, batch, oxx))) return rc;
    if ((rc = shapes_coef_box(s, kind, voff, S, par, npar, rval, recip, cell_area, batch, mmax, nmax, box))) return rc;
    if ((rc = orders_gather(s, TRX_C128, box, mn, N, mmax, nmax, batch, R))) return rc;
    if ((rc = convmat_orders_checked(s, TRX_C128, 0, nn, 3 * batch, n1, n2, mn, N, mmax, nmax, C, w + L.cws))) return rc;
    return nv_tensor_tail(s, dtype, batch, N, oxx, oxy, oyy, Exx, Exy, Eyy, info, R, C, w + L.inv, L.inv_bytes, (int*)(w + L.piv),
                          (int*)(w + L.iinfo));
}
