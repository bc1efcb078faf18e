// Fourier factorisation, normal-vector method (Schuster et al., JOSA A 24, 2880 (2007); Goetz et al., Opt. Express 16, 17295 (2008)):
// permittivity grid -> the in-plane 2 x 2 tensor of convolution matrices of a patterned layer with curved or oblique boundaries.
//
//   N(x, y): smooth in-plane unit field normal to the material interfaces (only N N^T enters, so the sign of N does not matter);
//   D = [eps] - [1/eps]^-1;   Exx = [eps] - {D, [Nx Nx]},   Exy = Eyx = -{D, [Nx Ny]},   Eyy = [eps] - {D, [Ny Ny]}
//   ([f]: Laurent's Toeplitz convolution matrix of a grid, trx_convmat; {D, C} = (D C + C D) / 2, the symmetrised product: D and C are
//   Hermitian for a lossless grid, and so is then the tensor -- the plain product D C is not, and breaks energy conservation at finite order).
//
// The field (trx_normal_field) comes from the grid itself:
//   1. structure tensor J = Re(grad eps grad eps^H) from periodic central differences (grid spacings hx, hy): independent of the
//      complex contrast, so metals work;
//   2. J blurred by a separable, truncated (radius ceil(3 sigma)), periodic Gaussian of width sigma cells: a pass along y with the
//      row in LDS, then a pass along x with lanes over y (coalesced rows);
//   3. N = principal eigenvector of the blurred J, in closed form: with d = Jxx - Jyy, o = 2 Jxy, r = hypot(d, o),
//      Nx^2 = (1 + d/r)/2, Nx Ny = o/(2r), Ny^2 = (1 - d/r)/2 -- a unit field wherever the coherence r / (Jxx + Jyy) exceeds
//      NV_TAU; elsewhere (uniform regions farther than the blur radius from any edge, isotropic points) N N^T = 0, i.e. Laurent's rule
//      (the fallback chosen by the study in profiles/normal_vector.txt).
// trx_convmat_nv chains the field, trx_convmat of eps, of 1/eps and of the three product grids, the inverse of [1/eps] (trx_inverse,
// complex128) and the six GEMMs of the three symmetrised products; all of it in fp64 for both dtypes.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace trx {
namespace {

typedef cx<double> zc;

constexpr double NV_TAU = 1e-3;          // coherence floor of a resolvable direction
constexpr double NV_SIGMA_MAX = 256.0;   // blur radius ceil(3 sigma) <= 768 cells: the weights stay a small LDS table

static inline int nv_radius(double sigma) { return sigma > 0.0 ? (int)std::ceil(3.0 * sigma) : 0; }

// w[k + R] = exp(-k^2 / (2 sigma^2)) / sum, k in [-R, R]  (every workgroup builds its own copy in LDS)
__device__ void nv_weights(double sigma, int R, double* w) {
    for (int k = threadIdx.x; k <= 2 * R; k += blockDim.x) {
        const double t = (double)(k - R);
        w[k] = R > 0 ? exp(-t * t / (2.0 * sigma * sigma)) : 1.0;
    }
    __syncthreads();
    double s = 0.0;                                // every thread sums in the same order: one normaliser for the workgroup
    for (int k = 0; k <= 2 * R; ++k) s += w[k];
    __syncthreads();
    for (int k = threadIdx.x; k <= 2 * R; k += blockDim.x) w[k] /= s;
    __syncthreads();
}

static inline __device__ int wrap(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

// g (T, real or complex) -> gz = g, rz = 1/g in complex128; a zero value sets info[b] = 1 (rz may be NULL)
template <class T, bool CPLX>
__global__ __launch_bounds__(256) void nv_convert_kernel(const T* __restrict__ grid, long per, zc* __restrict__ gz, zc* __restrict__ rz,
                                                         int* __restrict__ info) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per) return;
    const long o = (long)b * per + e;
    const zc v = CPLX ? zc((double)grid[2 * o], (double)grid[2 * o + 1]) : zc((double)grid[o], 0.0);
    gz[o] = v;
    if (rz) {
        if (v.x == 0.0 && v.y == 0.0) info[b] = 1;
        rz[o] = crecip(v);
    }
}

// Structure tensor of grid row x, blurred along y:  Jy[b, c, x, y] = sum_k w[k] J_c[x, y+k]   (c = xx, xy, yy)
// SKEW (trx_normal_field_lattice): the physical gradient is h^-1 (du, dv) of the index-space central differences, h^-1 = [[rhx, hi01],
// [hi10, rhy]]; otherwise (rhx du, rhy dv) with the rectangular spacings, exactly as trx_normal_field has always computed it.
template <bool SKEW>
__global__ __launch_bounds__(256) void nv_tensor_y_kernel(const zc* __restrict__ g, int nx, int ny, double sigma, int R, double rhx, double rhy,
                                                          double hi01, double hi10, double* __restrict__ Jy) {
    TRX_DYN_SMEM(smem);
    double* J = reinterpret_cast<double*>(smem);   // [3][ny]
    double* w = J + 3 * ny;                        // [2R+1]
    const int x = blockIdx.x, b = blockIdx.y;
    const zc* gb = g + (long)b * nx * ny;
    const zc* r0 = gb + (long)x * ny;
    const zc* rm = gb + (long)wrap(x - 1, nx) * ny;
    const zc* rp = gb + (long)wrap(x + 1, nx) * ny;
    for (int y = threadIdx.x; y < ny; y += blockDim.x) {
        zc gx, gy;
        if (SKEW) {
            const zc du = 0.5 * (rp[y] - rm[y]), dv = 0.5 * (r0[wrap(y + 1, ny)] - r0[wrap(y - 1, ny)]);
            gx = rhx * du + hi01 * dv;
            gy = hi10 * du + rhy * dv;
        } else {
            gx = (0.5 * rhx) * (rp[y] - rm[y]);
            gy = (0.5 * rhy) * (r0[wrap(y + 1, ny)] - r0[wrap(y - 1, ny)]);
        }
        J[y] = norm2(gx);
        J[ny + y] = gx.x * gy.x + gx.y * gy.y;     // Re(gx conj(gy))
        J[2 * ny + y] = norm2(gy);
    }
    nv_weights(sigma, R, w);                       // (ends with a barrier: J is visible too)
    const long nxy = (long)nx * ny;
    for (int y = threadIdx.x; y < ny; y += blockDim.x) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int k = -R; k <= R; ++k) {
            const int yy = wrap(y + k, ny);
            const double wk = w[k + R];
            a0 = fma(wk, J[yy], a0);
            a1 = fma(wk, J[ny + yy], a1);
            a2 = fma(wk, J[2 * ny + yy], a2);
        }
        double* o = Jy + (long)b * 3 * nxy + (long)x * ny + y;
        o[0] = a0;
        o[nxy] = a1;
        o[2 * nxy] = a2;
    }
}

// Blur along x and the closed-form principal direction:  nn[b, c, x, y] = (Nx^2, Nx Ny, Ny^2).  256 threads = 4 waves; lane = y
// (64 consecutive grid columns: every load of the k loop is a coalesced row segment), wave = one of 4 consecutive x.
__global__ __launch_bounds__(256) void nv_field_x_kernel(const double* __restrict__ Jy, int nx, int ny, double sigma, int R,
                                                         double* __restrict__ nn) {
    TRX_DYN_SMEM(smem);
    double* w = reinterpret_cast<double*>(smem);   // [2R+1]
    nv_weights(sigma, R, w);
    const int b = blockIdx.z;
    const int y = blockIdx.x * 64 + (threadIdx.x & 63);
    const int x = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= ny || x >= nx) return;
    const long nxy = (long)nx * ny;
    const double* J = Jy + (long)b * 3 * nxy;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = -R; k <= R; ++k) {
        const long e = (long)wrap(x + k, nx) * ny + y;
        const double wk = w[k + R];
        a0 = fma(wk, J[e], a0);
        a1 = fma(wk, J[nxy + e], a1);
        a2 = fma(wk, J[2 * nxy + e], a2);
    }
    const double d = a0 - a2, o = 2.0 * a1;
    const double r = sqrt(d * d + o * o);
    double pxx = 0.0, pxy = 0.0, pyy = 0.0;       // fallback: N N^T = 0 (Laurent's rule where no direction is resolvable)
    if (r > NV_TAU * (a0 + a2)) {
        const double c = d / r;
        pxx = 0.5 * (1.0 + c);
        pxy = 0.5 * (o / r);
        pyy = 0.5 * (1.0 - c);
    }
    double* out = nn + (long)b * 3 * nxy + (long)x * ny + y;
    out[0] = pxx;
    out[nxy] = pxy;
    out[2 * nxy] = pyy;
}

__global__ __launch_bounds__(256) void nv_delta_kernel(const zc* __restrict__ E, zc* __restrict__ D, long n) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) D[e] = E[e] - D[e];                 // D <- [eps] - [1/eps]^-1
}

__global__ __launch_bounds__(256) void nv_info_kernel(const int* __restrict__ inv_info, int batch, int* __restrict__ info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && info[b] == 0 && inv_info[b] != 0) info[b] = 2;
}

template <class T>
__global__ __launch_bounds__(256) void nv_store_kernel(const zc* __restrict__ in, cx<T>* __restrict__ out, long n) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = cx<T>((T)in[e].x, (T)in[e].y);
}

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace of the field from a complex128 grid: the y-blurred tensor [B, 3, nx, ny] fp64
static inline size_t field_core_bytes(int batch, int nx, int ny) { return al256(sizeof(double) * 3 * (size_t)batch * nx * ny); }

// hinv: NULL = the rectangular spacings hx, hy; else the row-major inverse of the cell matrix h (rows a1/nx, a2/ny) of a lattice
int field_core(hipStream_t s, const zc* gz, int batch, int nx, int ny, double sigma, double hx, double hy, double* nn, double* Jy,
               const double* hinv = nullptr) {
    const int R = nv_radius(sigma);
    const size_t lds1 = sizeof(double) * (3 * (size_t)ny + 2 * R + 1), lds2 = sizeof(double) * (2 * (size_t)R + 1);
    if (hinv) {
        if (set_max_dyn_smem((const void*)nv_tensor_y_kernel<true>, lds1)) return TRX_ERR_LAUNCH;
        TRX_LAUNCH(nv_tensor_y_kernel<true>, dim3(nx, batch), dim3(256), lds1, s, gz, nx, ny, sigma, R, hinv[0], hinv[3], hinv[1], hinv[2], Jy);
    } else {
        if (set_max_dyn_smem((const void*)nv_tensor_y_kernel<false>, lds1)) return TRX_ERR_LAUNCH;
        TRX_LAUNCH(nv_tensor_y_kernel<false>, dim3(nx, batch), dim3(256), lds1, s, gz, nx, ny, sigma, R, 1.0 / hx, 1.0 / hy, 0.0, 0.0, Jy);
    }
    TRX_LAUNCH(nv_field_x_kernel, dim3(cdiv_i(ny, 64), cdiv_i(nx, 4), batch), dim3(256), lds2, s, (const double*)Jy, nx, ny, sigma, R, nn);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <class T>
int convert(hipStream_t s, int cplx, const void* grid, int batch, long per, zc* gz, zc* rz, int* info) {
    const dim3 g(cdiv_i(per, 256), batch);
    if (cplx) TRX_LAUNCH((nv_convert_kernel<T, true>), g, dim3(256), 0, s, (const T*)grid, per, gz, rz, info);
    else      TRX_LAUNCH((nv_convert_kernel<T, false>), g, dim3(256), 0, s, (const T*)grid, per, gz, rz, info);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

bool field_args_ok(int batch, int nx, int ny, double sigma, double hx, double hy) {
    return batch > 0 && nx > 0 && ny > 0 && std::isfinite(sigma) && sigma >= 0.0 && std::isfinite(hx) && std::isfinite(hy) && hx > 0.0 &&
           hy > 0.0;
}

struct NvLayout {                   // byte offsets into the workspace of trx_convmat_nv
    size_t gz, rz, nn, jy, cws, R, C, inv, piv, iinfo, tmp, total;
    size_t cws_bytes, inv_bytes;
};

// Nlist < 0: the rectangle of (ox, oy); else a list of Nlist harmonics within |m| <= ox, |n| <= oy (trx_convmat_nv_orders)
NvLayout nv_layout(int dtype, int batch, int nx, int ny, int ox, int oy, int Nlist = -1) {
    NvLayout L;
    const size_t per = (size_t)nx * ny, N = Nlist < 0 ? (size_t)(2 * ox + 1) * (2 * oy + 1) : (size_t)Nlist, NN = N * N, B = (size_t)batch;
    size_t o = 0;
    L.gz = o;  o += al256(sizeof(zc) * B * per);
    L.rz = o;  o += al256(sizeof(zc) * B * per);
    L.nn = o;  o += al256(sizeof(double) * 3 * B * per);            // the field, when the caller supplies none
    L.jy = o;  o += field_core_bytes(batch, nx, ny);
    L.cws_bytes = trx_convmat_ws_bytes(TRX_C128, 3 * batch, nx, ny, ox, oy);
    L.cws = o; o += al256(L.cws_bytes);
    L.R = o;   o += al256(sizeof(zc) * B * NN);                     // [1/eps], then its inverse, then D
    L.C = o;   o += al256(sizeof(zc) * 3 * B * NN);                 // [Nx^2], [Nx Ny], [Ny^2]
    L.inv_bytes = trx_inverse_ws_bytes(TRX_C128, (int)N, batch);
    L.inv = o; o += al256(L.inv_bytes);
    L.piv = o; o += al256(sizeof(int) * B * N);
    L.iinfo = o; o += al256(sizeof(int) * B);
    L.tmp = o; o += dtype == TRX_C64 ? al256(sizeof(zc) * 3 * B * NN) : 0;   // complex128 results of a complex64 call
    L.total = o;
    return L;
}

// mn == NULL: the rectangle of (ox, oy) (trx_convmat); else the device list mn[Nlist] with mmax = ox, nmax = oy (trx_convmat_orders).
// hinv: NULL = spacings hx, hy; else the inverse cell matrix of a lattice (field_core).
template <class T>
int convmat_nv_t(int cplx, const void* grid, int batch, int nx, int ny, int ox, int oy, double sigma, double hx, double hy, const double* nn_in,
                 void* Exx, void* Exy, void* Eyy, int* info, char* ws, int dtype, hipStream_t s, const int* mn = nullptr, int Nlist = -1,
                 const double* hinv = nullptr) {
    const NvLayout L = nv_layout(dtype, batch, nx, ny, ox, oy, mn ? Nlist : -1);
    const long per = (long)nx * ny;
    const int N = mn ? Nlist : (2 * ox + 1) * (2 * oy + 1);
    // the list was checked once by trx_convmat_nv_orders: the three gathers below do not check (and synchronise) again
    auto conv = [&](int gc, const void* g, int nb, void* out) {
        return mn ? convmat_orders_checked(s, TRX_C128, gc, g, nb, nx, ny, mn, N, ox, oy, out, ws + L.cws)
                  : trx_convmat(TRX_C128, gc, g, nb, nx, ny, ox, oy, out, ws + L.cws, L.cws_bytes, s);
    };
    const long NN = (long)N * N, bNN = (long)batch * NN;
    zc* gz = (zc*)(ws + L.gz);
    zc* rz = (zc*)(ws + L.rz);
    zc* R = (zc*)(ws + L.R);
    zc* C = (zc*)(ws + L.C);
    int* piv = (int*)(ws + L.piv);
    int* iinfo = (int*)(ws + L.iinfo);
    zc *oxx, *oxy, *oyy;
    if (dtype == TRX_C128) {
        oxx = (zc*)Exx; oxy = (zc*)Exy; oyy = (zc*)Eyy;
    } else {
        oxx = (zc*)(ws + L.tmp); oxy = oxx + bNN; oyy = oxy + bNN;
    }
    if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s) != hipSuccess) return TRX_ERR_LAUNCH;
    int rc = convert<T>(s, cplx, grid, batch, per, gz, rz, info);
    if (rc) return rc;
    const double* nn = nn_in;
    if (!nn) {
        double* nw = (double*)(ws + L.nn);
        rc = field_core(s, gz, batch, nx, ny, sigma, hx, hy, nw, (double*)(ws + L.jy), hinv);
        if (rc) return rc;
        nn = nw;
    }
    // [eps] -> Exx (copied to Eyy below), [1/eps] -> R, [N_c] -> C[b*3 + c]
    if ((rc = conv(1, gz, batch, oxx))) return rc;
    if ((rc = conv(1, rz, batch, R))) return rc;
    if ((rc = conv(0, nn, 3 * batch, C))) return rc;
    return nv_tensor_tail(s, dtype, batch, N, oxx, oxy, oyy, Exx, Exy, Eyy, info, R, C, ws + L.inv, L.inv_bytes, piv, iinfo);
}

}  // namespace

// the tail every normal-vector entry shares (the grid entries above, trx_convmat_nv_shapes): [1/eps]^-1, D, the six GEMMs, the store
int nv_tensor_tail(hipStream_t s, int dtype, int batch, int N, zc* oxx, zc* oxy, zc* oyy, void* Exx, void* Exy, void* Eyy, int* info, zc* R, zc* C,
                   void* inv_ws, size_t inv_bytes, int* piv, int* iinfo) {
    const long NN = (long)N * N, bNN = (long)batch * NN;
    int rc;
    if (hipMemcpyAsync(oyy, oxx, sizeof(zc) * (size_t)bNN, hipMemcpyDeviceToDevice, s) != hipSuccess) return TRX_ERR_LAUNCH;
    if ((rc = trx_inverse(TRX_C128, R, N, batch, piv, iinfo, inv_ws, inv_bytes, s))) return rc;
    TRX_LAUNCH(nv_info_kernel, dim3(cdiv_i(batch, 256)), dim3(256), 0, s, (const int*)iinfo, batch, info);
    TRX_LAUNCH(nv_delta_kernel, dim3(cdiv_i(bNN, 256)), dim3(256), 0, s, (const zc*)oxx, R, bNN);
    TRX_CHECK_LAUNCH();
    // Exx = [eps] - (D [Nx^2] + [Nx^2] D) / 2,  Exy = -(D [Nx Ny] + [Nx Ny] D) / 2,  Eyy = [eps] - (D [Ny^2] + [Ny^2] D) / 2
    const zc mh(-0.5, 0.0), one(1.0, 0.0), zero(0.0, 0.0);
    zc* out[3] = {oxx, oxy, oyy};
    for (int c = 0; c < 3; ++c) {
        if ((rc = gemm<double>(s, TRX_OP_N, TRX_OP_N, N, N, N, mh, R, N, NN, C + c * NN, N, 3 * NN, c == 1 ? zero : one, out[c], N, NN, batch)))
            return rc;
        if ((rc = gemm<double>(s, TRX_OP_N, TRX_OP_N, N, N, N, mh, C + c * NN, N, 3 * NN, R, N, NN, one, out[c], N, NN, batch))) return rc;
    }
    if (dtype == TRX_C64) {
        const dim3 g(cdiv_i(bNN, 256));
        TRX_LAUNCH((nv_store_kernel<float>), g, dim3(256), 0, s, (const zc*)oxx, (cx<float>*)Exx, bNN);
        TRX_LAUNCH((nv_store_kernel<float>), g, dim3(256), 0, s, (const zc*)oxy, (cx<float>*)Exy, bNN);
        TRX_LAUNCH((nv_store_kernel<float>), g, dim3(256), 0, s, (const zc*)oyy, (cx<float>*)Eyy, bNN);
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_normal_field_ws_bytes(int dtype, int batch, int nx, int ny) {
    (void)dtype;
    if (batch <= 0 || nx <= 0 || ny <= 0) return 0;
    return al256(sizeof(zc) * (size_t)batch * nx * ny) + field_core_bytes(batch, nx, ny);
}

extern "C" int trx_normal_field(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, double sigma, double hx, double hy,
                                double* nn, void* ws, size_t ws_bytes, void* stream) {
    if (!grid || !nn || !ws || !field_args_ok(batch, nx, ny, sigma, hx, hy)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_normal_field_ws_bytes(dtype, batch, nx, ny)) return TRX_ERR_WORKSPACE;
    if (nx > 2048 || ny > 2048 || sigma > NV_SIGMA_MAX) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    zc* gz = (zc*)ws;
    double* Jy = (double*)((char*)ws + al256(sizeof(zc) * (size_t)batch * nx * ny));
    const long per = (long)nx * ny;
    int rc = dtype == TRX_C64 ? convert<float>(s, grid_is_complex, grid, batch, per, gz, nullptr, nullptr)
                              : convert<double>(s, grid_is_complex, grid, batch, per, gz, nullptr, nullptr);
    if (rc) return rc;
    return field_core(s, gz, batch, nx, ny, sigma, hx, hy, nn, Jy);
}

extern "C" size_t trx_convmat_nv_ws_bytes(int dtype, int batch, int nx, int ny, int ox, int oy) {
    if (batch <= 0 || ox < 0 || oy < 0 || nx <= 0 || ny <= 0) return 0;
    return nv_layout(dtype, batch, nx, ny, ox, oy).total;
}

extern "C" int trx_convmat_nv(int dtype, int grid_is_complex, const void* grid, int batch, int nx, int ny, int ox, int oy, double sigma, double hx,
                              double hy, const double* nn, void* Exx, void* Exy, void* Eyy, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (!grid || !Exx || !Exy || !Eyy || !info || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || ox < 0 || oy < 0 || nx <= 2 * ox || ny <= 2 * oy) return TRX_ERR_ARG;
    if (!nn && !field_args_ok(batch, nx, ny, sigma, hx, hy)) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_convmat_nv_ws_bytes(dtype, batch, nx, ny, ox, oy)) return TRX_ERR_WORKSPACE;
    if (nx > 2048 || ny > 2048 || (!nn && sigma > NV_SIGMA_MAX)) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    if (dtype == TRX_C64)
        return convmat_nv_t<float>(grid_is_complex, grid, batch, nx, ny, ox, oy, sigma, hx, hy, nn, Exx, Exy, Eyy, info, (char*)ws, dtype, s);
    return convmat_nv_t<double>(grid_is_complex, grid, batch, nx, ny, ox, oy, sigma, hx, hy, nn, Exx, Exy, Eyy, info, (char*)ws, dtype, s);
}

// inverse of the cell matrix h (row-major, rows a1/n1 and a2/n2); false if h is not finite or (nearly) singular
static bool cell_inverse(const double* h, double* hinv) {
    if (!h) return false;
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(h[k])) return false;
    const double det = h[0] * h[3] - h[1] * h[2];
    if (!(std::fabs(det) > 1e-9 * std::hypot(h[0], h[1]) * std::hypot(h[2], h[3]))) return false;
    hinv[0] = h[3] / det; hinv[1] = -h[1] / det; hinv[2] = -h[2] / det; hinv[3] = h[0] / det;
    return true;
}

static inline bool cell_is_rect(const double* h) { return h[1] == 0.0 && h[2] == 0.0 && h[0] > 0.0 && h[3] > 0.0; }

extern "C" int trx_normal_field_lattice(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, double sigma, const double* h,
                                        double* nn, void* ws, size_t ws_bytes, void* stream) {
    double hinv[4];
    if (!grid || !nn || !ws || !cell_inverse(h, hinv) || !field_args_ok(batch, n1, n2, sigma, 1.0, 1.0)) return TRX_ERR_ARG;
    if (cell_is_rect(h)) return trx_normal_field(dtype, grid_is_complex, grid, batch, n1, n2, sigma, h[0], h[3], nn, ws, ws_bytes, stream);
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_normal_field_ws_bytes(dtype, batch, n1, n2)) return TRX_ERR_WORKSPACE;
    if (n1 > 2048 || n2 > 2048 || sigma > NV_SIGMA_MAX) return TRX_ERR_UNSUPPORTED;
    hipStream_t s = trx::api_stream(stream);
    zc* gz = (zc*)ws;
    double* Jy = (double*)((char*)ws + al256(sizeof(zc) * (size_t)batch * n1 * n2));
    const long per = (long)n1 * n2;
    int rc = dtype == TRX_C64 ? convert<float>(s, grid_is_complex, grid, batch, per, gz, nullptr, nullptr)
                              : convert<double>(s, grid_is_complex, grid, batch, per, gz, nullptr, nullptr);
    if (rc) return rc;
    return field_core(s, gz, batch, n1, n2, sigma, 1.0, 1.0, nn, Jy, hinv);
}

extern "C" size_t trx_convmat_nv_orders_ws_bytes(int dtype, int batch, int n1, int n2, int N, int mmax, int nmax) {
    if (batch <= 0 || N <= 0 || mmax < 0 || nmax < 0 || n1 <= 0 || n2 <= 0) return 0;
    return nv_layout(dtype, batch, n1, n2, mmax, nmax, N).total;
}

extern "C" int trx_convmat_nv_orders(int dtype, int grid_is_complex, const void* grid, int batch, int n1, int n2, const int* mn, int N, int mmax,
                                     int nmax, double sigma, const double* h, const double* nn, void* Exx, void* Exy, void* Eyy, int* info,
                                     void* ws, size_t ws_bytes, void* stream) {
    double hinv[4] = {1.0, 0.0, 0.0, 1.0};
    if (!grid || !mn || !Exx || !Exy || !Eyy || !info || !ws) return TRX_ERR_ARG;
    if (batch <= 0 || N <= 0 || mmax < 0 || nmax < 0 || n1 <= 2 * mmax || n2 <= 2 * nmax) return TRX_ERR_ARG;
    if (!nn && (!cell_inverse(h, hinv) || !field_args_ok(batch, n1, n2, sigma, 1.0, 1.0))) return TRX_ERR_ARG;
    if (dtype != TRX_C64 && dtype != TRX_C128) return TRX_ERR_DTYPE;
    if (ws_bytes < trx_convmat_nv_orders_ws_bytes(dtype, batch, n1, n2, N, mmax, nmax)) return TRX_ERR_WORKSPACE;
    if (n1 > 2048 || n2 > 2048 || (!nn && sigma > NV_SIGMA_MAX)) return TRX_ERR_UNSUPPORTED;
    if ((size_t)16 * 2 * (size_t)(n1 > n2 ? n1 : n2) > 64 * 1024) return TRX_ERR_UNSUPPORTED;   // the DFT rows of trx_convmat_orders
    hipStream_t s = trx::api_stream(stream);
    if (int rc = orders_check(s, mn, N, mmax, nmax)) return rc;
    // a rectangular cell takes the spacings path of trx_normal_field (same field bit for bit)
    const bool rect = nn || cell_is_rect(h);
    const double hx = rect && h ? h[0] : 1.0, hy = rect && h ? h[3] : 1.0;
    if (dtype == TRX_C64)
        return convmat_nv_t<float>(grid_is_complex, grid, batch, n1, n2, mmax, nmax, sigma, hx, hy, nn, Exx, Exy, Eyy, info, (char*)ws, dtype, s,
                                   mn, N, rect ? nullptr : hinv);
    return convmat_nv_t<double>(grid_is_complex, grid, batch, n1, n2, mmax, nmax, sigma, hx, hy, nn, Exx, Exy, Eyy, info, (char*)ws, dtype, s,
                                mn, N, rect ? nullptr : hinv);
}
