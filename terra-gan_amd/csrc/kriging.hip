// Empirical semivariogram and ordinary kriging over the eight ray hits (mvp_gan/src/kriging.py).
//
//   tg_variogram   variogram_kernel: one pass over 32 x 64 tiles of z staged in LDS with a 32-px halo to the right, below and to
//                  the left, and one flag byte per staged pixel.  A pair is a known pixel x and a known pixel x + L u, L = 2^j px,
//                  u a unit step of the class (cls 0: (0,1), (1,0); cls 1: (1,1), (1,-1)): every unordered pair once.  Per scale
//                  s = 2 j + cls the number of pairs and the fp64 sum of d^2, d = (double)z(x) - (double)z(x + L u).
//                  variogram_finish_kernel: one workgroup reduces the per-workgroup rows in index order.
//   tg_krige       krige_kernel<MODEL>: one thread per pixel.  The samples of a void pixel are the first known pixels along the
//                  eight rays (tg_rayfill's hits); the ordinary-kriging system is reduced against the nearest sample r to a
//                  symmetric positive definite (n - 1) x (n - 1) system and factorised by Cholesky at a fixed 7 x 7 with static
//                  indices: a missing ray is an identity row with a zero right-hand side.
//
// Determinism: no floating-point atomics.  The variogram's grid is a function of the shape, a workgroup walks its tiles and a
// thread its pixels, octaves and steps in a fixed order, the wave and workgroup reductions are fixed trees, every workgroup writes
// one row of partials (zeros included) and the finish kernel adds the rows in index order; a tile without a known pixel adds exact
// zeros, so leaving it early changes no bit.  The counts use integer atomics.  A kriged pixel is a function of its own reads.
#include <math.h>

#include "raster_sweep.h"

// The fp64 sums are compared with a reference that does not fuse: no multiply-add contraction in this file.
#pragma clang fp contract(off)

// ---- the variogram: geometry --------------------------------------------------------------------------------------------
constexpr int VG_TY = 32, VG_TX = 64;          // tile: 4 waves x 8 rows, lane = column (texture.hip's)
constexpr int VG_HALO = 1 << (TG_VGM_OCTAVES - 1);
constexpr int VG_RY = VG_TY + VG_HALO;         // 64 staged rows: the tile and the halo below it
constexpr int VG_RX = VG_TX + 2 * VG_HALO;     // 128 staged columns: the halo to the left serves the (1, -1) step only
// A wave reads one staged row at a time, lane l the column l + const: 64 consecutive words at any stride, so no padding.
constexpr int VG_SX = VG_RX;
constexpr int VG_MAX_GRID = 2048;
constexpr int VG_ROW = TG_VGM_SCALES;          // doubles per row of partials
constexpr int VG_FIN_CHUNKS = 16;              // the finish kernel: 16 chunks x 16 columns = 256 threads
static_assert(VG_HALO == 32 && VG_ROW <= 16 && TG_VGM_SCALES == 2 * TG_VGM_OCTAVES, "variogram geometry");
// 32 KiB of heights, 8 KiB of flags and under 1 KiB of reduction scratch: 41 KiB, two workgroups in a CU's 160 KiB with room
static_assert(sizeof(float) * VG_RY * VG_SX + VG_RY * VG_SX + 4 * VG_ROW * (sizeof(double) + sizeof(int)) <= 48 * 1024,
              "two workgroups per CU");

static int vg_tiles_x(int W) { return (int)cdiv64(W, VG_TX); }
static int vg_tiles(int H, int W) { return (int)(cdiv64(H, VG_TY) * vg_tiles_x(W)); }       // < 2^31 / 2048 + 2^27

static int vg_grid(int H, int W) {
    const int64_t tiles = vg_tiles(H, W);
    return (int)(tiles < VG_MAX_GRID ? tiles : VG_MAX_GRID);
}

// one pair: the partner known -> the first difference in fp64 from the fp32 values, nothing fused
#define VG_PAIR(DY, DX, N, SUM)                                      \
    do {                                                             \
        if (sk[ly + (DY)][lx + (DX)]) {                              \
            const double d = zc - (double)sz[ly + (DY)][lx + (DX)];  \
            ++(N);                                                   \
            (SUM) = (SUM) + d * d;                                   \
        }                                                            \
    } while (0)

__global__ __launch_bounds__(256) void variogram_kernel(const float* __restrict__ z, const uint8_t* __restrict__ known, int H, int W,
                                                        int octaves, int tiles_x, int ntiles, ull* __restrict__ counts,
                                                        double* __restrict__ partials) {
    __shared__ float sz[VG_RY][VG_SX];
    __shared__ uint8_t sk[VG_RY][VG_SX];               // 1: inside the raster and known
    __shared__ double dred[4][VG_ROW];
    __shared__ int ired[4][VG_ROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[VG_ROW];
    int cnt[VG_ROW];
#pragma unroll
    for (int s = 0; s < VG_ROW; ++s) {
        cnt[s] = 0;
        acc[s] = 0.0;
    }

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = ty * VG_TY, x0 = tx * VG_TX;
        // the thread's eight known bytes, bit k = row w * 8 + k of column lane
        const int64_t x = (int64_t)x0 + lane;
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t y = (int64_t)y0 + w * 8 + k;
            if (y < H && x < W) mine |= (known[y * W + x] != 0 ? 1u : 0u) << k;
        }
        // uniform over the workgroup, and the barrier after which the previous tile's readers are done
        if (!__syncthreads_or((int)mine)) continue;
        for (int j = threadIdx.x; j < VG_RY * VG_RX; j += 256) {
            const int r = j / VG_RX, c = j - r * VG_RX;
            const int64_t y = (int64_t)y0 + r, xx = (int64_t)x0 - VG_HALO + c;
            float zv = 0.f;
            uint8_t f = 0;
            if (y < H && xx >= 0 && xx < W) {
                const int64_t i = y * W + xx;
                zv = z[i];
                f = known[i] != 0;
            }
            sz[r][c] = zv;
            sk[r][c] = f;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            if (!((mine >> k) & 1u)) continue;
            const int ly = w * 8 + k, lx = VG_HALO + lane;
            const double zc = sz[ly][lx];
#pragma unroll
            for (int o = 0; o < TG_VGM_OCTAVES; ++o) {
                if (o < octaves) {
                    const int h = 1 << o;
                    VG_PAIR(0, h, cnt[2 * o], acc[2 * o]);
                    VG_PAIR(h, 0, cnt[2 * o], acc[2 * o]);
                    VG_PAIR(h, h, cnt[2 * o + 1], acc[2 * o + 1]);
                    VG_PAIR(h, -h, cnt[2 * o + 1], acc[2 * o + 1]);
                }
            }
        }
    }

    // workgroup reduction in a fixed order: xor butterflies inside the waves, then waves 0..3
#pragma unroll
    for (int s = 0; s < VG_ROW; ++s) {
        const double v = wave_sum_d(acc[s]);
        int n = cnt[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) {
            dred[w][s] = v;
            ired[w][s] = n;
        }
    }
    __syncthreads();
    if (threadIdx.x < VG_ROW) {
        const int s = threadIdx.x;
        partials[(int64_t)blockIdx.x * VG_ROW + s] = ((dred[0][s] + dred[1][s]) + dred[2][s]) + dred[3][s];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + VG_ROW) {
        const int s = threadIdx.x - 64;
        const int64_t v = (int64_t)ired[0][s] + ired[1][s] + ired[2][s] + ired[3][s];
        if (v) atomicAdd(&counts[s], (ull)v);
    }
}

// thread (chunk, col) adds rows chunk, chunk + 16, ... of column col in that order; then column col adds its chunks 0..15
__global__ __launch_bounds__(256) void variogram_finish_kernel(const double* __restrict__ partials, int nwg,
                                                               double* __restrict__ sums) {
    __shared__ double red[VG_FIN_CHUNKS][16];
    const int col = threadIdx.x & 15, chunk = threadIdx.x >> 4;
    double v = 0.0;
    if (col < VG_ROW)
        for (int g = chunk; g < nwg; g += VG_FIN_CHUNKS) v = v + partials[(int64_t)g * VG_ROW + col];
    red[chunk][col] = v;
    __syncthreads();
    if (threadIdx.x < VG_ROW) {
        double s = red[0][col];
#pragma unroll
        for (int c = 1; c < VG_FIN_CHUNKS; ++c) s = s + red[c][col];
        sums[col] = s;
    }
}

// ---- kriging ------------------------------------------------------------------------------------------------------------
constexpr int KR_N = 7;                        // the reduced system: at most eight samples less the reference

struct KrigeModel {
    double cellsize, nugget, scale, shape;
};

struct KrigeArgs {
    const float* z;
    const uint8_t* known;
    const uint16_t* hits;
    int H, W;
    KrigeModel vg;
    const int32_t* d2;
    const int32_t* idx;
    float* out;
    float* var;
    ull* counts;
};

// gamma at the squared pixel distance n (an exact integer in a double, up to 2 * 65532^2), n > 0
template <int MODEL>
__host__ __device__ __forceinline__ double krige_gamma(double n, const KrigeModel& A) {
    const double h = A.cellsize * sqrt(n);
    if (MODEL == 0) return A.nugget + A.scale * exp2(A.shape * log2(h));         // h^shape, h > 0: no pow
    if (MODEL == 1) return A.nugget + A.scale * (1.0 - exp(-h / A.shape));
    double r = h / A.shape;
    r = r < 1.0 ? r : 1.0;
    return A.nugget + A.scale * (1.5 * r - 0.5 * ((r * r) * r));
}

// One pixel's system.  oy, ox: the offsets of the eight ray samples from the pixel, (0, 0): no sample; zs: their heights; r: the
// nearest sample (the first in ray order among equals), nr its squared pixel distance.  Host and device: the arithmetic has no
// other copy, and a host program can run it against a reference.
template <int MODEL>
__host__ __device__ __forceinline__ void krige_solve(int (&oy)[8], int (&ox)[8], double (&zs)[8], int r, int32_t nr,
                                                     const KrigeModel& A, double& est, double& var) {
    // the reference sample into scalars, ray 7 into its slot: slots 0..6 are the other samples, static indices
    int ry = 0, rx = 0;
    double zr = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j == r) {
            ry = oy[j];
            rx = ox[j];
            zr = zs[j];
        }
    }
#pragma unroll
    for (int j = 0; j < KR_N; ++j) {
        if (j == r) {
            oy[j] = oy[7];
            ox[j] = ox[7];
            zs[j] = zs[7];
        }
    }
    const double gr0 = krige_gamma<MODEL>((double)nr, A);
    double gir[KR_N], b[KR_N], M[KR_N][KR_N];           // the lower triangle of M is used
    bool have[KR_N];
#pragma unroll
    for (int i = 0; i < KR_N; ++i) {
        have[i] = (oy[i] | ox[i]) != 0;
        const double ay = (double)(oy[i] - ry), ax = (double)(ox[i] - rx);
        const double cy = (double)oy[i], cx = (double)ox[i];
        gir[i] = have[i] ? krige_gamma<MODEL>(ay * ay + ax * ax, A) : 0.0;
        const double gi0 = have[i] ? krige_gamma<MODEL>(cy * cy + cx * cx, A) : 0.0;
        b[i] = have[i] ? (gir[i] + gr0) - gi0 : 0.0;
        M[i][i] = have[i] ? gir[i] + gir[i] : 1.0;      // gamma(0) = 0
    }
#pragma unroll
    for (int i = 1; i < KR_N; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const bool both = have[i] && have[j];
            const double ay = (double)(oy[i] - oy[j]), ax = (double)(ox[i] - ox[j]);
            M[i][j] = both ? (gir[i] + gir[j]) - krige_gamma<MODEL>(ay * ay + ax * ax, A) : 0.0;
        }
    }
    // Cholesky M = L L^T in place, then L c = b; no pivoting: M is symmetric positive definite
#pragma unroll
    for (int j = 0; j < KR_N; ++j) {
        double d = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - M[j][k] * M[j][k];
        d = sqrt(d);
        const double inv = 1.0 / d;
        M[j][j] = inv;                                  // the reciprocal of the diagonal
#pragma unroll
        for (int i = j + 1; i < KR_N; ++i) {
            double s = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - M[i][k] * M[j][k];
            M[i][j] = s * inv;
        }
        double c = b[j];
#pragma unroll
        for (int k = 0; k < j; ++k) c = c - M[j][k] * b[k];
        b[j] = c * inv;
    }
    // var = 2 gamma_r0 - b^T M^-1 b = 2 gamma_r0 - |c|^2, before the back substitution overwrites c
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < KR_N; ++j) q = q + b[j] * b[j];
    // L^T w = c
#pragma unroll
    for (int j = KR_N - 1; j >= 0; --j) {
        double c = b[j];
#pragma unroll
        for (int k = j + 1; k < KR_N; ++k) c = c - M[k][j] * b[k];
        b[j] = c * M[j][j];
    }
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < KR_N; ++i) e = e + b[i] * (zs[i] - zr);     // a missing ray has w = 0 exactly
    const double s = (gr0 + gr0) - q;
    est = zr + e;
    var = s > 0.0 ? s : 0.0;
}

template <int MODEL>
__global__ __launch_bounds__(256) void krige_kernel(KrigeArgs A) {
    __shared__ int red[3][4];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int H = A.H, W = A.W;
    int by_rays = 0, by_near = 0, left = 0;
    if (x < W) {
        const int64_t p = (int64_t)y * W + x;
        const int64_t plane = (int64_t)H * W;
        if (A.known[p]) {
            A.out[p] = A.z[p];
            A.var[p] = 0.f;
        } else {
            const int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};          // N, NE, E, SE, S, SW, W, NW
            const int dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
            int oy[8], ox[8];                                       // the sample's offset from the pixel; (0, 0): no sample
            double zs[8];
            int r = -1;
            int32_t nr = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int kj = A.hits[j * plane + p];
                const int yy = y + kj * dy[j], xx = x + kj * dx[j];
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) kj = 0;
                oy[j] = kj * dy[j];
                ox[j] = kj * dx[j];
                zs[j] = kj ? (double)A.z[(int64_t)yy * W + xx] : 0.0;
                const int32_t n = kj * kj * ((j & 1) ? 2 : 1);      // <= 2 * 32766^2 < 2^31
                if (kj && n < nr) {                                 // the first in ray order among equals
                    nr = n;
                    r = j;
                }
            }
            float v = __uint_as_float(0x7fc00000u), s2 = v;
            if (r >= 0) {
                double est, s;
                krige_solve<MODEL>(oy, ox, zs, r, nr, A.vg, est, s);
                v = (float)est;
                s2 = (float)s;
                by_rays = 1;
            } else {
                int32_t i = A.idx ? A.idx[p] : -1;
                const int32_t d = A.d2 ? A.d2[p] : 0;
                if (i >= 0 && i < plane) {
                    v = A.z[i];
                    const double g = d > 0 ? krige_gamma<MODEL>((double)d, A.vg) : 0.0;        // gamma(0) = 0
                    s2 = (float)(g + g);
                    by_near = 1;
                } else {
                    left = 1;
                }
            }
            A.out[p] = v;
            A.var[p] = s2;
        }
    }
    // counters: per-wave popcounts, waves 0..3 through LDS, one integer atomic per counter and workgroup (rayfill_kernel's)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = __popcll(__ballot(by_rays)), c1 = __popcll(__ballot(by_near)), c2 = __popcll(__ballot(left));
    if (lane == 0) { red[0][w] = c0; red[1][w] = c1; red[2][w] = c2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (s) atomicAdd(&A.counts[threadIdx.x], (ull)s);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" size_t tg_variogram_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return (size_t)vg_grid(H, W) * VG_ROW * sizeof(double);
}

extern "C" int tg_variogram(const float* z, const uint8_t* known, int H, int W, int octaves, int64_t* counts, double* sums,
                            void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_variogram", H, W)) return rc;
    const void* const ptr[] = {z, known, counts, sums, ws};
    const char* const name[] = {"z", "known", "counts", "sums", "ws"};
    for (int i = 0; i < 5; ++i) TG_REQUIRE(ptr[i], "tg_variogram: null pointer %s", name[i]);
    TG_REQUIRE(octaves >= 1 && octaves <= TG_VGM_OCTAVES, "tg_variogram: octaves %d must lie in [1, %d]", octaves, TG_VGM_OCTAVES);
    const size_t need = tg_variogram_ws_bytes(H, W);
    TG_REQUIRE(ws_bytes >= need, "tg_variogram: workspace ws_bytes %zu < %zu", ws_bytes, need);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_VGM_SCALES * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_variogram: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int tiles_x = vg_tiles_x(W), ntiles = vg_tiles(H, W), grid = vg_grid(H, W);
    hipLaunchKernelGGL(variogram_kernel, dim3(grid), dim3(256), 0, s, z, known, H, W, octaves, tiles_x, ntiles,
                       reinterpret_cast<ull*>(counts), (double*)ws);
    TG_CHECK_LAUNCH("variogram_kernel");
    hipLaunchKernelGGL(variogram_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grid, sums);
    TG_CHECK_LAUNCH("variogram_finish_kernel");
    return TG_OK;
}

extern "C" int tg_krige(const float* z, const uint8_t* known, const uint16_t* hits, int H, int W, double cellsize, int model,
                        double nugget, double scale, double shape, const int32_t* d2, const int32_t* idx, float* out, float* var,
                        int64_t* counts, tg_stream_t stream) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= TG_EDT_MAX_SIDE && W <= TG_EDT_MAX_SIDE,
               "tg_krige: raster %dx%d: both sides must lie in [1, %d]", H, W, (int)TG_EDT_MAX_SIDE);
    TG_REQUIRE(z && known && hits && out && var && counts, "tg_krige: null pointer");
    TG_REQUIRE(!d2 == !idx, "tg_krige: d2 and idx go together (both NULL: no nearest-neighbour fallback)");
    TG_REQUIRE(out != z && var != z && out != var, "tg_krige: out, var and z must be distinct");
    TG_REQUIRE(isfinite(cellsize) && cellsize > 0.0, "tg_krige: cellsize %g must be finite and > 0", cellsize);
    TG_REQUIRE(model >= TG_VGM_POWER && model <= TG_VGM_SPHERICAL, "tg_krige: model %d must be 0 (power), 1 (exponential) or 2 "
               "(spherical)", model);
    TG_REQUIRE(isfinite(nugget) && nugget >= 0.0, "tg_krige: nugget %g must be finite and >= 0", nugget);
    TG_REQUIRE(isfinite(scale) && scale > 0.0, "tg_krige: scale %g must be finite and > 0", scale);
    if (model == TG_VGM_POWER)
        TG_REQUIRE(shape > 0.0 && shape < 2.0, "tg_krige: the power model's shape %g must lie in (0, 2)", shape);
    else
        TG_REQUIRE(isfinite(shape) && shape > 0.0, "tg_krige: shape %g (a range in metres) must be finite and > 0", shape);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_krige: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    KrigeArgs A;
    A.z = z; A.known = known; A.hits = hits; A.H = H; A.W = W;
    A.vg.cellsize = cellsize; A.vg.nugget = nugget; A.vg.scale = scale; A.vg.shape = shape;
    A.d2 = d2; A.idx = idx; A.out = out; A.var = var; A.counts = reinterpret_cast<ull*>(counts);
    const dim3 grid(cdiv(W, 256), H);
    if (model == TG_VGM_POWER) hipLaunchKernelGGL(krige_kernel<0>, grid, dim3(256), 0, s, A);
    else if (model == TG_VGM_EXPONENTIAL) hipLaunchKernelGGL(krige_kernel<1>, grid, dim3(256), 0, s, A);
    else hipLaunchKernelGGL(krige_kernel<2>, grid, dim3(256), 0, s, A);
    TG_CHECK_LAUNCH("krige_kernel");
    return TG_OK;
}
