// Raster resampling between a DSM's cell size and the generator's (mvp_gan/src/resample.py).
//
//   tg_resample_area     to a coarser grid (p >= q): exact integer footprint weights, coverage rule in integers, weighted mean of
//                        the known taps about a pivot
//   tg_resample_interp   to a finer grid (p <= q): Catmull-Rom where all 16 taps are known, else bilinear renormalised over the
//                        known ones of the 4 nearest, both about the pixel that contains the output centre; taps from LDS
//
// Geometry per axis, in units of 1/q source pixel: source pixel i covers [i q, (i+1) q), output pixel I covers [I p, (I+1) p)
// clipped to [0, N q), No = ceil(N q / p).  Everything that decides a mask bit is integer arithmetic.
// Both kernels take an optional second raster (keep) on the output grid: where it is known its bits are copied through, which
// makes one launch the return trip to the native grid.  n_nan counts the output pixels left NaN (one integer atomic per
// workgroup); out and out_mask may each be null, and with both null a launch only counts.  Every value is computed by one thread in a fixed order: bitwise deterministic.  No kernel uses scratch.
#include <math.h>

#include "common.h"
#include "raster_known.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

struct RsGeom {
    int H, W, Ho, Wo, p, q;
};

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 8192;      // staged source footprint of one area workgroup (32 KiB: five workgroups per CU)

// counts the NaN outputs of a workgroup into *n_nan
__device__ __forceinline__ void rs_count_nan(int miss, int32_t* __restrict__ n_nan) {
    __shared__ int sred[RS_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) miss += __shfl_xor(miss, o, 64);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = miss;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < RS_THREADS / 64; ++w) t += sred[w];
        if (t) atomicAdd(n_nan, t);          // integer: the total does not depend on the order
    }
}

// ---- area: a workgroup owns ty x (1 << txl2) output pixels and stages their clipped source footprint into LDS ------------------
// An unknown source pixel is staged as NaN (a known one is finite), so one float carries value and flag.  Row r of the
// footprint starts at the 16-byte boundary at or below its first pixel: its chunks of 4 are aligned in HBM and in LDS, whatever
// W is; chunks that straddle the footprint's ends, and everything when a base pointer is not 16-byte aligned, go pixel by pixel.
__global__ __launch_bounds__(RS_THREADS) void resample_area_kernel(RasterIn in, RasterIn keep, RsGeom g, int ty, int txl2,
                                                                   int tiles_x, int sstride, int cov_num, int cov_den, int vec_ok,
                                                                   float* __restrict__ out, float* __restrict__ omask,
                                                                   int32_t* __restrict__ n_nan) {
    extern __shared__ f32x4 rs_smem4[];
    float* sm = reinterpret_cast<float*>(rs_smem4);
    const int tid = threadIdx.x;
    const int tx = 1 << txl2;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int Y0 = by * ty, X0 = bx * tx;
    const int Hq = g.H * g.q, Wq = g.W * g.q;
    const int sy0 = (Y0 * g.p) / g.q, sx0 = (X0 * g.p) / g.q;
    const int sy1 = (min((Y0 + ty) * g.p, Hq) + g.q - 1) / g.q, sx1 = (min((X0 + tx) * g.p, Wq) + g.q - 1) / g.q;
    const int rows = sy1 - sy0, cols = sx1 - sx0;
    const int C = sstride >> 2;

    for (int idx = tid; idx < rows * C; idx += RS_THREADS) {
        const int r = idx / C, k = idx - r * C;
        const int64_t g0 = (int64_t)(sy0 + r) * g.W + sx0, g1 = g0 + cols;
        const int64_t e = (g0 & ~(int64_t)3) + 4 * k;
        if (e >= g1) continue;
        f32x4 v;
        if (vec_ok && e >= g0 && e + 4 <= g1) {
            const f32x4 z = *reinterpret_cast<const f32x4*>(in.dem + e);
            f32x4 m = {1.f, 1.f, 1.f, 1.f};
            if (in.mask) m = *reinterpret_cast<const f32x4*>(in.mask + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bool kn = isfinite(z[j]) && m[j] != 0.f;
                if (in.use_nodata) kn = kn && z[j] != in.nodata;
                v[j] = kn ? z[j] : NAN;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float z = NAN;
                if (e + j >= g0 && e + j < g1 && !rs_known(in, e + j, z)) z = NAN;
                v[j] = z;
            }
        }
        *reinterpret_cast<f32x4*>(sm + r * sstride + 4 * k) = v;
    }
    __syncthreads();

    int miss = 0;
    for (int j = tid; j < (ty << txl2); j += RS_THREADS) {
        const int Y = Y0 + (j >> txl2), X = X0 + (j & (tx - 1));
        if (Y >= g.Ho || X >= g.Wo) continue;
        const int64_t o = (int64_t)Y * g.Wo + X;
        float kz;
        if (keep.dem && rs_known(keep, o, kz)) {
            if (out) out[o] = kz;                // bit for bit
            if (omask) omask[o] = 1.f;
            continue;
        }
        const int ylo = Y * g.p, yhi = min(ylo + g.p, Hq), xlo = X * g.p, xhi = min(xlo + g.p, Wq);
        const int i0 = ylo / g.q, i1 = (yhi + g.q - 1) / g.q, j0 = xlo / g.q, j1 = (xhi + g.q - 1) / g.q;
        int ck = 0, ct = 0;
        bool have = false;
        float z0 = 0.f, num = 0.f;
        for (int i = i0; i < i1; ++i) {
            const int wy = min((i + 1) * g.q, yhi) - max(i * g.q, ylo);
            const uint32_t off = ((uint32_t)i * (uint32_t)g.W + (uint32_t)sx0) & 3u;      // that row's shift in LDS
            const float* row = sm + (i - sy0) * sstride + (int)off - sx0;
            for (int jj = j0; jj < j1; ++jj) {
                const int w = wy * (min((jj + 1) * g.q, xhi) - max(jj * g.q, xlo));
                const float z = row[jj];
                ct += w;
                if (z == z) {
                    if (!have) {
                        have = true;
                        z0 = z;                  // the pivot: the first known tap in row-major order
                    }
                    ck += w;
                    num = __fmaf_rn((float)w, __fsub_rn(z, z0), num);
                }
            }
        }
        const bool kn = ck > 0 && (int64_t)ck * cov_den >= (int64_t)cov_num * ct;
        float val = NAN;
        if (kn) val = num == 0.f ? z0 : __fadd_rn(z0, __fdiv_rn(num, (float)ck));
        if (out) out[o] = val;
        if (omask) omask[o] = kn ? 1.f : 0.f;
        miss += kn ? 0 : 1;
    }
    rs_count_nan(miss, n_nan);
}

// ---- interp: a workgroup owns a 16 x 64 output tile and stages the source pixels its taps read into LDS -----------------------
// The 16 taps of an output pixel are shared with up to 16 neighbours (4 x 4 at 1/4).  Staged once, NaN-coded and already
// clamped to the raster, they cost one LDS read each instead of a dem and a mask load from L1 (DESIGN.md section 8m records
// the plain gather's times: 2.6 to 3.2 times slower).
// Catmull-Rom (Keys a = -0.5) weights at t = r / m, m = 2 q <= 2048: the numerators over 2 m^3 are exact integers (below 2^36),
// the quotient is formed in fp64, so each fp32 weight is the exact one rounded to fp32
__device__ __forceinline__ void rs_cubic(int r, int m, float w[4]) {
    const int64_t r2m = (int64_t)r * r * m, r3 = (int64_t)r * r * r, rm2 = (int64_t)r * m * m, m3 = (int64_t)m * m * m;
    const double inv = 1.0 / (double)(2 * m3);
    w[0] = (float)((double)(-r3 + 2 * r2m - rm2) * inv);
    w[1] = (float)((double)(3 * r3 - 5 * r2m + 2 * m3) * inv);
    w[2] = (float)((double)(-3 * r3 + 4 * r2m + rm2) * inv);
    w[3] = (float)((double)(r3 - r2m) * inv);
}

// centre of output pixel I in source pixel-centre coordinates: ((2 I + 1) p - q) / (2 q) = f + r / (2 q)
__device__ __forceinline__ void rs_centre(int I, int p, int q, int& f, int& r) {
    const int num = (2 * I + 1) * p - q, m = 2 * q;
    f = num >= 0 ? num / m : -((-num + m - 1) / m);
    r = num - f * m;
}

// value of one output pixel from its taps: tap(a, b) is the NaN-coded source pixel (f_y - 1 + a, f_x - 1 + b), clamped to the
// raster, a, b = 0 .. 3; ry, rx the fractions over m = 2 q.  NaN when the pixel that contains the centre is unknown.
template <class Tap>
__device__ __forceinline__ float rs_interp_value(Tap&& tap, int ry, int rx, int q) {
    const int m = 2 * q;
    // the source pixel that contains the centre: f when the fraction is below 1/2, else f + 1
    const float zc = tap(ry < q ? 1 : 2, rx < q ? 1 : 2);
    if (!(zc == zc)) return NAN;
    float d[4][4];
    bool all = true;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float z = tap(a, b);
            all = all && z == z;
            d[a][b] = __fsub_rn(z, zc);          // NaN where the tap is unknown
        }
    float v;
    if (all) {
        float wy[4], wx[4];
        rs_cubic(ry, m, wy);
        rs_cubic(rx, m, wx);
        v = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float h = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) h = __fmaf_rn(wx[b], d[a][b], h);
            v = __fmaf_rn(wy[a], h, v);
        }
    } else {
        const int wy2[2] = {m - ry, ry}, wx2[2] = {m - rx, rx};
        int s = 0;
        v = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float dd = d[1 + a][1 + b];
                const int w = wy2[a] * wx2[b];
                if (dd == dd) {
                    s += w;
                    v = __fmaf_rn((float)w, dd, v);
                }
            }
        v = __fdiv_rn(v, (float)s);              // s > 0: the containing pixel is one of the four and has a positive weight
    }
    return v == 0.f ? zc : __fadd_rn(zc, v);
}

constexpr int RI_TY = 16, RI_TX = 64;            // output tile; p <= q, so its taps span at most RI_TY + 3 by RI_TX + 3 pixels
constexpr int RI_SH = RI_TY + 3, RI_SW = RI_TX + 3, RI_STRIDE = RI_SW + 1;

__global__ __launch_bounds__(RS_THREADS) void resample_interp_kernel(RasterIn in, RasterIn keep, RsGeom g, int tiles_x,
                                                                     float* __restrict__ out, float* __restrict__ omask,
                                                                     int32_t* __restrict__ n_nan) {
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int Y0 = by * RI_TY, X0 = bx * RI_TX;
    __shared__ float sm[RI_SH * RI_STRIDE];
    int sy0, sx0, r0;
    rs_centre(Y0, g.p, g.q, sy0, r0);
    rs_centre(X0, g.p, g.q, sx0, r0);
    --sy0;                                       // the first tap row and column of the tile, before clamping
    --sx0;
    for (int idx = threadIdx.x; idx < RI_SH * RI_SW; idx += RS_THREADS) {
        const int a = idx / RI_SW, b = idx - a * RI_SW;
        const int sy = min(max(sy0 + a, 0), g.H - 1), sx = min(max(sx0 + b, 0), g.W - 1);
        float z;
        if (!rs_known(in, (int64_t)sy * g.W + sx, z)) z = NAN;
        sm[a * RI_STRIDE + b] = z;
    }
    __syncthreads();
    int miss = 0;
    const int X = X0 + (threadIdx.x & 63);
    for (int Y = Y0 + (threadIdx.x >> 6); Y < min(Y0 + RI_TY, g.Ho); Y += RS_THREADS / 64) {
        if (X >= g.Wo) break;
        const int64_t o = (int64_t)Y * g.Wo + X;
        float kz;
        if (keep.dem && rs_known(keep, o, kz)) {
            if (out) out[o] = kz;                // bit for bit
            if (omask) omask[o] = 1.f;
            continue;
        }
        int fy, ry, fx, rx;
        rs_centre(Y, g.p, g.q, fy, ry);
        rs_centre(X, g.p, g.q, fx, rx);
        const float* t0 = sm + (fy - 1 - sy0) * RI_STRIDE + (fx - 1 - sx0);
        const float val = rs_interp_value([&](int a, int b) { return t0[a * RI_STRIDE + b]; }, ry, rx, g.q);
        const bool kn = val == val;
        if (out) out[o] = val;
        if (omask) omask[o] = kn ? 1.f : 0.f;
        miss += kn ? 0 : 1;
    }
    rs_count_nan(miss, n_nan);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int rs_check(const char* who, const float* dem, int H, int W, int p, int q, int Ho, int Wo, const int32_t* n_nan) {
    TG_REQUIRE(dem && n_nan, "%s: null pointer", who);
    TG_REQUIRE(H > 0 && W > 0, "%s: empty raster %dx%d", who, H, W);
    TG_REQUIRE(p >= 1 && q >= 1 && p <= 1024 && q <= 1024, "%s: scale %d/%d must have 1 <= p, q <= 1024", who, p, q);
    TG_REQUIRE((int64_t)H * q + 2 * (int64_t)p < ((int64_t)1 << 30) && (int64_t)W * q + 2 * (int64_t)p < ((int64_t)1 << 30),
               "%s: raster %dx%d too large at scale %d/%d", who, H, W, p, q);
    const int64_t ho = cdiv64((int64_t)H * q, p), wo = cdiv64((int64_t)W * q, p);
    // a smaller output is the top-left crop of the planned one: the return trip to a native grid needs it
    TG_REQUIRE(Ho >= 1 && Wo >= 1 && Ho <= ho && Wo <= wo, "%s: output %dx%d inconsistent with the plan (at most %lldx%lld)", who, Ho,
               Wo, (long long)ho, (long long)wo);
    TG_REQUIRE((int64_t)H * W < ((int64_t)1 << 40) && ho * wo < ((int64_t)1 << 40), "%s: raster too large", who);
    return TG_OK;
}

static int rs_zero(const char* who, int32_t* n_nan, hipStream_t s) {
    if (hipMemsetAsync(n_nan, 0, sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("%s: hipMemsetAsync failed", who);
        return TG_ERR_LAUNCH;
    }
    return TG_OK;
}

static inline bool rs_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int tg_resample_area(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, int p, int q,
                                int cov_num, int cov_den, const float* keep_dem, const float* keep_mask, int keep_use_nodata,
                                float keep_nodata, int Ho, int Wo, float* out, float* out_mask, int32_t* n_nan,
                                tg_stream_t stream) {
    if (int rc = rs_check("tg_resample_area", dem, H, W, p, q, Ho, Wo, n_nan)) return rc;
    TG_REQUIRE(p >= q && p <= 16 * q, "tg_resample_area: scale %d/%d must be in [1, 16] (tg_resample_interp goes to a finer grid)", p,
               q);
    TG_REQUIRE(cov_den >= 1 && cov_den <= 1000 && cov_num >= 0 && cov_num <= cov_den,
               "tg_resample_area: coverage %d/%d must be in [0, 1] with a denominator in [1, 1000]", cov_num, cov_den);
    TG_REQUIRE(keep_dem || !keep_mask, "tg_resample_area: keep_mask without keep_dem");
    // the largest tile whose footprint, ceil(t p / q) + 1 source pixels per axis (+ 3 of row alignment), fits the LDS budget
    int ty = 16, txl2 = 6, sh = 0, sstride = 0;
    for (;;) {
        sh = (int)cdiv64((int64_t)ty * p, q) + 1;
        sstride = (((int)cdiv64((int64_t)(1 << txl2) * p, q) + 1 + 3) + 3) & ~3;
        if ((int64_t)sh * sstride <= RS_LDS_FLOATS) break;
        if (ty > 1) ty >>= 1;
        else --txl2;                             // 17 x 24 floats at one output pixel and p / q = 16: always reached
    }
    const int tiles_x = cdiv(Wo, 1 << txl2);
    const int64_t tiles = (int64_t)cdiv(Ho, ty) * tiles_x;
    TG_REQUIRE(tiles < ((int64_t)1 << 31), "tg_resample_area: too many tiles");
    if (int rc = rs_zero("tg_resample_area", n_nan, S(stream))) return rc;
    const RasterIn in{dem, mask, use_nodata, nodata}, keep{keep_dem, keep_mask, keep_use_nodata, keep_nodata};
    const RsGeom g{H, W, Ho, Wo, p, q};
    const int vec_ok = rs_al16(dem) && (!mask || rs_al16(mask));
    hipLaunchKernelGGL(resample_area_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), (size_t)sh * sstride * sizeof(float), S(stream),
                       in, keep, g, ty, txl2, tiles_x, sstride, cov_num, cov_den, vec_ok, out, out_mask, n_nan);
    TG_CHECK_LAUNCH("resample_area_kernel");
    return TG_OK;
}

extern "C" int tg_resample_interp(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, int p, int q,
                                  const float* keep_dem, const float* keep_mask, int keep_use_nodata, float keep_nodata, int Ho,
                                  int Wo, float* out, float* out_mask, int32_t* n_nan, tg_stream_t stream) {
    if (int rc = rs_check("tg_resample_interp", dem, H, W, p, q, Ho, Wo, n_nan)) return rc;
    TG_REQUIRE(p <= q && 16 * p >= q, "tg_resample_interp: scale %d/%d must be in [1/16, 1] (tg_resample_area goes to a coarser grid)",
               p, q);
    TG_REQUIRE(keep_dem || !keep_mask, "tg_resample_interp: keep_mask without keep_dem");
    const int tiles_x = cdiv(Wo, RI_TX);
    const int64_t tiles = (int64_t)cdiv(Ho, RI_TY) * tiles_x;
    TG_REQUIRE(tiles < ((int64_t)1 << 31), "tg_resample_interp: too many tiles");
    if (int rc = rs_zero("tg_resample_interp", n_nan, S(stream))) return rc;
    const RasterIn in{dem, mask, use_nodata, nodata}, keep{keep_dem, keep_mask, keep_use_nodata, keep_nodata};
    const RsGeom g{H, W, Ho, Wo, p, q};
    hipLaunchKernelGGL(resample_interp_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), 0, S(stream), in, keep, g, tiles_x, out,
                       out_mask, n_nan);
    TG_CHECK_LAUNCH("resample_interp_kernel");
    return TG_OK;
}
