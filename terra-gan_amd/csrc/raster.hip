// Whole-raster inpainting around the generator: overlapping windows are cut from a float32 DSM, min-max normalised over
// their known pixels, run through the generator in batches, and blended back in metres (mvp_gan/src/inpaint_raster.py).
//
//   tg_raster_window_stats   per window: lo / hi over its known pixels, known count, hole count (one workgroup per window)
//   tg_raster_gather         normalised network input x = (z - lo) / (hi - lo) and mask for a list of windows
//   tg_raster_blend          gather-form composite: one thread per raster pixel, its covering windows derived from the plan,
//                            weights summed in a fixed order (window row, then column) -- bitwise deterministic, no atomics
//                            on the raster (one integer atomic per workgroup for the unfilled-pixel count)
//
// The plan is regular: per axis the window starts are min(i * s, N - w), i = 0 .. n - 1, s = w - overlap,
// n = ceil((N - w) / s) + 1 (no duplicates: (n - 2) * s < N - w).  The kernels derive every start from that formula.
#include <math.h>

#include "common.h"
#include "raster_known.h"                // RasterIn, rs_known

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

__device__ __forceinline__ int rs_start(int i, int N, int w, int s) { return min(i * s, N - w); }

// window indices [a, b] along one axis that cover coordinate y (a contiguous range: starts are nondecreasing)
__device__ __forceinline__ void rs_cover(int y, int N, int w, int s, int n, int& a, int& b) {
    b = y >= N - w ? n - 1 : y / s;
    a = b;
    while (a > 0 && rs_start(a - 1, N, w, s) + w > y) --a;
}

// 1-D blend weight at offset t of a window of side w: min(1, (t+0.5)/ov, (w-t-0.5)/ov); a ramp on a raster border side is 1
__device__ __forceinline__ float rs_ramp(int t, int w, int ov, bool first, bool last) {
    if (ov == 0) return 1.f;
    float r = 1.f;
    if (!first) r = fminf(r, __fdiv_rn((float)t + 0.5f, (float)ov));
    if (!last) r = fminf(r, __fdiv_rn((float)(w - t) - 0.5f, (float)ov));
    return r;
}

// ---- stats: one 1024-thread workgroup per window; each wave walks rows, lanes walk columns (coalesced) -------------------
constexpr int ST_THREADS = 1024;
constexpr int ST_WAVES = ST_THREADS / 64;

__global__ __launch_bounds__(ST_THREADS) void raster_stats_kernel(RasterIn in, TgRasterPlan p, int sy, int sx,
                                                                  float* __restrict__ lo, float* __restrict__ hi,
                                                                  int32_t* __restrict__ counts) {
    __shared__ float smin[ST_WAVES], smax[ST_WAVES];
    __shared__ int skn[ST_WAVES], shole[ST_WAVES];
    const int win = blockIdx.x;
    const int iy = win / p.nx, ix = win - iy * p.nx;
    const int y0 = rs_start(iy, p.H, p.wh, sy), x0 = rs_start(ix, p.W, p.ww, sx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn = INFINITY, mx = -INFINITY;
    int kn = 0, hole = 0;
    for (int r = wave; r < p.wh; r += ST_WAVES) {
        const int64_t row = (int64_t)(y0 + r) * p.W + x0;
        for (int c = lane; c < p.ww; c += 64) {
            float z;
            if (rs_known(in, row + c, z)) {
                mn = fminf(mn, z);
                mx = fmaxf(mx, z);
                ++kn;
            } else {
                ++hole;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        kn += __shfl_xor(kn, o, 64);
        hole += __shfl_xor(hole, o, 64);
    }
    if (lane == 0) {
        smin[wave] = mn; smax[wave] = mx; skn[wave] = kn; shole[wave] = hole;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ST_WAVES; ++w) {
            mn = fminf(mn, smin[w]); mx = fmaxf(mx, smax[w]); kn += skn[w]; hole += shole[w];
        }
        // + 0.f turns a -0 extreme into +0, so lo / hi (and z - lo) do not depend on which zero the min met first
        lo[win] = kn ? mn + 0.f : 0.f;
        hi[win] = kn ? mx + 0.f : 0.f;
        counts[2 * win] = kn;
        counts[2 * win + 1] = hole;
    }
}

// ---- gather: grid.y = window of the list, grid.x strides over its wh * ww pixels ----------------------------------------
__global__ __launch_bounds__(256) void raster_gather_kernel(RasterIn in, TgRasterPlan p, int sy, int sx,
                                                            const float* __restrict__ lo, const float* __restrict__ hi,
                                                            const int32_t* __restrict__ win_idx, float* __restrict__ xo,
                                                            float* __restrict__ mo) {
    const int j = blockIdx.y;
    const int win = win_idx[j];
    const int64_t npx = (int64_t)p.wh * p.ww;
    float* xw = xo + (int64_t)j * npx;
    float* mw = mo + (int64_t)j * npx;
    const bool valid = win >= 0 && win < p.ny * p.nx;
    const int iy = valid ? win / p.nx : 0, ix = valid ? win - iy * p.nx : 0;
    const int y0 = rs_start(iy, p.H, p.wh, sy), x0 = rs_start(ix, p.W, p.ww, sx);
    const float l = valid ? lo[win] : 0.f, h = valid ? hi[win] : 0.f;
    const float d = __fsub_rn(h, l);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / p.ww), c = (int)(i - (int64_t)r * p.ww);
        float z;
        const bool k = valid && rs_known(in, (int64_t)(y0 + r) * p.W + x0 + c, z);
        xw[i] = (k && h != l) ? __fdiv_rn(__fsub_rn(z, l), d) : 0.f;
        mw[i] = k ? 1.f : 0.f;
    }
}

// ---- blend: grid.x covers a row (256 pixels per workgroup), grid.y strides over rows ------------------------------------
__global__ __launch_bounds__(256) void raster_blend_kernel(RasterIn in, TgRasterPlan p, int sy, int sx,
                                                           const float* __restrict__ lo, const float* __restrict__ hi,
                                                           const int32_t* __restrict__ run_of, const float* __restrict__ wout,
                                                           int n_run, float* __restrict__ out, int32_t* __restrict__ unfilled) {
    __shared__ int sred[4];
    const int x = blockIdx.x * 256 + threadIdx.x;
    int miss = 0;
    for (int y = blockIdx.y; y < p.H; y += gridDim.y) {
        if (x >= p.W) continue;
        const int64_t i = (int64_t)y * p.W + x;
        float z;
        if (rs_known(in, i, z)) {
            out[i] = z;                      // known pixels pass through bit for bit
            continue;
        }
        int ay, by, ax, bx;
        rs_cover(y, p.H, p.wh, sy, p.ny, ay, by);
        rs_cover(x, p.W, p.ww, sx, p.nx, ax, bx);
        float num = 0.f, den = 0.f;
        for (int iy = ay; iy <= by; ++iy) {
            const int wy0 = rs_start(iy, p.H, p.wh, sy), ty = y - wy0;
            const float ry = rs_ramp(ty, p.wh, p.overlap, wy0 == 0, wy0 + p.wh == p.H);
            for (int ix = ax; ix <= bx; ++ix) {
                const int win = iy * p.nx + ix;
                const int k = run_of[win];
                if (k < 0 || k >= n_run) continue;
                const int wx0 = rs_start(ix, p.W, p.ww, sx), tx = x - wx0;
                const float wgt = ry * rs_ramp(tx, p.ww, p.overlap, wx0 == 0, wx0 + p.ww == p.W);
                const float l = lo[win], h = hi[win];
                const float o = wout[((int64_t)k * p.wh + ty) * p.ww + tx];
                const float dn = __fmaf_rn(o, __fsub_rn(h, l), l);         // lo + out * (hi - lo)
                num = __fmaf_rn(wgt, dn, num);
                den += wgt;
            }
        }
        if (den > 0.f) {
            out[i] = __fdiv_rn(num, den);
        } else {
            out[i] = NAN;
            ++miss;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) miss += __shfl_xor(miss, o, 64);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = miss;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = sred[0] + sred[1] + sred[2] + sred[3];
        if (t) atomicAdd(unfilled, t);       // integer: the total does not depend on the order
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int plan_check(const char* who, const TgRasterPlan* p, int& sy, int& sx) {
    TG_REQUIRE(p, "%s: null plan", who);
    TG_REQUIRE(p->H > 0 && p->W > 0 && (int64_t)p->H * p->W < ((int64_t)1 << 40), "%s: bad raster size %dx%d", who, p->H, p->W);
    TG_REQUIRE(p->wh > 0 && p->wh <= p->H && p->ww > 0 && p->ww <= p->W, "%s: window %dx%d does not fit the raster %dx%d", who,
               p->wh, p->ww, p->H, p->W);
    TG_REQUIRE(p->overlap >= 0 && p->overlap < p->wh && p->overlap < p->ww, "%s: overlap %d must be in [0, window side)", who,
               p->overlap);
    sy = p->wh - p->overlap;
    sx = p->ww - p->overlap;
    const int ny = (p->H - p->wh + sy - 1) / sy + 1, nx = (p->W - p->ww + sx - 1) / sx + 1;
    TG_REQUIRE(p->ny == ny && p->nx == nx, "%s: window grid %dx%d inconsistent with the plan (expected %dx%d)", who, p->ny, p->nx,
               ny, nx);
    TG_REQUIRE((int64_t)ny * nx < ((int64_t)1 << 31), "%s: too many windows", who);
    return TG_OK;
}

extern "C" int tg_raster_window_stats(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                                      float* lo, float* hi, int32_t* counts, tg_stream_t stream) {
    int sy, sx;
    if (int rc = plan_check("tg_raster_window_stats", plan, sy, sx)) return rc;
    TG_REQUIRE(dem && lo && hi && counts, "tg_raster_window_stats: null pointer");
    const RasterIn in{dem, mask, use_nodata, nodata};
    hipLaunchKernelGGL(raster_stats_kernel, dim3(plan->ny * plan->nx), dim3(ST_THREADS), 0, S(stream), in, *plan, sy, sx, lo, hi,
                       counts);
    TG_CHECK_LAUNCH("raster_stats_kernel");
    return TG_OK;
}

extern "C" int tg_raster_gather(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                                const float* lo, const float* hi, const int32_t* win_idx, int n, float* x, float* m,
                                tg_stream_t stream) {
    int sy, sx;
    if (int rc = plan_check("tg_raster_gather", plan, sy, sx)) return rc;
    TG_REQUIRE(dem && lo && hi && win_idx && x && m, "tg_raster_gather: null pointer");
    TG_REQUIRE(n > 0 && n <= 65535, "tg_raster_gather: window count %d out of range [1, 65535]", n);
    const RasterIn in{dem, mask, use_nodata, nodata};
    const int64_t npx = (int64_t)plan->wh * plan->ww;
    const int gx = (int)(cdiv64(npx, 256) < 256 ? cdiv64(npx, 256) : 256);
    hipLaunchKernelGGL(raster_gather_kernel, dim3(gx, n), dim3(256), 0, S(stream), in, *plan, sy, sx, lo, hi, win_idx, x, m);
    TG_CHECK_LAUNCH("raster_gather_kernel");
    return TG_OK;
}

extern "C" int tg_raster_blend(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                               const float* lo, const float* hi, const int32_t* run_of_window, const float* wout, int n_run,
                               float* out, int32_t* unfilled, tg_stream_t stream) {
    int sy, sx;
    if (int rc = plan_check("tg_raster_blend", plan, sy, sx)) return rc;
    TG_REQUIRE(dem && lo && hi && run_of_window && out && unfilled && (wout || n_run == 0), "tg_raster_blend: null pointer");
    TG_REQUIRE(n_run >= 0 && n_run <= plan->ny * plan->nx, "tg_raster_blend: n_run %d out of range", n_run);
    const RasterIn in{dem, mask, use_nodata, nodata};
    if (hipMemsetAsync(unfilled, 0, sizeof(int32_t), S(stream)) != hipSuccess) {
        tg_set_error("tg_raster_blend: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int gy = plan->H < 4096 ? plan->H : 4096;
    hipLaunchKernelGGL(raster_blend_kernel, dim3(cdiv(plan->W, 256), gy), dim3(256), 0, S(stream), in, *plan, sy, sx, lo, hi,
                       run_of_window, wout, n_run, out, unfilled);
    TG_CHECK_LAUNCH("raster_blend_kernel");
    return TG_OK;
}
