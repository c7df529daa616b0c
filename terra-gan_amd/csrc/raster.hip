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

// ==== test-time augmentation: the windows under the flips and rotations of the square (inpaint_raster(tta=...)) =============
//
//   tg_raster_gather_ops     tg_raster_gather with a transform per list item, written in the member's frame
//   tg_raster_tta_reduce     undoes each member's transform: per window pixel the mean and the sample variance of the members
//   tg_raster_blend_tta      tg_raster_blend of the means (bitwise) plus the spread map in metres
//
// Encoding of raster_train.hip (src_of): member pixel (i, j) reads window pixel (a, b) = op & 4 ? (j, i) : (i, j), then
// a = wh-1-a if op & 2, b = ww-1-b if op & 1.  Ops 4..7 transpose and need wh == ww, so a member frame is always [wh][ww].
// Both kernels walk 64 x 64 tiles and pass what a transposed read would fetch column-wise through LDS (rows of 64 + 1
// floats, as stage_tile does): every global read and write is row-contiguous for all eight ops.
constexpr int TT_TILE = 64;
constexpr int TT_THREADS = 256;
constexpr int TT_ROWS = TT_THREADS / 64;         // tile rows in flight per pass
constexpr int TT_SLICE = 2048;                   // list items per gather launch: their ops travel as kernel arguments

struct TtaItemOps { uint32_t w[TT_SLICE / 8]; };  // 4 bits per item
struct TtaMemberOps { int op[8]; };

__device__ __forceinline__ void tt_src_of(int op, int wh, int ww, int i, int j, int& a, int& b) {
    a = (op & 4) ? j : i;
    b = (op & 4) ? i : j;
    if (op & 2) a = wh - 1 - a;
    if (op & 1) b = ww - 1 - b;
}

// the rectangle of window pixels that the member tile [i0, i1] x [j0, j1] reads: origin (a0, b0), na x nb <= 64 x 64
__device__ __forceinline__ void tt_src_rect(int op, int wh, int ww, int i0, int i1, int j0, int j1, int& a0, int& b0, int& na,
                                            int& nb) {
    int aa, ab, ba, bb;
    tt_src_of(op, wh, ww, i0, j0, aa, ab);
    tt_src_of(op, wh, ww, i1, j1, ba, bb);
    a0 = min(aa, ba); b0 = min(ab, bb);
    na = max(aa, ba) - a0 + 1; nb = max(ab, bb) - b0 + 1;
}

// ---- gather with a transform: grid.x = member tile, grid.y = list item ---------------------------------------------------
__global__ __launch_bounds__(TT_THREADS) void raster_gather_ops_kernel(RasterIn in, TgRasterPlan p, int sy, int sx,
                                                                       const float* __restrict__ lo, const float* __restrict__ hi,
                                                                       const int32_t* __restrict__ win_idx, TtaItemOps ops,
                                                                       int tiles_x, float* __restrict__ xo, float* __restrict__ mo) {
    __shared__ float tx[TT_TILE][TT_TILE + 1], tm[TT_TILE][TT_TILE + 1];
    const int k = blockIdx.y;
    const int win = win_idx[k];
    const int op = (ops.w[k >> 3] >> ((k & 7) * 4)) & 7;
    const int64_t npx = (int64_t)p.wh * p.ww;
    float* xw = xo + (int64_t)k * npx;
    float* mw = mo + (int64_t)k * npx;
    const bool valid = win >= 0 && win < p.ny * p.nx;
    const int iy = valid ? win / p.nx : 0, ix = valid ? win - iy * p.nx : 0;
    const int y0 = rs_start(iy, p.H, p.wh, sy), x0 = rs_start(ix, p.W, p.ww, sx);
    const float l = valid ? lo[win] : 0.f, h = valid ? hi[win] : 0.f;
    const float d = __fsub_rn(h, l);
    const int ty = blockIdx.x / tiles_x, tx_ = blockIdx.x - ty * tiles_x;
    const int i0 = ty * TT_TILE, j0 = tx_ * TT_TILE;
    const int i1 = min(i0 + TT_TILE, p.wh) - 1, j1 = min(j0 + TT_TILE, p.ww) - 1;
    int a0, b0, na, nb;
    tt_src_rect(op, p.wh, p.ww, i0, i1, j0, j1, a0, b0, na, nb);
    const int c = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < na; r += TT_ROWS) {
        if (c >= nb) continue;
        float z;
        const bool kn = valid && rs_known(in, (int64_t)(y0 + a0 + r) * p.W + x0 + b0 + c, z);
        tx[r][c] = (kn && h != l) ? __fdiv_rn(__fsub_rn(z, l), d) : 0.f;       // the value tg_raster_gather writes
        tm[r][c] = kn ? 1.f : 0.f;
    }
    __syncthreads();
    const int j = j0 + c;
    for (int r = threadIdx.x >> 6; r < TT_TILE; r += TT_ROWS) {
        const int i = i0 + r;
        if (i > i1 || j > j1) continue;
        int sa, sb;
        tt_src_of(op, p.wh, p.ww, i, j, sa, sb);
        xw[(int64_t)i * p.ww + j] = tx[sa - a0][sb - b0];
        mw[(int64_t)i * p.ww + j] = tm[sa - a0][sb - b0];
    }
}

// ---- reduce: grid.x = window tile, grid.y = window; T members held in registers, summed in member order -------------------
// Window pixel (a, b) is member pixel (i, j) with, for a plain op, i = a or wh-1-a and j = b or ww-1-b (a row read, possibly
// reversed), and for a transposing op j = a or wh-1-a and i = b or ww-1-b (the member tile goes through LDS).
template <int T>
__global__ __launch_bounds__(TT_THREADS) void raster_tta_reduce_kernel(const float* __restrict__ gout, TtaMemberOps ops, int wh,
                                                                       int ww, int tiles_x, float* __restrict__ mean,
                                                                       float* __restrict__ var) {
    __shared__ float t[TT_TILE][TT_TILE + 1];
    constexpr int NP = TT_TILE / TT_ROWS;                      // window pixels per thread
    const int64_t npx = (int64_t)wh * ww;
    const float* gw = gout + (int64_t)blockIdx.y * T * npx;
    const int ty = blockIdx.x / tiles_x, tx_ = blockIdx.x - ty * tiles_x;
    const int a0 = ty * TT_TILE, b0 = tx_ * TT_TILE;
    const int a1 = min(a0 + TT_TILE, wh) - 1, b1 = min(b0 + TT_TILE, ww) - 1;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int b = b0 + c;
    float v[NP][T];
#pragma unroll
    for (int m = 0; m < T; ++m) {
        const int op = ops.op[m];
        const float* g = gw + (int64_t)m * npx;
        if (op & 4) {
            // member rows i <- window columns [b0, b1], member columns j <- window rows [a0, a1]
            const int ilo = (op & 1) ? ww - 1 - b1 : b0, jlo = (op & 2) ? wh - 1 - a1 : a0;
            const int ni = b1 - b0 + 1, nj = a1 - a0 + 1;
            __syncthreads();                                   // the previous member's reads of t are done
            for (int r = r0; r < ni; r += TT_ROWS)
                if (c < nj) t[r][c] = g[(int64_t)(ilo + r) * ww + jlo + c];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int a = a0 + r0 + q * TT_ROWS;
                float o = 0.f;
                if (a <= a1 && b <= b1) {
                    const int j = (op & 2) ? wh - 1 - a : a, i = (op & 1) ? ww - 1 - b : b;
                    o = t[i - ilo][j - jlo];
                }
                v[q][m] = o;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int a = a0 + r0 + q * TT_ROWS;
                float o = 0.f;
                if (a <= a1 && b <= b1) {
                    const int i = (op & 2) ? wh - 1 - a : a, j = (op & 1) ? ww - 1 - b : b;
                    o = g[(int64_t)i * ww + j];
                }
                v[q][m] = o;
            }
        }
    }
    float* mn = mean + (int64_t)blockIdx.y * npx;
    float* vr = var + (int64_t)blockIdx.y * npx;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int a = a0 + r0 + q * TT_ROWS;
        if (a > a1 || b > b1) continue;
        float s = v[q][0];
#pragma unroll
        for (int m = 1; m < T; ++m) s = __fadd_rn(s, v[q][m]);
        const float mu = __fmul_rn(s, 1.f / T);                // 1 / T is a power of two: exact
        float e = __fsub_rn(v[q][0], mu);
        float ss = __fmul_rn(e, e);
#pragma unroll
        for (int m = 1; m < T; ++m) {
            e = __fsub_rn(v[q][m], mu);
            ss = __fadd_rn(ss, __fmul_rn(e, e));
        }
        mn[(int64_t)a * ww + b] = mu;
        vr[(int64_t)a * ww + b] = __fdiv_rn(ss, (float)(T - 1));
    }
}

// ---- blend of the means with the spread: raster_blend_kernel's walk, then a second one for the mixture's variance ----------
__global__ __launch_bounds__(256) void raster_blend_tta_kernel(RasterIn in, TgRasterPlan p, int sy, int sx,
                                                               const float* __restrict__ lo, const float* __restrict__ hi,
                                                               const int32_t* __restrict__ run_of, const float* __restrict__ wmean,
                                                               const float* __restrict__ wvar, int n_run, float* __restrict__ out,
                                                               float* __restrict__ spread, int32_t* __restrict__ unfilled) {
    __shared__ int sred[4];
    const int x = blockIdx.x * 256 + threadIdx.x;
    int miss = 0;
    for (int y = blockIdx.y; y < p.H; y += gridDim.y) {
        if (x >= p.W) continue;
        const int64_t i = (int64_t)y * p.W + x;
        float z;
        if (rs_known(in, i, z)) {
            out[i] = z;                      // known pixels pass through bit for bit
            spread[i] = 0.f;
            continue;
        }
        int ay, by, ax, bx;
        rs_cover(y, p.H, p.wh, sy, p.ny, ay, by);
        rs_cover(x, p.W, p.ww, sx, p.nx, ax, bx);
        // first walk: the operations of raster_blend_kernel in its order
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
                const float o = wmean[((int64_t)k * p.wh + ty) * p.ww + tx];
                const float dn = __fmaf_rn(o, __fsub_rn(h, l), l);         // lo + mean * (hi - lo)
                num = __fmaf_rn(wgt, dn, num);
                den += wgt;
            }
        }
        if (!(den > 0.f)) {
            out[i] = NAN;
            spread[i] = NAN;
            ++miss;
            continue;
        }
        const float o_px = __fdiv_rn(num, den);
        out[i] = o_px;
        // second walk: sum_j w_j (var_j d_j^2 + (dn_j - out)^2), the disagreement taken as a difference of heights, not of squares
        float acc = 0.f;
        for (int iy = ay; iy <= by; ++iy) {
            const int wy0 = rs_start(iy, p.H, p.wh, sy), ty = y - wy0;
            const float ry = rs_ramp(ty, p.wh, p.overlap, wy0 == 0, wy0 + p.wh == p.H);
            for (int ix = ax; ix <= bx; ++ix) {
                const int win = iy * p.nx + ix;
                const int k = run_of[win];
                if (k < 0 || k >= n_run) continue;
                const int wx0 = rs_start(ix, p.W, p.ww, sx), tx = x - wx0;
                const float wgt = __fmul_rn(ry, rs_ramp(tx, p.ww, p.overlap, wx0 == 0, wx0 + p.ww == p.W));
                const float l = lo[win], h = hi[win];
                const int64_t q = ((int64_t)k * p.wh + ty) * p.ww + tx;
                const float d = __fsub_rn(h, l);
                const float e = __fsub_rn(__fmaf_rn(wmean[q], d, l), o_px);
                const float within = __fmul_rn(wvar[q], __fmul_rn(d, d));
                acc = __fmaf_rn(wgt, __fmaf_rn(e, e, within), acc);
            }
        }
        spread[i] = __fsqrt_rn(__fdiv_rn(acc, den));
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

// ---- host side of the augmentation -----------------------------------------------------------------------------------------
static int op_check(const char* who, int op, const TgRasterPlan* p) {
    TG_REQUIRE(op >= 0 && op <= 7, "%s: op %d out of range [0, 7]", who, op);
    TG_REQUIRE(!(op & 4) || p->wh == p->ww, "%s: op %d transposes and needs a square window, got %dx%d", who, op, p->wh, p->ww);
    return TG_OK;
}

extern "C" int tg_raster_gather_ops(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                                    const float* lo, const float* hi, const int32_t* win_idx, const int32_t* op_idx, int n, float* x,
                                    float* m, tg_stream_t stream) {
    int sy, sx;
    if (int rc = plan_check("tg_raster_gather_ops", plan, sy, sx)) return rc;
    TG_REQUIRE(dem && lo && hi && win_idx && op_idx && x && m, "tg_raster_gather_ops: null pointer");
    TG_REQUIRE(n > 0 && n <= 65535, "tg_raster_gather_ops: item count %d out of range [1, 65535]", n);
    for (int k = 0; k < n; ++k)
        if (int rc = op_check("tg_raster_gather_ops", op_idx[k], plan)) return rc;
    const RasterIn in{dem, mask, use_nodata, nodata};
    const int64_t npx = (int64_t)plan->wh * plan->ww;
    const int tiles_y = cdiv(plan->wh, TT_TILE), tiles_x = cdiv(plan->ww, TT_TILE);
    for (int k0 = 0; k0 < n; k0 += TT_SLICE) {
        const int nk = n - k0 < TT_SLICE ? n - k0 : TT_SLICE;
        TtaItemOps ops{};
        for (int k = 0; k < nk; ++k) ops.w[k >> 3] |= (uint32_t)op_idx[k0 + k] << ((k & 7) * 4);
        hipLaunchKernelGGL(raster_gather_ops_kernel, dim3(tiles_y * tiles_x, nk), dim3(TT_THREADS), 0, S(stream), in, *plan, sy, sx,
                           lo, hi, win_idx + k0, ops, tiles_x, x + k0 * npx, m + k0 * npx);
        TG_CHECK_LAUNCH("raster_gather_ops_kernel");
    }
    return TG_OK;
}

extern "C" int tg_raster_tta_reduce(const float* gout, const int32_t* ops, int T, int n, int wh, int ww, float* mean, float* var,
                                    tg_stream_t stream) {
    TG_REQUIRE(T == 2 || T == 4 || T == 8, "tg_raster_tta_reduce: T %d must be 2, 4 or 8", T);
    TG_REQUIRE(gout && ops && mean && var, "tg_raster_tta_reduce: null pointer");
    TG_REQUIRE(n > 0 && n <= 65535, "tg_raster_tta_reduce: window count %d out of range [1, 65535]", n);
    TG_REQUIRE(wh > 0 && ww > 0 && wh <= 32768 && ww <= 32768, "tg_raster_tta_reduce: bad window %dx%d", wh, ww);
    TtaMemberOps mo{};
    for (int t = 0; t < T; ++t) {
        TG_REQUIRE(ops[t] >= 0 && ops[t] <= 7, "tg_raster_tta_reduce: op %d out of range [0, 7]", ops[t]);
        TG_REQUIRE(!(ops[t] & 4) || wh == ww, "tg_raster_tta_reduce: op %d transposes and needs a square window, got %dx%d", ops[t],
                   wh, ww);
        mo.op[t] = ops[t];
    }
    const int tiles_y = cdiv(wh, TT_TILE), tiles_x = cdiv(ww, TT_TILE);
    const dim3 grid(tiles_y * tiles_x, n), block(TT_THREADS);
    if (T == 2) hipLaunchKernelGGL(raster_tta_reduce_kernel<2>, grid, block, 0, S(stream), gout, mo, wh, ww, tiles_x, mean, var);
    else if (T == 4) hipLaunchKernelGGL(raster_tta_reduce_kernel<4>, grid, block, 0, S(stream), gout, mo, wh, ww, tiles_x, mean, var);
    else hipLaunchKernelGGL(raster_tta_reduce_kernel<8>, grid, block, 0, S(stream), gout, mo, wh, ww, tiles_x, mean, var);
    TG_CHECK_LAUNCH("raster_tta_reduce_kernel");
    return TG_OK;
}

extern "C" int tg_raster_blend_tta(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                                   const float* lo, const float* hi, const int32_t* run_of_window, const float* wmean,
                                   const float* wvar, int n_run, float* out, float* spread, int32_t* unfilled, tg_stream_t stream) {
    int sy, sx;
    if (int rc = plan_check("tg_raster_blend_tta", plan, sy, sx)) return rc;
    TG_REQUIRE(dem && lo && hi && run_of_window && out && spread && unfilled && ((wmean && wvar) || n_run == 0),
               "tg_raster_blend_tta: null pointer");
    TG_REQUIRE(n_run >= 0 && n_run <= plan->ny * plan->nx, "tg_raster_blend_tta: n_run %d out of range", n_run);
    const RasterIn in{dem, mask, use_nodata, nodata};
    if (hipMemsetAsync(unfilled, 0, sizeof(int32_t), S(stream)) != hipSuccess) {
        tg_set_error("tg_raster_blend_tta: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int gy = plan->H < 4096 ? plan->H : 4096;
    hipLaunchKernelGGL(raster_blend_tta_kernel, dim3(cdiv(plan->W, 256), gy), dim3(256), 0, S(stream), in, *plan, sy, sx, lo, hi,
                       run_of_window, wmean, wvar, n_run, out, spread, unfilled);
    TG_CHECK_LAUNCH("raster_blend_tta_kernel");
    return TG_OK;
}
