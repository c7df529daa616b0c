// Depression filling (pit removal) of a raster (mvp_gan/src/fill_depressions.py).
//
// For every known pixel p, W(p) = min over c-connected paths of known pixels from p to an outlet of the max of z along the path
// (c = 8 or 4; an outlet is a known pixel on the raster's edge or with an unknown c-neighbour).  W is the smallest fixed point of
//     W(p) <- max(z(p), min(W(p), min over the c-neighbours n of W(n)))
// below the start W = z at the outlets, +inf elsewhere.  Only comparisons, fminf and fmaxf of fp32 values occur, so the result
// is exact, independent of the order of the updates and bitwise equal to a priority-flood.
//
//   depfill_init_kernel    W = z at outlets, +inf at the other known pixels, NaN at unknown ones
//   sweep_begin_kernel     (raster_sweep.h) one thread: zero `changed`, advance the sweep counter by n
//   depfill_sweep_kernel   one workgroup per 64x64 tile: z and W with a one-pixel halo in LDS, relaxed to a local fixed point
//                          by directional line scans (down, up, right, left), written back if anything was lowered
//   depfill_stats_kernel   counts, the fp64 depth sum and the largest depth: per-workgroup partials in a fixed order
//   depfill_stats_finish_kernel  the partials in one ordered pass
//   depfill_finish_kernel  out, depth, flags
//
// The tile-sweep protocol (one W plane in place, stale halos, the dirty planes, the line scans) is raster_sweep.h's; here an old and
// a new W of a pixel are both upper bounds of the answer.
//
// Determinism: the raster is the unique fixed point.  Integer atomics only (`changed`, `visits`); the fp64 sum is taken in a
// fixed order.  The number of sweeps and visits may differ between runs.
#include <math.h>

#include "raster_sweep.h"

// The fp64 depth sums are compared with a reference that does not fuse: no multiply-add contraction in this file.
#pragma clang fp contract(off)

constexpr int DF_T = SW_T, DF_R = SW_R, DF_S = SW_S;
constexpr int DF_ROUNDS = 64;            // cap on the inner rounds of one visit; a tile that hits it stays dirty
constexpr int DF_STAT_PIX = 4096;        // pixels per workgroup of the statistics
constexpr int DF_STAT_MAX_BLOCKS = 1024;
constexpr int DF_STAT_WORDS = 5;         // per workgroup: sum, max (double); raised, unreached, counted (int64)

struct DfLayout : SweepLayout {
    size_t stats, total;
    int nstat;
};

static DfLayout df_layout(int H, int W) {
    DfLayout L;
    size_t o;
    static_cast<SweepLayout&>(L) = sweep_layout(H, W, o);
    int64_t nb = cdiv64((int64_t)H * W, DF_STAT_PIX);
    L.nstat = (int)(nb > DF_STAT_MAX_BLOCKS ? DF_STAT_MAX_BLOCKS : nb);
    L.stats = o; o += al256((size_t)L.nstat * DF_STAT_WORDS * 8);
    L.total = o;
    return L;
}

__device__ __forceinline__ float df_inf() { return __uint_as_float(0x7f800000u); }
__device__ __forceinline__ float df_nan() { return __uint_as_float(0x7fc00000u); }

// ---- init ---------------------------------------------------------------------------------------------------------------
template <int CONN>
__global__ __launch_bounds__(256) void depfill_init_kernel(const float* __restrict__ z, const uint8_t* __restrict__ known, int H,
                                                           int W, float* __restrict__ w) {
    const int64_t n = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!known[p]) {
            w[p] = df_nan();
            continue;
        }
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        bool outlet = y == 0 || x == 0 || y == H - 1 || x == W - 1;
        if (!outlet) {                                              // all eight neighbours are inside the raster
            outlet = !known[p - W] || !known[p + W] || !known[p - 1] || !known[p + 1];
            if (CONN == 8) outlet = outlet || !known[p - W - 1] || !known[p - W + 1] || !known[p + W - 1] || !known[p + W + 1];
        }
        w[p] = outlet ? z[p] : df_inf();
    }
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------
template <int CONN>
__global__ __launch_bounds__(256) void depfill_sweep_kernel(const float* __restrict__ z, const uint8_t* __restrict__ known, int H,
                                                            int W, int tiles_y, int tiles_x, float* w,
                                                            const int32_t* __restrict__ ctl, int n, int j, uint8_t* plane0,
                                                            uint8_t* plane1, int32_t* changed, ull* visits) {
    __shared__ float zs[DF_R * DF_S];
    __shared__ float ws[DF_R * DF_S];
    SweepVisit v = sweep_visit_begin(ctl, n, j, plane0, plane1);
    if (!v.marked) return;                                          // uniform: a clean tile
    sweep_visit_place(v, tiles_x);
    const int t = threadIdx.x;
    const int y0 = v.y0, x0 = v.x0;
    const float inf = df_inf();

    // stage: unknown and out-of-raster positions hold +inf in both images, so the loop below has no bounds or mask tests
    for (int i = t; i < DF_R * DF_R; i += 256) {
        const SweepStage g = sweep_stage(i, y0, x0, H, W);
        float wv = inf, zz = inf;
        if (g.in_raster) {
            const int64_t p = (int64_t)g.gy * W + g.gx;
            if (g.interior()) {
                wv = w[p];
                if (known[p]) zz = z[p];
            } else {
                wv = __hip_atomic_load(w + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (!(wv == wv)) wv = inf;                              // NaN: an unknown pixel
        }
        ws[g.ly * DF_S + g.lx] = wv;
        zs[g.ly * DF_S + g.lx] = zz;
    }
    __syncthreads();

    // relax by the line scans of raster_sweep.h: thread = one line and one band of 16 pixels along it; the three values across
    // the line are carried from pixel to pixel, so a pixel costs three new W reads and one z read.  A value read may be a
    // neighbour's old or new one: both are upper bounds, and the last round, in which nobody writes, sees final values.
    const int line = t & 63, band = t >> 6;
    const bool line_rim = line == 0 || line == DF_T - 1;
    int any = 0, rim = 0, round = 0, live = 1;
    for (; round < DF_ROUNDS && live; ++round) {
        const int dir = round & 3;
        const int back = dir & 1;
        int c = band * 16 + (back ? 15 : 0);                        // coordinate along the line
        const int sgn = back ? -1 : 1;
        int ds, dp, idx;
        if (dir < 2) { ds = sgn * DF_S; dp = 1; idx = (c + 1) * DF_S + line + 1; }
        else         { ds = sgn; dp = DF_S; idx = (line + 1) * DF_S + c + 1; }
        float ul = ws[idx - ds - dp], uc = ws[idx - ds], ur = ws[idx - ds + dp];
        float ml = ws[idx - dp], mc = ws[idx], mr = ws[idx + dp];
        int lowered = 0;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const float dl = ws[idx + ds - dp], dc = ws[idx + ds], dr = ws[idx + ds + dp];
            float nb = fminf(fminf(uc, dc), fminf(ml, mr));
            if (CONN == 8) nb = fminf(nb, fminf(fminf(ul, ur), fminf(dl, dr)));
            const float nw = fmaxf(zs[idx], fminf(mc, nb));
            if (nw < mc) {
                ws[idx] = nw;
                mc = nw;
                lowered = 1;
                if (line_rim || c == 0 || c == DF_T - 1) rim = 1;
            }
            ul = ml; uc = mc; ur = mr;
            ml = dl; mc = dc; mr = dr;
            idx += ds;
            c += sgn;
        }
        any |= lowered;
        live = __syncthreads_or(lowered);
    }
    any = __syncthreads_or(any);
    if (!any) {                                                     // nothing to write, nobody to wake
        sweep_visit_end(v, tiles_y, tiles_x, visits, false, false);
        return;
    }
    rim = __syncthreads_or(rim);

    // write back the finite values (an unknown pixel keeps its NaN, an unreached one its +inf)
    for (int i = t; i < DF_T * DF_T; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < H && gx < W) {
            const float wv = ws[(ly + 1) * DF_S + lx + 1];
            if (wv < inf) __hip_atomic_store(w + (int64_t)gy * W + gx, wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (t == 0 && j == n - 1) atomicAdd(changed, 1);
    sweep_visit_end(v, tiles_y, tiles_x, visits, true, rim != 0);   // marks: itself, and after a lowered rim value its neighbours
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
// Workgroup b owns the pixels [b * chunk, (b + 1) * chunk); thread t takes b * chunk + t, + 256, ... in that order; then the
// lanes of a wave by xor-shuffles, then waves 0..3 in order.  Every step is a function of the shape alone.
__global__ __launch_bounds__(256) void depfill_stats_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                            const uint8_t* __restrict__ known, const uint8_t* __restrict__ sel,
                                                            int64_t n, int64_t chunk, double* __restrict__ part) {
    __shared__ double rs[4], rm[4];
    __shared__ long long rc[3][4];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    double sum = 0.0, mx = 0.0;
    long long raised = 0, unreached = 0, counted = 0;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
        if (!known[p] || (sel && !sel[p])) continue;
        ++counted;
        const float wv = w[p], zv = z[p];
        if (wv > zv) {
            ++raised;
            if (wv == df_inf()) {
                ++unreached;
            } else {
                const double d = (double)wv - (double)zv;
                sum = sum + d;
                mx = d > mx ? d : mx;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum = sum + __shfl_xor(sum, o, 64);
        const double m2 = __shfl_xor(mx, o, 64);
        mx = m2 > mx ? m2 : mx;
        raised += __shfl_xor(raised, o, 64);
        unreached += __shfl_xor(unreached, o, 64);
        counted += __shfl_xor(counted, o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { rs[wv] = sum; rm[wv] = mx; rc[0][wv] = raised; rc[1][wv] = unreached; rc[2][wv] = counted; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = rs[0], m = rm[0];
        long long c0 = rc[0][0], c1 = rc[1][0], c2 = rc[2][0];
        for (int q = 1; q < 4; ++q) {
            s = s + rs[q];
            m = rm[q] > m ? rm[q] : m;
            c0 += rc[0][q]; c1 += rc[1][q]; c2 += rc[2][q];
        }
        double* o = part + (int64_t)blockIdx.x * DF_STAT_WORDS;
        o[0] = s;
        o[1] = m;
        long long* oc = reinterpret_cast<long long*>(o + 2);
        oc[0] = c0; oc[1] = c1; oc[2] = c2;
    }
}

__global__ void depfill_stats_finish_kernel(const double* __restrict__ part, int nb, int64_t* __restrict__ counts,
                                            double* __restrict__ sums) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, m = 0.0;
    long long c0 = 0, c1 = 0, c2 = 0;
    for (int b = 0; b < nb; ++b) {                                  // <= 1024 partials, in order
        const double* o = part + (int64_t)b * DF_STAT_WORDS;
        const long long* oc = reinterpret_cast<const long long*>(o + 2);
        s = s + o[0];
        m = o[1] > m ? o[1] : m;
        c0 += oc[0]; c1 += oc[1]; c2 += oc[2];
    }
    counts[0] = c0; counts[1] = c1; counts[2] = c2;
    sums[0] = s;
    sums[1] = m;
}

// ---- finish -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depfill_finish_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                             const uint8_t* __restrict__ known, int64_t n, float* __restrict__ out,
                                                             float* __restrict__ depth, uint8_t* __restrict__ flags) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        float o = df_nan(), d = df_nan();
        uint8_t f = 0;
        if (known[p]) {
            const float wv = w[p], zv = z[p];
            if (wv == df_inf()) {
                f = 1;                                              // raised, by an amount not known yet
            } else if (wv > zv) {
                o = wv; d = wv - zv; f = 1;
            } else {
                o = zv; d = 0.f;
            }
        }
        out[p] = o;
        if (depth) depth[p] = d;
        if (flags) flags[p] = f;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" size_t tg_depfill_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return df_layout(H, W).total;
}

extern "C" int tg_depfill_init(const float* z, const uint8_t* known, int H, int W, int conn, float* w, void* ws, size_t ws_bytes,
                               tg_stream_t stream) {
    if (int rc = raster_size_check("tg_depfill_init", H, W)) return rc;
    TG_REQUIRE(z && known && w && ws, "tg_depfill_init: null pointer");
    TG_REQUIRE(conn == 8 || conn == 4, "tg_depfill_init: connectivity %d must be 8 or 4", conn);
    TG_REQUIRE(w != z, "tg_depfill_init: w must not alias z");
    const DfLayout L = df_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_depfill_init: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    if (!sweep_reset(L, ws, s)) {
        tg_set_error("tg_depfill_init: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const dim3 grid(ew_grid((int64_t)H * W, 256));
    if (conn == 8) hipLaunchKernelGGL(depfill_init_kernel<8>, grid, dim3(256), 0, s, z, known, H, W, w);
    else hipLaunchKernelGGL(depfill_init_kernel<4>, grid, dim3(256), 0, s, z, known, H, W, w);
    TG_CHECK_LAUNCH("depfill_init_kernel");
    return TG_OK;
}

extern "C" int tg_depfill_sweep(const float* z, const uint8_t* known, int H, int W, int conn, int n, float* w, int32_t* changed,
                                int64_t* visits, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_depfill_sweep", H, W)) return rc;
    TG_REQUIRE(z && known && w && changed && visits && ws, "tg_depfill_sweep: null pointer");
    TG_REQUIRE(conn == 8 || conn == 4, "tg_depfill_sweep: connectivity %d must be 8 or 4", conn);
    TG_REQUIRE(n >= 1 && n <= (1 << 20), "tg_depfill_sweep: n = %d sweeps must lie in [1, 2^20]", n);
    TG_REQUIRE(w != z, "tg_depfill_sweep: w must not alias z");
    const DfLayout L = df_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_depfill_sweep: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    const auto sweep = conn == 8 ? depfill_sweep_kernel<8> : depfill_sweep_kernel<4>;
    return sweep_run(L, ws, n, changed, s, "depfill_begin_kernel", "depfill_sweep_kernel",
                     [&](dim3 grid, const int32_t* ctl, int j, uint8_t* p0, uint8_t* p1) {
                         hipLaunchKernelGGL(sweep, grid, dim3(256), 0, s, z, known, H, W, L.ty, L.tx, w, ctl, n, j, p0, p1, changed,
                                            reinterpret_cast<ull*>(visits));
                     });
}

extern "C" int tg_depfill_stats(const float* z, const float* w, const uint8_t* known, const uint8_t* sel, int H, int W,
                                int64_t* counts, double* sums, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_depfill_stats", H, W)) return rc;
    TG_REQUIRE(z && w && known && counts && sums && ws, "tg_depfill_stats: null pointer");
    const DfLayout L = df_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_depfill_stats: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    double* part = (double*)((char*)ws + L.stats);
    const int64_t n = (int64_t)H * W;
    const int64_t chunk = cdiv64(n, L.nstat);
    hipLaunchKernelGGL(depfill_stats_kernel, dim3(L.nstat), dim3(256), 0, s, z, w, known, sel, n, chunk, part);
    TG_CHECK_LAUNCH("depfill_stats_kernel");
    hipLaunchKernelGGL(depfill_stats_finish_kernel, dim3(1), dim3(64), 0, s, part, L.nstat, counts, sums);
    TG_CHECK_LAUNCH("depfill_stats_finish_kernel");
    return TG_OK;
}

extern "C" int tg_depfill_finish(const float* z, const float* w, const uint8_t* known, int H, int W, float* out, float* depth,
                                 uint8_t* flags, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_depfill_finish", H, W)) return rc;
    TG_REQUIRE(z && w && known && out, "tg_depfill_finish: null pointer");
    TG_REQUIRE(out != z && out != w && depth != z && depth != w, "tg_depfill_finish: out and depth must not alias z or w");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(depfill_finish_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, S(stream), z, w, known, n, out, depth, flags);
    TG_CHECK_LAUNCH("depfill_finish_kernel");
    return TG_OK;
}
