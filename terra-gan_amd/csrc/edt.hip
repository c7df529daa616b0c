// Exact Euclidean distance to the nearest known pixel, and terrain errors by that depth (mvp_gan/src/distance.py,
// mvp_gan/src/evaluate_raster.py).
//
//   edt_mask_kernel      one thread per column and 64-row band: the band's seeds of that column as one 64-bit word
//   edt_carry_kernel     one thread per column: the nearest seed row above and below every band, carried across the bands
//   edt_g_kernel         g[y][x] = vertical distance to the nearest seed of column x (uint16, 0xffff: none, or too far for the
//                        cap), from the band's word by count-leading / count-trailing zeros and the two carried rows
//   edt_row_kernel       one workgroup per row: the row of g staged in LDS, every lane searches outward from its own x,
//                        d2 = min over x' of (x - x')^2 + g[x']^2, while k^2 < the best so far (and < cap2)
//   edt_gs_kernel        (feature transform) the same column distance with the side in bit 15: set when the nearest seed of the
//                        column lies below (a tie goes to the one above), so its row is y - g or y + g
//   edt_row_idx_kernel   (feature transform) the row search over (d2, seed row, seed column), lexicographically: d2 as
//                        edt_row_kernel's, idx = row * W + column of the winner, -1 where nothing is nearer than the cap
//   depth_errors_kernel  |error| by depth class: per-workgroup fp64 partials, integer counters and maxima, per-hole max d2
//   depth_errors_finish_kernel   one workgroup reduces the partials in a fixed order
//
// Exactness: 2 * 32767^2 < 2^31, so every squared distance is an int32 and everything is integer arithmetic up to the optional
// metres (one fp64 sqrt and one fp64 multiply, rounded to fp32 once).  Determinism: no floating-point atomics; the integer
// atomics (add, max) commute, and the grid of the depth profile is a function of the shape.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

constexpr int EDT_BAND = 64;              // rows per band: one bit per row of a 64-bit word
constexpr uint32_t EDT_NONE = 0xffffu;    // g: no seed in the column, or not nearer than the cap
constexpr int EDT_INF = 1 << 30;          // a vertical distance no raster reaches
constexpr int EDT_ROW_LDS = 65536;        // the row kernel's dynamic LDS at the largest admitted side (2 B x 32767, rounded up)

// ---- column pass --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edt_mask_kernel(const uint8_t* __restrict__ seed, int H, int W,
                                                       uint64_t* __restrict__ mask) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int b = blockIdx.y, y0 = b * EDT_BAND;
    const int rows = H - y0 < EDT_BAND ? H - y0 : EDT_BAND;
    const uint8_t* p = seed + (int64_t)y0 * W + x;
    uint64_t m = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) m |= (uint64_t)(p[(int64_t)r * W] != 0) << r;
    mask[(int64_t)b * W + x] = m;
}

// up[b][x] = the last seed row of column x above band b, down[b][x] = the first one below it; -1: none
__global__ __launch_bounds__(256) void edt_carry_kernel(const uint64_t* __restrict__ mask, int nb, int W,
                                                        int32_t* __restrict__ up, int32_t* __restrict__ down) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    int last = -1;
    for (int b = 0; b < nb; ++b) {
        const int64_t i = (int64_t)b * W + x;
        up[i] = last;
        const uint64_t m = mask[i];
        if (m) last = b * EDT_BAND + 63 - __clzll((long long)m);
    }
    int next = -1;
    for (int b = nb - 1; b >= 0; --b) {
        const int64_t i = (int64_t)b * W + x;
        down[i] = next;
        const uint64_t m = mask[i];
        if (m) next = b * EDT_BAND + __ffsll((long long)m) - 1;
    }
}

// glimit: a vertical distance >= glimit cannot lower the result (its square is >= cap2); 0xffff without a cap
__global__ __launch_bounds__(256) void edt_g_kernel(const uint64_t* __restrict__ mask, const int32_t* __restrict__ up,
                                                    const int32_t* __restrict__ down, int H, int W, int glimit,
                                                    uint16_t* __restrict__ g) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int b = blockIdx.y, y0 = b * EDT_BAND;
    const int rows = H - y0 < EDT_BAND ? H - y0 : EDT_BAND;
    const int64_t i = (int64_t)b * W + x;
    const uint64_t m = mask[i];
    const int u = up[i], d = down[i];
    uint16_t* out = g + (int64_t)y0 * W + x;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const uint64_t lo = m & (~0ull >> (63 - r));      // seeds of rows y0 .. y
        const uint64_t hi = m >> r;                       // seeds of rows y .. y0 + 63, row y at bit 0
        const int du = lo ? r - (63 - __clzll((long long)lo)) : (u >= 0 ? y - u : EDT_INF);
        const int dd = hi ? __ffsll((long long)hi) - 1 : (d >= 0 ? d - y : EDT_INF);
        const int v = du < dd ? du : dd;
        out[(int64_t)r * W] = (uint16_t)(v >= glimit ? EDT_NONE : (uint32_t)v);
    }
}

// ---- row pass -----------------------------------------------------------------------------------------------------------
// Every lane starts at lim = cap2 (TG_EDT_FAR without a cap), so the result is min(exact, cap2) by construction.  The search
// ends at k > max(x, W - 1 - x) or k^2 >= best: a row without any finite g (no seed in reach of any column) is written without
// a search, and a lane among sentinels stops at the row's end.
__global__ __launch_bounds__(256) void edt_row_kernel(const uint16_t* __restrict__ g, int W, int32_t lim, double cellsize,
                                                      int32_t* __restrict__ d2, float* __restrict__ dist_m) {
    extern __shared__ __attribute__((aligned(16))) uint16_t sg[];
    const int64_t base = (int64_t)blockIdx.x * W;
    int mine = 0;
    for (int x = threadIdx.x; x < W; x += 256) {
        const uint16_t v = g[base + x];
        sg[x] = v;
        mine |= v != EDT_NONE;
    }
    const int some = __syncthreads_or(mine);
    for (int x = threadIdx.x; x < W; x += 256) {
        int32_t best = lim;
        if (some) {
            const int32_t g0 = sg[x];
            if (g0 != (int32_t)EDT_NONE && g0 * g0 < best) best = g0 * g0;
            const int kmax = x > W - 1 - x ? x : W - 1 - x;
            for (int k = 1; k <= kmax && k * k < best; ++k) {
                const int32_t k2 = k * k;
                if (k <= x) {
                    const int32_t a = sg[x - k];
                    if (a != (int32_t)EDT_NONE && k2 + a * a < best) best = k2 + a * a;
                }
                if (x + k < W) {
                    const int32_t a = sg[x + k];
                    if (a != (int32_t)EDT_NONE && k2 + a * a < best) best = k2 + a * a;
                }
            }
        }
        d2[base + x] = best;
        if (dist_m) dist_m[base + x] = best == TG_EDT_FAR ? INFINITY : (float)(cellsize * sqrt((double)best));
    }
}

// ---- feature transform: which seed is the nearest ---------------------------------------------------
// Tie rule: among the seeds at the smallest squared distance the smallest row, then the smallest column.  Within a column the
// seed above wins a tie (its row is smaller); across columns the candidates are compared as (d2, row, column).  A column
// distance is at most 32766, so bit 15 of g is free for the side and the plane stays 2 B per pixel.
constexpr uint32_t EDT_BELOW = 0x8000u;

__global__ __launch_bounds__(256) void edt_gs_kernel(const uint64_t* __restrict__ mask, const int32_t* __restrict__ up,
                                                     const int32_t* __restrict__ down, int H, int W, int glimit,
                                                     uint16_t* __restrict__ g) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int b = blockIdx.y, y0 = b * EDT_BAND;
    const int rows = H - y0 < EDT_BAND ? H - y0 : EDT_BAND;
    const int64_t i = (int64_t)b * W + x;
    const uint64_t m = mask[i];
    const int u = up[i], d = down[i];
    uint16_t* out = g + (int64_t)y0 * W + x;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const uint64_t lo = m & (~0ull >> (63 - r));
        const uint64_t hi = m >> r;
        const int du = lo ? r - (63 - __clzll((long long)lo)) : (u >= 0 ? y - u : EDT_INF);
        const int dd = hi ? __ffsll((long long)hi) - 1 : (d >= 0 ? d - y : EDT_INF);
        const bool below = dd < du;
        const int v = below ? dd : du;
        out[(int64_t)r * W] = (uint16_t)(v >= glimit ? EDT_NONE : (uint32_t)v | (below ? EDT_BELOW : 0u));
    }
}

// (d2, row, col) < (best, brow, bcol); a candidate that does not get below lim never counts
#define EDT_CAND(xc, kk2)                                                                          \
    do {                                                                                           \
        const uint32_t s_ = sg[xc];                                                                \
        if (s_ != EDT_NONE) {                                                                      \
            const int32_t a_ = (int32_t)(s_ & 0x7fffu);                                            \
            const int32_t c_ = (kk2) + a_ * a_;                                                    \
            const int32_t r_ = (s_ & EDT_BELOW) ? y + a_ : y - a_;                                 \
            if (c_ < lim && (c_ < best || (c_ == best && (r_ < brow || (r_ == brow && (xc) < bcol))))) { \
                best = c_; brow = r_; bcol = (xc);                                                 \
            }                                                                                      \
        }                                                                                          \
    } while (0)

// As edt_row_kernel, but the search goes on while k^2 <= best: a seed at the same distance may have a smaller row or column.
__global__ __launch_bounds__(256) void edt_row_idx_kernel(const uint16_t* __restrict__ g, int W, int32_t lim,
                                                          int32_t* __restrict__ d2, int32_t* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) uint16_t sg[];
    const int y = blockIdx.x;
    const int64_t base = (int64_t)y * W;
    int mine = 0;
    for (int x = threadIdx.x; x < W; x += 256) {
        const uint16_t v = g[base + x];
        sg[x] = v;
        mine |= v != EDT_NONE;
    }
    const int some = __syncthreads_or(mine);
    for (int x = threadIdx.x; x < W; x += 256) {
        int32_t best = lim, brow = 0x7fffffff, bcol = 0x7fffffff;
        if (some) {
            EDT_CAND(x, 0);
            const int kmax = x > W - 1 - x ? x : W - 1 - x;
            for (int k = 1; k <= kmax && k * k <= best && k * k < lim; ++k) {
                const int32_t k2 = k * k;
                if (k <= x) EDT_CAND(x - k, k2);
                if (x + k < W) EDT_CAND(x + k, k2);
            }
        }
        d2[base + x] = best;
        idx[base + x] = best < lim ? brow * W + bcol : -1;
    }
}
#undef EDT_CAND

// ---- errors by depth ----------------------------------------------------------------------------------------------------
constexpr int DE_NSUM = 2 * TG_DEPTH_MAX_CLASSES;

static int de_grid(int H, int W) { return ew_grid((int64_t)H * W, 256); }

struct DeArgs {
    const float* a;
    const int32_t* d2;
    const int32_t* labels;
    const int32_t* slot;
    int nholes;
    int64_t n;
    TgDepthClasses cls;
    int64_t* counts;
    uint32_t* max_bits;
    int32_t* hole_d2;
    double* partials;
};

__global__ __launch_bounds__(256) void depth_errors_kernel(DeArgs A) {
    __shared__ double dred[4][DE_NSUM];
    __shared__ int ired[4][TG_DEPTH_MAX_CLASSES];
    __shared__ uint32_t mred[4][TG_DEPTH_MAX_CLASSES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double sa[TG_DEPTH_MAX_CLASSES], sa2[TG_DEPTH_MAX_CLASSES];
    int cnt[TG_DEPTH_MAX_CLASSES];
    uint32_t mx[TG_DEPTH_MAX_CLASSES];
#pragma unroll
    for (int q = 0; q < TG_DEPTH_MAX_CLASSES; ++q) { sa[q] = 0.0; sa2[q] = 0.0; cnt[q] = 0; mx[q] = 0; }

    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * 256) {
        const int32_t d = A.d2[i];
        const int32_t lab = A.labels[i];
        if (lab >= 0 && lab < A.n) {
            const int s = A.slot[lab];
            // the plain read may be stale, but only ever too small: then the atomic runs and settles it
            if (s >= 0 && s < A.nholes && d > __atomic_load_n(&A.hole_d2[s], __ATOMIC_RELAXED)) atomicMax(&A.hole_d2[s], d);
        }
        const float a = A.a[i];
        if (a == a) {
            int c = 0;
            for (int e = 0; e < A.cls.n_edges; ++e) c += d >= A.cls.d2[e];
            const double ad = a, a2 = ad * ad;
            const uint32_t ab = __float_as_uint(a);
#pragma unroll
            for (int q = 0; q < TG_DEPTH_MAX_CLASSES; ++q) {
                if (q == c) {
                    sa[q] += ad;
                    sa2[q] += a2;
                    ++cnt[q];
                    mx[q] = ab > mx[q] ? ab : mx[q];
                }
            }
        }
    }

    // workgroup reduction in a fixed order: xor butterflies inside the waves, then waves 0..3
#pragma unroll
    for (int q = 0; q < TG_DEPTH_MAX_CLASSES; ++q) {
        const double v = wave_sum_d(sa[q]), v2 = wave_sum_d(sa2[q]);
        int n = cnt[q];
        uint32_t m = mx[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_xor(n, o, 64);
            const uint32_t u = __shfl_xor(m, o, 64);
            m = u > m ? u : m;
        }
        if (lane == 0) { dred[w][2 * q] = v; dred[w][2 * q + 1] = v2; ired[w][q] = n; mred[w][q] = m; }
    }
    __syncthreads();
    if (threadIdx.x < DE_NSUM) {
        const int s = threadIdx.x;
        A.partials[(int64_t)blockIdx.x * DE_NSUM + s] = ((dred[0][s] + dred[1][s]) + dred[2][s]) + dred[3][s];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + TG_DEPTH_MAX_CLASSES) {
        const int q = threadIdx.x - 64;
        const ull v = (ull)(ired[0][q] + ired[1][q] + ired[2][q] + ired[3][q]);
        if (v) atomicAdd(reinterpret_cast<ull*>(&A.counts[q]), v);
    } else if (threadIdx.x >= 128 && threadIdx.x < 128 + TG_DEPTH_MAX_CLASSES) {
        const int q = threadIdx.x - 128;
        uint32_t m = 0;
        for (int k = 0; k < 4; ++k) m = mred[k][q] > m ? mred[k][q] : m;
        if (m) atomicMax(&A.max_bits[q], m);
    }
}

__global__ __launch_bounds__(256) void depth_errors_finish_kernel(const double* __restrict__ partials, int nwg,
                                                                  double* __restrict__ sums) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = 0; s < DE_NSUM; ++s) {
        double v = 0.0;
        for (int g = threadIdx.x; g < nwg; g += 256) v += partials[(int64_t)g * DE_NSUM + s];
        v = wave_sum_d(v);
        if (lane == 0) red[w] = v;
        __syncthreads();
        if (threadIdx.x == 0) sums[s] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int side_check(const char* who, int H, int W) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= TG_EDT_MAX_SIDE && W <= TG_EDT_MAX_SIDE,
               "%s: raster %dx%d: both sides must lie in [1, %d]", who, H, W, (int)TG_EDT_MAX_SIDE);
    return TG_OK;
}

static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

struct EdtLayout {
    size_t mask, up, down, g, total;
};

static EdtLayout edt_layout(int H, int W) {
    const size_t nbw = (size_t)cdiv(H, EDT_BAND) * W;
    EdtLayout L;
    L.mask = 0;
    L.up = L.mask + al256(nbw * sizeof(uint64_t));
    L.down = L.up + al256(nbw * sizeof(int32_t));
    L.g = L.down + al256(nbw * sizeof(int32_t));
    L.total = L.g + al256((size_t)H * W * sizeof(uint16_t));
    return L;
}

extern "C" size_t tg_edt_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > TG_EDT_MAX_SIDE || W > TG_EDT_MAX_SIDE) return 0;
    return edt_layout(H, W).total;
}

extern "C" int tg_edt(const uint8_t* seed, int H, int W, int32_t cap2, double cellsize, int32_t* d2, float* dist_m, void* ws,
                      size_t ws_bytes, tg_stream_t stream) {
    if (int rc = side_check("tg_edt", H, W)) return rc;
    TG_REQUIRE(seed && d2 && ws, "tg_edt: null pointer");
    TG_REQUIRE(!dist_m || (isfinite(cellsize) && cellsize > 0.0), "tg_edt: cellsize %g must be finite and > 0", cellsize);
    const EdtLayout L = edt_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_edt: workspace %zu bytes < %zu", ws_bytes, L.total);
    int glimit = (int)EDT_NONE;
    if (cap2 > 0) {                                     // the smallest s with s^2 >= cap2 (at most 46341)
        int64_t s = (int64_t)sqrt((double)cap2);
        while (s * s >= cap2 && s > 0) --s;
        while (s * s < cap2) ++s;
        if (s < glimit) glimit = (int)s;
    }
    static bool opted[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !opted[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(edt_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                EDT_ROW_LDS) != hipSuccess) {
            tg_set_error("tg_edt: LDS opt-in failed");
            return TG_ERR_LAUNCH;
        }
        if (dev >= 0 && dev < 64) opted[dev] = true;
    }
    char* base = (char*)ws;
    uint64_t* mask = (uint64_t*)(base + L.mask);
    int32_t* up = (int32_t*)(base + L.up);
    int32_t* down = (int32_t*)(base + L.down);
    uint16_t* g = (uint16_t*)(base + L.g);
    const int nb = cdiv(H, EDT_BAND), gx = cdiv(W, 256);
    hipLaunchKernelGGL(edt_mask_kernel, dim3(gx, nb), dim3(256), 0, S(stream), seed, H, W, mask);
    TG_CHECK_LAUNCH("edt_mask_kernel");
    hipLaunchKernelGGL(edt_carry_kernel, dim3(gx), dim3(256), 0, S(stream), mask, nb, W, up, down);
    TG_CHECK_LAUNCH("edt_carry_kernel");
    hipLaunchKernelGGL(edt_g_kernel, dim3(gx, nb), dim3(256), 0, S(stream), mask, up, down, H, W, glimit, g);
    TG_CHECK_LAUNCH("edt_g_kernel");
    const size_t lds = ((size_t)W * sizeof(uint16_t) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(edt_row_kernel, dim3(H), dim3(256), lds, S(stream), g, W, cap2 > 0 ? cap2 : (int32_t)TG_EDT_FAR, cellsize,
                       d2, dist_m);
    TG_CHECK_LAUNCH("edt_row_kernel");
    return TG_OK;
}

extern "C" size_t tg_edt_nearest_ws_bytes(int H, int W) { return tg_edt_ws_bytes(H, W); }

extern "C" int tg_edt_nearest(const uint8_t* seed, int H, int W, int32_t cap2, int32_t* d2, int32_t* idx, void* ws,
                              size_t ws_bytes, tg_stream_t stream) {
    if (int rc = side_check("tg_edt_nearest", H, W)) return rc;
    TG_REQUIRE(seed && d2 && idx && ws, "tg_edt_nearest: null pointer");
    const EdtLayout L = edt_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_edt_nearest: workspace %zu bytes < %zu", ws_bytes, L.total);
    int glimit = (int)EDT_NONE;
    if (cap2 > 0) {                                     // the smallest s with s^2 >= cap2, as in tg_edt
        int64_t s = (int64_t)sqrt((double)cap2);
        while (s * s >= cap2 && s > 0) --s;
        while (s * s < cap2) ++s;
        if (s < glimit) glimit = (int)s;
    }
    static bool opted[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !opted[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(edt_row_idx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                EDT_ROW_LDS) != hipSuccess) {
            tg_set_error("tg_edt_nearest: LDS opt-in failed");
            return TG_ERR_LAUNCH;
        }
        if (dev >= 0 && dev < 64) opted[dev] = true;
    }
    char* base = (char*)ws;
    uint64_t* mask = (uint64_t*)(base + L.mask);
    int32_t* up = (int32_t*)(base + L.up);
    int32_t* down = (int32_t*)(base + L.down);
    uint16_t* g = (uint16_t*)(base + L.g);
    const int nb = cdiv(H, EDT_BAND), gx = cdiv(W, 256);
    hipLaunchKernelGGL(edt_mask_kernel, dim3(gx, nb), dim3(256), 0, S(stream), seed, H, W, mask);
    TG_CHECK_LAUNCH("edt_mask_kernel");
    hipLaunchKernelGGL(edt_carry_kernel, dim3(gx), dim3(256), 0, S(stream), mask, nb, W, up, down);
    TG_CHECK_LAUNCH("edt_carry_kernel");
    hipLaunchKernelGGL(edt_gs_kernel, dim3(gx, nb), dim3(256), 0, S(stream), mask, up, down, H, W, glimit, g);
    TG_CHECK_LAUNCH("edt_gs_kernel");
    const size_t lds = ((size_t)W * sizeof(uint16_t) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(edt_row_idx_kernel, dim3(H), dim3(256), lds, S(stream), g, W, cap2 > 0 ? cap2 : (int32_t)TG_EDT_FAR, d2,
                       idx);
    TG_CHECK_LAUNCH("edt_row_idx_kernel");
    return TG_OK;
}

extern "C" size_t tg_depth_errors_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > TG_EDT_MAX_SIDE || W > TG_EDT_MAX_SIDE) return 0;
    return (size_t)de_grid(H, W) * DE_NSUM * sizeof(double);
}

extern "C" int tg_depth_errors(const float* a, const int32_t* d2, const int32_t* labels, const int32_t* slot, int nholes, int H,
                               int W, const TgDepthClasses* cls, int64_t* counts, uint32_t* max_bits, int32_t* hole_d2, void* ws,
                               size_t ws_bytes, tg_stream_t stream) {
    if (int rc = side_check("tg_depth_errors", H, W)) return rc;
    TG_REQUIRE(nholes >= 0, "tg_depth_errors: nholes %d < 0", nholes);
    TG_REQUIRE(a && d2 && labels && slot && cls && counts && max_bits && ws && (hole_d2 || !nholes),
               "tg_depth_errors: null pointer");
    TG_REQUIRE(cls->n_edges >= 0 && cls->n_edges < TG_DEPTH_MAX_CLASSES, "tg_depth_errors: %d class edges out of range [0, %d]",
               cls->n_edges, TG_DEPTH_MAX_CLASSES - 1);
    for (int e = 1; e < cls->n_edges; ++e)
        TG_REQUIRE(cls->d2[e] >= cls->d2[e - 1], "tg_depth_errors: class edges must be nondecreasing");
    const size_t need = tg_depth_errors_ws_bytes(H, W);
    TG_REQUIRE(ws_bytes >= need, "tg_depth_errors: workspace %zu bytes < %zu", ws_bytes, need);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_DEPTH_MAX_CLASSES * sizeof(int64_t), s) != hipSuccess ||
        hipMemsetAsync(max_bits, 0, TG_DEPTH_MAX_CLASSES * sizeof(uint32_t), s) != hipSuccess ||
        (nholes && hipMemsetAsync(hole_d2, 0, (size_t)nholes * sizeof(int32_t), s) != hipSuccess)) {
        tg_set_error("tg_depth_errors: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    DeArgs A;
    A.a = a; A.d2 = d2; A.labels = labels; A.slot = slot; A.nholes = nholes; A.n = (int64_t)H * W; A.cls = *cls;
    A.counts = counts; A.max_bits = max_bits; A.hole_d2 = hole_d2; A.partials = (double*)ws;
    hipLaunchKernelGGL(depth_errors_kernel, dim3(de_grid(H, W)), dim3(256), 0, s, A);
    TG_CHECK_LAUNCH("depth_errors_kernel");
    return TG_OK;
}

extern "C" int tg_depth_errors_finish(int H, int W, const void* ws, size_t ws_bytes, double* sums, tg_stream_t stream) {
    if (int rc = side_check("tg_depth_errors_finish", H, W)) return rc;
    TG_REQUIRE(ws && sums, "tg_depth_errors_finish: null pointer");
    const size_t need = tg_depth_errors_ws_bytes(H, W);
    TG_REQUIRE(ws_bytes >= need, "tg_depth_errors_finish: workspace %zu bytes < %zu", ws_bytes, need);
    hipLaunchKernelGGL(depth_errors_finish_kernel, dim3(1), dim3(256), 0, S(stream), (const double*)ws, de_grid(H, W), sums);
    TG_CHECK_LAUNCH("depth_errors_finish_kernel");
    return TG_OK;
}
