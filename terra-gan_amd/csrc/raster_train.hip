// Training windows from a whole float32 DSM (mvp_gan/src/utils/raster_dataset.py): synthetic hole masks rasterised from
// integer primitives, and windows cut from the raster under a dihedral transform and min-max normalised.
//
//   tg_hole_masks      one workgroup per 64x64 tile of a window's mask: the window's primitives are staged in LDS, the
//                      ones whose bounding box meets the tile are kept, and each pixel is tested against those in exact
//                      integer arithmetic (the union is order-independent: bit-exact)
//   tg_raster_sample   three launches on the stream: per-window lo / hi initialised (NaN for a draw that leaves the
//                      raster), per-tile partial min / max folded into lo / hi with integer atomics on the float bits
//                      (exact, order-independent), then the normalising pass x = (z - lo) / (hi - lo) per tile.  Each tile
//                      of the source window goes through LDS, so both the raster reads and the output writes are
//                      row-contiguous whatever the transform.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

constexpr int RT_TILE = 64;            // output tile side
constexpr int RT_THREADS = 256;        // 4 waves; a thread walks rows (threadIdx.x >> 6) + 4k of the tile, column = lane
constexpr int RT_MAX_PRIMS = 32;

// ---- hole masks ---------------------------------------------------------------------------------------------------------
struct Prim {
    int32_t v[8];
};

// conservative bounding box [y0, y1] x [x0, x1] of a primitive (see terragan_hip.h): |dy|, |dx| <= a + b for the rotated
// rectangle and ellipse (|dx| L2 = |p u - q v| <= (a |u| + b |v|) sqrt(L2)), the end points +- r for the segment
__device__ __forceinline__ void prim_bbox(const Prim& p, int& y0, int& y1, int& x0, int& x1) {
    const int k = p.v[0];
    y0 = 1; y1 = 0; x0 = 1; x1 = 0;          // empty: unknown kind, a direction (0, 0), an ellipse with a or b = 0
    if ((k == TG_HOLE_RECT || (k == TG_HOLE_ELLIPSE && p.v[3] > 0 && p.v[4] > 0)) && (p.v[5] != 0 || p.v[6] != 0)) {
        const int e = p.v[3] + p.v[4];
        y0 = p.v[1] - e; y1 = p.v[1] + e; x0 = p.v[2] - e; x1 = p.v[2] + e;
    } else if (k == TG_HOLE_STROKE) {
        const int r = p.v[5];
        y0 = min(p.v[1], p.v[3]) - r; y1 = max(p.v[1], p.v[3]) + r;
        x0 = min(p.v[2], p.v[4]) - r; x1 = max(p.v[2], p.v[4]) + r;
    }
}

__device__ __forceinline__ bool prim_covers(const Prim& p, int y, int x) {
    const int k = p.v[0];
    if (k == TG_HOLE_STROKE) {
        const int64_t wy = y - p.v[1], wx = x - p.v[2];
        const int64_t dy = p.v[3] - p.v[1], dx = p.v[4] - p.v[2];
        const int64_t r2 = (int64_t)p.v[5] * p.v[5];
        const int64_t wd = wy * dy + wx * dx, dd = dy * dy + dx * dx;
        if (wd <= 0) return wy * wy + wx * wx <= r2;
        if (wd >= dd) {
            const int64_t ey = y - p.v[3], ex = x - p.v[4];
            return ey * ey + ex * ex <= r2;
        }
        const int64_t c = wy * dx - wx * dy;
        return c * c <= r2 * dd;
    }
    const int64_t dy = y - p.v[1], dx = x - p.v[2];
    const int64_t a = p.v[3], b = p.v[4], u = p.v[5], v = p.v[6];
    const int64_t l2 = u * u + v * v;
    const int64_t pp = dx * u + dy * v, qq = dy * u - dx * v;
    if (k == TG_HOLE_RECT) return pp * pp <= a * a * l2 && qq * qq <= b * b * l2;
    return pp * pp * (b * b) + qq * qq * (a * a) <= a * a * b * b * l2;     // TG_HOLE_ELLIPSE
}

__global__ __launch_bounds__(RT_THREADS) void hole_mask_kernel(const int32_t* __restrict__ prims, const int32_t* __restrict__ offsets,
                                                               int side, int tiles_x, float* __restrict__ mask) {
    __shared__ Prim sp[RT_MAX_PRIMS];
    __shared__ int s_n;
    const int win = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int i0 = ty * RT_TILE, j0 = tx * RT_TILE;
    const int i1 = min(i0 + RT_TILE, side) - 1, j1 = min(j0 + RT_TILE, side) - 1;
    const int first = offsets[win];
    const int cnt = min(max(offsets[win + 1] - first, 0), RT_MAX_PRIMS);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    // wave 0 stages the primitives whose box meets the tile, in their list order (a ballot + prefix keeps it stable)
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        Prim p;
        bool keep = false;
        if (l < cnt) {
#pragma unroll
            for (int t = 0; t < 8; ++t) p.v[t] = prims[(int64_t)(first + l) * 8 + t];
            int by0, by1, bx0, bx1;
            prim_bbox(p, by0, by1, bx0, bx1);
            keep = by0 <= by1 && bx0 <= bx1 && by0 <= i1 && by1 >= i0 && bx0 <= j1 && bx1 >= j0;
        }
        const uint64_t bal = __ballot(keep);
        if (keep) sp[__popcll(bal & ((1ull << l) - 1))] = p;
        if (l == 0) s_n = __popcll(bal);
    }
    __syncthreads();
    const int np = s_n;
    const int c = threadIdx.x & 63;
    const int j = j0 + c;
    float* mw = mask + (int64_t)win * side * side;
    for (int r = threadIdx.x >> 6; r < RT_TILE; r += RT_THREADS / 64) {
        const int i = i0 + r;
        if (i > i1 || j > j1) continue;
        bool hole = false;
        for (int q = 0; q < np && !hole; ++q) hole = prim_covers(sp[q], i, j);
        mw[(int64_t)i * side + j] = hole ? 0.f : 1.f;
    }
}

// ---- windows ------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    const float* dem;
    int64_t H, W;
    const int32_t* draws;   // [n][3] = (y0, x0, op)
    int side, tiles_x;
    const float* mask;      // [n][side][side], output coordinates
    int norm_known;
    float* x;
    float* lo;
    float* hi;
};

__device__ __forceinline__ bool draw_ok(const SampleArgs& a, int win, int& y0, int& x0, int& op) {
    y0 = a.draws[3 * win]; x0 = a.draws[3 * win + 1]; op = a.draws[3 * win + 2];
    return y0 >= 0 && x0 >= 0 && (int64_t)y0 + a.side <= a.H && (int64_t)x0 + a.side <= a.W && op >= 0 && op <= 7;
}

// source offset (a, b) inside the window of output pixel (i, j) under transform op
__device__ __forceinline__ void src_of(int op, int side, int i, int j, int& a, int& b) {
    a = (op & 4) ? j : i;
    b = (op & 4) ? i : j;
    if (op & 2) a = side - 1 - a;
    if (op & 1) b = side - 1 - b;
}

// Stage the source rectangle an output tile [i0, i1] x [j0, j1] reads into LDS (rows of 64 + 1 floats: the transposed
// read of op & 4 walks a column, stride 65 keeps it on distinct banks).  Returns the rectangle's origin (a0, b0).
__device__ __forceinline__ void stage_tile(const SampleArgs& a, float (*t)[RT_TILE + 1], int y0, int x0, int op, int i0, int i1,
                                           int j0, int j1, int& a0, int& b0) {
    int aa, ab, ba, bb;
    src_of(op, a.side, i0, j0, aa, ab);
    src_of(op, a.side, i1, j1, ba, bb);
    a0 = min(aa, ba); b0 = min(ab, bb);
    const int na = max(aa, ba) - a0 + 1, nb = max(ab, bb) - b0 + 1;
    const int c = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < na; r += RT_THREADS / 64)
        if (c < nb) t[r][c] = a.dem[((int64_t)y0 + a0 + r) * a.W + x0 + b0 + c];
}

__global__ __launch_bounds__(64) void sample_init_kernel(SampleArgs a, int n) {
    const int win = blockIdx.x * 64 + threadIdx.x;
    if (win >= n) return;
    int y0, x0, op;
    const bool ok = draw_ok(a, win, y0, x0, op);
    a.lo[win] = ok ? INFINITY : NAN;
    a.hi[win] = ok ? -INFINITY : NAN;
}

// float min / max as integer atomics on the IEEE bits: for v >= 0 the signed order of the bits is the float order, for
// v < 0 the unsigned order is the reverse of it; -0 never arrives (values are canonicalised by + 0.f).  Exact and
// independent of the order in which workgroups arrive.
__device__ __forceinline__ void atomic_min_f32(float* p, float v) {
    if (v >= 0.f) atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* p, float v) {
    if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}

__global__ __launch_bounds__(RT_THREADS) void sample_minmax_kernel(SampleArgs a) {
    __shared__ float t[RT_TILE][RT_TILE + 1];
    __shared__ float smin[RT_THREADS / 64], smax[RT_THREADS / 64];
    const int win = blockIdx.y;
    int y0, x0, op;
    if (!draw_ok(a, win, y0, x0, op)) return;                 // uniform over the workgroup
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int i0 = ty * RT_TILE, j0 = tx * RT_TILE;
    const int i1 = min(i0 + RT_TILE, a.side) - 1, j1 = min(j0 + RT_TILE, a.side) - 1;
    int a0, b0;
    stage_tile(a, t, y0, x0, op, i0, i1, j0, j1, a0, b0);
    __syncthreads();
    const float* mw = a.mask + (int64_t)win * a.side * a.side;
    const int c = threadIdx.x & 63, j = j0 + c;
    float mn = INFINITY, mx = -INFINITY;
    for (int r = threadIdx.x >> 6; r < RT_TILE; r += RT_THREADS / 64) {
        const int i = i0 + r;
        if (i > i1 || j > j1) continue;
        if (a.norm_known && mw[(int64_t)i * a.side + j] == 0.f) continue;
        int sa, sb;
        src_of(op, a.side, i, j, sa, sb);
        const float z = t[sa - a0][sb - b0] + 0.f;             // + 0.f: a -0 extreme becomes +0
        mn = fminf(mn, z);
        mx = fmaxf(mx, z);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (c == 0) { smin[threadIdx.x >> 6] = mn; smax[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RT_THREADS / 64; ++w) { mn = fminf(mn, smin[w]); mx = fmaxf(mx, smax[w]); }
        if (mn <= mx) {                                        // the tile counted at least one pixel
            atomic_min_f32(a.lo + win, mn);
            atomic_max_f32(a.hi + win, mx);
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void sample_norm_kernel(SampleArgs a) {
    __shared__ float t[RT_TILE][RT_TILE + 1];
    const int win = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int i0 = ty * RT_TILE, j0 = tx * RT_TILE;
    const int i1 = min(i0 + RT_TILE, a.side) - 1, j1 = min(j0 + RT_TILE, a.side) - 1;
    float* xw = a.x + (int64_t)win * a.side * a.side;
    const int c = threadIdx.x & 63, j = j0 + c;
    int y0, x0, op;
    if (!draw_ok(a, win, y0, x0, op)) {                        // memory-safe answer to a draw the host should have rejected
        for (int r = threadIdx.x >> 6; r < RT_TILE; r += RT_THREADS / 64)
            if (i0 + r <= i1 && j <= j1) xw[(int64_t)(i0 + r) * a.side + j] = NAN;
        return;
    }
    int a0, b0;
    stage_tile(a, t, y0, x0, op, i0, i1, j0, j1, a0, b0);
    __syncthreads();
    const float l = a.lo[win], h = a.hi[win];
    const bool span = l < h;                                   // false when flat (hi == lo) or nothing was counted
    const float d = __fsub_rn(h, l);
    for (int r = threadIdx.x >> 6; r < RT_TILE; r += RT_THREADS / 64) {
        const int i = i0 + r;
        if (i > i1 || j > j1) continue;
        int sa, sb;
        src_of(op, a.side, i, j, sa, sb);
        xw[(int64_t)i * a.side + j] = span ? __fdiv_rn(__fsub_rn(t[sa - a0][sb - b0], l), d) : 0.f;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int window_check(const char* who, int n, int side) {
    TG_REQUIRE(side >= 40 && side <= 1024, "%s: window side %d out of range [40, 1024]", who, side);
    TG_REQUIRE(n >= 1 && n <= 65535, "%s: window count %d out of range [1, 65535]", who, n);
    return TG_OK;
}

extern "C" int tg_hole_masks(const int32_t* prims, const int32_t* offsets, int n, int side, float* mask, tg_stream_t stream) {
    if (int rc = window_check("tg_hole_masks", n, side)) return rc;
    TG_REQUIRE(prims && offsets && mask, "tg_hole_masks: null pointer");
    const int tiles_x = cdiv(side, RT_TILE);
    hipLaunchKernelGGL(hole_mask_kernel, dim3(tiles_x * tiles_x, n), dim3(RT_THREADS), 0, S(stream),
                       prims, offsets, side, tiles_x, mask);
    TG_CHECK_LAUNCH("hole_mask_kernel");
    return TG_OK;
}

extern "C" int tg_raster_sample(const float* dem, int64_t H, int64_t W, const int32_t* draws, int n, int side, const float* mask,
                                int norm_known, float* x, float* lo, float* hi, tg_stream_t stream) {
    if (int rc = window_check("tg_raster_sample", n, side)) return rc;
    TG_REQUIRE(dem && draws && mask && x && lo && hi, "tg_raster_sample: null pointer");
    TG_REQUIRE(H >= side && W >= side && H * W < ((int64_t)1 << 40), "tg_raster_sample: raster %lldx%lld smaller than the "
               "window side %d or too large", (long long)H, (long long)W, side);
    const int tiles_x = cdiv(side, RT_TILE);
    const SampleArgs a{dem, H, W, draws, side, tiles_x, mask, norm_known ? 1 : 0, x, lo, hi};
    hipLaunchKernelGGL(sample_init_kernel, dim3(cdiv(n, 64)), dim3(64), 0, S(stream), a, n);
    TG_CHECK_LAUNCH("sample_init_kernel");
    hipLaunchKernelGGL(sample_minmax_kernel, dim3(tiles_x * tiles_x, n), dim3(RT_THREADS), 0, S(stream), a);
    TG_CHECK_LAUNCH("sample_minmax_kernel");
    hipLaunchKernelGGL(sample_norm_kernel, dim3(tiles_x * tiles_x, n), dim3(RT_THREADS), 0, S(stream), a);
    TG_CHECK_LAUNCH("sample_norm_kernel");
    return TG_OK;
}
