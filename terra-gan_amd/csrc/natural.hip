// Natural-neighbour (discrete Sibson) void fill (mvp_gan/src/natural.py).
//
// Every void raster pixel q hands the height of its nearest known pixel, nn(q), to every pixel p that lies strictly inside the
// disc around q whose squared radius is c(q) = min(d2(q), radius^2): the pixels whose insertion as a site would claim q.  A void
// pixel p becomes the mean of what it is handed.  The kernel gathers: one thread owns one output pixel and walks the window of
// candidate q around it in row-major order.
//
//   natural_tilemax_kernel  one workgroup per NAT_TH x NAT_TW tile: the largest c of the tile as a uint16 in the workspace
//   natural_fill_kernel     one workgroup per tile.  A tile whose own maximum is 0 holds no void pixel and is copied through.
//                           Else the tile derives its effective radius R from the maxima of the tiles its window can touch: a
//                           contributor q of p has |p - q|^2 < c(q) <= M, so both offsets are at most isqrt(M - 1); the maxima are
//                           taken again over the tiles within that R until R stops shrinking.  Only the tile plus an R halo of c
//                           (uint16) and nn (float) is staged in LDS, and the loops run over (2R + 1)^2 offsets.
//
// Summation order (part of the interface): row-major over q, i.e. dy = -R..R outside, dx = -R..R inside, in fp64 from 0.0.  A
// candidate that does not contribute adds +0.0, which leaves every sum that started at +0.0 unchanged bit for bit, so the
// result does not depend on R and equals the sum over the contributors alone in that order.  No atomics on the sums; the two
// counters are integer atomics.
//
// LDS: the rows of a wave are contiguous (NAT_TW = 64 = one wave per tile row), so a ds_read of 64 consecutive uint16 or float
// has every lane of a 32-lane group on its own bank (or sharing a dword) at any halo width: no padding is needed.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

constexpr int NAT_TW = 64;           // tile width: one wave per tile row
constexpr int NAT_TH = 4;            // tile height: four waves
constexpr int NAT_MAX_RADIUS = 32;

static size_t nat_lds_bytes(int radius) {
    const int h = radius - 1;
    return (size_t)(NAT_TH + 2 * h) * (NAT_TW + 2 * h) * (sizeof(float) + sizeof(uint16_t));
}

__global__ __launch_bounds__(256) void natural_tilemax_kernel(const int32_t* __restrict__ d2, int H, int W, int r2,
                                                              uint16_t* __restrict__ tmax) {
    __shared__ int red[4];
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = blockIdx.x * NAT_TW + lx, y = blockIdx.y * NAT_TH + ly;
    int c = 0;
    if (x < W && y < H) {
        const int32_t d = d2[(int64_t)y * W + x];
        c = d < r2 ? (d > 0 ? d : 0) : r2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(c, o, 64);
        c = t > c ? t : c;
    }
    if (lx == 0) red[ly] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = red[0];
        m = red[1] > m ? red[1] : m;
        m = red[2] > m ? red[2] : m;
        m = red[3] > m ? red[3] : m;
        tmax[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (uint16_t)m;
    }
}

// the largest k with k * k <= v, 0 <= v < 2^20
__device__ __forceinline__ int nat_isqrt(int v) {
    int k = (int)sqrtf((float)v);
    while (k * k > v) --k;
    while ((k + 1) * (k + 1) <= v) ++k;
    return k;
}

__global__ __launch_bounds__(256) void natural_fill_kernel(const float* __restrict__ nn, const int32_t* __restrict__ d2,
                                                           const uint8_t* __restrict__ known, int H, int W, int radius,
                                                           int32_t lim2, const uint16_t* __restrict__ tmax,
                                                           float* __restrict__ out, int32_t* __restrict__ support,
                                                           ull* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char nat_lds[];
    __shared__ int red[2][4];
    const int tx = blockIdx.x, ty = blockIdx.y, ntx = gridDim.x, nty = gridDim.y;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x0 = tx * NAT_TW, y0 = ty * NAT_TH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < W && y < H;
    const int64_t p = (int64_t)y * W + x;
    const int r2 = radius * radius;

    if (tmax[(int64_t)ty * ntx + tx] == 0) {                       // workgroup-uniform: no void pixel in this tile
        if (inside) {
            out[p] = nn[p];
            if (support) support[p] = 0;
        }
        return;
    }

    // the effective radius: shrink until the maxima of the tiles within reach no longer allow less (all of it uniform)
    int R = radius - 1;
    for (;;) {
        const int ky = (R + NAT_TH - 1) / NAT_TH, kx = (R + NAT_TW - 1) / NAT_TW;
        const int ta = ty - ky > 0 ? ty - ky : 0, tb = ty + ky < nty - 1 ? ty + ky : nty - 1;
        const int sa = tx - kx > 0 ? tx - kx : 0, sb = tx + kx < ntx - 1 ? tx + kx : ntx - 1;
        int M = 0;
        for (int t = ta; t <= tb; ++t)
            for (int s = sa; s <= sb; ++s) {
                const int v = tmax[(int64_t)t * ntx + s];
                M = v > M ? v : M;
            }
        const int Rn = nat_isqrt(M - 1);                            // M >= this tile's own maximum >= 1
        if (Rn >= R) break;
        R = Rn;
    }

    // the pixel's own flag and distance, from a clamped (always valid) address so that neither load waits behind a branch
    const int64_t pc = inside ? p : 0;
    const uint8_t kp = known[pc];
    const int32_t dp = d2[pc];

    // stage c and nn of the tile and its halo; outside the raster c = 0 (never contributes)
    const int SW = NAT_TW + 2 * R, SH = NAT_TH + 2 * R;
    float* nnS = reinterpret_cast<float*>(nat_lds);
    uint16_t* cS = reinterpret_cast<uint16_t*>(nat_lds + (size_t)SH * SW * sizeof(float));
    for (int hy = ly; hy < SH; hy += NAT_TH) {
        const int gy = y0 - R + hy;
        const bool yin = gy >= 0 && gy < H;
        const int64_t row = (int64_t)(yin ? gy : 0) * W;
        for (int hx = lx; hx < SW; hx += NAT_TW) {
            const int gx = x0 - R + hx;
            const bool in = yin && gx >= 0 && gx < W;
            const int64_t g = row + (in ? gx : 0);                  // always a valid address: the load is not behind a branch
            const int32_t d = d2[g];
            const float v = nn[g];
            const int c = d < r2 ? (d > 0 ? d : 0) : r2;
            cS[hy * SW + hx] = (uint16_t)(in ? c : 0);
            nnS[hy * SW + hx] = in ? v : 0.0f;
        }
    }
    __syncthreads();

    int filled = 0, left = 0;
    if (inside) {
        if (kp) {
            out[p] = nnS[(ly + R) * SW + lx + R];                   // nn[p] as staged, bit for bit
            if (support) support[p] = 0;
        } else {
            double s = 0.0;
            int n = 0;
            for (int dy = -R; dy <= R; ++dy) {
                const int base = (ly + R + dy) * SW + lx + R;
                const int dy2 = dy * dy;
#pragma unroll 4
                for (int dx = -R; dx <= R; ++dx) {
                    const int c = cS[base + dx];
                    const float v = nnS[base + dx];
                    const bool ok = dy2 + dx * dx < c;
                    s = s + (double)(ok ? v : 0.0f);
                    n += ok ? 1 : 0;
                }
            }
            const bool nan = dp == TG_EDT_FAR || (lim2 > 0 && dp > lim2);
            out[p] = nan ? __uint_as_float(0x7fc00000u) : (float)(s / (double)n);     // n >= 1: the pixel itself
            if (support) support[p] = n;
            filled = nan ? 0 : 1;
            left = nan ? 1 : 0;
        }
    }
    const int c0 = __popcll(__ballot(filled)), c1 = __popcll(__ballot(left));
    if (lx == 0) { red[0][ly] = c0; red[1][ly] = c1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (t) atomicAdd(&counts[threadIdx.x], (ull)t);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t tg_natural_fill_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > TG_EDT_MAX_SIDE || W > TG_EDT_MAX_SIDE) return 0;
    return al256((size_t)cdiv(H, NAT_TH) * cdiv(W, NAT_TW) * sizeof(uint16_t));
}

static int nat_check(const char* who, int H, int W, int radius, const void* ws, size_t ws_bytes) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= TG_EDT_MAX_SIDE && W <= TG_EDT_MAX_SIDE,
               "%s: raster %dx%d: both sides must lie in [1, %d]", who, H, W, (int)TG_EDT_MAX_SIDE);
    TG_REQUIRE(radius >= 1 && radius <= NAT_MAX_RADIUS, "%s: radius %d must lie in [1, %d]", who, radius, (int)NAT_MAX_RADIUS);
    TG_REQUIRE(ws, "%s: null pointer", who);
    const size_t need = tg_natural_fill_ws_bytes(H, W);
    TG_REQUIRE(ws_bytes >= need, "%s: workspace %zu bytes < %zu", who, ws_bytes, need);
    return TG_OK;
}

extern "C" int tg_natural_tile_maxima(const int32_t* d2, int H, int W, int radius, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = nat_check("tg_natural_tile_maxima", H, W, radius, ws, ws_bytes)) return rc;
    TG_REQUIRE(d2, "tg_natural_tile_maxima: null pointer");
    hipLaunchKernelGGL(natural_tilemax_kernel, dim3(cdiv(W, NAT_TW), cdiv(H, NAT_TH)), dim3(256), 0, S(stream), d2, H, W,
                       radius * radius, (uint16_t*)ws);
    TG_CHECK_LAUNCH("natural_tilemax_kernel");
    return TG_OK;
}

extern "C" int tg_natural_fill(const float* nn, const int32_t* d2, const uint8_t* known, int H, int W, int radius, int32_t lim2,
                               float* out, int32_t* support, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream) {
    TG_REQUIRE(nn && d2 && known && out && counts && ws, "tg_natural_fill: null pointer");
    if (int rc = nat_check("tg_natural_fill", H, W, radius, ws, ws_bytes)) return rc;
    TG_REQUIRE(out != nn, "tg_natural_fill: out must not alias nn");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_natural_fill: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    uint16_t* tmax = (uint16_t*)ws;
    const dim3 grid(cdiv(W, NAT_TW), cdiv(H, NAT_TH));
    hipLaunchKernelGGL(natural_tilemax_kernel, grid, dim3(256), 0, s, d2, H, W, radius * radius, tmax);
    TG_CHECK_LAUNCH("natural_tilemax_kernel");
    hipLaunchKernelGGL(natural_fill_kernel, grid, dim3(256), nat_lds_bytes(radius), s, nn, d2, known, H, W, radius,
                       lim2 > 0 ? lim2 : 0, tmax, out, support, reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("natural_fill_kernel");
    return TG_OK;
}
