// Directional inverse-distance and nearest-neighbour void fills (mvp_gan/src/interpolate.py).
//
// Eight rays leave every unknown pixel (N, NE, E, SE, S, SW, W, NW); each stops at the first known pixel.  The rays are not
// walked: the column pass of csrc/edt.hip is applied to four families of lines (columns, rows, and the diagonals stepping
// (1, +1) and (1, -1)), 64 consecutive pixels of a line per 64-bit word, and the first known pixel before and after each word
// is carried along the line.  The fill kernel then reads four words per pixel, gets the eight ray lengths by count-leading /
// count-trailing zeros (a carry only where the word has no bit on that side), gathers at most eight heights and writes once.
//
//   ray_line_mask_kernel  one thread per line and 64-row band of the column and diagonal families: the band's known pixels of
//                         that line as one word (a pixel outside the raster is a 0 bit: a ray never re-enters a rectangle)
//   ray_row_mask_kernel   one wave per 64 pixels of a row: the word by ballot, stored [band][row] like the other families
//   ray_carry_kernel      one thread per line: the last known position before and the first one after every band
//   rayfill_kernel        the fill: fp64 sums without contraction, one division, one rounding to fp32
//   gather_fill_kernel    out = known ? z : z[idx] (NaN at idx < 0)
//   void_smooth_kernel    one Jacobi step of the 3x3 mean over the non-NaN pixels, on the unknown pixels only
//
// Determinism: integer atomics only (the three counters); every pixel's value is a function of its own reads.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

// The fp64 sums are compared bit for bit with a reference that does not fuse: no multiply-add contraction in this file.
#pragma clang fp contract(off)

constexpr int RAY_BAND = 64;
constexpr int RAY_MAX_SIDE = TG_EDT_MAX_SIDE;

// One family of lines.  Position t along a line is the row (columns, diagonals) or the column (rows); line l of the column
// family is column l, of the row family row l, of the (1, +1) diagonals x - y + H - 1, of the (1, -1) diagonals x + y.
struct RayFamily {
    uint64_t* word;      // [nb][lines]
    int32_t* before;     // [nb][lines]: the last known position before the band, -1: none
    int32_t* after;      // [nb][lines]: the first known position after the band, -1: none
    int nb, lines;
};

struct RayLayout {
    size_t word[4], before[4], after[4], total;
    int nb[4], lines[4];
};

static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

enum { FAM_COL = 0, FAM_ROW = 1, FAM_DIAG_SE = 2, FAM_DIAG_SW = 3 };

static RayLayout ray_layout(int H, int W) {
    RayLayout L;
    const int nbh = cdiv(H, RAY_BAND), nbw = cdiv(W, RAY_BAND);
    L.nb[FAM_COL] = nbh; L.lines[FAM_COL] = W;
    L.nb[FAM_ROW] = nbw; L.lines[FAM_ROW] = H;
    L.nb[FAM_DIAG_SE] = nbh; L.lines[FAM_DIAG_SE] = W + H - 1;
    L.nb[FAM_DIAG_SW] = nbh; L.lines[FAM_DIAG_SW] = W + H - 1;
    size_t o = 0;
    for (int f = 0; f < 4; ++f) {
        const size_t n = (size_t)L.nb[f] * L.lines[f];
        L.word[f] = o; o += al256(n * sizeof(uint64_t));
        L.before[f] = o; o += al256(n * sizeof(int32_t));
        L.after[f] = o; o += al256(n * sizeof(int32_t));
    }
    L.total = o;
    return L;
}

// ---- the words ----------------------------------------------------------------------------------------------------------
// step = 0: columns (line = x); step = +1: x = line - (H - 1) + y; step = -1: x = line - y.  Lanes run along the line index,
// so at a fixed row consecutive lanes read consecutive bytes whatever the step.
__global__ __launch_bounds__(256) void ray_line_mask_kernel(const uint8_t* __restrict__ known, int H, int W, int step, int lines,
                                                            uint64_t* __restrict__ word) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= lines) return;
    const int b = blockIdx.y, y0 = b * RAY_BAND;
    const int rows = H - y0 < RAY_BAND ? H - y0 : RAY_BAND;
    const int xbase = step > 0 ? l - (H - 1) : l;
    uint64_t m = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r, x = xbase + step * y;
        if (x >= 0 && x < W) m |= (uint64_t)(known[(int64_t)y * W + x] != 0) << r;
    }
    word[(int64_t)b * lines + l] = m;
}

__global__ __launch_bounds__(256) void ray_row_mask_kernel(const uint8_t* __restrict__ known, int H, int W, int nbw,
                                                           uint64_t* __restrict__ word) {
    const int y = blockIdx.y;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);            // wave-uniform
    if (b >= nbw) return;
    const int x = b * RAY_BAND + (threadIdx.x & 63);
    const int k = x < W ? known[(int64_t)y * W + x] != 0 : 0;
    const uint64_t m = __ballot(k);
    if ((threadIdx.x & 63) == 0) word[(int64_t)b * H + y] = m;
}

__global__ __launch_bounds__(256) void ray_carry_kernel(const uint64_t* __restrict__ word, int nb, int lines,
                                                        int32_t* __restrict__ before, int32_t* __restrict__ after) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= lines) return;
    int last = -1;
    for (int b = 0; b < nb; ++b) {
        const int64_t i = (int64_t)b * lines + l;
        before[i] = last;
        const uint64_t m = word[i];
        if (m) last = b * RAY_BAND + 63 - __clzll((long long)m);
    }
    int next = -1;
    for (int b = nb - 1; b >= 0; --b) {
        const int64_t i = (int64_t)b * lines + l;
        after[i] = next;
        const uint64_t m = word[i];
        if (m) next = b * RAY_BAND + __ffsll((long long)m) - 1;
    }
}

// ---- the fill -----------------------------------------------------------------------------------------------------------
// The distances from position t of a line to the nearest known position before (kb) and after (ka) it, 0: none.  The pixel
// itself is unknown, so its own bit is 0.
__device__ __forceinline__ void ray_pair(const RayFamily& F, int line, int t, int& kb, int& ka) {
    const int r = t & 63;
    const int64_t i = (int64_t)(t >> 6) * F.lines + line;
    const uint64_t m = F.word[i];
    const uint64_t lo = m & (~0ull >> (63 - r));
    const uint64_t hi = m >> r;
    if (lo) {
        kb = r - (63 - __clzll((long long)lo));
    } else {
        const int p = F.before[i];
        kb = p >= 0 ? t - p : 0;
    }
    if (hi) {
        ka = __ffsll((long long)hi) - 1;
    } else {
        const int p = F.after[i];
        ka = p >= 0 ? p - t : 0;
    }
}

struct RayArgs {
    const float* z;
    const uint8_t* known;
    int H, W;
    int32_t lim2;
    double nexp;         // -power / 2, read by the general-power kernel only
    const int32_t* d2;
    const int32_t* idx;
    float* out;
    uint16_t* hits;
    ull* counts;
    RayFamily fam[4];
};

template <int MODE>
__device__ __forceinline__ double ray_weight(int32_t n, double nexp) {
    const double d = (double)n;
    if (MODE == 2) return 1.0 / d;
    if (MODE == 1) return 1.0 / sqrt(d);
    return pow(d, nexp);
}

template <int MODE>
__global__ __launch_bounds__(256) void rayfill_kernel(RayArgs A) {
    __shared__ int red[3][4];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int H = A.H, W = A.W;
    int by_rays = 0, by_near = 0, left = 0;
    if (x < W) {
        const int64_t p = (int64_t)y * W + x;
        const int64_t plane = (int64_t)H * W;
        if (A.known[p]) {
            A.out[p] = A.z[p];
            if (A.hits) {
#pragma unroll
                for (int j = 0; j < 8; ++j) A.hits[j * plane + p] = 0;
            }
        } else {
            int k[8];                                               // N, NE, E, SE, S, SW, W, NW
            ray_pair(A.fam[FAM_COL], x, y, k[0], k[4]);
            ray_pair(A.fam[FAM_ROW], y, x, k[6], k[2]);
            ray_pair(A.fam[FAM_DIAG_SE], x - y + H - 1, y, k[7], k[3]);
            ray_pair(A.fam[FAM_DIAG_SW], x + y, y, k[1], k[5]);
            const int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
            const int dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
            double num = 0.0, den = 0.0;
            int nhit = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int kj = k[j];
                const int32_t n = kj * kj * ((j & 1) ? 2 : 1);      // <= 2 * 32766^2 < 2^31
                const int yy = y + kj * dy[j], xx = x + kj * dx[j];
                if ((A.lim2 > 0 && n > A.lim2) || (unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) kj = 0;
                if (A.hits) A.hits[j * plane + p] = (uint16_t)kj;
                if (kj) {
                    const double w = ray_weight<MODE>(n, A.nexp);
                    const double zj = (double)A.z[(int64_t)yy * W + xx];
                    num = num + w * zj;
                    den = den + w;
                    ++nhit;
                }
            }
            float v;
            if (nhit) {
                v = (float)(num / den);
                by_rays = 1;
            } else {
                v = __uint_as_float(0x7fc00000u);
                int32_t i = -1;
                if (A.idx) {
                    i = A.idx[p];
                    if (A.lim2 > 0) {
                        const int32_t d = A.d2[p];
                        if (d < 0 || d > A.lim2) i = -1;
                    }
                }
                if (i >= 0 && i < plane) {
                    v = A.z[i];
                    by_near = 1;
                } else {
                    left = 1;
                }
            }
            A.out[p] = v;
        }
    }
    // counters: per-wave popcounts, waves 0..3 through LDS, one integer atomic per counter and workgroup
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = __popcll(__ballot(by_rays)), c1 = __popcll(__ballot(by_near)), c2 = __popcll(__ballot(left));
    if (lane == 0) { red[0][w] = c0; red[1][w] = c1; red[2][w] = c2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (s) atomicAdd(&A.counts[threadIdx.x], (ull)s);
    }
}

__global__ __launch_bounds__(256) void gather_fill_kernel(const float* __restrict__ z, const uint8_t* __restrict__ known,
                                                          const int32_t* __restrict__ idx, int64_t n, float* __restrict__ out,
                                                          ull* __restrict__ counts) {
    __shared__ int red[2][4];
    int filled = 0, left = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (known[p]) {
            out[p] = z[p];
        } else {
            const int32_t i = idx[p];
            if (i >= 0 && i < n) {
                out[p] = z[i];
                ++filled;
            } else {
                out[p] = __uint_as_float(0x7fc00000u);
                ++left;
            }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        filled += __shfl_xor(filled, o, 64);
        left += __shfl_xor(left, o, 64);
    }
    if (lane == 0) { red[0][w] = filled; red[1][w] = left; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (s) atomicAdd(&counts[threadIdx.x], (ull)s);
    }
}

__global__ __launch_bounds__(256) void void_smooth_kernel(const float* __restrict__ in, const uint8_t* __restrict__ known, int H,
                                                          int W, float* __restrict__ out) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t p = (int64_t)y * W + x;
    const float c = in[p];
    if (known[p] || c != c) {
        out[p] = c;
        return;
    }
    double s = 0.0;
    int n = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const float v = in[(int64_t)yy * W + xx];
            if (v == v) {
                s = s + (double)v;
                ++n;
            }
        }
    }
    out[p] = (float)(s / (double)n);                                // n >= 1: the pixel itself
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int side_check(const char* who, int H, int W) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= RAY_MAX_SIDE && W <= RAY_MAX_SIDE, "%s: raster %dx%d: both sides must lie in [1, %d]",
               who, H, W, (int)RAY_MAX_SIDE);
    return TG_OK;
}

extern "C" size_t tg_rayfill_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > RAY_MAX_SIDE || W > RAY_MAX_SIDE) return 0;
    return ray_layout(H, W).total;
}

extern "C" int tg_rayfill(const float* z, const uint8_t* known, int H, int W, int32_t lim2, double power, const int32_t* d2,
                          const int32_t* idx, float* out, uint16_t* hits, int64_t* counts, void* ws, size_t ws_bytes,
                          tg_stream_t stream) {
    if (int rc = side_check("tg_rayfill", H, W)) return rc;
    TG_REQUIRE(z && known && out && counts && ws, "tg_rayfill: null pointer");
    TG_REQUIRE(!d2 == !idx, "tg_rayfill: d2 and idx go together (both NULL: no nearest-neighbour fallback)");
    TG_REQUIRE(isfinite(power) && power > 0.0 && power <= 8.0, "tg_rayfill: power %g must lie in (0, 8]", power);
    TG_REQUIRE(out != z, "tg_rayfill: out must not alias z");
    const RayLayout L = ray_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_rayfill: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_rayfill: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    RayArgs A;
    A.z = z; A.known = known; A.H = H; A.W = W; A.lim2 = lim2 > 0 ? lim2 : 0;
    A.nexp = -power / 2.0;
    A.d2 = d2; A.idx = idx; A.out = out; A.hits = hits; A.counts = reinterpret_cast<ull*>(counts);
    char* base = (char*)ws;
    for (int f = 0; f < 4; ++f) {
        A.fam[f].word = (uint64_t*)(base + L.word[f]);
        A.fam[f].before = (int32_t*)(base + L.before[f]);
        A.fam[f].after = (int32_t*)(base + L.after[f]);
        A.fam[f].nb = L.nb[f];
        A.fam[f].lines = L.lines[f];
    }
    const int steps[4] = {0, 0, 1, -1};
    for (int f = 0; f < 4; ++f) {
        const RayFamily& F = A.fam[f];
        if (f == FAM_ROW) {
            hipLaunchKernelGGL(ray_row_mask_kernel, dim3(cdiv(F.nb, 4), H), dim3(256), 0, s, known, H, W, F.nb, F.word);
            TG_CHECK_LAUNCH("ray_row_mask_kernel");
        } else {
            hipLaunchKernelGGL(ray_line_mask_kernel, dim3(cdiv(F.lines, 256), F.nb), dim3(256), 0, s, known, H, W, steps[f],
                               F.lines, F.word);
            TG_CHECK_LAUNCH("ray_line_mask_kernel");
        }
        hipLaunchKernelGGL(ray_carry_kernel, dim3(cdiv(F.lines, 256)), dim3(256), 0, s, F.word, F.nb, F.lines, F.before, F.after);
        TG_CHECK_LAUNCH("ray_carry_kernel");
    }
    const dim3 grid(cdiv(W, 256), H);
    if (power == 2.0) hipLaunchKernelGGL(rayfill_kernel<2>, grid, dim3(256), 0, s, A);
    else if (power == 1.0) hipLaunchKernelGGL(rayfill_kernel<1>, grid, dim3(256), 0, s, A);
    else hipLaunchKernelGGL(rayfill_kernel<0>, grid, dim3(256), 0, s, A);
    TG_CHECK_LAUNCH("rayfill_kernel");
    return TG_OK;
}

extern "C" int tg_gather_fill(const float* z, const uint8_t* known, const int32_t* idx, int H, int W, float* out, int64_t* counts,
                              tg_stream_t stream) {
    if (int rc = side_check("tg_gather_fill", H, W)) return rc;
    TG_REQUIRE(z && known && idx && out && counts, "tg_gather_fill: null pointer");
    TG_REQUIRE(out != z, "tg_gather_fill: out must not alias z");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_gather_fill: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(gather_fill_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, z, known, idx, n, out,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("gather_fill_kernel");
    return TG_OK;
}

extern "C" int tg_void_smooth(const float* in, const uint8_t* known, int H, int W, float* out, tg_stream_t stream) {
    if (int rc = side_check("tg_void_smooth", H, W)) return rc;
    TG_REQUIRE(in && known && out, "tg_void_smooth: null pointer");
    TG_REQUIRE(in != out, "tg_void_smooth: in and out must be distinct");
    hipLaunchKernelGGL(void_smooth_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, S(stream), in, known, H, W, out);
    TG_CHECK_LAUNCH("void_smooth_kernel");
    return TG_OK;
}
