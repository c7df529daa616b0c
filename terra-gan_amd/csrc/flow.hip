// D8 flow directions, flat resolution and flow accumulation of a raster (mvp_gan/src/flow_routing.py).
//
// Codes (uint8): 0 unknown; 1..8 the receiver E, SE, S, SW, W, NW, N, NE; 9 OUT (an outlet without a lower neighbour); 255 PIT;
// 254 "undecided" between tg_flow_slope and tg_flow_flat_dir.  Ties go E, S, W, N, SE, SW, NW, NE.
//
//   flow_slope_kernel      the steepest positive drop s = w(p) - w(n), times 0x1.6a09e6p-1f for a diagonal n (fp32, no
//                          contraction), or OUT, or undecided; D = 0 decided, INT32_MAX undecided, -1 unknown; known and outlet counts
//   flow_begin_kernel      one thread: zero `changed`, advance the sweep counter by n
//   flow_flat_sweep_kernel one workgroup per 64x64 tile: D(p) <- min(D(p), 1 + min over the equal-height neighbours D(n)), w and D
//                          with a one-pixel halo in LDS, relaxed to a local fixed point by directional line scans
//   flow_flat_dir_kernel   an undecided pixel with finite D flows to the equal-height neighbour with the smallest D below its own
//                          (D - 1 at the fixed point), else PIT; counts of both
//   flow_acc_init_kernel   next0 = the receiver's index or -1, S0 = 1 on known pixels, the other S plane 0, live[0]
//   flow_acc_round_kernel  round k of the pointer doubling: S(k+1)[p] += S(k)[p], S(k+1)[next(p)] += S(k)[p] by integer atomics,
//                          next <- next(next); the plane it read is left zero for round k + 1; live[k + 1]
//   flow_acc_state_kernel  one thread: the live count after the rounds enqueued and the number of rounds that ran
//   flow_acc_finish_kernel the S plane of the last round -> acc, and its maximum
//
// The flat sweep is depfill.hip's scheme: one D plane in place, halo loads and the write-back relaxed atomic 32-bit accesses, two
// dirty byte planes.  D only ever decreases towards the shortest-path distance, every value held is the length of a real path of
// equal-height pixels to a decided pixel or INT32_MAX, so a stale halo value delays the fixed point and never moves it.
//
// Determinism: directions and D are the unique fixed point; the accumulation is a sum of integers by integer atomics, exact in
// any order.  The number of sweeps and visits may differ between runs.
#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

// s = d * 0x1.6a09e6p-1f is one fp32 multiply after one fp32 subtract: nothing is fused in this file.
#pragma clang fp contract(off)

constexpr int FL_T = 64;                 // tile side
constexpr int FL_R = FL_T + 2;           // rows and columns with the halo
constexpr int FL_S = FL_T + 3;           // LDS row stride in words: odd, so a wave is conflict-free along rows and along columns
constexpr int FL_ROUNDS = 64;            // cap on the inner rounds of one visit; a tile that hits it stays dirty
constexpr int FL_CTL_BYTES = 256;        // int32 [0]: sweeps enqueued since tg_flow_slope; [8 .. 40]: live[k] of the doubling
constexpr int FL_LIVE = 8;               // first word of live[0 .. 32]
constexpr int FL_MAX_ROUNDS = 32;
constexpr int FL_FAR = 0x7fffffff;
constexpr int FL_UNDECIDED = TG_FLOW_UNDECIDED;

static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

struct FlLayout {
    size_t ctl, plane[2], next[2], sum[2], total;
    int ty, tx;
};

static FlLayout fl_layout(int H, int W) {
    FlLayout L;
    L.ty = cdiv(H, FL_T);
    L.tx = cdiv(W, FL_T);
    const size_t tiles = (size_t)L.ty * L.tx, px = al256((size_t)H * W * 4);
    size_t o = 0;
    L.ctl = o; o += FL_CTL_BYTES;
    L.plane[0] = o; o += al256(tiles);
    L.plane[1] = o; o += al256(tiles);
    L.next[0] = o; o += px;
    L.next[1] = o; o += px;
    L.sum[0] = o; o += px;
    L.sum[1] = o; o += px;
    L.total = o;
    return L;
}

// code - 1 -> (dy, dx): E, SE, S, SW, W, NW, N, NE; the order of preference as codes - 1
__host__ __device__ constexpr int fl_dy(int k) { return ((0x01a9 >> (2 * k)) & 3) - 1; }     // 0, 1, 1, 1, 0, -1, -1, -1
__host__ __device__ constexpr int fl_dx(int k) { return ((0x901a >> (2 * k)) & 3) - 1; }     // 1, 1, 0, -1, -1, -1, 0, 1
static_assert(fl_dy(0) == 0 && fl_dy(1) == 1 && fl_dy(2) == 1 && fl_dy(3) == 1 && fl_dy(4) == 0 && fl_dy(5) == -1 &&
              fl_dy(6) == -1 && fl_dy(7) == -1, "dy");
static_assert(fl_dx(0) == 1 && fl_dx(1) == 1 && fl_dx(2) == 0 && fl_dx(3) == -1 && fl_dx(4) == -1 && fl_dx(5) == -1 &&
              fl_dx(6) == 0 && fl_dx(7) == 1, "dx");
#define FL_PREF(i) ((((i) & 3) << 1) | ((i) >> 2))          // 0, 2, 4, 6, 1, 3, 5, 7

// ---- slope --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_slope_kernel(const float* __restrict__ w, const uint8_t* __restrict__ known, int H, int W,
                                                         uint8_t* __restrict__ dir, int32_t* __restrict__ D,
                                                         ull* __restrict__ counts) {
    const int64_t n = (int64_t)H * W;
    int nk = 0, no = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!known[p]) {
            dir[p] = 0;
            D[p] = -1;
            continue;
        }
        ++nk;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const float wp = w[p];
        bool outlet = false;
        float best = 0.f;
        int code = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = FL_PREF(i);
            const int yy = y + fl_dy(k), xx = x + fl_dx(k);
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) {
                outlet = true;
                continue;
            }
            const int64_t q = (int64_t)yy * W + xx;
            if (!known[q]) {
                outlet = true;
                continue;
            }
            float s = wp - w[q];
            if (k & 1) s = s * 0x1.6a09e6p-1f;
            if (s > best) {                                         // strict: the first of equals in the order of preference
                best = s;
                code = k + 1;
            }
        }
        if (!code) {
            if (outlet) code = TG_FLOW_OUT;
            else code = FL_UNDECIDED;
        }
        if (outlet) ++no;
        dir[p] = (uint8_t)code;
        D[p] = code == FL_UNDECIDED ? FL_FAR : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nk += __shfl_xor(nk, o, 64);
        no += __shfl_xor(no, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nk) atomicAdd(counts, (ull)nk);
        if (no) atomicAdd(counts + 1, (ull)no);
    }
}

__global__ void flow_begin_kernel(int32_t* __restrict__ ctl, int n, int32_t* __restrict__ changed) {
    if (threadIdx.x == 0) {
        ctl[0] = (ctl[0] + n) & 0x3fffffff;                         // only its parity is used
        changed[0] = 0;
    }
}

// ---- the flat sweep -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_flat_sweep_kernel(const float* __restrict__ w, int H, int W, int tiles_y, int tiles_x,
                                                              int32_t* D, const int32_t* __restrict__ ctl, int n, int j,
                                                              uint8_t* plane0, uint8_t* plane1, int32_t* changed, ull* visits) {
    __shared__ float hs[FL_R * FL_S];                               // heights (NaN: not a pixel), then the interior's neighbour masks
    __shared__ int32_t ds[FL_R * FL_S];
    const int tile = blockIdx.x;
    const int sweep = ctl[0] - n + j;                               // begin_kernel has added n already
    uint8_t* cur = (sweep & 1) ? plane1 : plane0;
    uint8_t* nxt = (sweep & 1) ? plane0 : plane1;
    if (!cur[tile]) return;                                         // uniform: a clean tile
    const int t = threadIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * FL_T, x0 = tx * FL_T;
    const float nan = __uint_as_float(0x7fc00000u);

    // stage: unknown and out-of-raster positions hold NaN and INT32_MAX, so no neighbour test below needs a bounds or mask test
    int open = 0;
    for (int i = t; i < FL_R * FL_R; i += 256) {
        const int ly = i / FL_R, lx = i - ly * FL_R;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        float h = nan;
        int32_t d = FL_FAR;
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
            const int64_t p = (int64_t)gy * W + gx;
            const bool interior = ly >= 1 && ly <= FL_T && lx >= 1 && lx <= FL_T;
            d = interior ? D[p] : __hip_atomic_load(D + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d >= 0) {
                h = w[p];
                if (interior && d > 0) open = 1;
            } else {
                d = FL_FAR;                                         // unknown
            }
        }
        hs[ly * FL_S + lx] = h;
        ds[ly * FL_S + lx] = d;
    }
    if (!__syncthreads_or(open)) {                                  // every pixel of the tile is decided or unknown
        if (t == 0) {
            cur[tile] = 0;
            atomicAdd(visits, 1ull);
        }
        return;
    }

    // the heights never change: bit k of a pixel's mask says that neighbour k (code k + 1) has its height; 0 for a decided or
    // unknown pixel, which is never updated.  The masks replace the interior of the height image.
    uint32_t mk[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = t + 256 * q;
        const int idx = ((i >> 6) + 1) * FL_S + (i & 63) + 1;
        const float h = hs[idx];
        uint32_t m = 0;
        if (ds[idx] > 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (hs[idx + fl_dy(k) * FL_S + fl_dx(k)] == h) m |= 1u << k;
        }
        mk[q] = m;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = t + 256 * q;
        hs[((i >> 6) + 1) * FL_S + (i & 63) + 1] = __uint_as_float(mk[q]);
    }
    __syncthreads();

    // relax: thread = one line (a column in rounds 0, 1; a row in rounds 2, 3) and one band of 16 pixels along it, scanned
    // forwards or backwards, so a lowered value travels a whole band within the round.  A value read may be a neighbour
    // thread's old or new one: both are lengths of real paths, and the last round, in which nobody writes, sees final values.
    const int line = t & 63, band = t >> 6;
    const bool line_rim = line == 0 || line == FL_T - 1;
    int any = 0, rim = 0, round = 0, live = 1;
    for (; round < FL_ROUNDS && live; ++round) {
        const int dirn = round & 3;
        const int back = dirn & 1;
        int c = band * 16 + (back ? 15 : 0);                        // coordinate along the line
        const int sgn = back ? -1 : 1;
        int step, idx;
        if (dirn < 2) { step = sgn * FL_S; idx = (c + 1) * FL_S + line + 1; }
        else          { step = sgn; idx = (line + 1) * FL_S + c + 1; }
        int lowered = 0;
        for (int k = 0; k < 16; ++k) {
            const uint32_t m = __float_as_uint(hs[idx]);
            if (m) {
                uint32_t nb = (uint32_t)FL_FAR;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const uint32_t v = (uint32_t)ds[idx + fl_dy(b) * FL_S + fl_dx(b)];
                    nb = (m >> b & 1) ? (v < nb ? v : nb) : nb;
                }
                if (nb + 1u < (uint32_t)ds[idx]) {                  // INT32_MAX + 1 is larger than every D as unsigned
                    ds[idx] = (int32_t)(nb + 1u);
                    lowered = 1;
                    if (line_rim || c == 0 || c == FL_T - 1) rim = 1;
                }
            }
            idx += step;
            c += sgn;
        }
        any |= lowered;
        live = __syncthreads_or(lowered);
    }
    any = __syncthreads_or(any);
    if (!any) {                                                     // nothing to write, nobody to wake
        if (t == 0) {
            cur[tile] = 0;
            atomicAdd(visits, 1ull);
        }
        return;
    }
    rim = __syncthreads_or(rim);

    // write back the reached undecided pixels (a decided one keeps its 0, an unknown one its -1, an unreached one INT32_MAX)
    for (int i = t; i < FL_T * FL_T; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < H && gx < W) {
            const int32_t v = ds[(ly + 1) * FL_S + lx + 1];
            if (v > 0 && v < FL_FAR) __hip_atomic_store(D + (int64_t)gy * W + gx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (t == 0) {
        cur[tile] = 0;
        atomicAdd(visits, 1ull);
        if (j == n - 1) atomicAdd(changed, 1);
    }
    // marks: itself, and after a lowered rim value the eight neighbour tiles (the same byte value from every writer)
    if (t < 9) {
        const int ny = ty + t / 3 - 1, nx = tx + t % 3 - 1;
        if ((t == 4 || rim) && ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
            __hip_atomic_store(nxt + (int64_t)ny * tiles_x + nx, (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- flat directions ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_flat_dir_kernel(const float* __restrict__ w, const int32_t* __restrict__ D, int H, int W,
                                                            uint8_t* __restrict__ dir, ull* __restrict__ counts) {
    const int64_t n = (int64_t)H * W;
    int nf = 0, np = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (dir[p] != FL_UNDECIDED) continue;
        const int32_t dp = D[p];
        int code = TG_FLOW_PIT;
        if (dp > 0 && dp < FL_FAR) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            const float wp = w[p];
            int32_t best = dp;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = FL_PREF(i);
                const int yy = y + fl_dy(k), xx = x + fl_dx(k);
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                const int64_t q = (int64_t)yy * W + xx;
                const int32_t dq = D[q];
                if (dq >= 0 && dq < best && w[q] == wp) {           // strict: the first of equals in the order of preference
                    best = dq;
                    code = k + 1;
                }
            }
        }
        if (code == TG_FLOW_PIT) ++np;
        else ++nf;
        dir[p] = (uint8_t)code;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o, 64);
        np += __shfl_xor(np, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(counts, (ull)nf);
        if (np) atomicAdd(counts + 1, (ull)np);
    }
}

// ---- accumulation -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fl_count_live(int alive, int32_t* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o, 64);
    if ((threadIdx.x & 63) == 0 && alive) atomicAdd(dst, alive);
}

__global__ __launch_bounds__(256) void flow_acc_init_kernel(const uint8_t* __restrict__ dir, int H, int W, int32_t* __restrict__ next,
                                                            int32_t* __restrict__ s0, int32_t* __restrict__ s1,
                                                            int32_t* __restrict__ live) {
    const int64_t n = (int64_t)H * W;
    int alive = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int code = dir[p];
        int32_t nx = -1;
        if (code >= 1 && code <= 8) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            const int yy = y + fl_dy(code - 1), xx = x + fl_dx(code - 1);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) nx = (int32_t)((int64_t)yy * W + xx);
        }
        next[p] = nx;
        s0[p] = code != 0;
        s1[p] = 0;
        alive += nx >= 0;
    }
    fl_count_live(alive, live);
}

// live points at live[k]: round k runs only while a pointer is left, and counts those left after it into live[k + 1]
__global__ __launch_bounds__(256) void flow_acc_round_kernel(int64_t n, const int32_t* __restrict__ next_in,
                                                             int32_t* __restrict__ next_out, int32_t* s_in, int32_t* s_out,
                                                             int32_t* live) {
    if (live[0] == 0) return;                                       // uniform: nothing is left to add
    int alive = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int32_t nx = next_in[p];
        const int32_t s = s_in[p];                                  // only this thread touches s_in[p] in this round
        int32_t nn = -1;
        if (s) {
            s_in[p] = 0;                                            // the zero plane of the next round
            atomicAdd(s_out + p, s);
            if (nx >= 0) {
                atomicAdd(s_out + nx, s);
                nn = next_in[nx];
            }
        }
        next_out[p] = nn;
        alive += nn >= 0;
    }
    fl_count_live(alive, live + 1);
}

__global__ void flow_acc_state_kernel(const int32_t* __restrict__ live, int k_end, int32_t* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int k = 0;
    while (k < k_end && live[k] != 0) ++k;                          // round k ran iff live[k] != 0
    state[0] = live[k];
    state[1] = k;
}

__global__ __launch_bounds__(256) void flow_acc_finish_kernel(const int32_t* __restrict__ s, int64_t n, int32_t* __restrict__ acc,
                                                              int32_t* __restrict__ amax) {
    int32_t m = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int32_t v = s[p];
        acc[p] = v;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t m2 = __shfl_xor(m, o, 64);
        m = m2 > m ? m2 : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(amax, m);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int fl_size_check(const char* who, int H, int W) {
    TG_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: raster %dx%d must be non-empty with H*W < 2^31", who,
               H, W);
    return TG_OK;
}

extern "C" size_t tg_flow_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    return fl_layout(H, W).total;
}

extern "C" int tg_flow_slope(const float* w, const uint8_t* known, int H, int W, uint8_t* dir, int32_t* D, int64_t* counts,
                             void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_slope", H, W)) return rc;
    TG_REQUIRE(w && known && dir && D && counts && ws, "tg_flow_slope: null pointer");
    TG_REQUIRE(dir != known && (const void*)D != (const void*)w, "tg_flow_slope: dir must not alias known, nor D w");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_slope: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    const size_t tiles = (size_t)L.ty * L.tx;
    if (hipMemsetAsync(base + L.ctl, 0, FL_CTL_BYTES, s) != hipSuccess ||
        hipMemsetAsync(base + L.plane[0], 1, tiles, s) != hipSuccess ||
        hipMemsetAsync(base + L.plane[1], 0, tiles, s) != hipSuccess ||
        hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flow_slope: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(flow_slope_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, w, known, H, W, dir, D,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("flow_slope_kernel");
    return TG_OK;
}

extern "C" int tg_flow_flat_sweep(const float* w, int H, int W, int n, int32_t* D, int32_t* changed, int64_t* visits, void* ws,
                                  size_t ws_bytes, tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_flat_sweep", H, W)) return rc;
    TG_REQUIRE(w && D && changed && visits && ws, "tg_flow_flat_sweep: null pointer");
    TG_REQUIRE(n >= 1 && n <= (1 << 20), "tg_flow_flat_sweep: n = %d sweeps must lie in [1, 2^20]", n);
    TG_REQUIRE((const void*)D != (const void*)w, "tg_flow_flat_sweep: D must not alias w");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_flat_sweep: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* ctl = (int32_t*)(base + L.ctl);
    uint8_t* p0 = (uint8_t*)(base + L.plane[0]);
    uint8_t* p1 = (uint8_t*)(base + L.plane[1]);
    hipLaunchKernelGGL(flow_begin_kernel, dim3(1), dim3(64), 0, s, ctl, n, changed);
    TG_CHECK_LAUNCH("flow_begin_kernel");
    const dim3 grid(L.ty * L.tx);                                   // < 2^31 / 4096
    for (int j = 0; j < n; ++j) {
        hipLaunchKernelGGL(flow_flat_sweep_kernel, grid, dim3(256), 0, s, w, H, W, L.ty, L.tx, D, ctl, n, j, p0, p1, changed,
                           reinterpret_cast<ull*>(visits));
        TG_CHECK_LAUNCH("flow_flat_sweep_kernel");
    }
    return TG_OK;
}

extern "C" int tg_flow_flat_dir(const float* w, const int32_t* D, int H, int W, uint8_t* dir, int64_t* counts,
                                tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_flat_dir", H, W)) return rc;
    TG_REQUIRE(w && D && dir && counts, "tg_flow_flat_dir: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flow_flat_dir: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(flow_flat_dir_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, w, D, H, W, dir,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("flow_flat_dir_kernel");
    return TG_OK;
}

extern "C" int tg_flow_accum_init(const uint8_t* dir, int H, int W, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_accum_init", H, W)) return rc;
    TG_REQUIRE(dir && ws, "tg_flow_accum_init: null pointer");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_accum_init: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* live = (int32_t*)(base + L.ctl) + FL_LIVE;
    if (hipMemsetAsync(live, 0, (FL_MAX_ROUNDS + 1) * sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("tg_flow_accum_init: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(flow_acc_init_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, dir, H, W,
                       (int32_t*)(base + L.next[0]), (int32_t*)(base + L.sum[0]), (int32_t*)(base + L.sum[1]), live);
    TG_CHECK_LAUNCH("flow_acc_init_kernel");
    return TG_OK;
}

extern "C" int tg_flow_accum(int H, int W, int k0, int n, int32_t* state, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_accum", H, W)) return rc;
    TG_REQUIRE(state && ws, "tg_flow_accum: null pointer");
    TG_REQUIRE(k0 >= 0 && n >= 1 && k0 <= FL_MAX_ROUNDS && n <= FL_MAX_ROUNDS - k0,
               "tg_flow_accum: rounds k0 = %d, n = %d must satisfy k0 >= 0, n >= 1, k0 + n <= %d", k0, n, FL_MAX_ROUNDS);
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_accum: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* live = (int32_t*)(base + L.ctl) + FL_LIVE;
    const int64_t px = (int64_t)H * W;
    const dim3 grid(ew_grid(px, 256));
    for (int k = k0; k < k0 + n; ++k) {
        const int a = k & 1, b = a ^ 1;
        hipLaunchKernelGGL(flow_acc_round_kernel, grid, dim3(256), 0, s, px, (const int32_t*)(base + L.next[a]),
                           (int32_t*)(base + L.next[b]), (int32_t*)(base + L.sum[a]), (int32_t*)(base + L.sum[b]), live + k);
        TG_CHECK_LAUNCH("flow_acc_round_kernel");
    }
    hipLaunchKernelGGL(flow_acc_state_kernel, dim3(1), dim3(64), 0, s, live, k0 + n, state);
    TG_CHECK_LAUNCH("flow_acc_state_kernel");
    return TG_OK;
}

extern "C" int tg_flow_accum_finish(int H, int W, int rounds, int32_t* acc, int32_t* amax, void* ws, size_t ws_bytes,
                                    tg_stream_t stream) {
    if (int rc = fl_size_check("tg_flow_accum_finish", H, W)) return rc;
    TG_REQUIRE(acc && amax && ws, "tg_flow_accum_finish: null pointer");
    TG_REQUIRE(rounds >= 0 && rounds <= FL_MAX_ROUNDS, "tg_flow_accum_finish: rounds = %d must lie in [0, %d]", rounds,
               FL_MAX_ROUNDS);
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_accum_finish: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(amax, 0, sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("tg_flow_accum_finish: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(flow_acc_finish_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s,
                       (const int32_t*)((char*)ws + L.sum[rounds & 1]), px, acc, amax);
    TG_CHECK_LAUNCH("flow_acc_finish_kernel");
    return TG_OK;
}
