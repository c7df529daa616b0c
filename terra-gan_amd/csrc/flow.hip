// D8 flow directions, flat resolution and flow accumulation of a raster (mvp_gan/src/flow_routing.py).
//
// Codes (uint8): 0 unknown; 1..8 the receiver E, SE, S, SW, W, NW, N, NE; 9 OUT (an outlet without a lower neighbour); 255 PIT;
// 254 "undecided" between tg_flow_slope and tg_flow_flat_dir.  Ties go E, S, W, N, SE, SW, NW, NE.
//
//   flow_slope_kernel      the steepest positive drop s = w(p) - w(n), times 0x1.6a09e6p-1f for a diagonal n (fp32, no
//                          contraction), or OUT, or undecided; D = 0 decided, INT32_MAX undecided, -1 unknown; known and outlet counts
//   sweep_begin_kernel     (raster_sweep.h) one thread: zero `changed`, advance the sweep counter by n
//   flow_flat_sweep_kernel one workgroup per 64x64 tile: D(p) <- min(D(p), 1 + min over the equal-height neighbours D(n)), w and D
//                          with a one-pixel halo in LDS, relaxed to a local fixed point by directional line scans
//   flow_flat_dir_kernel   an undecided pixel with finite D flows to the equal-height neighbour with the smallest D below its own
//                          (D - 1 at the fixed point), else PIT; counts of both
//   flow_acc_init_kernel   next0 = the receiver's index or -1, S0 = 1 on known pixels, the other S plane 0, live[0]
//   flow_acc_round_kernel  round k of the pointer doubling: S(k+1)[p] += S(k)[p], S(k+1)[next(p)] += S(k)[p] by integer atomics,
//                          next <- next(next); the plane it read is left zero for round k + 1; live[k + 1]
//   doubling_state_kernel  (raster_sweep.h) one thread: the live count after the rounds enqueued and the number of rounds that ran
//   flow_acc_finish_kernel the S plane of the last round -> acc, and its maximum
//
// The flat sweep follows the tile-sweep protocol and the accumulation the pointer-doubling protocol of raster_sweep.h.  D only ever
// decreases towards the shortest-path distance, and every value held is the length of a real path of equal-height pixels to a
// decided pixel or INT32_MAX.
//
// Determinism: directions and D are the unique fixed point; the accumulation is a sum of integers by integer atomics, exact in
// any order.  The number of sweeps and visits may differ between runs.
#include "raster_sweep.h"

// s = d * 0x1.6a09e6p-1f is one fp32 multiply after one fp32 subtract: nothing is fused in this file.
#pragma clang fp contract(off)

constexpr int FL_T = SW_T, FL_R = SW_R, FL_S = SW_S;
constexpr int FL_ROUNDS = 64;            // cap on the inner rounds of one visit; a tile that hits it stays dirty
constexpr int FL_FAR = 0x7fffffff;
constexpr int FL_UNDECIDED = TG_FLOW_UNDECIDED;

struct FlLayout : SweepLayout {
    size_t next[2], sum[2], total;
};

static FlLayout fl_layout(int H, int W) {
    FlLayout L;
    size_t o;
    static_cast<SweepLayout&>(L) = sweep_layout(H, W, o);
    const size_t px = al256((size_t)H * W * 4);
    L.next[0] = o; o += px;
    L.next[1] = o; o += px;
    L.sum[0] = o; o += px;
    L.sum[1] = o; o += px;
    L.total = o;
    return L;
}

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
            const int yy = y + d8_dy(k), xx = x + d8_dx(k);
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

// ---- the flat sweep -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_flat_sweep_kernel(const float* __restrict__ w, int H, int W, int tiles_y, int tiles_x,
                                                              int32_t* D, const int32_t* __restrict__ ctl, int n, int j,
                                                              uint8_t* plane0, uint8_t* plane1, int32_t* changed, ull* visits) {
    __shared__ float hs[FL_R * FL_S];                               // heights (NaN: not a pixel), then the interior's neighbour masks
    __shared__ int32_t ds[FL_R * FL_S];
    SweepVisit v = sweep_visit_begin(ctl, n, j, plane0, plane1);
    if (!v.marked) return;                                          // uniform: a clean tile
    sweep_visit_place(v, tiles_x);
    const int t = threadIdx.x;
    const int y0 = v.y0, x0 = v.x0;
    const float nan = __uint_as_float(0x7fc00000u);

    // stage: unknown and out-of-raster positions hold NaN and INT32_MAX, so no neighbour test below needs a bounds or mask test
    int open = 0;
    for (int i = t; i < FL_R * FL_R; i += 256) {
        const SweepStage g = sweep_stage(i, y0, x0, H, W);
        float h = nan;
        int32_t d = FL_FAR;
        if (g.in_raster) {
            const int64_t p = (int64_t)g.gy * W + g.gx;
            d = g.interior() ? D[p] : __hip_atomic_load(D + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d >= 0) {
                h = w[p];
                if (g.interior() && d > 0) open = 1;
            } else {
                d = FL_FAR;                                         // unknown
            }
        }
        hs[g.ly * FL_S + g.lx] = h;
        ds[g.ly * FL_S + g.lx] = d;
    }
    if (!__syncthreads_or(open)) {                                  // every pixel of the tile is decided or unknown
        sweep_visit_end(v, tiles_y, tiles_x, visits, false, false);
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
                if (hs[idx + d8_dy(k) * FL_S + d8_dx(k)] == h) m |= 1u << k;
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

    // relax by the line scans of raster_sweep.h: thread = one line and one band of 16 pixels along it.  A value read may be a
    // neighbour thread's old or new one: both are lengths of real paths, and the last round, in which nobody writes, sees final
    // values.
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
                    const uint32_t dn = (uint32_t)ds[idx + d8_dy(b) * FL_S + d8_dx(b)];
                    nb = (m >> b & 1) ? (dn < nb ? dn : nb) : nb;
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
        sweep_visit_end(v, tiles_y, tiles_x, visits, false, false);
        return;
    }
    rim = __syncthreads_or(rim);

    // write back the reached undecided pixels (a decided one keeps its 0, an unknown one its -1, an unreached one INT32_MAX)
    for (int i = t; i < FL_T * FL_T; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < H && gx < W) {
            const int32_t d = ds[(ly + 1) * FL_S + lx + 1];
            if (d > 0 && d < FL_FAR) __hip_atomic_store(D + (int64_t)gy * W + gx, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (t == 0 && j == n - 1) atomicAdd(changed, 1);
    sweep_visit_end(v, tiles_y, tiles_x, visits, true, rim != 0);   // marks: itself, and after a lowered rim value its neighbours
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
                const int yy = y + d8_dy(k), xx = x + d8_dx(k);
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
            const int yy = y + d8_dy(code - 1), xx = x + d8_dx(code - 1);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) nx = (int32_t)((int64_t)yy * W + xx);
        }
        next[p] = nx;
        s0[p] = code != 0;
        s1[p] = 0;
        alive += nx >= 0;
    }
    count_live(alive, live);
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
    count_live(alive, live + 1);
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
extern "C" size_t tg_flow_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return fl_layout(H, W).total;
}

extern "C" int tg_flow_slope(const float* w, const uint8_t* known, int H, int W, uint8_t* dir, int32_t* D, int64_t* counts,
                             void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_slope", H, W)) return rc;
    TG_REQUIRE(w && known && dir && D && counts && ws, "tg_flow_slope: null pointer");
    TG_REQUIRE(dir != known && (const void*)D != (const void*)w, "tg_flow_slope: dir must not alias known, nor D w");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_slope: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    if (!sweep_reset(L, ws, s) || hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
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
    if (int rc = raster_size_check("tg_flow_flat_sweep", H, W)) return rc;
    TG_REQUIRE(w && D && changed && visits && ws, "tg_flow_flat_sweep: null pointer");
    TG_REQUIRE(n >= 1 && n <= (1 << 20), "tg_flow_flat_sweep: n = %d sweeps must lie in [1, 2^20]", n);
    TG_REQUIRE((const void*)D != (const void*)w, "tg_flow_flat_sweep: D must not alias w");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_flat_sweep: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    return sweep_run(L, ws, n, changed, s, "flow_begin_kernel", "flow_flat_sweep_kernel",
                     [&](dim3 grid, const int32_t* ctl, int j, uint8_t* p0, uint8_t* p1) {
                         hipLaunchKernelGGL(flow_flat_sweep_kernel, grid, dim3(256), 0, s, w, H, W, L.ty, L.tx, D, ctl, n, j, p0, p1,
                                            changed, reinterpret_cast<ull*>(visits));
                     });
}

extern "C" int tg_flow_flat_dir(const float* w, const int32_t* D, int H, int W, uint8_t* dir, int64_t* counts,
                                tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_flat_dir", H, W)) return rc;
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
    if (int rc = raster_size_check("tg_flow_accum_init", H, W)) return rc;
    TG_REQUIRE(dir && ws, "tg_flow_accum_init: null pointer");
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_accum_init: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* live = (int32_t*)(base + L.ctl) + DBL_LIVE;
    if (hipMemsetAsync(live, 0, (DBL_MAX_ROUNDS + 1) * sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("tg_flow_accum_init: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(flow_acc_init_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, dir, H, W,
                       (int32_t*)(base + L.next[0]), (int32_t*)(base + L.sum[0]), (int32_t*)(base + L.sum[1]), live);
    TG_CHECK_LAUNCH("flow_acc_init_kernel");
    return TG_OK;
}

extern "C" int tg_flow_accum(int H, int W, int k0, int n, int32_t* state, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_accum", H, W)) return rc;
    TG_REQUIRE(state && ws, "tg_flow_accum: null pointer");
    if (int rc = doubling_rounds_check("tg_flow_accum", k0, n)) return rc;
    const FlLayout L = fl_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_accum: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    const int64_t px = (int64_t)H * W;
    const dim3 grid(ew_grid(px, 256));
    return doubling_run(k0, n, (int32_t*)(base + L.ctl) + DBL_LIVE, state, s, "flow_acc_round_kernel", "flow_acc_state_kernel",
                        [&](int k, int32_t* live) {
                            const int a = k & 1, b = a ^ 1;
                            hipLaunchKernelGGL(flow_acc_round_kernel, grid, dim3(256), 0, s, px, (const int32_t*)(base + L.next[a]),
                                               (int32_t*)(base + L.next[b]), (int32_t*)(base + L.sum[a]),
                                               (int32_t*)(base + L.sum[b]), live);
                        });
}

extern "C" int tg_flow_accum_finish(int H, int W, int rounds, int32_t* acc, int32_t* amax, void* ws, size_t ws_bytes,
                                    tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_accum_finish", H, W)) return rc;
    TG_REQUIRE(acc && amax && ws, "tg_flow_accum_finish: null pointer");
    TG_REQUIRE(rounds >= 0 && rounds <= DBL_MAX_ROUNDS, "tg_flow_accum_finish: rounds = %d must lie in [0, %d]", rounds,
               DBL_MAX_ROUNDS);
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
