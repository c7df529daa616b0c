// Watersheds, flow length and the drainage comparison of two routings (mvp_gan/src/flow_routing.py watersheds,
// mvp_gan/src/evaluate_raster.py drainage_errors); below them the stream classes, links and Strahler orders,
// the height above the nearest drainage and the flood comparison (stream_network, hand, flood_errors), which
// run the same doubling upstream along the streams.
//
// A pixel's state is one 16-byte record (next, last, nc, nd): the pixel 2^k steps downstream (-1: the path has ended), the last
// pixel reached, and the cardinal and diagonal steps taken to it.  Two planes of records in the workspace: round k reads plane
// k & 1 and writes the other, so no record a round reads is written by it, and the four words of q = next(p) come from one
// iterate in one 16-byte load.
//
//   basin_init_kernel     the start state (next0, p, c0, d0) into plane 0; (-1, -1, 0, 0) at unknown pixels; live[0]; pour counts
//   basin_round_kernel    a live pixel takes (next(q), last(q), nc + nc(q), nd + nd(q)); any other pixel copies its record, so the
//                         plane of every later round holds its final record; live[k + 1]
//   doubling_state_kernel (raster_sweep.h) one thread: the live count after the rounds enqueued and the number of rounds that ran
//   basin_finish_kernel  last -> basin, nc, nd, the length in metres; terminals, the largest nc + nd and length
//   flow_compare_kernel   the 19 integer counters of two routings over the selected pixels
//
// live[], the rounds and the state follow the pointer-doubling protocol of raster_sweep.h, whose D8 tables these kernels use too.
// A round moves 32 bytes per pixel (its record read and written) and 16 more per pixel whose pointer is live (the gather).
//
// Determinism: gathers and plain stores only on the rasters; the counters are sums and maxima of integers by integer atomics,
// exact in any order.
#include "raster_sweep.h"

// length_m is one fp64 multiply, one add, one multiply, one rounding to fp32: nothing is fused in this file.
#pragma clang fp contract(off)

constexpr int DR_NCMP = TG_FLOW_COMPARE_COUNTS;

struct DrLayout {
    size_t ctl, rec[2], total;
};

static DrLayout dr_layout(int H, int W) {
    DrLayout L;
    const size_t px = al256((size_t)H * W * 16);
    size_t o = 0;
    L.ctl = o; o += SW_CTL_BYTES;
    L.rec[0] = o; o += px;
    L.rec[1] = o; o += px;
    L.total = o;
    return L;
}

// ---- the doubling -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void basin_init_kernel(const uint8_t* __restrict__ dir, const uint8_t* __restrict__ pour, int H,
                                                         int W, int4* __restrict__ rec, int32_t* __restrict__ live,
                                                         ull* __restrict__ counts) {
    const int64_t n = (int64_t)H * W;
    int alive = 0, used = 0, ignored = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int code = dir[p];
        const bool pp = pour && pour[p] != 0;
        int4 r = make_int4(-1, code ? (int32_t)p : -1, 0, 0);
        if (pp) {
            if (code) ++used;
            else ++ignored;
        } else if (code >= 1 && code <= 8) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            const int yy = y + d8_dy(code - 1), xx = x + d8_dx(code - 1);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                r.x = (int32_t)((int64_t)yy * W + xx);
                r.z = (code & 1) ? 1 : 0;                           // codes 1, 3, 5, 7 are E, S, W, N
                r.w = (code & 1) ? 0 : 1;
            }
        }
        rec[p] = r;
        alive += r.x >= 0;
    }
    count_live(alive, live);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        used += __shfl_xor(used, o, 64);
        ignored += __shfl_xor(ignored, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (used) atomicAdd(counts, (ull)used);
        if (ignored) atomicAdd(counts + 1, (ull)ignored);
    }
}

// live points at live[k]: round k runs only while a pointer is left, and counts those left after it into live[k + 1]
__global__ __launch_bounds__(256) void basin_round_kernel(int64_t n, const int4* __restrict__ in, int4* __restrict__ out,
                                                          int32_t* live) {
    if (live[0] == 0) return;                                       // uniform: every path has ended
    int alive = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        int4 r = in[p];
        if ((uint32_t)r.x < (uint32_t)n) {                          // a receiver's index (n < 2^31; -1 is not below it)
            const int4 q = in[r.x];                                 // one 16-byte load: the four words of one iterate
            r.x = q.x;
            r.y = q.y;
            r.z += q.z;
            r.w += q.w;
        }
        out[p] = r;
        alive += r.x >= 0;
    }
    count_live(alive, live + 1);
}

__global__ __launch_bounds__(256) void basin_finish_kernel(const int4* __restrict__ rec, int64_t n, double cellsize,
                                                           int32_t* __restrict__ basin, int32_t* __restrict__ nc,
                                                           int32_t* __restrict__ nd, float* __restrict__ length_m,
                                                           ull* __restrict__ counts) {
    int term = 0;
    uint32_t steps = 0, bits = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int4 r = rec[p];
        basin[p] = r.y;
        if (nc) nc[p] = r.z;
        if (nd) nd[p] = r.w;
        const double diag = 1.4142135623730951 * (double)r.w;
        const double sum = (double)r.z + diag;
        const float len = (float)(cellsize * sum);
        if (length_m) length_m[p] = len;
        term += (int64_t)r.y == p;
        const uint32_t s = (uint32_t)r.z + (uint32_t)r.w, b = __float_as_uint(len);
        steps = s > steps ? s : steps;
        bits = b > bits ? b : bits;                                 // len >= 0: its bits order as integers
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        term += __shfl_xor(term, o, 64);
        const uint32_t s2 = __shfl_xor(steps, o, 64), b2 = __shfl_xor(bits, o, 64);
        steps = s2 > steps ? s2 : steps;
        bits = b2 > bits ? b2 : bits;
    }
    if ((threadIdx.x & 63) == 0) {
        if (term) atomicAdd(counts, (ull)term);
        if (steps) atomicMax(counts + 1, (ull)steps);
        if (bits) atomicMax(counts + 2, (ull)bits);
    }
}

// ---- the comparison -----------------------------------------------------------------------------------------------------
// counters 6, 14 and 18 are maxima, the others sums
__host__ __device__ constexpr bool dr_is_max(int i) { return i == 6 || i == 14 || i == 18; }

__global__ __launch_bounds__(256) void flow_compare_kernel(const uint8_t* __restrict__ sel, const uint8_t* __restrict__ dir_t,
                                                           const uint8_t* __restrict__ dir_p, const int32_t* __restrict__ basin_t,
                                                           const int32_t* __restrict__ basin_p, const int32_t* __restrict__ acc_t,
                                                           const int32_t* __restrict__ acc_p, const int32_t* __restrict__ d2_t,
                                                           const int32_t* __restrict__ d2_p, int64_t n, int W, int32_t stream_cells,
                                                           int32_t tol2, ull* __restrict__ counts) {
    ull c[DR_NCMP];
#pragma unroll
    for (int i = 0; i < DR_NCMP; ++i) c[i] = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!sel[p]) continue;
        const int ct = dir_t[p], cp = dir_p[p];
        if (!ct || !cp) continue;
        c[0] += 1;
        c[1] += ct == cp;
        if (ct <= 8 && cp <= 8) {
            c[2] += 1;
            int d = ct - cp;
            d = d < 0 ? -d : d;
            d = d > 4 ? 8 - d : d;
            c[3] += d <= 1;
        }
        const int32_t bt = basin_t[p], bp = basin_p[p];
        c[4] += bt == bp;
        if (bt >= 0 && bp >= 0 && bt != bp) {
            const int64_t yt = bt / W, yp = bp / W;
            const int64_t dy = yt - yp, dx = (bt - yt * W) - (bp - yp * W);
            const ull d2 = (ull)(dy * dy + dx * dx);
            c[5] += d2;
            c[6] = d2 > c[6] ? d2 : c[6];
        }
        const int32_t at = acc_t[p], ap = acc_p[p];
        const int ot = 31 - __clz(at < 1 ? 1 : at), op = 31 - __clz(ap < 1 ? 1 : ap);
        c[7] += (ull)(ot > op ? ot - op : op - ot);
        const bool st = at >= stream_cells, sp = ap >= stream_cells;
        c[8] += st;
        c[9] += sp;
        c[10] += st && sp;
        if (sp) {
            const int32_t d = d2_t[p];
            c[11] += d <= tol2;
            if (d == TG_EDT_FAR) {
                c[12] += 1;
            } else {
                c[13] += (ull)d;
                c[14] = (ull)d > c[14] ? (ull)d : c[14];
            }
        }
        if (st) {
            const int32_t d = d2_p[p];
            c[15] += d <= tol2;
            if (d == TG_EDT_FAR) {
                c[16] += 1;
            } else {
                c[17] += (ull)d;
                c[18] = (ull)d > c[18] ? (ull)d : c[18];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < DR_NCMP; ++i) {
        ull v = c[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const ull v2 = __shfl_xor(v, o, 64);
            v = dr_is_max(i) ? (v2 > v ? v2 : v) : v + v2;
        }
        if ((threadIdx.x & 63) == 0 && v) {
            if (dr_is_max(i)) atomicMax(counts + i, v);
            else atomicAdd(counts + i, v);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" size_t tg_flow_basin_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return dr_layout(H, W).total;
}

extern "C" int tg_flow_basin_init(const uint8_t* dir, const uint8_t* pour, int H, int W, int64_t* counts, void* ws,
                                  size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_basin_init", H, W)) return rc;
    TG_REQUIRE(dir && counts && ws, "tg_flow_basin_init: null pointer");
    const DrLayout L = dr_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_basin_init: workspace %zu bytes < %zu", ws_bytes, L.total);
    TG_REQUIRE(((uintptr_t)ws & 15) == 0, "tg_flow_basin_init: workspace must be aligned to 16 bytes");
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* live = (int32_t*)(base + L.ctl) + DBL_LIVE;
    if (hipMemsetAsync(base + L.ctl, 0, SW_CTL_BYTES, s) != hipSuccess ||
        hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flow_basin_init: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(basin_init_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, dir, pour, H, W,
                       (int4*)(base + L.rec[0]), live, reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("basin_init_kernel");
    return TG_OK;
}

extern "C" int tg_flow_basin(int H, int W, int k0, int n, int32_t* state, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_basin", H, W)) return rc;
    TG_REQUIRE(state && ws, "tg_flow_basin: null pointer");
    if (int rc = doubling_rounds_check("tg_flow_basin", k0, n)) return rc;
    const DrLayout L = dr_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_basin: workspace %zu bytes < %zu", ws_bytes, L.total);
    TG_REQUIRE(((uintptr_t)ws & 15) == 0, "tg_flow_basin: workspace must be aligned to 16 bytes");
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    const int64_t px = (int64_t)H * W;
    const dim3 grid(ew_grid(px, 256));
    return doubling_run(k0, n, (int32_t*)(base + L.ctl) + DBL_LIVE, state, s, "basin_round_kernel", "basin_state_kernel",
                        [&](int k, int32_t* live) {
                            const int a = k & 1, b = a ^ 1;
                            hipLaunchKernelGGL(basin_round_kernel, grid, dim3(256), 0, s, px, (const int4*)(base + L.rec[a]),
                                               (int4*)(base + L.rec[b]), live);
                        });
}

extern "C" int tg_flow_basin_finish(int H, int W, int rounds, double cellsize, int32_t* basin, int32_t* nc, int32_t* nd,
                                    float* length_m, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flow_basin_finish", H, W)) return rc;
    TG_REQUIRE(basin && counts && ws, "tg_flow_basin_finish: null pointer");
    TG_REQUIRE(rounds >= 0 && rounds <= DBL_MAX_ROUNDS, "tg_flow_basin_finish: rounds = %d must lie in [0, %d]", rounds,
               DBL_MAX_ROUNDS);
    TG_REQUIRE(cellsize > 0 && cellsize * 0.0 == 0.0, "tg_flow_basin_finish: cellsize %g must be finite and > 0", cellsize);
    const DrLayout L = dr_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_flow_basin_finish: workspace %zu bytes < %zu", ws_bytes, L.total);
    TG_REQUIRE(((uintptr_t)ws & 15) == 0, "tg_flow_basin_finish: workspace must be aligned to 16 bytes");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_FLOW_BASIN_COUNTS * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flow_basin_finish: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(basin_finish_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s,
                       (const int4*)((char*)ws + L.rec[rounds & 1]), px, cellsize, basin, nc, nd, length_m,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("basin_finish_kernel");
    return TG_OK;
}

extern "C" int tg_flow_compare(const uint8_t* sel, const uint8_t* dir_t, const uint8_t* dir_p, const int32_t* basin_t,
                               const int32_t* basin_p, const int32_t* acc_t, const int32_t* acc_p, const int32_t* d2_t,
                               const int32_t* d2_p, int H, int W, int32_t stream_cells, int32_t tol2, int64_t* counts,
                               tg_stream_t stream) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= TG_EDT_MAX_SIDE && W <= TG_EDT_MAX_SIDE,
               "tg_flow_compare: raster %dx%d: both sides must lie in [1, %d]", H, W, (int)TG_EDT_MAX_SIDE);
    TG_REQUIRE(sel && dir_t && dir_p && basin_t && basin_p && acc_t && acc_p && d2_t && d2_p && counts,
               "tg_flow_compare: null pointer");
    TG_REQUIRE(stream_cells >= 1, "tg_flow_compare: stream_cells = %d must be >= 1", stream_cells);
    TG_REQUIRE(tol2 >= 0 && tol2 < TG_EDT_FAR, "tg_flow_compare: tol2 = %d must lie in [0, TG_EDT_FAR)", tol2);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, DR_NCMP * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flow_compare: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(flow_compare_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s, sel, dir_t, dir_p, basin_t, basin_p, acc_t,
                       acc_p, d2_t, d2_p, px, W, stream_cells, tol2, reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("flow_compare_kernel");
    return TG_OK;
}

// ---- stream classes, links, Strahler order, HAND, flood comparison ---------------------------------------
//   stream_class_kernel         class, the node-order plane and the start records (up, p, c, d) of the upstream doubling, which
//                               basin_round_kernel and basin_finish_kernel then run unchanged: last = top, nc / nd from top to p
//   stream_order_kernel         one round over the junction list: order[j] <- max(order[j], max(m1, m2 + 1)) over the donors' links
//   stream_order_finish_kernel  out = order[top] on the streams; the histograms by wave ballots
//   hand_kernel                 the gather w(T) and one fp32 subtract
//   flood_compare_kernel        the 6 + 3 k integer counters of two HAND planes
constexpr int DR_NORD = TG_STREAM_ORDER_BINS;
constexpr int DR_NFLOOD = TG_FLOOD_COUNTS;
constexpr uint32_t DR_NAN = 0x7fc00000u;

__device__ __forceinline__ bool dr_is_stream(const uint8_t* __restrict__ dir, const int32_t* __restrict__ acc, int64_t p,
                                             int32_t min_cells) {
    return dir[p] != 0 && acc[p] >= min_cells;
}

__global__ __launch_bounds__(256) void stream_class_kernel(const uint8_t* __restrict__ dir, const int32_t* __restrict__ acc, int H,
                                                           int W, int32_t min_cells, uint8_t* __restrict__ cls,
                                                           int32_t* __restrict__ order, int4* __restrict__ rec,
                                                           int32_t* __restrict__ live, ull* __restrict__ counts) {
    const int64_t n = (int64_t)H * W;
    int alive = 0, ns = 0, nh = 0, nj = 0, nt = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int code = dir[p];
        int4 r = make_int4(-1, -1, 0, 0);
        int c = 0;
        if (code != 0 && acc[p] >= min_cells) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            int sd = 0, up = -1, upcode = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {                           // the neighbour at offset k flows here with the opposite code
                const int yy = y + d8_dy(k), xx = x + d8_dx(k);
                if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                    const int64_t q = (int64_t)yy * W + xx;
                    const int back = ((k + 4) & 7) + 1;
                    if (dir[q] == back && acc[q] >= min_cells) {
                        ++sd;
                        up = (int)q;
                        upcode = back;
                    }
                }
            }
            c = sd == 0 ? TG_STREAM_HEAD : sd == 1 ? TG_STREAM_INTERIOR : TG_STREAM_JUNCTION;
            r.y = (int32_t)p;
            if (sd == 1) {
                r.x = up;
                r.z = (upcode & 1) ? 1 : 0;
                r.w = (upcode & 1) ? 0 : 1;
            }
            bool terminal = true;                                   // the receiver is no stream pixel
            if (code >= 1 && code <= 8) {
                const int yy = y + d8_dy(code - 1), xx = x + d8_dx(code - 1);
                if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                    terminal = !dr_is_stream(dir, acc, (int64_t)yy * W + xx, min_cells);
            }
            ++ns;
            nh += sd == 0;
            nj += sd >= 2;
            nt += terminal;
        }
        cls[p] = (uint8_t)c;
        order[p] = c ? 1 : 0;
        rec[p] = r;
        alive += r.x >= 0;
    }
    count_live(alive, live);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ns += __shfl_xor(ns, o, 64);
        nh += __shfl_xor(nh, o, 64);
        nj += __shfl_xor(nj, o, 64);
        nt += __shfl_xor(nt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ns) atomicAdd(counts, (ull)ns);
        if (nh) atomicAdd(counts + 1, (ull)nh);
        if (nj) atomicAdd(counts + 2, (ull)nj);
        if (nt) atomicAdd(counts + 3, (ull)nt);
    }
}

// order is read and written by other workgroups during the pass: relaxed atomic loads at agent scope, atomicMax to write
__global__ __launch_bounds__(256) void stream_order_kernel(const uint8_t* __restrict__ dir, const uint8_t* __restrict__ cls,
                                                           const int32_t* __restrict__ top, const int32_t* __restrict__ junctions,
                                                           int nj, int H, int W, int32_t* order, int last,
                                                           int32_t* __restrict__ changed) {
    const uint32_t n = (uint32_t)((int64_t)H * W);
    int raised = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nj; i += (int64_t)gridDim.x * 256) {
        const uint32_t j = (uint32_t)junctions[i];
        if (j >= n) continue;
        const int y = (int)(j / (uint32_t)W), x = (int)(j - (uint32_t)y * (uint32_t)W);
        int m1 = 0, m2 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int yy = y + d8_dy(k), xx = x + d8_dx(k);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const int64_t q = (int64_t)yy * W + xx;
                if (cls[q] != 0 && dir[q] == ((k + 4) & 7) + 1) {
                    const uint32_t t = (uint32_t)top[q];
                    if (t < n) {
                        const int o = __hip_atomic_load(order + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (o > m1) {
                            m2 = m1;
                            m1 = o;
                        } else if (o > m2) {
                            m2 = o;
                        }
                    }
                }
            }
        }
        int v = m2 + 1 > m1 ? m2 + 1 : m1;
        v = v > 255 ? 255 : v;
        const int cur = __hip_atomic_load(order + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v > cur) {
            atomicMax(order + j, v);
            ++raised;
        }
    }
    if (last) count_live(raised, changed);
}

__global__ __launch_bounds__(256) void stream_order_finish_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ top,
                                                                  const int32_t* __restrict__ order, int64_t n,
                                                                  uint8_t* __restrict__ out, ull* __restrict__ counts) {
    uint32_t cells[DR_NORD], links[DR_NORD];                       // wave-uniform: sums of ballots, static indices only
#pragma unroll
    for (int i = 0; i < DR_NORD; ++i) cells[i] = links[i] = 0;
    int omax = 0;
    const int64_t start = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t base = start - (threadIdx.x & 63); base < n; base += step) {          // a wave stays together for the ballots
        const int64_t p = base + (threadIdx.x & 63);
        int o = 0, c = 0;
        if (p < n) {
            c = cls[p];
            if (c != 0) {
                const uint32_t t = (uint32_t)top[p];
                if (t < (uint32_t)n) o = order[t];
                o = o > 255 ? 255 : o;
            }
            out[p] = (uint8_t)(o < 0 ? 0 : o);
        }
        if (__ballot(o > 0) == 0) continue;                          // wave-uniform
        omax = o > omax ? o : omax;
        const int b = o > DR_NORD ? DR_NORD : o;
        const bool lk = c == TG_STREAM_HEAD || c == TG_STREAM_JUNCTION;
#pragma unroll
        for (int i = 0; i < DR_NORD; ++i) {
            cells[i] += (uint32_t)__popcll(__ballot(b == i + 1));
            links[i] += (uint32_t)__popcll(__ballot(lk && b == i + 1));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int m = __shfl_xor(omax, o, 64);
        omax = m > omax ? m : omax;
    }
    if ((threadIdx.x & 63) == 0) {
        if (omax) atomicMax(counts, (ull)omax);
#pragma unroll
        for (int i = 0; i < DR_NORD; ++i) {
            if (cells[i]) atomicAdd(counts + 1 + i, (ull)cells[i]);
            if (links[i]) atomicAdd(counts + 1 + DR_NORD + i, (ull)links[i]);
        }
    }
}

__global__ __launch_bounds__(256) void hand_kernel(const float* __restrict__ w, const int32_t* __restrict__ basin,
                                                   const uint8_t* __restrict__ smask, const float* __restrict__ length_m, int64_t n,
                                                   float* __restrict__ hand, float* __restrict__ distance_m,
                                                   ull* __restrict__ counts) {
    int drained = 0, undrained = 0, ns = 0;
    uint32_t bits = 0;
    const float nan = __uint_as_float(DR_NAN);
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int32_t t = basin[p];
        float h = nan, d = nan;
        if ((uint32_t)t < (uint32_t)n) {
            ns += smask[p] != 0;
            if (smask[t] != 0) {
                h = w[p] - w[t];
                if (h != h) h = nan;
                if (length_m) d = length_m[p];
                ++drained;
                if (h > 0.f) {
                    const uint32_t b = __float_as_uint(h);
                    bits = b > bits ? b : bits;
                }
            } else {
                ++undrained;
            }
        }
        hand[p] = h;
        if (distance_m) distance_m[p] = d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        drained += __shfl_xor(drained, o, 64);
        undrained += __shfl_xor(undrained, o, 64);
        ns += __shfl_xor(ns, o, 64);
        const uint32_t b2 = __shfl_xor(bits, o, 64);
        bits = b2 > bits ? b2 : bits;
    }
    if ((threadIdx.x & 63) == 0) {
        if (drained) atomicAdd(counts, (ull)drained);
        if (undrained) atomicAdd(counts + 1, (ull)undrained);
        if (ns) atomicAdd(counts + 2, (ull)ns);
        if (bits) atomicMax(counts + 3, (ull)bits);
    }
}

__global__ __launch_bounds__(256) void flood_compare_kernel(const uint8_t* __restrict__ sel, const float* __restrict__ hand_t,
                                                            const float* __restrict__ hand_p, int64_t n, tg_flood_stages st, int k,
                                                            ull* __restrict__ counts) {
    ull c[DR_NFLOOD];                                              // c[4] is a signed sum in two's complement
#pragma unroll
    for (int i = 0; i < DR_NFLOOD; ++i) c[i] = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!sel[p]) continue;
        const float ht = hand_t[p], hp = hand_p[p];
        const bool nt = ht != ht, np_ = hp != hp;
        c[1] += nt;
        c[2] += np_;
        if (nt || np_) continue;
        c[0] += 1;
        const float d = hp - ht, a = fabsf(d);
        c[3] += (ull)__double2ll_rn((double)a * 1024.0);            // exact product, half-to-even
        c[4] += (ull)__double2ll_rn((double)d * 1024.0);
        const ull b = __float_as_uint(a);
        c[5] = b > c[5] ? b : c[5];
#pragma unroll
        for (int i = 0; i < TG_FLOOD_MAX_STAGES; ++i) {
            if (i < k) {
                const bool wt = ht <= st.s[i], wp = hp <= st.s[i];
                c[6 + 3 * i] += wt;
                c[7 + 3 * i] += wp;
                c[8 + 3 * i] += wt && wp;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < DR_NFLOOD; ++i) {
        ull v = c[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const ull v2 = __shfl_xor(v, o, 64);
            v = i == 5 ? (v2 > v ? v2 : v) : v + v2;
        }
        if ((threadIdx.x & 63) == 0 && v) {
            if (i == 5) atomicMax(counts + i, v);
            else atomicAdd(counts + i, v);
        }
    }
}

extern "C" int tg_stream_class(const uint8_t* dir, const int32_t* acc, int H, int W, int32_t min_cells, uint8_t* cls,
                               int32_t* order, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_stream_class", H, W)) return rc;
    TG_REQUIRE(dir && acc && cls && order && counts && ws, "tg_stream_class: null pointer");
    TG_REQUIRE(min_cells >= 1, "tg_stream_class: min_cells = %d must be >= 1", min_cells);
    const DrLayout L = dr_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_stream_class: workspace %zu bytes < %zu", ws_bytes, L.total);
    TG_REQUIRE(((uintptr_t)ws & 15) == 0, "tg_stream_class: workspace must be aligned to 16 bytes");
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    int32_t* live = (int32_t*)(base + L.ctl) + DBL_LIVE;
    if (hipMemsetAsync(base + L.ctl, 0, SW_CTL_BYTES, s) != hipSuccess ||
        hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_stream_class: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(stream_class_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, s, dir, acc, H, W, min_cells, cls,
                       order, (int4*)(base + L.rec[0]), live, reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("stream_class_kernel");
    return TG_OK;
}

extern "C" int tg_stream_order(const uint8_t* dir, const uint8_t* cls, const int32_t* top, const int32_t* junctions, int nj, int H,
                               int W, int n, int32_t* order, int32_t* changed, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_stream_order", H, W)) return rc;
    TG_REQUIRE(dir && cls && top && order && changed, "tg_stream_order: null pointer");
    TG_REQUIRE(nj >= 0 && (int64_t)nj <= (int64_t)H * W, "tg_stream_order: nj = %d must lie in [0, H * W]", nj);
    TG_REQUIRE(junctions || nj == 0, "tg_stream_order: null junction list with nj = %d", nj);
    TG_REQUIRE(n >= 1 && n <= (1 << 20), "tg_stream_order: n = %d must lie in [1, 2^20]", n);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(changed, 0, sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("tg_stream_order: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    if (nj == 0) return TG_OK;
    const dim3 grid(ew_grid(nj, 256));
    for (int r = 0; r < n; ++r) {
        hipLaunchKernelGGL(stream_order_kernel, grid, dim3(256), 0, s, dir, cls, top, junctions, nj, H, W, order, (int)(r == n - 1),
                           changed);
        TG_CHECK_LAUNCH("stream_order_kernel");
    }
    return TG_OK;
}

extern "C" int tg_stream_order_finish(const uint8_t* cls, const int32_t* top, const int32_t* order, int H, int W, uint8_t* out,
                                      int64_t* counts, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_stream_order_finish", H, W)) return rc;
    TG_REQUIRE(cls && top && order && out && counts, "tg_stream_order_finish: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_STREAM_ORDER_COUNTS * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_stream_order_finish: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(stream_order_finish_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s, cls, top, order, px, out,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("stream_order_finish_kernel");
    return TG_OK;
}

extern "C" int tg_hand(const float* w, const int32_t* basin, const uint8_t* smask, const float* length_m, int H, int W, float* hand,
                       float* distance_m, int64_t* counts, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_hand", H, W)) return rc;
    TG_REQUIRE(w && basin && smask && hand && counts, "tg_hand: null pointer");
    TG_REQUIRE((length_m == nullptr) == (distance_m == nullptr), "tg_hand: length_m and distance_m go together");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_hand: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(hand_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s, w, basin, smask, length_m, px, hand, distance_m,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("hand_kernel");
    return TG_OK;
}

extern "C" int tg_flood_compare(const uint8_t* sel, const float* hand_t, const float* hand_p, int H, int W, tg_flood_stages stages,
                                int k, int64_t* counts, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_flood_compare", H, W)) return rc;
    TG_REQUIRE(sel && hand_t && hand_p && counts, "tg_flood_compare: null pointer");
    TG_REQUIRE(k >= 1 && k <= TG_FLOOD_MAX_STAGES, "tg_flood_compare: k = %d stages must lie in [1, %d]", k, TG_FLOOD_MAX_STAGES);
    for (int i = 0; i < k; ++i) {
        const float v = stages.s[i];
        TG_REQUIRE(v > 0.f && v * 0.f == 0.f, "tg_flood_compare: stage %d = %g must be finite and > 0", i, (double)v);
        TG_REQUIRE(i == 0 || v > stages.s[i - 1], "tg_flood_compare: stages must be strictly increasing (stage %d = %g)", i,
                   (double)v);
    }
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, DR_NFLOOD * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_flood_compare: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(flood_compare_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, s, sel, hand_t, hand_p, px, stages, k,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("flood_compare_kernel");
    return TG_OK;
}
