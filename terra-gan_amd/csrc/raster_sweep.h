// What the hydrology kernels share (depfill.hip, flow.hip, drainage.hip, mfd.hip): host-side basics, the
// D8 neighbour tables, the tile-sweep protocol and the pointer-doubling protocol.  Only what is identical between the callers is
// here; what a visit or a round computes stays in its own file.  No floating-point arithmetic in this header, so each file's
// `#pragma clang fp contract(off)` covers all of its own.
//
// The tile sweep.  One workgroup per 64x64 tile relaxes the tile with a one-pixel halo in LDS to a local fixed point and writes it
// back to the one plane that all tiles share, in place.
//   * A tile's halo belongs to neighbour tiles that may be writing it in the same launch.  Halo loads and the write-back are
//     relaxed atomic accesses at agent scope, so a halo value is an old or a new value of that pixel, never a torn one.  Every
//     caller's values move one way only (depfill: W falls towards the answer; flow: D falls towards the distance; mfd: not final
//     -> final, once), and an old value is always one the iteration may legally hold, so a stale halo delays the fixed point and
//     never moves it.
//   * Marks.  Two byte planes; plane (s & 1) is read in sweep s ("visit me"), the other one is written ("visit next").  A visit
//     clears its own byte of the plane it read.  A visit that changed a pixel on its rim marks its eight neighbour tiles, whose
//     halo has changed, so no changed value is ever missed; a visit that may have work left marks itself.  Every writer stores
//     the same byte value 1, so concurrent marks need no ordering.  The marks change which visits happen and never what a visit
//     computes: the result is the fixed point whatever the order, while the number of sweeps and visits may differ between runs.
//   * The sweep counter is ctl[0]; the one-thread begin kernel adds the n sweeps of a call before they run, and sweep j of the
//     call reads ctl[0] - n + j.  Only its parity is used.
//   * Inside a visit a thread owns one line (a column in rounds 0 and 1, a row in rounds 2 and 3) and one band of 16 pixels along
//     it, scanned forwards (even rounds) or backwards (odd rounds), so a value travels a whole band within a round.  The rounds
//     repeat until one changes nothing (__syncthreads_or) or the caller's cap.
//   * LDS rows of the 66x66 image are 67 words apart: odd, so a wave is conflict-free along rows and along columns.
//
// The pointer doubling.  live[k] (int32, word 8 + k of the control block) counts the pointers left before round k.  Round k runs
// only while live[k] != 0 and counts those left after it into live[k + 1]; the one-thread state kernel then reports the count
// after the rounds enqueued and the number of rounds that ran, so the host reads one pair per batch of rounds.
#pragma once

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

static inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

static inline bool raster_size_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }

static inline int raster_size_check(const char* who, int H, int W) {
    TG_REQUIRE(raster_size_ok(H, W), "%s: raster %dx%d must be non-empty with H*W < 2^31", who, H, W);
    return TG_OK;
}

// ---- D8 neighbours ------------------------------------------------------------------------------------------------------
// code - 1 -> (dy, dx): E, SE, S, SW, W, NW, N, NE; the order of preference as codes - 1
__host__ __device__ constexpr int d8_dy(int k) { return ((0x01a9 >> (2 * k)) & 3) - 1; }     // 0, 1, 1, 1, 0, -1, -1, -1
__host__ __device__ constexpr int d8_dx(int k) { return ((0x901a >> (2 * k)) & 3) - 1; }     // 1, 1, 0, -1, -1, -1, 0, 1
static_assert(d8_dy(0) == 0 && d8_dy(1) == 1 && d8_dy(2) == 1 && d8_dy(3) == 1 && d8_dy(4) == 0 && d8_dy(5) == -1 &&
              d8_dy(6) == -1 && d8_dy(7) == -1, "dy");
static_assert(d8_dx(0) == 1 && d8_dx(1) == 1 && d8_dx(2) == 0 && d8_dx(3) == -1 && d8_dx(4) == -1 && d8_dx(5) == -1 &&
              d8_dx(6) == 0 && d8_dx(7) == 1, "dx");
#define FL_PREF(i) ((((i) & 3) << 1) | ((i) >> 2))          // 0, 2, 4, 6, 1, 3, 5, 7

// ---- the tile sweep: workspace and host side ----------------------------------------------------------------------------
constexpr int SW_T = 64;                 // tile side
constexpr int SW_R = SW_T + 2;           // rows and columns with the halo
constexpr int SW_S = SW_T + 3;           // LDS row stride in elements: odd
constexpr int SW_CTL_BYTES = 256;        // int32 [0]: sweeps enqueued since the reset; [8 .. 40]: live[k] of a doubling

// the head of a sweeping workspace: the control block, then two mark planes of al256(tiles) bytes
struct SweepLayout {
    size_t ctl, plane[2];
    int ty, tx;
    size_t tiles() const { return (size_t)ty * tx; }
};

// `own` tile planes of the caller's lie between the control block and the marks; o: the first byte after the marks
static inline SweepLayout sweep_layout(int H, int W, size_t& o, int own = 0) {
    SweepLayout L;
    L.ty = cdiv(H, SW_T);
    L.tx = cdiv(W, SW_T);
    L.ctl = 0;
    L.plane[0] = SW_CTL_BYTES + own * al256(L.tiles());
    L.plane[1] = L.plane[0] + al256(L.tiles());
    o = L.plane[1] + al256(L.tiles());
    return L;
}

// the sweep counter to 0, every tile marked for sweep 0, none for sweep 1
static inline bool sweep_reset(const SweepLayout& L, void* ws, hipStream_t s) {
    char* base = (char*)ws;
    return hipMemsetAsync(base + L.ctl, 0, SW_CTL_BYTES, s) == hipSuccess &&
           hipMemsetAsync(base + L.plane[0], 1, L.tiles(), s) == hipSuccess &&
           hipMemsetAsync(base + L.plane[1], 0, L.tiles(), s) == hipSuccess;
}

// internal linkage: every file that includes this header has its own copy in the one library; drainage.hip has no use for it
[[maybe_unused]] static __global__ void sweep_begin_kernel(int32_t* __restrict__ ctl, int n, int32_t* __restrict__ changed) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ctl[0] = (ctl[0] + n) & 0x3fffffff;                         // only its parity is used
        if (changed) changed[0] = 0;
    }
}

// the begin kernel, then n sweeps: launch(grid, ctl, j, plane0, plane1) enqueues the caller's kernel for sweep j of the call
template <typename Launch>
static int sweep_run(const SweepLayout& L, void* ws, int n, int32_t* changed, hipStream_t s, const char* begin_name,
                     const char* sweep_name, Launch launch) {
    char* base = (char*)ws;
    int32_t* ctl = (int32_t*)(base + L.ctl);
    uint8_t* p0 = (uint8_t*)(base + L.plane[0]);
    uint8_t* p1 = (uint8_t*)(base + L.plane[1]);
    hipLaunchKernelGGL(sweep_begin_kernel, dim3(1), dim3(64), 0, s, ctl, n, changed);
    TG_CHECK_LAUNCH(begin_name);
    const dim3 grid(L.ty * L.tx);                                   // < 2^31 / 4096
    for (int j = 0; j < n; ++j) {
        launch(grid, (const int32_t*)ctl, j, p0, p1);
        TG_CHECK_LAUNCH(sweep_name);
    }
    return TG_OK;
}

// ---- the tile sweep: device side ----------------------------------------------------------------------------------------
struct SweepVisit {
    uint8_t *cur, *nxt;                  // the mark plane this sweep reads, the one it writes
    int tile, ty, tx, y0, x0;
    bool marked;                         // uniform over the workgroup
};

// Two steps, because most workgroups of a launch find their tile unmarked and leave: the first costs them one word and one byte,
// and the division by tiles_x comes after the caller's `if (!v.marked) return;`.
__device__ __forceinline__ SweepVisit sweep_visit_begin(const int32_t* __restrict__ ctl, int n, int j, uint8_t* plane0,
                                                        uint8_t* plane1) {
    SweepVisit v;
    v.tile = blockIdx.x;
    const int sweep = ctl[0] - n + j;                               // the begin kernel has added n already
    v.cur = (sweep & 1) ? plane1 : plane0;
    v.nxt = (sweep & 1) ? plane0 : plane1;
    v.marked = v.cur[v.tile] != 0;
    return v;
}

__device__ __forceinline__ void sweep_visit_place(SweepVisit& v, int tiles_x) {
    v.ty = v.tile / tiles_x;
    v.tx = v.tile - v.ty * tiles_x;
    v.y0 = v.ty * SW_T;
    v.x0 = v.tx * SW_T;
}

// position i of the 66x66 staged image
struct SweepStage {
    int ly, lx, gy, gx;
    bool in_raster, on_tile;             // a pixel of the raster; not on the halo, computed here
    // not on the halo, computed where the caller asks, inside its `if (g.in_raster)`.  The same test twice because where its
    // compares stand against the bounds test, which the staging loads wait on, was measured both ways on the 8192x8192 scenes
    // (DESIGN.md section 8u.1): depfill's sweeps are 0.6 to 1.4 % slower with the field, mfd's 1.0 to 1.5 % slower with the
    // method.  depfill and flow call interior(), mfd reads on_tile.
    __device__ __forceinline__ bool interior() const { return ly >= 1 && ly <= SW_T && lx >= 1 && lx <= SW_T; }
};

__device__ __forceinline__ SweepStage sweep_stage(int i, int y0, int x0, int H, int W) {
    SweepStage g;
    g.ly = i / SW_R;
    g.lx = i - g.ly * SW_R;
    g.gy = y0 - 1 + g.ly;
    g.gx = x0 - 1 + g.lx;
    g.in_raster = (unsigned)g.gy < (unsigned)H && (unsigned)g.gx < (unsigned)W;
    g.on_tile = g.ly >= 1 && g.ly <= SW_T && g.lx >= 1 && g.lx <= SW_T;
    return g;
}

// The start of a thread's scan (line, band, c, sgn, the LDS index and its steps) is written out at the head of each caller's
// rounds, nine lines, and not a helper here: through one, the compiler scheduled the LDS reads of the unrolled scans later and
// kept more address registers (profiles/hydrology_line_scan_helper_depfill_isa_diff.txt), and on the 8192x8192 scenes the sweeps of
// depfill took 0.35 to 0.50 ms of 21 more than the parent's, a flow_routing call 0.37 to 0.75 ms of 58 more
// (profiles/hydrology_line_scan_helper_parent_vs_variant_8192.jsonl).

// the visit's own mark cleared and the visit counted by thread 0; the marks for the next sweep by threads 0..8
__device__ __forceinline__ void sweep_visit_end(const SweepVisit& v, int tiles_y, int tiles_x, ull* visits, bool mark_self,
                                                bool mark_neighbours) {
    const int t = threadIdx.x;
    if (t == 0) {
        v.cur[v.tile] = 0;
        atomicAdd(visits, 1ull);
    }
    if (t < 9) {
        const int ny = v.ty + t / 3 - 1, nx = v.tx + t % 3 - 1;
        if ((t == 4 ? mark_self : mark_neighbours) && ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x)
            __hip_atomic_store(v.nxt + (int64_t)ny * tiles_x + nx, (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the pointer doubling -----------------------------------------------------------------------------------------------
constexpr int DBL_LIVE = 8;              // first word of live[0 .. 32] in the control block
constexpr int DBL_MAX_ROUNDS = TG_FLOW_MAX_ROUNDS;
static_assert((DBL_LIVE + DBL_MAX_ROUNDS + 1) * 4 <= SW_CTL_BYTES, "live[] fits the control block");

__device__ __forceinline__ void count_live(int alive, int32_t* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o, 64);
    if ((threadIdx.x & 63) == 0 && alive) atomicAdd(dst, alive);
}

[[maybe_unused]] static __global__ void doubling_state_kernel(const int32_t* __restrict__ live, int k_end,
                                                              int32_t* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int k = 0;
    while (k < k_end && live[k] != 0) ++k;                          // round k ran iff live[k] != 0
    state[0] = live[k];
    state[1] = k;
}

// the caller's k0 and n, checked where its own argument checks stand (before those of the workspace)
static inline int doubling_rounds_check(const char* who, int k0, int n) {
    TG_REQUIRE(k0 >= 0 && n >= 1 && k0 <= DBL_MAX_ROUNDS && n <= DBL_MAX_ROUNDS - k0,
               "%s: rounds k0 = %d, n = %d must satisfy k0 >= 0, n >= 1, k0 + n <= %d", who, k0, n, DBL_MAX_ROUNDS);
    return TG_OK;
}

// rounds k0 .. k0 + n - 1, then the state: launch(k, live + k) enqueues the caller's kernel for round k
template <typename Launch>
static int doubling_run(int k0, int n, int32_t* live, int32_t* state, hipStream_t s, const char* round_name,
                        const char* state_name, Launch launch) {
    for (int k = k0; k < k0 + n; ++k) {
        launch(k, live + k);
        TG_CHECK_LAUNCH(round_name);
    }
    hipLaunchKernelGGL(doubling_state_kernel, dim3(1), dim3(64), 0, s, (const int32_t*)live, k0 + n, state);
    TG_CHECK_LAUNCH(state_name);
    return TG_OK;
}
