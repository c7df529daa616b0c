// Winograd F(2x2,3x3) on the fp32 MFMA -- included by igemm.hip (uses its helpers: xcd_remap, tile_rows4, epilogue4,
// igemm_splitk_epilogue, choose_splits, ProfScope).
//
// Every stride-1 3x3 convolution of the step (decoder PConvs, the VGG trunk, and their dgrads = 85 % of the conv FLOPs)
// is   Y = At [ (G g Gt) (.) (Bt d B) ] A   per 2x2 output tile: 16 independent [tiles x Cin] x [Cin x Cout] products
// instead of 9 taps over 4 pixels -- 2.25x fewer multiplies, the only lever left once the direct kernel sits at
// ~75 % of the fp32-MFMA peak.  The arithmetic stays fp32 (fp32 transforms, fp32 MFMA, fp32 accumulate).
//
// One 512-thread workgroup (8 waves, two per SIMD) owns a 16x16 block of output pixels (8x8 Winograd tiles) of one
// image x 64 output channels.  Wave (mw, nw, xh) holds transform points xi = 8*xh .. 8*xh+7 for tiles 32*mw .. +31 and
// channels 32*nw .. +31: 8 accumulator tiles = 128 registers.  K (= Cin) is walked in 8-channel steps through
// double-buffered LDS images: the 18x18x8 input patch is staged into LDS (mask multiply + zero padding there) and
// transformed by all 512 threads into V [xi][tile][8]; the pre-transformed weights U arrive from global memory already
// in their LDS image ([k/8][n/64][xi][64][8], written that way by wino_weights_kernel).
// A step is 32 MFMAs per wave; the staging work for the NEXT step (patch store, transform, U store, global loads two
// steps ahead, fragment fetches) is cut into pieces of one or two instructions and placed between the MFMAs by hand
// (sched_barrier pins the order): LDS traffic (~250 KB per step and workgroup) and the MFMA pipe (4096 cycles per step
// and SIMD) then run concurrently instead of in phases.
// Rows are 8 floats (32 B); the two 16-byte halves of a row are swapped when bit 4 of the row is set, which makes the
// ds_read_b128 lane groups ({0-3,12-15,20-27},{4-11,16-19,28-31},...) hit 64 distinct banks.  The output transform
// needs all 16 points of an element: the two xi-halves exchange half of their row sums through LDS and each stores two
// of the four output positions.
#pragma once
#include <utility>

struct WinoGeom {
    int tiles_x, tiles_y, total_work, chunks_per_split, nt;
    int sy_min, sx_min;
    int interleave;     // work distribution, see wino_distribute
    int* qctr;          // work-stealing counter block of this launch (nullptr: static distribution), see WinoWork
    // tile map (wino_pipe_kernel<.., SPARSE>, TgSparseMap): sp_tiles = nb x tiles.  SPARSE = 1: the prediction half of a
    // [pred; target] batch; SPARSE = 2: a batch of nb images of which only the listed tiles are computed
    const uint32_t* sp_bits;
    const int* sp_list;
    const int* sp_count;
    int sp_tiles, sp_nb;
};
struct WinoWeights {
    long sn, sk, stap;      // element strides of the raw weights: output row n, contraction index k, tap (ky*3+kx)
    int kyu[3], kxv[3];     // source offset u (0..2 from the patch origin) -> ky ; v -> kx
    int k_fast;             // thread order: consecutive threads walk k (1) or n (0), whichever is contiguous in memory
};
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int WINO_BN = 64;
constexpr int WINO_V = 16 * 64 * 8;           // floats of one V image (one 8-channel step)
constexpr int WINO_U = 16 * WINO_BN * 8;      // floats of one U slice
constexpr int WINO_PPIX = 18 * 18;
constexpr int WINO_P = WINO_PPIX * 8;
constexpr int WINO_LDS_FLOATS = 2 * WINO_V + 2 * WINO_U + WINO_P;
constexpr int WINO_THREADS = 512;

// Workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait for the global
// loads of the next steps' operands that are deliberately left in flight across it.
__device__ __forceinline__ void wino_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class F, int... T>
__device__ __forceinline__ void wino_static_for(std::integer_sequence<int, T...>, F&& f) {
    (f(std::integral_constant<int, T>{}), ...);
}

// Work distribution of the persistent Winograd kernels.  Hardware deals workgroup ids round-robin over the 8 XCDs (ids b and
// b+8 share an L2) and every XCD owns a CONTIGUOUS chunk of the items (patch-major, N tile fastest).
//   interleave = 1: the XCD's workgroups walk the chunk interleaved (workgroup `slot` of `nslots` takes items slot,
//     slot + nslots, ...): at any moment the XCD is busy with ~32 consecutive items, so the N tiles of a patch and the
//     neighbouring patches run at the same time on the same L2 and the patch (and the halo it shares) leaves memory once
//     instead of once per N tile.  Measured (FETCH_SIZE per dispatch): 256->256 at 64x64: 655 -> 407 MB, 128->128 at
//     128x128: 663 -> 412 MB.  The price is that the whole U is in use at any time: right while it fits the 4 MB L2.
//   interleave = 0: every workgroup takes a contiguous range (its few N tiles of one patch in turn; workgroups in step share
//     the U slices) -- better when U is several L2s large (768->256: 151 MB against 324 MB interleaved).
__device__ __forceinline__ void wino_distribute(int total, int interleave, int& item, int& item_end, int& step) {
    const int G = gridDim.x;
    if (interleave) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = (G - xcd + 7) >> 3;
        const int ch_q = total >> 3, ch_r = total & 7;
        const int chunk0 = xcd < ch_r ? xcd * (ch_q + 1) : ch_r * (ch_q + 1) + (xcd - ch_r) * ch_q;
        item = chunk0 + slot;
        item_end = chunk0 + ch_q + (xcd < ch_r ? 1 : 0);
        step = nslots;
    } else {
        const int rblk = xcd_remap(blockIdx.x, G);
        const int per = total / G, rem = total % G;
        item = rblk * per + min(rblk, rem);
        item_end = item + per + (rblk < rem ? 1 : 0);
        step = 1;
    }
}

// ---- work queue of the persistent Winograd workgroups ------------------------------------------------------------------------
// Static mode (default, single GPU): wino_distribute above -- no memory traffic, the item list of a workgroup is fixed.
// Work-stealing mode (tg_set_work_stealing, switched on by data-parallel runs): a launch of 256 one-per-CU workgroups shares
// the chip with RCCL's long-running reduction kernels.  A workgroup that cannot become resident (its CU is held by RCCL) starts
// only when another one exits -- with a static item list its items wait for a whole round and the launch takes twice as long.
// Here the items behind the first round sit in per-XCD queues (one atomic counter per XCD chunk and grid slice, the same
// contiguous chunks as the interleaved static walk, so the L2 locality is the static walk's): a workgroup owns ONE item (its
// rank in its chunk) and pulls every further one from its XCD's queue -- resident workgroups drain the queues, a late one
// computes its own item and finds the queue empty.  WHICH workgroup computes an item never changes a result (every item
// writes its own tile / slab), so both modes are bitwise equal.  The kernels need the NEXT item one item ahead (they request
// its first operands ahead of the current stores / stage it in the current item's last K steps): a workgroup always holds
// `item` and `next`; the one after is fetched by ONE lane during the epilogue (the atomic's round trip hides under the
// stores), published through an LDS word and picked up behind the barrier that ends the item.  The last workgroup to finish
// zeroes the counters.
constexpr int WQ_Z = 16;                       // grid slices (split-K) a counter block serves (= WQ_HOST_Z in igemm.hip)
constexpr int WQ_INTS = 8 * WQ_Z + 8;          // 8 chunk counters per slice, then the done counter
__device__ __forceinline__ int wq_chunk0(int total, int c) { const int q = total >> 3, r = total & 7; return c < r ? c * (q + 1) : r * (q + 1) + (c - r) * q; }
__device__ __forceinline__ int wq_len(int total, int c) { return (total >> 3) + (c < (total & 7) ? 1 : 0); }
// No stealing ACROSS chunks: the hardware deals workgroups -- RCCL's as well as these -- round-robin over the XCDs, so every chunk
// keeps about the same number of resident pullers.  One atomic and one compare per pull.
// STEAL = false is the static walk with exactly the state the kernels carried before (item, item_end, step).  STEAL = true is a
// second instantiation of the same kernel, chosen per launch: the current item and a parity bit in registers, the home chunk's
// counter address / first item / length in scalars, and the following items in two LDS words -- slot[par] = the item after the
// current one, slot[par ^ 1] = where the one after that is published during the current item.
// Everything wave-uniform that a one-lane block needs (block indices, kernel arguments, the chunk bounds) is computed AHEAD of
// the branch in init(): an expression that first appears inside `if (threadIdx.x == 0)` and again behind it is made "partially
// redundant" by GVN -- it becomes a phi at the join of a divergent branch, i.e. a divergent value, and everything derived from it
// (blockIdx.z -> the K range -> the scalar offsets of the K loop's buffer loads) moves into vector registers and waterfall
// loops (measured: +40 % on the launch).
template <bool STEAL>
struct WinoWork {
    int item;                                  // current item (-1: none); wave-uniform
    int item_end, step;                        // static: the walk; work-stealing: step = parity, item_end unused
    int* home_ctr;                             // work-stealing: the home chunk's counter of this grid slice,
    int home_c0, home_len;                     //                its first item and its length

    // `slot`: two ints of LDS outside the kernel's staging areas.  Contains workgroup barriers in work-stealing mode.
    __device__ __forceinline__ void init(int total, int interleave, int* ctr, int* slot) {
        if constexpr (!STEAL) {
            wino_distribute(total, interleave, item, item_end, step);
            if (item >= item_end) item = -1;
        } else {
            // the FIRST item of a workgroup is static (its rank in the home chunk), the queue hands out the items behind the
            // first round: with every item in the queue a launch of about one item per workgroup came out unbalanced (whoever
            // arrives first pulls its current AND its next item; late arrivals found the queue empty: +80 % on such layers)
            const int home = blockIdx.x & 7, rank = blockIdx.x >> 3;
            const int nwg = (gridDim.x - home + 7) >> 3;              // workgroups whose home is this chunk
            const int len = wq_len(total, home), c0 = wq_chunk0(total, home);
            home_ctr = ctr + 8 * blockIdx.z + home;
            home_c0 = c0 + nwg;
            home_len = len - nwg;
            item = rank < len ? c0 + rank : -1;
            step = 0; item_end = 0;
            if (threadIdx.x == 0) {
                int nx = -1;
                if (item >= 0 && home_len > 0) {
                    const int i = atomicAdd(home_ctr, 1);
                    if (i < home_len) nx = home_c0 + i;
                }
                slot[0] = nx;
            }
            __syncthreads();
        }
    }
    // the item after the current one (-1: none)
    __device__ __forceinline__ int next(const int* slot) const {
        if constexpr (!STEAL) return item + step < item_end ? item + step : -1;
        else return __builtin_amdgcn_readfirstlane(slot[step]);
    }
    // epilogue, ahead of the stores: request the item after `nxt` (one lane; the round trip hides under the stores)
    __device__ __forceinline__ int request(int nxt) const {
        int r = -1;
        if constexpr (STEAL) {
            if (threadIdx.x == 0 && nxt >= 0) {
                const int i = atomicAdd(home_ctr, 1);
                r = i < home_len ? home_c0 + i : -1;
            }
        }
        return r;
    }
    // epilogue, behind the stores and ahead of a workgroup barrier: publish it
    __device__ __forceinline__ void publish(int pulled, int* slot) const {
        if constexpr (STEAL) { if (threadIdx.x == 0) slot[step ^ 1] = pulled; }
    }
    // move on to `nxt` (behind that barrier in work-stealing mode)
    __device__ __forceinline__ void advance(int nxt) {
        item = nxt;
        if constexpr (STEAL) step ^= 1;
    }
    // every exit path: the last workgroup to leave zeroes the launch's counters (the next launch on the stream finds them clean)
    __device__ __forceinline__ void done(int* ctr) const {
        if constexpr (STEAL) {
            if (threadIdx.x == 0) {
                const int n = gridDim.x * gridDim.z;
                if (atomicAdd(ctr + 8 * WQ_Z, 1) == n - 1) {
                    for (int i = 0; i <= 8 * WQ_Z; ++i) __hip_atomic_store(ctr + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
};

static bool wino_interleave_ok(size_t u_bytes) {
    static const char* e = getenv("TG_WINO_INTERLEAVE");          // 0 / 1 force, default: by the size of U
    if (e) return atoi(e) != 0;
    return u_bytes <= ((size_t)6 << 20);
}

__host__ __device__ __forceinline__ int wino_swz(int row, int kk) { return ((((kk >> 2) ^ (row >> 4)) & 1) << 2) + (kk & 3); }

// U[k/8][n/64][xi][n%64][k%8 (half-swizzled)] = (G g Gt)[xi] for every (n, k)
// S2D: `w` is the raw [Cout][5][5][cin5] weight of a 5x5 stride-2 layer and the 3x3 taps over the 4*cin5 space-to-depth
// channels are gathered from it on the fly (w2[co][ty][tx][(dy,dx,c)] = w[co][2ty+dy][2tx+dx][c], 0 beyond the 5x5): the
// regrouped copy is never needed once U exists.
template <bool S2D>
__device__ __forceinline__ void wino_weights_body(const float* __restrict__ w, float* __restrict__ U, int N, int K,
                                                  const WinoWeights& ww, int cin5 = 0) {
    const int NT = N / WINO_BN;
    const size_t total = (size_t)N * K;
    const int KC = K >> 3;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        // thread order = the order of the U image: (k % 8, n % 64) inside one 2 KB block of a transform point -- the sixteen
        // stores of 512 consecutive threads are sixteen contiguous 2 KB runs (ordering by the source made them 32-byte pieces:
        // 4x write amplification on 1.8x the bytes of the read side)
        const int blk = (int)(idx >> 9);
        const int k = (blk % KC) * 8 + (int)(idx & 7), n = (blk / KC) * WINO_BN + (int)((idx >> 3) & 63);
        float g[3][3];
        if constexpr (S2D) {
            const int c2 = ww.k_fast ? k : n, co = ww.k_fast ? n : k;          // forward: n = co, k = (phase, c); dgrad: the reverse
            const int ph = c2 / cin5, c = c2 - ph * cin5, dy = ph >> 1, dx = ph & 1;
            const float* wp = w + (size_t)co * 25 * cin5 + c;
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const int ky = 2 * ww.kyu[u] + dy, kx = 2 * ww.kxv[v] + dx;
                    g[u][v] = (ky < 5 && kx < 5) ? wp[(size_t)(ky * 5 + kx) * cin5] : 0.f;
                }
        } else {
            const float* wp = w + (size_t)n * ww.sn + (size_t)k * ww.sk;
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v) g[u][v] = wp[(size_t)(ww.kyu[u] * 3 + ww.kxv[v]) * ww.stap];
        }
        float tg[4][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            tg[0][v] = g[0][v];
            tg[1][v] = 0.5f * (g[0][v] + g[1][v] + g[2][v]);
            tg[2][v] = 0.5f * (g[0][v] - g[1][v] + g[2][v]);
            tg[3][v] = g[2][v];
        }
        const int row = n % WINO_BN;
        float* ub = U + ((size_t)(k >> 3) * NT + n / WINO_BN) * WINO_U + row * 8 + wino_swz(row, k & 7);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ub[(a * 4 + 0) * (WINO_BN * 8)] = tg[a][0];
            ub[(a * 4 + 1) * (WINO_BN * 8)] = 0.5f * (tg[a][0] + tg[a][1] + tg[a][2]);
            ub[(a * 4 + 2) * (WINO_BN * 8)] = 0.5f * (tg[a][0] - tg[a][1] + tg[a][2]);
            ub[(a * 4 + 3) * (WINO_BN * 8)] = tg[a][2];
        }
    }
}
__global__ __launch_bounds__(256) void wino_weights_kernel(const float* __restrict__ w, float* __restrict__ U, int N, int K,
                                                           WinoWeights ww) {
    wino_weights_body<false>(w, U, N, K, ww);
}

// Weight preparation of MANY layers in one launch (tg_conv_wprep_run): one descriptor per (layer, mode), blockIdx.y = descriptor.
// kind 1: the Winograd transform above; kind 2: the [Cout][taps][Cin] -> [Cin][taps][Cout] transpose of the gather dgrads;
// kind 3: the F(2x2,2x2) transform of the 4x4 stride-2 layers (wino22.inc); kind 4: kind 1 for a 5x5 stride-2 layer, gathered
// straight from the 5x5 weights.
struct W22Weights {
    long sn, sk;        // element strides of the raw 4x4 weights: output row n, contraction index k (within a phase)
    int cin;            // Cin of the raw weights
    int by_phase;       // 1 (forward): k = (phase, c), the phase picks (dy, dx); 0 (dgrad): (dy, dx) = the class of the slice
    int ncls;
    int tyu[2], txv[2]; // patch tap u (0..1 from the patch origin) -> kernel tap ty ; v -> tx
    int k_fast;
};
__device__ void wino22_weights_body(const float* __restrict__ w, float* __restrict__ U, int N, int K, const W22Weights& ww);   // wino22.inc
__device__ void wino_weights16_body(const float* __restrict__ w, __bf16* __restrict__ U, int N, int K, const WinoWeights& ww);  // wino16.inc
struct TgWprepItem {
    int kind, N, K, taps;
    const float* w;
    float* out;
    WinoWeights ww;
    W22Weights w22;
};
static thread_local TgWprepItem* g_wprep_capture = nullptr;       // set by tg_conv_wprep_item: describe instead of launching
static thread_local int g_wprep_captured = 0;                     // 1: item filled, -1: this (geometry, mode) cannot be batched
__global__ __launch_bounds__(256) void wprep_multi_kernel(const TgWprepItem* __restrict__ items) {
    const TgWprepItem it = items[blockIdx.y];
    if (it.kind == 1) {
        wino_weights_body<false>(it.w, it.out, it.N, it.K, it.ww);
    } else if (it.kind == 4) {
        wino_weights_body<true>(it.w, it.out, it.N, it.K, it.ww, it.taps);      // taps = Cin of the 5x5 layer
    } else if (it.kind == 3) {
        wino22_weights_body(it.w, it.out, it.N, it.K, it.w22);
    } else if (it.kind == 5) {
        wino_weights16_body(it.w, reinterpret_cast<__bf16*>(it.out), it.N, it.K, it.ww);      // bf16 mode's U image
    } else {
        // transpose [cout][taps][cin] -> [cin][taps][cout] (N = cout, K = cin) in 32 x 32 tiles through LDS: both the reads
        // (cin-contiguous) and the writes (cout-contiguous) are 128-byte rows (the element-wise form read 4 bytes per line)
        __shared__ float tile[32][33];
        const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8 threads
        const int nco = (it.N + 31) >> 5, nci = (it.K + 31) >> 5;
        const int ntiles = nco * nci * it.taps;
        for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
            const int t = tl % it.taps, r = tl / it.taps;
            const int co0 = (r % nco) * 32, ci0 = (r / nco) * 32;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + ty + 8 * j, ci = ci0 + tx;
                tile[ty + 8 * j][tx] = (co < it.N && ci < it.K) ? it.w[((size_t)co * it.taps + t) * it.K + ci] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ci = ci0 + ty + 8 * j, co = co0 + tx;
                if (co < it.N && ci < it.K) it.out[((size_t)ci * it.taps + t) * it.N + co] = tile[tx][ty + 8 * j];
            }
        }
    }
}

// FAST (no source mask, source and U below 2 GB): the operands come through buffer descriptors -- the per-step part of every
// address rides in the instruction's SCALAR offset and padding slots read zeros through the bounds check, so a K step
// carries no address arithmetic and no patch scaling on the vector ALU (every VALU instruction beside the fp32 MFMAs costs
// the matrix pipe ~2.5 ns: tools/micro/mfma_issue_mix.hip).
// GATED: the launch carries a fused activation-backward gate and writes its outputs directly (no split-K slabs): the gate
// quads are fetched ahead of the stores, which costs 12 registers the ungated instantiation keeps.
template <bool FAST, bool GATED, bool STEAL>
__global__ __launch_bounds__(WINO_THREADS) void wino_kernel(const IGemmParams p, const WinoGeom q, const float* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                            // [2][16][64][8]
    float* Us = smem + 2 * WINO_V;               // [2][16][64][8]
    float* Ps = smem + 2 * WINO_V + 2 * WINO_U;  // [18*18][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    // Persistent workgroup walking work items (patch x N tile, N tile fastest).  The next item's first operands are requested
    // BEFORE the current item's output stores (vmcnt retires in order: a load behind the stores would have to wait for their
    // write acknowledgements) and the stores then drain underneath the next item's prologue -- with one workgroup per CU
    // (141 KB LDS) nothing else would hide either latency.
    __shared__ int wq_slot[2];
    WinoWork<STEAL> wk;
    wk.init(q.total_work, q.interleave, q.qctr, wq_slot);

    int n0, oy0, ox0, b;
    const float* Ub;
    uint32_t poff[2];
    float pmul[2];
    int i_nt, i_tx, i_ty;
    auto locate = [&]() {       // (N tile, patch x, patch y, image) of the current item
        const int item = wk.item;
        i_nt = item % q.nt;
        int tile = item / q.nt;
        i_tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        i_ty = tile % q.tiles_y;
        b = tile / q.tiles_y;
    };
    auto decode = [&]() {
        n0 = i_nt * WINO_BN; oy0 = i_ty * 16; ox0 = i_tx * 16;
        Ub = U + (size_t)i_nt * WINO_U;
        const int py0 = oy0 + q.sy_min, px0 = ox0 + q.sx_min;
        // patch slots of this thread (pixel, channel quad), fixed over the K loop of the item
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (tid + WINO_THREADS * i) >> 1, spy = pp / 18, spx = pp - spy * 18;   // slot -> patch (row, column)
            const int iy = py0 + spy, ix = px0 + spx;
            poff[i] = FAST ? 0x80000000u : 0u;          // FAST: byte offset, out of range = beyond the descriptor's 2 GB limit
            pmul[i] = 0.f;
            if (pp < WINO_PPIX && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) {
                const uint32_t pix = ((uint32_t)b * p.IH + iy) * p.IW + ix;
                poff[i] = pix * (uint32_t)p.C + 4 * (tid & 1);
                if constexpr (FAST) poff[i] *= 4u;
                else pmul[i] = p.amask ? p.amask[pix] : 1.f;
            }
        }
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src), 0, FAST ? (int)((size_t)p.B * p.IH * p.IW * p.C * 4) : 0,
                                                         0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U), 0, FAST ? (int)((size_t)16 * p.N * p.C * 4) : 0, 0x00020000);
    const uint32_t u_voff = tid * 16;
    const bool p1_ok = ((tid + WINO_THREADS) >> 1) < WINO_PPIX;
    const int c_begin = blockIdx.z * q.chunks_per_split;
    const int c_end = min(p.C >> 3, c_begin + q.chunks_per_split);
    const int c_last = c_end - 1;
    const size_t ustep = (size_t)q.nt * WINO_U;

    f32x4 ru[4], rp[2];
    // unconditional loads (padding / unused slots read pixel 0 and are zeroed at pstore): a branch here would put an
    // s_waitcnt vmcnt(0) right behind each load
    auto pload1 = [&](int c, int i) {
        if constexpr (FAST) rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, poff[i], c * 32, 0));
        else rp[i] = *reinterpret_cast<const f32x4*>(p.src + poff[i] + c * 8);
    };
    auto uload1 = [&](int c, int j) {
        if constexpr (FAST)
            ru[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                ursrc, u_voff, (int)(((size_t)i_nt * WINO_U + (size_t)c * ustep) * 4) + 16 * WINO_THREADS * j, 0));
        else ru[j] = *reinterpret_cast<const f32x4*>(Ub + (size_t)c * ustep + 4 * (tid + WINO_THREADS * j));
    };
    auto pstore1 = [&](int i) {
        f32x4 v = rp[i];
        if constexpr (!FAST) {
            v = v * pmul[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pmul[i] != 0.f ? v[e] : 0.f;     // padding is 0 even next to inf/nan data
        }
        if (i == 0 || p1_ok) *reinterpret_cast<f32x4*>(Ps + 4 * (tid + WINO_THREADS * i)) = v;
    };
    auto ustore1 = [&](int buf, int j) { *reinterpret_cast<f32x4*>(Us + buf * WINO_U + 4 * (tid + WINO_THREADS * j)) = ru[j]; };

    // input transform: thread = (tile, channel quad, row a of V = Bt d B); a is wave-uniform
    //   a = 0: d0 - d2   a = 1: d1 + d2   a = 2: d2 - d1   a = 3: d1 - d3
    const int t_quad = lane & 1, t_tile = (lane >> 1) + 32 * (wave & 1), t_a = wave >> 1;
    // (rows ordered so that the first one always enters with +1: a = 2 reads d2 first -- ONE fma per element instead of
    //  mul + fma; on gfx950 every VALU instruction beside an fp32 MFMA costs ~2.4 cycles of the matrix pipe,
    //  tools/micro/mfma_valu_overlap.hip)
    const int t_r0 = t_a == 0 ? 0 : (t_a == 2 ? 2 : 1), t_r1 = t_a == 3 ? 3 : (t_a == 2 ? 1 : 2);
    const float t_s1 = t_a == 1 ? 1.f : -1.f;
    const int t_src0 = ((2 * (t_tile >> 3) + t_r0) * 18 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_src1 = ((2 * (t_tile >> 3) + t_r1) * 18 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_dst = (t_a * 4) * 512 + t_tile * 8 + (((t_quad ^ (t_tile >> 4)) & 1) << 2);
    f32x4 td[2][4], tt[4];
    auto t_read1 = [&](int k) {     // k = 0..7: (row k/4, column k%4)
        td[k >> 2][k & 3] = *reinterpret_cast<const f32x4*>(Ps + ((k >> 2) ? t_src1 : t_src0) + (k & 3) * 8);
    };
    auto t_row1 = [&](int j) { tt[j] = td[0][j] + td[1][j] * t_s1; };
    auto t_col1 = [&](int buf, int k) {
        const f32x4 v = k == 0 ? tt[0] - tt[2] : k == 1 ? tt[1] + tt[2] : k == 2 ? tt[2] - tt[1] : tt[1] - tt[3];
        *reinterpret_cast<f32x4*>(Vs + buf * WINO_V + t_dst + k * 512) = v;
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * 512 + arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = (8 * xh) * 512 + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    if (wk.item < 0 || c_begin >= c_end) { wk.done(q.qctr); return; }
    locate();
    decode();
#pragma unroll
    for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) uload1(c_begin, j);

    for (;;) {
    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    {
        // prologue: rp / ru hold step c_begin (requested before the previous item's stores); it is staged synchronously
        // while the operands of step c_begin+1 are in flight
#pragma unroll
        for (int i = 0; i < 2; ++i) pstore1(i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ustore1(0, j);
#pragma unroll
        for (int i = 0; i < 2; ++i) pload1(min(c_begin + 1, c_last), i);
#pragma unroll
        for (int j = 0; j < 4; ++j) uload1(min(c_begin + 1, c_last), j);
        wino_barrier();
#pragma unroll
        for (int k = 0; k < 8; ++k) t_read1(k);
#pragma unroll
        for (int j = 0; j < 4; ++j) t_row1(j);
#pragma unroll
        for (int k = 0; k < 4; ++k) t_col1(0, k);
        wino_barrier();
        // fragments of ONE transform point at a time, double-buffered (the micro-benchmark shows that back-to-back MFMAs
        // on one accumulator issue at the full rate, so no accumulator rotation -- and 16 fewer registers -- is needed)
        f32x4 fa[2], fb[2];
        fa[0] = *reinterpret_cast<const f32x4*>(Vs + a_off);
        fb[0] = *reinterpret_cast<const f32x4*>(Us + b_off);
        int cur = 0;
        for (int c = c_begin; c < c_end; ++c) {
            const int nxt = cur ^ 1;
            const int c2 = min(c + 2, c_last);               // tail steps: redundant staging instead of branches
            const float* Vc = Vs + cur * WINO_V + a_off;
            const float* Uc = Us + cur * WINO_U + b_off;
            const float* Vn = Vs + nxt * WINO_V + a_off;
            const float* Un = Us + nxt * WINO_U + b_off;
            // 32 MFMA ticks: t = 4*xi + e  (transform point xi of this wave's 8, k-pair e)
            wino_static_for(std::make_integer_sequence<int, 32>{}, [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int xi = t >> 2, e = t & 3;
                // rp / ru hold the operands of step c+1 (loaded during step c-1)
                if constexpr (t < 2) pstore1(t);                           // patch c+1 -> LDS (readers of patch c are done)
                if constexpr (t >= 2 && t < 4) pload1(c2, t - 2);          // patch c+2 -> rp
                if constexpr (t == 4) wino_barrier();                      // patch c+1 visible
                if constexpr (t >= 5 && t < 9) { t_read1(t - 5); t_read1(4 + t - 5); }      // column t-5 of both patch rows
                if constexpr (t >= 8 && t < 12) { t_row1(t - 8); }                          // ... combined three ticks later
                if constexpr (t >= 14 && t < 18) t_col1(nxt, t - 14);
                if constexpr (t >= 18 && t < 22) ustore1(nxt, t - 18);
                if constexpr (t >= 22 && t < 26) uload1(c2, t - 22);       // U c+2 -> ru
                if constexpr (t == 26) wino_barrier();                     // V / U images of step c+1 complete
                // fragments of the next point go to the other buffer while this point's four MFMAs run; the last point
                // fetches point 0 of the next step (behind barrier t = 26)
                if constexpr (e == 0 && xi < 7) {
                    fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Vc + (xi + 1) * 512);
                    fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Uc + (xi + 1) * 512);
                }
                if constexpr (e == 0 && xi == 7) {
                    fa[0] = *reinterpret_cast<const f32x4*>(Vn);
                    fb[0] = *reinterpret_cast<const f32x4*>(Un);
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
            cur = nxt;
        }
    }
    const int e_n0 = n0, e_oy0 = oy0, e_ox0 = ox0, e_b = b;      // output coordinates of the finished item
    const int wq_next = wk.next(wq_slot);
    const bool more_items = wq_next >= 0;
    const int wq_pulled = wk.request(wq_next);
    wino_barrier();        // the exchange area and the epilogue scratch overlay V / U

    // Output transform Y = At M A.  This wave holds rows a = 2*xh, 2*xh+1 of M; row sums s[a][j] = sum_b At[j][b] M[a][b]
    // are local.  Y[0][j] = s0j + s1j + s2j and Y[1][j] = s1j - s2j - s3j: the xh = 0 waves finish output row 0 (they
    // need s2j from their partner), the xh = 1 waves output row 1 (they need s1j).
    float* X = smem;                                         // [xh][nw][mw][j][16][64]
    float* scratch = smem + 16 * 1024 + wave * (32 * 36);
    f32x16 own[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float* xs = X + (((xh * 2 + nw) * 2 + mw) * 2 + j) * 1024 + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s0 = j == 0 ? acc[0][r] + acc[1][r] + acc[2][r] : acc[1][r] - acc[2][r] - acc[3][r];
            const float s1 = j == 0 ? acc[4][r] + acc[5][r] + acc[6][r] : acc[5][r] - acc[6][r] - acc[7][r];
            own[j][r] = xh == 0 ? s0 + s1 : -s0 - s1;
            xs[r * 64] = xh == 0 ? s1 : s0;
        }
    }
    // the accumulators are dead now: switch the staging state to the next item and request its first operands -- ahead of
    // the stores below (see the head of the kernel)
    if (more_items) {
        wk.item = wq_next;       // (the staging state switches to the next item here; wk.advance() below completes the move)
        locate();
        decode();
#pragma unroll
        for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
        for (int j = 0; j < 4; ++j) uload1(c_begin, j);
    }
    wino_barrier();
    constexpr bool gated = GATED;
    // bias (the same four channels for every row of this lane) and the row scales are fetched ahead of the stores too
    f32x4 bq = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && p.splits == 1) bq = *reinterpret_cast<const f32x4*>(p.bias + e_n0 + 32 * nw + 4 * (lane & 7));
    float rsq[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};       // the row scales of both halves: eight registers
    if (p.rowscale && p.splits == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int t = 32 * mw + (lane >> 3) + 8 * t4;
                const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                rsq[j][t4] = p.rowscale[((size_t)e_b * p.DH + (oy * p.ds + p.dy0)) * p.DW + (ox * p.ds + p.dx0)];
            }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // A fused activation-backward gate is fetched for the four rows of this half BEFORE its stores: on gfx9 vmcnt counts
        // stores too, so a gate load issued between two stores waits for the earlier rows' write acknowledgements -- eight
        // exposed round trips per work item (29.7 us against 24.7 us ungated on the 64-channel VGG dgrad); this way it is two.
        f32x4 gq[GATED ? 4 : 1];
        if constexpr (gated) {
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int t = 32 * mw + (lane >> 3) + 8 * t4;
                const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + p.dy0)) * p.DW + (ox * p.ds + p.dx0);
                gq[t4] = *reinterpret_cast<const f32x4*>(p.gate + pix * p.N + e_n0 + 32 * nw + 4 * (lane & 7));
            }
        }
        const float* xr = X + ((((xh ^ 1) * 2 + nw) * 2 + mw) * 2 + j) * 1024 + lane;
        f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = own[j][r] + xr[r * 64];
        tile_rows4i(scratch, y, lane, [&](int t4, int rr, int cc, f32x4 v4) {
            const int t = 32 * mw + rr;
            const int oy = e_oy0 + 2 * (t >> 3) + xh, ox = e_ox0 + 2 * (t & 7) + j;
            const int nb = e_n0 + 32 * nw + cc;
            if (oy >= p.OH || ox >= p.OW) return;
            if (p.splits > 1) {
                const size_t m = ((size_t)e_b * p.OH + oy) * p.OW + ox;
                *reinterpret_cast<f32x4*>(p.ws + ((size_t)blockIdx.z * p.M + m) * p.N + nb) = v4;
            } else {
                const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + p.dy0)) * p.DW + (ox * p.ds + p.dx0);
                *reinterpret_cast<f32x4*>(p.dst + pix * p.N + nb) = epilogue4(p, v4, pix, nb, gated ? &gq[gated ? t4 : 0] : nullptr, &rsq[j][t4], &bq);
            }
        });
    }
    wk.publish(wq_pulled, wq_slot);
    if (!more_items) break;
    wino_barrier();        // every wave is done with the exchange area / scratch before the next prologue stages into it
    wk.advance(wq_next);
    }
    wk.done(q.qctr);
}

// wino_kernel<FAST> with the staging pipeline running ACROSS work items.  The K loop of wino_kernel stages "the next step"
// while the MFMAs consume the current one -- and in an item's last step that staging is redundant work, after which the next
// item begins with a synchronous prologue (load, stage, transform: ~2.2 us per item with the matrix pipe idle, 9 % of an
// 8-step item).  Here the last two steps of an item load and stage the FIRST two steps of the next item instead, so every
// item but a workgroup's first starts with its step-0 images already in LDS.  The output transform then has to live in what
// the pipeline leaves free -- the V / U buffer of the step just consumed and the patch area -- so the two output halves are
// exchanged one after the other (32 KB) and the eighth wave's transposition scratch sits in the patch area.
// Needs at least two K steps per item and split.
// POOL: the 2x2 max-pool of the activated output goes out with it (p.pool_dst, VGG trunk conv1_2 / conv2_2): a 2x2 output tile IS a
// pooling window -- its two columns are the two halves j of the epilogue (same lane), its two rows sit in the waves xh = 0 / 1, so the
// xh = 1 wave hands its row maxima over through the exchange slot it has just consumed (no extra barrier) and the xh = 0 wave stores.
// GBITS (with GATED): the ReLU gate comes as p.gate_bits -- one dword per pixel and 32-channel group, shared by the 8 lanes of a
// row of tile_rows4i, each of which takes its nibble (channels e_nb0 + 4 (lane & 7) .. + 3; e_nb0 is a multiple of 32 here).
// SPARSE (static walk, one split, ungated): the batch is [pred; target] (2 nb images) and q.sp_* is its tile map (tg_vgg_sparse_map).
// The items are the target half's, dense, followed by `count` list entries of the prediction half (x q.nt, N tile fastest
// in both parts); a target item whose tile is NOT in the map repeats its stores -- the same registers -- into image b - nb,
// whose result is that one bit for bit.  Prediction items write only mapped tiles, mirrors only the others: one writer per tile.
// SPARSE = 2 (static walk, one split; gated or not): the batch is nb images and the items are the `count` list entries alone (x q.nt)
// -- no dense half, no mirror stores; tiles outside the map are not written at all (the trunk's dgrads, tg_conv_dgrad_sparse).  An
// output pixel of F(2x2,3x3) is a function of its own 3x3 input window (y0 = m0 + m1 + m2 never sees d3, y1 never d0, and the two
// xi-halves exchange only the sums the partner's rows take), so a listed tile's pixels do not depend on what the rest of the patch
// holds beyond their windows: bit for bit the dense launch's values wherever those windows are valid.  These forms compile the
// split-K, row-scale and accumulate paths out, which is what keeps them at 0 bytes of scratch with the list pointer in scalar
// registers (254 VGPRs, 86-96 SGPRs on ROCm 7): re-check that with --save-temps whenever the compiler changes.
template <bool GATED, bool STEAL, bool POOL = false, bool GBITS = false, int SPARSE = 0>
__global__ __launch_bounds__(WINO_THREADS) void wino_pipe_kernel(const IGemmParams p, const WinoGeom q, const float* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                            // [2][16][64][8]
    float* Us = smem + 2 * WINO_V;               // [2][16][64][8]
    float* Ps = smem + 2 * WINO_V + 2 * WINO_U;  // [18*18][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    __shared__ int wq_slot[2];
    WinoWork<STEAL> wk;
    int total = q.total_work;
    if constexpr (SPARSE != 0) {
        const int cnt = __builtin_amdgcn_readfirstlane(*q.sp_count);
        total = ((SPARSE == 1 ? q.sp_tiles : 0) + min(max(cnt, 0), q.sp_tiles)) * q.nt;
    }
    wk.init(total, q.interleave, q.qctr, wq_slot);

    // coordinates and patch slots of an item
    struct Item { int nt, n0, oy0, ox0, b, mirror; uint32_t poff[2]; };
    auto decode_item = [&](int it) {
        Item r;
        r.nt = it % q.nt;
        int tile = it / q.nt;
        r.mirror = 0;
        if constexpr (SPARSE == 2) tile = __builtin_amdgcn_readfirstlane(q.sp_list[tile]);
        if constexpr (SPARSE == 1) {
            if (tile < q.sp_tiles) {             // target image nb + b: mirrored into b where the map leaves the tile out
                r.mirror = (__builtin_amdgcn_readfirstlane(q.sp_bits[tile >> 5]) >> (tile & 31)) & 1 ? 0 : 1;
                tile += q.sp_tiles;
            } else {
                tile = __builtin_amdgcn_readfirstlane(q.sp_list[tile - q.sp_tiles]);
            }
        }
        const int tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        const int ty = tile % q.tiles_y;
        r.b = tile / q.tiles_y;
        r.n0 = r.nt * WINO_BN; r.oy0 = ty * 16; r.ox0 = tx * 16;
        const int py0 = r.oy0 + q.sy_min, px0 = r.ox0 + q.sx_min;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (tid + WINO_THREADS * i) >> 1, spy = pp / 18, spx = pp - spy * 18;
            const int iy = py0 + spy, ix = px0 + spx;
            r.poff[i] = 0x80000000u;          // out of range = beyond the descriptor's 2 GB limit: reads 0
            if (pp < WINO_PPIX && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW)
                r.poff[i] = ((((uint32_t)r.b * p.IH + iy) * p.IW + ix) * (uint32_t)p.C + 4 * (tid & 1)) * 4u;
        }
        return r;
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src), 0, (int)((size_t)p.B * p.IH * p.IW * p.C * 4), 0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U), 0, (int)((size_t)16 * p.N * p.C * 4), 0x00020000);
    const uint32_t u_voff = tid * 16;
    const bool p1_ok = ((tid + WINO_THREADS) >> 1) < WINO_PPIX;
    const int c_begin = blockIdx.z * q.chunks_per_split;
    const int c_end = min(p.C >> 3, c_begin + q.chunks_per_split);
    const size_t ustep = (size_t)q.nt * WINO_U;

    f32x4 ru[4], rp[2];
    auto pload1 = [&](uint32_t voff, int c, int i) { rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, voff, c * 32, 0)); };
    auto uload1 = [&](int nt, int c, int j) {
        ru[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            ursrc, u_voff, (int)(((size_t)nt * WINO_U + (size_t)c * ustep) * 4) + 16 * WINO_THREADS * j, 0));
    };
    auto pstore1 = [&](int i) { if (i == 0 || p1_ok) *reinterpret_cast<f32x4*>(Ps + 4 * (tid + WINO_THREADS * i)) = rp[i]; };
    auto ustore1 = [&](int buf, int j) { *reinterpret_cast<f32x4*>(Us + buf * WINO_U + 4 * (tid + WINO_THREADS * j)) = ru[j]; };

    // input transform: thread = (tile, channel quad, row a of V = Bt d B); a is wave-uniform (see wino_kernel)
    const int t_quad = lane & 1, t_tile = (lane >> 1) + 32 * (wave & 1), t_a = wave >> 1;
    const int t_r0 = t_a == 0 ? 0 : (t_a == 2 ? 2 : 1), t_r1 = t_a == 3 ? 3 : (t_a == 2 ? 1 : 2);
    const float t_s1 = t_a == 1 ? 1.f : -1.f;
    const int t_src0 = ((2 * (t_tile >> 3) + t_r0) * 18 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_src1 = ((2 * (t_tile >> 3) + t_r1) * 18 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_dst = (t_a * 4) * 512 + t_tile * 8 + (((t_quad ^ (t_tile >> 4)) & 1) << 2);
    f32x4 td[2][4], tt[4];
    auto t_read1 = [&](int k) { td[k >> 2][k & 3] = *reinterpret_cast<const f32x4*>(Ps + ((k >> 2) ? t_src1 : t_src0) + (k & 3) * 8); };
    auto t_row1 = [&](int j) { tt[j] = td[0][j] + td[1][j] * t_s1; };
    auto t_col1 = [&](int buf, int k) {
        const f32x4 v = k == 0 ? tt[0] - tt[2] : k == 1 ? tt[1] + tt[2] : k == 2 ? tt[2] - tt[1] : tt[1] - tt[3];
        *reinterpret_cast<f32x4*>(Vs + buf * WINO_V + t_dst + k * 512) = v;
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * 512 + arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = (8 * xh) * 512 + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    if (wk.item < 0 || c_begin >= c_end) { wk.done(q.qctr); return; }
    Item ci = decode_item(wk.item);
    // prologue of the workgroup's FIRST item: step c_begin staged synchronously, step c_begin + 1 in flight
#pragma unroll
    for (int i = 0; i < 2; ++i) pload1(ci.poff[i], c_begin, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) uload1(ci.nt, c_begin, j);
#pragma unroll
    for (int i = 0; i < 2; ++i) pstore1(i);
#pragma unroll
    for (int j = 0; j < 4; ++j) ustore1(0, j);
#pragma unroll
    for (int i = 0; i < 2; ++i) pload1(ci.poff[i], c_begin + 1, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) uload1(ci.nt, c_begin + 1, j);
    wino_barrier();
#pragma unroll
    for (int k = 0; k < 8; ++k) t_read1(k);
#pragma unroll
    for (int j = 0; j < 4; ++j) t_row1(j);
#pragma unroll
    for (int k = 0; k < 4; ++k) t_col1(0, k);
    wino_barrier();
    int cur = 0;

    for (;;) {
        f32x16 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        const int wq_next = wk.next(wq_slot);
        const bool more_items = wq_next >= 0;
        const Item ni = decode_item(more_items ? wq_next : wk.item);         // the last item restages itself (unused)
        f32x4 fa[2], fb[2];
        fa[0] = *reinterpret_cast<const f32x4*>(Vs + cur * WINO_V + a_off);
        fb[0] = *reinterpret_cast<const f32x4*>(Us + cur * WINO_U + b_off);
        // one K step: MFMAs on buffer `cur`, the following step staged into the other buffer, the operands of step c2 of the
        // item with patch offsets pv0 / pv1 and N tile unt requested
        auto kstep = [&](uint32_t pv0, uint32_t pv1, int unt, int c2) {
            const int nxt = cur ^ 1;
            const float* Vc = Vs + cur * WINO_V + a_off;
            const float* Uc = Us + cur * WINO_U + b_off;
            const float* Vn = Vs + nxt * WINO_V + a_off;
            const float* Un = Us + nxt * WINO_U + b_off;
            wino_static_for(std::make_integer_sequence<int, 32>{}, [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int xi = t >> 2, e = t & 3;
                if constexpr (t < 2) pstore1(t);                           // patch of the following step -> LDS
                if constexpr (t == 2) pload1(pv0, c2, 0);
                if constexpr (t == 3) pload1(pv1, c2, 1);
                if constexpr (t == 4) wino_barrier();
                if constexpr (t >= 5 && t < 9) { t_read1(t - 5); t_read1(4 + t - 5); }
                if constexpr (t >= 8 && t < 12) { t_row1(t - 8); }
                if constexpr (t >= 14 && t < 18) t_col1(nxt, t - 14);
                if constexpr (t >= 18 && t < 22) ustore1(nxt, t - 18);
                if constexpr (t >= 22 && t < 26) uload1(unt, c2, t - 22);
                if constexpr (t == 26) wino_barrier();                     // V / U images of the following step complete
                if constexpr (e == 0 && xi < 7) {
                    fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Vc + (xi + 1) * 512);
                    fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Uc + (xi + 1) * 512);
                }
                if constexpr (e == 0 && xi == 7) {
                    fa[0] = *reinterpret_cast<const f32x4*>(Vn);
                    fb[0] = *reinterpret_cast<const f32x4*>(Un);
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
            cur = nxt;
        };
        // all steps but the last two request step c + 2 of this item; the last two request steps 0 and 1 of the next one
        for (int c = c_begin; c < c_end - 2; ++c) kstep(ci.poff[0], ci.poff[1], ci.nt, c + 2);
        kstep(ni.poff[0], ni.poff[1], ni.nt, c_begin);
        kstep(ni.poff[0], ni.poff[1], ni.nt, c_begin + 1);
        // `cur` now holds the next item's step-0 images; the buffer of the step just consumed (cur ^ 1) and the patch area are
        // free (every read of them completed before the last barrier of the loop)
        // the item after the next one: requested now, its round trip hides under the epilogue (the next item is re-read from its
        // LDS word / recomputed instead of being kept alive across the K loop)
        const int wq_pulled = wk.request(wk.next(wq_slot));
        const int fr = cur ^ 1;
        float* X = Vs + fr * WINO_V;                                 // [xh][nw][mw][16][64] of ONE output half
        float* scratch = wave < 7 ? Us + fr * WINO_U + wave * (32 * 36) : Ps;
        // Addresses of the epilogue (splits == 1): dst / gate / row-scale pixels of this lane are
        //     row  (oy0 + 8 mw + 2 t4 + xh) * ds + dy0        -- wave-uniform, t4 = 0..3 the row group of tile_rows4i
        //     col  (ox0 + 2 (lane >> 3) + j) * ds + dx0       -- a lane constant + uniform terms
        // so every access is a buffer instruction with ONE lane offset (computed once per half) and a scalar offset; a lane
        // beyond the right edge gets the out-of-range marker (loads give 0, stores are dropped), a row beyond the bottom edge
        // is a scalar branch.  The generic form -- 64-bit pixel arithmetic, clamps and act / bias / accumulate switches per
        // store -- was ~1000 vector and ~600 scalar instructions per item and wave: 6.5 us of a 27 us item on the
        // 64-channel layers (tools/wino_item_overhead.py).
        const int e_wave = __builtin_amdgcn_readfirstlane(wave);
        const int e_mw = e_wave & 1, e_nw = (e_wave >> 1) & 1, e_xh = e_wave >> 2;
        const int e_row0 = ci.oy0 + 8 * e_mw + e_xh;                             // + 2 * t4
        const int e_pitch = p.DW * p.ds;                                         // dst pixels per output row
        const int e_pix0 = (ci.b * p.DH + p.dy0) * p.DW + p.dx0 + ci.ox0 * p.ds; // + row * e_pitch + (2 (lane >> 3) + j) * ds
        const int e_nb0 = ci.n0 + 32 * e_nw;
        const uint32_t e_lane_px = 2 * (lane >> 3) * p.ds;
        const bool e_single = SPARSE == 2 || p.splits == 1;      // (the list-only form: one split, no row scales, no accumulation)
        const float act_neg = p.act == TG_ACT_RELU ? 0.f : (p.act == TG_ACT_LEAKY ? p.slope : 1.f);
        const float gate_neg = p.gate_act == TG_ACT_LEAKY ? p.gate_slope : 0.f;
        const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(p.dst, 0, (int)((size_t)p.B * p.DH * p.DW * p.N * 4), 0x00020000);
        const int e_mdelta = SPARSE == 1 ? q.sp_nb * p.DH * p.DW * p.N * 4 : 0;       // bytes from image nb + b to image b
        f32x4 bq = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && e_single) bq = *reinterpret_cast<const f32x4*>(p.bias + e_nb0 + 4 * (lane & 7));
        f32x4 pmx[POOL ? 4 : 1];
        uint32_t jbits = 0;            // POOL: bit (4 t4 + e) = the row maximum of that element sits in column j = 1
        if constexpr (POOL) {
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) pmx[t4] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float rsq[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};
        if (SPARSE != 2 && p.rowscale && e_single) {
            const auto rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.rowscale), 0, (int)((size_t)p.B * p.DH * p.DW * 4), 0x00020000);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t voff = ci.ox0 + 2 * (lane >> 3) + j < p.OW ? e_lane_px * 4u : 0x80000000u;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int row = min(e_row0 + 2 * t4, p.OH - 1);              // (rows beyond the edge are never stored)
                    rsq[j][t4] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        rrsrc, voff, (e_pix0 + row * e_pitch + j * p.ds) * 4, 0));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // row sums of this half (see wino_kernel): own part stays, the partner's part goes through X
            f32x16 own;
            {
                float* xs = X + ((xh * 2 + nw) * 2 + mw) * 1024 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s0 = j == 0 ? acc[0][r] + acc[1][r] + acc[2][r] : acc[1][r] - acc[2][r] - acc[3][r];
                    const float s1 = j == 0 ? acc[4][r] + acc[5][r] + acc[6][r] : acc[5][r] - acc[6][r] - acc[7][r];
                    own[r] = xh == 0 ? s0 + s1 : -s0 - s1;
                    xs[r * 64] = xh == 0 ? s1 : s0;
                }
            }
            // lane offset of this half inside dst / gate ([pixel][N] floats), marker beyond the right edge
            const uint32_t e_voff = ci.ox0 + 2 * (lane >> 3) + j < p.OW
                                        ? ((e_lane_px + j * p.ds) * (uint32_t)p.N + 4 * (lane & 7)) * 4u : 0x80000000u;
            f32x4 gq[GATED && !GBITS ? 4 : 1];
            uint32_t gw[GBITS ? 4 : 1];
            if constexpr (GBITS) {
                const int nw32 = p.N >> 5;
                const auto brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(p.gate_bits), 0, (int)((size_t)p.B * p.DH * p.DW * nw32 * 4), 0x00020000);
                const uint32_t b_voff = ci.ox0 + 2 * (lane >> 3) + j < p.OW ? (e_lane_px + j * p.ds) * (uint32_t)nw32 * 4u : 0x80000000u;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int row = min(e_row0 + 2 * t4, p.OH - 1);
                    gw[t4] = __builtin_amdgcn_raw_buffer_load_b32(brsrc, b_voff, ((e_pix0 + row * e_pitch) * nw32 + (e_nb0 >> 5)) * 4, 0)
                             >> (4 * (lane & 7));
                }
            } else if constexpr (GATED) {
                const auto grsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gate), 0, (int)((size_t)p.B * p.DH * p.DW * p.N * 4), 0x00020000);
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int row = min(e_row0 + 2 * t4, p.OH - 1);
                    gq[t4] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                        grsrc, e_voff, ((e_pix0 + row * e_pitch) * p.N + e_nb0) * 4, 0));
                }
            }
            wino_barrier();                  // the partners' sums are in X
            const float* xr = X + (((xh ^ 1) * 2 + nw) * 2 + mw) * 1024 + lane;
            f32x16 y;
#pragma unroll
            for (int r = 0; r < 16; ++r) y[r] = own[r] + xr[r * 64];
            tile_rows4i(scratch, y, lane, [&](int t4, int rr, int cc, f32x4 v4) {
                if (e_single) {
                    const int row = e_row0 + 2 * t4;
                    if (row >= p.OH) return;                                     // wave-uniform
                    const int soff = ((e_pix0 + row * e_pitch) * p.N + e_nb0) * 4;
                    f32x4 o = (v4 + bq) * rsq[j][t4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = o[e] > 0.f ? o[e] : o[e] * act_neg + 0.f;     // none / ReLU / leaky (act_neg = 1 / 0 / slope); + 0: ReLU gives +0
                    if constexpr (GBITS) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] *= (gw[t4] >> e) & 1u ? 1.f : 0.f;
                    } else if constexpr (GATED) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] *= gq[t4][e] > 0.f ? 1.f : gate_neg;
                    }
                    if (SPARSE != 2 && p.accumulate) o += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, e_voff, soff, 0));
                    if constexpr (POOL) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool gt = j == 1 && o[e] > pmx[t4][e];           // strictly greater: the first maximum wins
                            pmx[t4][e] = (j == 0 || gt) ? o[e] : pmx[t4][e];
                            jbits |= (gt ? 1u : 0u) << (4 * t4 + e);
                        }
                        if (p.pool_only) return;                                  // dst has no reader left: not written
                    }
                    // The row offset goes into the VECTOR offset of the store, not into its scalar offset: with
                    // `buffer_store_dwordx4 v[d:d+3], voff, rsrc, sN offen` a vector instruction that overwrote v[d] two
                    // instructions later changed the stored value in lanes 12-15 of each row on gfx950 (seen as integers in dx
                    // of the gated dgrad, gone with `s_nop 3` behind the store).  The compiler guards the documented hazard
                    // (a store of more than 64 bits followed by a write of its data registers) only for stores WITHOUT a
                    // scalar-register offset, as the ISA manual specifies it.
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), drsrc, e_voff + (uint32_t)soff, 0, 0);
                    if constexpr (SPARSE == 1) {
                        if (ci.mirror)
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), drsrc, e_voff + (uint32_t)(soff - e_mdelta), 0, 0);
                    }
                } else {
                    const int t = 32 * mw + rr;
                    const int oy = ci.oy0 + 2 * (t >> 3) + xh, ox = ci.ox0 + 2 * (t & 7) + j;
                    if (oy >= p.OH || ox >= p.OW) return;
                    const size_t m = ((size_t)ci.b * p.OH + oy) * p.OW + ox;
                    *reinterpret_cast<f32x4*>(p.ws + ((size_t)blockIdx.z * p.M + m) * p.N + ci.n0 + 32 * nw + cc) = v4;
                }
            });
            if constexpr (POOL) {
                // row maxima of the odd rows -> the slot this wave read its partner's sums from (nobody else touches it)
                if (j == 1 && e_xh == 1) {
                    // (with a code requested the outputs are ReLU outputs, >= 0: the column bit rides in the sign)
                    float* ps = X + ((0 * 2 + nw) * 2 + mw) * 1024 + lane;
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float v = pmx[t4][e];
                            ps[(t4 * 4 + e) * 64] = (p.pool_code && ((jbits >> (4 * t4 + e)) & 1u)) ? -v : v;
                        }
                }
            }
            wino_barrier();                  // X and the scratch areas are free again (second half / the next item's staging)
        }
        if constexpr (POOL) {
            // (the next item's staging writes X only behind the first barrier of its K step: these reads are ahead of it)
            if (e_xh == 0 && e_single) {
                const float* pr = X + ((0 * 2 + nw) * 2 + mw) * 1024 + lane;
                const int PH = p.OH >> 1, PW = p.OW >> 1;
                const auto prsrc = __builtin_amdgcn_make_buffer_rsrc(p.pool_dst, 0, (int)((size_t)p.B * PH * PW * p.N * 4), 0x00020000);
                const uint32_t p_voff = (ci.ox0 >> 1) + (lane >> 3) < PW ? ((uint32_t)(lane >> 3) * p.N + 4 * (lane & 7)) * 4u : 0x80000000u;
                const auto crsrc = __builtin_amdgcn_make_buffer_rsrc(p.pool_code ? p.pool_code : reinterpret_cast<unsigned char*>(p.pool_dst), 0,
                                                                     (int)((size_t)p.B * PH * PW * p.N), 0x00020000);
                const uint32_t c_voff = (ci.ox0 >> 1) + (lane >> 3) < PW ? (uint32_t)(lane >> 3) * p.N + 4 * (lane & 7) : 0x80000000u;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int prow = (ci.oy0 >> 1) + 4 * e_mw + t4;
                    if (prow >= PH) continue;                                    // wave-uniform
                    f32x4 m;
                    uint32_t code = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float raw = pr[(t4 * 4 + e) * 64];
                        const float r0 = pmx[t4][e], r1 = p.pool_code ? fabsf(raw) : raw;
                        const bool row1 = r1 > r0;                                 // first maximum wins: row 0 on a tie
                        m[e] = row1 ? r1 : r0;
                        const uint32_t j0 = (jbits >> (4 * t4 + e)) & 1u, j1 = __float_as_uint(raw) >> 31;
                        code |= ((row1 ? 2u + j1 : j0) | (m[e] > 0.f ? 4u : 0u)) << (8 * e);
                    }
                    const int pix = (ci.b * PH + prow) * PW + (ci.ox0 >> 1);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), prsrc, p_voff + (uint32_t)((pix * p.N + e_nb0) * 4), 0, 0);
                    if (p.pool_code) __builtin_amdgcn_raw_buffer_store_b32(code, crsrc, c_voff + (uint32_t)(pix * p.N + e_nb0), 0, 0);
                    if constexpr (SPARSE == 1) {
                        if (ci.mirror) {
                            const int mpix = pix - q.sp_nb * PH * PW;
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), prsrc, p_voff + (uint32_t)((mpix * p.N + e_nb0) * 4), 0, 0);
                            if (p.pool_code) __builtin_amdgcn_raw_buffer_store_b32(code, crsrc, c_voff + (uint32_t)(mpix * p.N + e_nb0), 0, 0);
                        }
                    }
                }
            }
        }
        wk.publish(wq_pulled, wq_slot);
        const int wq_nxt2 = wk.next(wq_slot);
        if (wq_nxt2 < 0) break;
        ci = ni;
        if constexpr (STEAL) wino_barrier();       // one more barrier per item: the published word becomes visible, the old one is dead
        wk.advance(wq_nxt2);
    }
    wk.done(q.qctr);
}

// ---- host side: planning and the steps every Winograd launcher shares ------------------------------

// F(2x2,3x3) geometry, fp32 (wino_kernel: K steps of 8 channels) or bf16 operands (wino16_kernel: 16).  The TgConv-level
// questions (wino_fwd_geom_ok / wino_dgrad_geom_ok) ask it of the params their launches are built from.
static int wino_kc(const IGemmParams& p) { return p.bf16 ? 16 : 8; }
static bool wino_geom_ok(const IGemmParams& p) {
    static const bool off = getenv("TG_NO_WINO") != nullptr, off16 = getenv("TG_NO_WINO16") != nullptr;
    if (off || (p.bf16 && off16)) return false;
    if (p.TH != 3 || p.TW != 3 || p.ss != 1 || (p.tstep != 1 && p.tstep != -1) || (p.kstep != 1 && p.kstep != -1)) return false;
    return (p.C % wino_kc(p)) == 0 && (p.N % WINO_BN) == 0 && p.OH >= 16 && p.OW >= 16;
}
static size_t wino_u_floats(int N, int C) { return (size_t)16 * N * C; }

// source offset -> weight tap of the 3x3 transform (the tap walk of p: forward, or flipped for a dgrad)
static WinoWeights wino_weights_map(const IGemmParams& p, int sy_min, int sx_min) {
    WinoWeights ww = {};
    ww.sn = p.w_sn; ww.sk = p.w_sk; ww.stap = p.w_stap;
    ww.k_fast = p.w_sk == 1;
    for (int t = 0; t < 3; ++t) {
        ww.kyu[p.sy0 + t * p.tstep - sy_min] = p.ky0 + t * p.kstep;
        ww.kxv[p.sx0 + t * p.tstep - sx_min] = p.kx0 + t * p.kstep;
    }
    return ww;
}

// Everything an F(2x2,3x3) launch decides, from its params and its split-K room alone: no allocation, no launch, no stream.
// launch_wino runs it; tg_conv_pool_code_supported asks it whether the pool would be fused.
struct WinoPlan {
    WinoGeom q;             // tile grid, work count, K chunking (qctr and the tile-map fields are the launch's)
    WinoWeights ww;
    int splits;
    bool fast, pipe, gated, pool, gbits;
    bool sparse;            // the prediction-half tile map can be honoured, by a launch without a work-stealing queue
    bool sparse_list;       // ... or the list-only form of a batch of nb images (the trunk's dgrads), likewise
    // index into launch_wino's kernel tables: 0-7 the static walk, 8-15 the same with a work-stealing queue, 16-17 the tile map,
    // 18-20 its list-only form (plain, fp32 gate, bit gate)
    int kernel(bool queued) const {
        if (sparse_list && !queued) return gbits ? 20 : gated ? 19 : 18;
        if (sparse && !queued) return pool ? 17 : 16;
        return (queued ? 8 : 0) + (gbits ? 7 : pool ? 6 : pipe ? 4 + gated : (fast ? 2 : 0) + gated);
    }
};
static WinoPlan wino_plan(const IGemmParams& p, size_t ws_floats_avail) {
    WinoPlan pl = {};
    WinoGeom& q = pl.q;
    q.tiles_x = cdiv(p.OW, 16);
    q.tiles_y = cdiv(p.OH, 16);
    q.nt = p.N / WINO_BN;
    q.total_work = q.tiles_x * q.tiles_y * p.B * q.nt;
    const size_t u_bytes = wino_u_floats(p.N, p.C) * (p.bf16 ? sizeof(__bf16) : sizeof(float));
    q.interleave = wino_interleave_ok(u_bytes);
    const int sy_b = p.sy0 + 2 * p.tstep, sx_b = p.sx0 + 2 * p.tstep;
    q.sy_min = p.sy0 < sy_b ? p.sy0 : sy_b;
    q.sx_min = p.sx0 < sx_b ? p.sx0 : sx_b;
    pl.ww = wino_weights_map(p, q.sy_min, q.sx_min);
    const int nchunks = p.C / wino_kc(p);
    int splits = 1;
    if (nchunks >= 16) {
        int smax = nchunks / 8 < 16 ? nchunks / 8 : 16;
        while (smax > 1 && (size_t)smax * p.M * p.N > ws_floats_avail) --smax;
        splits = choose_splits(q.total_work, smax, WINO_PLAN_CUS);
    }
    q.chunks_per_split = cdiv(nchunks, splits);
    pl.splits = cdiv(nchunks, q.chunks_per_split);
    const bool one = pl.splits == 1;
    static const bool no_fast = getenv("TG_WINO_NO_FAST") != nullptr;
    pl.fast = !no_fast && p.amask == nullptr && (size_t)p.B * p.IH * p.IW * p.C * 4 < ((size_t)1 << 31) && u_bytes < ((size_t)1 << 31);
    pl.gated = p.gate != nullptr && one;
    // the cross-item pipeline needs two K steps in every split
    static const bool no_pipe = getenv("TG_WINO_NO_PIPE") != nullptr;
    // ... and its epilogue addresses dst / gate through buffer descriptors (32-bit byte offsets)
    pl.pipe = pl.fast && !no_pipe && nchunks - (pl.splits - 1) * q.chunks_per_split >= 2 && q.chunks_per_split >= 2 &&
              (size_t)p.B * p.DH * p.DW * p.N * 4 < ((size_t)1 << 31);
    // the fused 2x2 max-pool: whole pooling windows inside the output, one split, the plain dst grid
    const bool plain_dst = p.ds == 1 && p.dy0 == 0 && p.dx0 == 0 && p.DH == p.OH && p.DW == p.OW && !p.accumulate;
    static const bool no_pool = getenv("TG_NO_FUSED_POOL") != nullptr;
    pl.pool = p.pool_dst && !no_pool && pl.pipe && !pl.gated && one && !(p.OH & 1) && !(p.OW & 1) && plain_dst;
    // bit gates (p.gate_bits): read by the pipelined kernel in one split; any other launch runs ungated and the caller applies them
    pl.gbits = p.gate_bits != nullptr && pl.pipe && one;
    // the prediction-half tile map (tg_conv_fwd_sparse; fp32 only) is honoured by the pipelined kernel's static walk in one split,
    // ungated, on the plain dst grid of a [pred; target] batch whose tile grid is the map's; everything else runs dense -- the same bits
    const TgSparseMap* sm = p.sparse;
    pl.sparse = !p.bf16 && sm && pl.pipe && !pl.gated && !pl.gbits && one && !p.rowscale && plain_dst && (pl.pool || !p.pool_dst) &&
                sm->nb > 0 && p.B == 2 * sm->nb && sm->tiles_y == q.tiles_y && sm->tiles_x == q.tiles_x && sm->bits && sm->list && sm->count;
    // the list-only form (tg_conv_dgrad_sparse): a batch of exactly the map's nb images, gated or not, no pool; tiles outside the
    // list stay unwritten.  Splits > 1, a queue walk, row scales, accumulation and bf16 run dense: the same bits on listed tiles
    pl.sparse_list = !p.bf16 && sm && pl.pipe && one && !p.rowscale && plain_dst && !p.pool_dst && (p.gate == nullptr || pl.gated) &&
                     (p.gate_bits == nullptr || pl.gbits) && sm->nb > 0 && p.B == sm->nb && sm->tiles_y == q.tiles_y &&
                     sm->tiles_x == q.tiles_x && sm->list && sm->count;
    return pl;
}

// The weight-preparation step every Winograd launcher starts with.  wino_ready < 0 (tg_conv_wprep): transform into wino_u and
// stop -- or, while tg_conv_wprep_item captures, only describe the transform (`it`; kind 0: not batchable).  wino_ready == 0:
// transform per call.  Returns true when the call ends here, with *rc its result.
template <class Transform>
static bool wino_prep(const IGemmParams& p, const TgWprepItem& it, Transform transform, int* rc) {
    *rc = TG_OK;
    if (p.wino_ready < 0 && g_wprep_capture) {
        if (it.kind) *g_wprep_capture = it;
        g_wprep_captured = it.kind ? 1 : -1;
        return true;
    }
    if (p.wino_ready <= 0 && (*rc = transform()) != TG_OK) return true;
    return p.wino_ready < 0;
}

// The launch every Winograd launcher ends with: LDS opt-in, the profile record (ALGORITHMIC flops of the direct form), the
// persistent grid -- one workgroup per CU (or per work item, if fewer), each walking a contiguous range of items or pulling from
// the launch's work-stealing queues, p.splits deep -- and the split-K epilogue of a single-class launch (`reduce`).
struct WinoProf {
    int kind, cfg, M;
    double flops, bytes;
    int route;              // WinoRoute (igemm_params.h): WR_FIRST + the index of `kern` in the launcher's table
};
template <class Geom, class UT>
static int wino_launch(void (*kern)(const IGemmParams, const Geom, const UT*), LdsOptIn& opt, size_t lds, const char* name,
                       const IGemmParams& p, const Geom& q, const WinoProf& pf, bool reduce, hipStream_t s) {
    if (int rc = lds_opt_in(opt, reinterpret_cast<const void*>(kern), lds, name)) return rc;
    {
        ProfScope ps(s, pf.kind, pf.flops, pf.bytes, pf.M, p.N, p.Ktot, p.C, p.splits, pf.cfg);
        ps.r.route = pf.route;
        const int grid = q.total_work < wino_cus() ? q.total_work : wino_cus();
        hipLaunchKernelGGL(kern, dim3(grid, 1, p.splits), dim3(WINO_THREADS), lds, s, p, q, reinterpret_cast<const UT*>(p.wino_u));
    }
    TG_CHECK_LAUNCH(name);
    if (reduce && p.splits > 1) {
        hipLaunchKernelGGL(igemm_splitk_epilogue, dim3(ew_grid((int64_t)p.M * p.N, 256)), dim3(256), 0, s, p);
        TG_CHECK_LAUNCH("igemm_splitk_epilogue");
    }
    return TG_OK;
}

// =================================================================================================
// Winograd wgrad  F(3x3, 2x2):  dW = Gt [ sum_tiles (A dY At) (.) (Bt X B) ] G
// =================================================================================================
// Same 16 independent products, now contracted over the TILES: per transform point xi
//     dU[xi][co][ci] = sum_tiles Yt[xi][tile][co] * V[xi][tile][ci]
// i.e. M = Cout, N = Cin, K = tiles.  A 512-thread workgroup owns 64 co x 64 ci x 16 points (8 accumulator tiles per
// wave, exactly the MFMA schedule of wino_kernel) and walks a range of tile strips (8 tiles in a row = one K step of 8):
// BOTH operands are transformed on the fly -- thread (tile k, channel quad, row a) loads its 2x4 input pixels /
// 2x2 output-gradient pixels straight from global memory one step ahead (buffer loads: out-of-range pixels read 0),
// forms row a of Bt X B / A dY At and writes it K-contiguous into the LDS images [xi][channel][8 tiles].  Channel c of
// the 64-channel tile sits in image row (c>>2) + 16*(c&3): a thread's four channels then land in four different
// 16-row groups and the transposing ds_write_b32 are bank-conflict free.  Split-K over strips; the slabs hold dU
// (raw accumulator layout), wino_wgrad_reduce_kernel sums them in fixed order and applies Gt . G -> dW[co][3][3][ci].
struct WinoWgradGeom {
    int strips_x, tiles_y, nstrips, steps_per_split, splits, ntco, ntci;
};

constexpr int WG_PITCH = 72;                      // floats per raw pixel (64 channels + 8): conflict-free b128 transform reads
constexpr int WG_XR = 4 * 18 * WG_PITCH;          // raw input strip: 4 rows x 18 pixels
constexpr int WG_DR = 2 * 16 * WG_PITCH;          // raw output-gradient strip: 2 rows x 16 pixels
constexpr int WINO_WG_LDS_FLOATS = 4 * WINO_V + WG_XR + WG_DR;

__global__ __launch_bounds__(WINO_THREADS) void wino_wgrad_kernel(const WgradParams p, const WinoWgradGeom q, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                    // [2][16][64][8]   Yt, rows = co (permuted)
    float* Bs = smem + 2 * WINO_V;       // [2][16][64][8]   V,  rows = ci (permuted)
    float* Xr = smem + 4 * WINO_V;       // raw strip of x:  [4][18][WG_PITCH]
    float* Dr = Xr + WG_XR;              // raw strip of dy: [2][16][WG_PITCH]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    const int work = xcd_remap(blockIdx.x, q.ntco * q.ntci * q.splits);
    const int tco = work % q.ntco, tci = (work / q.ntco) % q.ntci, split = work / (q.ntco * q.ntci);
    const int s_begin = split * q.steps_per_split;
    const int s_end = min(q.nstrips, s_begin + q.steps_per_split);

    // transform role: tile k of the strip, channel quad qd, row a of the 4x4 transform (wave-uniform)
    const int k = lane & 7, qd = (lane >> 3) + 8 * (wave & 1), a = wave >> 1;
    const int r0 = a == 0 ? 0 : (a == 2 ? 2 : 1), r1 = a == 3 ? 3 : (a == 2 ? 1 : 2);
    const float xs1 = a == 1 ? 1.f : -1.f;                                              // Bt row a = d[r0] + xs1*d[r1] (one fma)
    const float dc0 = a == 3 ? 0.f : 1.f, dc1 = a == 0 ? 0.f : (a == 1 ? 1.f : -1.f);  // A row a  = dc0*D0 + dc1*D1
    int icol[4];          // image column of channel e of this thread's quad: row (qd + 16 e), k-slot swizzled
#pragma unroll
    for (int e = 0; e < 4; ++e) icol[e] = (4 * a) * 512 + (qd + 16 * e) * 8 + ((((k >> 2) ^ e) & 1) << 2) + (k & 3);
    const int xrd0 = (r0 * 18 + 2 * k) * WG_PITCH + 4 * qd, xrd1 = (r1 * 18 + 2 * k) * WG_PITCH + 4 * qd;   // + j * WG_PITCH
    const int drd = (2 * k) * WG_PITCH + 4 * qd;                                                                // + (i*16 + j) * WG_PITCH

    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((size_t)p.B * p.H * p.W * p.C * 4), 0x00020000);
    const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)((size_t)p.B * p.Ho * p.Wo * p.Cout * 4), 0x00020000);
    const uint32_t OOB = 0xFFFFFFF0u;

    // Raw staging slots of this thread: the strip's pixels are fetched ONCE, coalesced (a thread per 16 bytes), into LDS --
    // the transform roles above then read their 2x4 / 2x2 pixels from there.  (Fetching them per role straight from global
    // memory asked the texture path for 12 x 16 B per thread and step, 3.7x redundantly: TA address / command FIFOs full
    // 14 % of the time, MFMA pipe 59 % busy.)  Out-of-range pixels read 0 through the buffer descriptor.
    int xs_r[3], xs_px[3], xs_lds[3];
    bool xs_on[3];
    uint32_t xs_ch;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int idx = tid + WINO_THREADS * i;            // (pixel slot, channel quad)
        const int ps = idx >> 4;
        xs_on[i] = ps < 4 * 18;
        xs_r[i] = ps / 18;
        xs_px[i] = ps - xs_r[i] * 18;
        xs_lds[i] = ps * WG_PITCH + 4 * (idx & 15);
    }
    xs_ch = (uint32_t)(tci * 64 + 4 * (tid & 15)) * 4u;
    const int ds_i = tid >> 8, ds_px = (tid >> 4) & 15, ds_lds = (tid >> 4) * WG_PITCH + 4 * (tid & 15);
    const uint32_t ds_ch = (uint32_t)(tco * 64 + 4 * (tid & 15)) * 4u;

    f32x4 rx[3], rd;
    // load cursor: strip ls = (lb, lty, lsx)
    int ls = s_begin, lsx = s_begin % q.strips_x, lty = (s_begin / q.strips_x) % q.tiles_y, lb = s_begin / (q.strips_x * q.tiles_y);
    auto raw_load = [&]() {      // raw pixels of strip ls -> rx / rd (everything out of range, or past this split's range, reads 0)
        const bool live = ls < s_end;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int py = 2 * lty - p.pad + xs_r[i], px = 16 * lsx - p.pad + xs_px[i];
            const bool ok = live && xs_on[i] && py >= 0 && py < p.H && px >= 0 && px < p.W;
            const uint32_t off = ok ? (((uint32_t)(lb * p.H + py) * p.W + px) * (uint32_t)p.C) * 4u + xs_ch : OOB;
            rx[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0));
        }
        {
            const int oy = 2 * lty + ds_i, ox = 16 * lsx + ds_px;
            const bool ok = live && oy < p.Ho && ox < p.Wo;
            const uint32_t off = ok ? (((uint32_t)(lb * p.Ho + oy) * p.Wo + ox) * (uint32_t)p.Cout) * 4u + ds_ch : OOB;
            rd = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, off, 0, 0));
        }
        ++ls;
        if (++lsx == q.strips_x) { lsx = 0; if (++lty == q.tiles_y) { lty = 0; ++lb; } }
    };
    auto raw_store = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (xs_on[i]) *reinterpret_cast<f32x4*>(Xr + xs_lds[i]) = rx[i];
        *reinterpret_cast<f32x4*>(Dr + ds_lds) = rd;
    };
    f32x4 xr[2][4], dr[2][2], tt[4], rr[2];
    auto x_read = [&](int j) {      // column j of both rows
        xr[0][j] = *reinterpret_cast<const f32x4*>(Xr + xrd0 + j * WG_PITCH);
        xr[1][j] = *reinterpret_cast<const f32x4*>(Xr + xrd1 + j * WG_PITCH);
    };
    auto d_read = [&](int i) {      // row i, both columns
        dr[i][0] = *reinterpret_cast<const f32x4*>(Dr + drd + (i * 16) * WG_PITCH);
        dr[i][1] = *reinterpret_cast<const f32x4*>(Dr + drd + (i * 16 + 1) * WG_PITCH);
    };
    auto x_rows = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) tt[j] = xr[0][j] + xr[1][j] * xs1;
    };
    auto d_rows = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j) rr[j] = dr[0][j] * dc0 + dr[1][j] * dc1;
    };
    // output b (0..3) of the column transform; half h writes channels 2h, 2h+1
    auto x_out = [&](int buf, int b, int h) {
        const f32x4 v = b == 0 ? tt[0] - tt[2] : b == 1 ? tt[1] + tt[2] : b == 2 ? tt[2] - tt[1] : tt[1] - tt[3];
        float* dst = Bs + buf * WINO_V + b * 512;
        dst[icol[2 * h]] = v[2 * h];
        dst[icol[2 * h + 1]] = v[2 * h + 1];
    };
    auto d_out = [&](int buf, int b, int h) {
        const f32x4 v = b == 0 ? rr[0] : b == 1 ? rr[0] + rr[1] : b == 2 ? rr[0] - rr[1] : -rr[1];
        float* dst = As + buf * WINO_V + b * 512;
        dst[icol[2 * h]] = v[2 * h];
        dst[icol[2 * h + 1]] = v[2 * h + 1];
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * 512 + arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = (8 * xh) * 512 + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    if (s_begin < s_end) {
        raw_load();                 // strip s_begin
        raw_store();
        raw_load();                 // strip s_begin + 1: in flight while the first images are built
        wino_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j) x_read(j);
        d_read(0);
        d_read(1);
        x_rows();
        d_rows();
#pragma unroll
        for (int b = 0; b < 4; ++b) { x_out(0, b, 0); x_out(0, b, 1); d_out(0, b, 0); d_out(0, b, 1); }
        wino_barrier();
        f32x4 fa[2], fb[2];        // one transform point at a time, double-buffered (see wino_kernel)
        fa[0] = *reinterpret_cast<const f32x4*>(As + a_off);
        fb[0] = *reinterpret_cast<const f32x4*>(Bs + b_off);
        int cur = 0;
        for (int s = s_begin; s < s_end; ++s) {
            const int nxt = cur ^ 1;
            const float* Ac = As + cur * WINO_V + a_off;
            const float* Bc = Bs + cur * WINO_V + b_off;
            const float* An = As + nxt * WINO_V + a_off;
            const float* Bn = Bs + nxt * WINO_V + b_off;
            // rx / rd hold the raw strip s+1 (requested during step s-1): it goes to LDS, is transformed into the images of
            // buffer nxt while the MFMAs consume strip s from buffer cur, and the raw registers take strip s+2
            wino_static_for(std::make_integer_sequence<int, 32>{}, [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int xi = t >> 2, e = t & 3;
                if constexpr (t == 0) raw_store();
                if constexpr (t == 1) raw_load();
                if constexpr (t == 3) wino_barrier();                      // raw strip visible
                if constexpr (t >= 4 && t < 8) x_read(t - 4);
                if constexpr (t == 8) { d_read(0); d_read(1); }
                if constexpr (t == 9) x_rows();
                if constexpr (t >= 10 && t < 18) x_out(nxt, (t - 10) >> 1, t & 1);
                if constexpr (t == 17) d_rows();
                if constexpr (t >= 18 && t < 26) d_out(nxt, (t - 18) >> 1, t & 1);
                if constexpr (t == 27) wino_barrier();                     // images of strip s+1 complete
                if constexpr (e == 0 && xi < 7) {
                    fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Ac + (xi + 1) * 512);
                    fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Bc + (xi + 1) * 512);
                }
                if constexpr (e == 0 && xi == 7) {           // t = 28, behind the barrier: first point of the next strip
                    fa[0] = *reinterpret_cast<const f32x4*>(An);
                    fb[0] = *reinterpret_cast<const f32x4*>(Bn);
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
            cur = nxt;
        }
    }
    // dU slab of this (split, ci tile, co tile): [xi][row 64][col 64], raw accumulator layout (permuted channels)
    float* slab = slabs + ((size_t)work * 16 + 8 * xh) * 4096;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * mw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            slab[(size_t)i * 4096 + row * 64 + 32 * nw + (lane & 31)] = acc[i][r];
        }
}

// dW[co][u][v][ci] = sum_{a,b} G[a][u] (sum_splits dU[a][b][co][ci]) G[b][v]
__global__ __launch_bounds__(256) void wino_wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int Cout,
                                                                int Cin, int ntco, int ntci, int splits) {
    const int total = Cout * Cin;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int col = idx & 63, row = (idx >> 6) & 63, tile = idx >> 12;       // tile = tci * ntco + tco
        const int tco = tile % ntco, tci = tile / ntco;
        float u[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] = 0.f;
        const size_t sstride = (size_t)ntci * ntco * 16 * 4096;
        const float* sl = slabs + ((size_t)tile * 16) * 4096 + row * 64 + col;
        int sp = 0;
        for (; sp + 4 <= splits; sp += 4) {          // 64 independent loads per trip, summed in slab order
            float v[4][16];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < 16; ++i) v[k][i] = sl[(size_t)(sp + k) * sstride + (size_t)i * 4096];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < 16; ++i) u[i] += v[k][i];
        }
        for (; sp < splits; ++sp)
#pragma unroll
            for (int i = 0; i < 16; ++i) u[i] += sl[(size_t)sp * sstride + (size_t)i * 4096];
        float t[3][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            t[0][b] = u[0 * 4 + b] + 0.5f * (u[1 * 4 + b] + u[2 * 4 + b]);
            t[1][b] = 0.5f * (u[1 * 4 + b] - u[2 * 4 + b]);
            t[2][b] = 0.5f * (u[1 * 4 + b] + u[2 * 4 + b]) + u[3 * 4 + b];
        }
        const int co = tco * 64 + 4 * (row & 15) + (row >> 4), ci = tci * 64 + 4 * (col & 15) + (col >> 4);
        float* o = dw + ((size_t)co * 9) * Cin + ci;
#pragma unroll
        for (int uu = 0; uu < 3; ++uu) {
            o[(size_t)(uu * 3 + 0) * Cin] = t[uu][0] + 0.5f * (t[uu][1] + t[uu][2]);
            o[(size_t)(uu * 3 + 1) * Cin] = 0.5f * (t[uu][1] - t[uu][2]);
            o[(size_t)(uu * 3 + 2) * Cin] = 0.5f * (t[uu][1] + t[uu][2]) + t[uu][3];
        }
    }
}

static bool wino_wgrad_ok(const TgConv* g, const float* in_mask) {
    static const bool off = getenv("TG_NO_WINO") != nullptr || getenv("TG_NO_WINO_WGRAD") != nullptr;
    if (off || in_mask != nullptr) return false;
    // bf16 mode: the direct bf16 wgrad kernel wins on the deep layers (220-250 TF); up to 256 input channels this fp32
    // Winograd kernel is the faster one (dec1 233 against 168 TF) -- and the more accurate: its operands are not rounded
    if (g->precision == TG_PREC_BF16 && g->Cin > 256) return false;
    if (g->k != 3 || g->stride != 1 || (g->Cin % 64) != 0 || (g->Cout % 64) != 0 || g->Ho < 16 || g->Wo < 16) return false;
    if ((size_t)g->B * g->H * g->W * g->Cin * 4 >= ((size_t)1 << 31) || (size_t)g->B * g->Ho * g->Wo * g->Cout * 4 >= ((size_t)1 << 31))
        return false;         // 32-bit buffer offsets
    return true;
}
static WinoWgradGeom wino_wgrad_plan(const TgConv* g) {
    WinoWgradGeom q = {};
    q.strips_x = cdiv(g->Wo, 16);
    q.tiles_y = cdiv(g->Ho, 2);
    q.nstrips = g->B * q.tiles_y * q.strips_x;
    q.ntco = g->Cout / 64;
    q.ntci = g->Cin / 64;
    const int tiles = q.ntco * q.ntci;
    // at least 8 strips per split (small batches: 32 left three quarters of the chip idle -- 48-64 workgroups of 32 strips)
    int smax = q.nstrips / 8 < 512 ? q.nstrips / 8 : 512;
    if (smax < 1) smax = 1;
    const int splits = choose_splits_k(tiles, smax, WINO_PLAN_CUS, q.nstrips, 0.03);
    q.steps_per_split = cdiv(q.nstrips, splits);
    q.splits = cdiv(q.nstrips, q.steps_per_split);
    return q;
}
static size_t wino_wgrad_ws_floats(const TgConv* g) {
    if (!wino_wgrad_ok(g, nullptr)) return 0;
    const WinoWgradGeom q = wino_wgrad_plan(g);
    return (size_t)q.splits * q.ntco * q.ntci * 16 * 4096;
}
static int launch_wino_wgrad(const TgConv* g, const WgradParams& p, float* dw, float* ws, hipStream_t s) {
    const WinoWgradGeom q = wino_wgrad_plan(g);
    const size_t lds = (size_t)WINO_WG_LDS_FLOATS * sizeof(float);
    static LdsOptIn opt;
    if (int rc = lds_opt_in(opt, reinterpret_cast<const void*>(wino_wgrad_kernel), lds, "wino wgrad")) return rc;
    {
        const double by = 4.0 * ((double)p.B * p.H * p.W * p.C + (double)p.Mpix * p.Cout + (double)p.Cout * p.Ktot);
        ProfScope ps(s, 1, 2.0 * p.Mpix * (double)p.Cout * p.Ktot * g_alg_scale, by, p.Cout, p.Ktot, p.Mpix, p.C, q.splits, 4164);
        ps.r.route = WR_WGRAD;
        hipLaunchKernelGGL(wino_wgrad_kernel, dim3(q.ntco * q.ntci * q.splits), dim3(WINO_THREADS), lds, s, p, q, ws);
    }
    TG_CHECK_LAUNCH("wino_wgrad_kernel");
    hipLaunchKernelGGL(wino_wgrad_reduce_kernel, dim3(ew_grid((int64_t)g->Cout * g->Cin, 256)), dim3(256), 0, s, ws, dw, g->Cout,
                       g->Cin, q.ntco, q.ntci, q.splits);
    TG_CHECK_LAUNCH("wino_wgrad_reduce_kernel");
    return TG_OK;
}
