// Second-difference spectrum of a fill against the truth (mvp_gan/src/evaluate_raster.py texture_errors, mvp_gan/src/texture.py,
// DESIGN.md section 8ad).
//
//   tg_texture_compare   texture_kernel: one pass over 32 x 64 tiles of z and p staged in LDS with a 16-px halo and one flag byte
//                        per staged pixel.  A triple is a centre x with sel and known, a unit step u and a lag h = 2^j whose two
//                        arms x -+ h u are known; per scale s = 2 j + cls (cls 0: u = (0,1), (1,0); cls 1: u = (1,1), (1,-1)) the
//                        number of triples and the fp64 sums of d_z^2, d_p^2 and d_z d_p, d = (s(x - hu) + s(x + hu)) - 2 s(x).
//                        texture_finish_kernel: one workgroup reduces the per-workgroup rows in index order.
//
// Determinism: no floating-point atomics.  The grid is a function of the shape, a workgroup walks its tiles and a thread its pixels,
// octaves and directions in a fixed order, the wave and workgroup reductions are fixed trees, every workgroup writes one row of
// partials (zeros included) and the finish kernel adds the rows in index order.  The counts use integer atomics.  A tile without a
// sel pixel adds exact zeros, so leaving it early changes no bit of the result.
#include "raster_sweep.h"

// ---- geometry -----------------------------------------------------------------------------------------------------------
constexpr int TX_TY = 32, TX_TX = 64;          // output tile: 4 waves x 8 rows, lane = column (TE_TY x TE_TX of terrain_eval.hip)
constexpr int TX_HALO = 1 << (TG_TEX_OCTAVES - 1);
constexpr int TX_RY = TX_TY + 2 * TX_HALO;     // 64 staged rows
constexpr int TX_RX = TX_TX + 2 * TX_HALO;     // 96 staged columns
// LDS row stride in elements.  A wave reads one staged row at a time, lane l the column l + const, for the centre and for every
// arm (row walk, column walk and both diagonals shift the whole wave alike), so a half-wave always reads 32 consecutive words: 32
// different banks at any stride.  No padding is needed for the reads, and with none the staged image is contiguous, so the staging
// loop writes consecutive words too.
constexpr int TX_SX = TX_RX;
constexpr int TX_MAX_GRID = 2048;
constexpr int TX_ROW = TG_TEX_SCALES * TG_TEX_NSUM;   // doubles per row of partials
constexpr int TX_FIN_CHUNKS = 8;                       // the finish kernel: 8 chunks x 32 columns = 256 threads
static_assert(TX_HALO == 16 && TX_ROW <= 32, "texture geometry");
static_assert(sizeof(float) * 2 * TX_RY * TX_SX + TX_RY * TX_SX <= 56 * 1024, "two workgroups per CU");

// sides go up to 2^31 - 1: tile counts and pixel coordinates past a tile's origin are 64-bit
static int tx_tiles_x(int W) { return (int)cdiv64(W, TX_TX); }
static int tx_tiles(int H, int W) { return (int)(cdiv64(H, TX_TY) * tx_tiles_x(W)); }      // < 2^31 / 2048 + 2^27

static int tx_grid(int H, int W) {
    const int64_t tiles = tx_tiles(H, W);
    return (int)(tiles < TX_MAX_GRID ? tiles : TX_MAX_GRID);
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------
// one triple: both arms known -> the second differences of z and p in fp64 from the fp32 values, nothing fused
#define TX_TRIPLE(DY, DX, N, SZZ, SPP, SZP)                                                      \
    do {                                                                                        \
        const int ay = ly - (DY), ax = lx - (DX), by = ly + (DY), bx = lx + (DX);               \
        if (sk[ay][ax] & sk[by][bx]) {                                                          \
            const double dz = ((double)sz[ay][ax] + (double)sz[by][bx]) - 2.0 * zc;             \
            const double dp = ((double)sp[ay][ax] + (double)sp[by][bx]) - 2.0 * pc;             \
            ++(N);                                                                              \
            (SZZ) = (SZZ) + dz * dz;                                                            \
            (SPP) = (SPP) + dp * dp;                                                            \
            (SZP) = (SZP) + dz * dp;                                                            \
        }                                                                                       \
    } while (0)

__global__ __launch_bounds__(256) void texture_kernel(const float* __restrict__ z, const float* __restrict__ p,
                                                      const uint8_t* __restrict__ sel, const uint8_t* __restrict__ known, int H,
                                                      int W, int octaves, int tiles_x, int ntiles, ull* __restrict__ counts,
                                                      double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float sz[TX_RY][TX_SX], sp[TX_RY][TX_SX];
    __shared__ uint8_t sk[TX_RY][TX_SX];               // 1: inside the raster and known
    __shared__ double dred[4][TX_ROW];
    __shared__ int ired[4][TG_TEX_SCALES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double acc[TG_TEX_SCALES][TG_TEX_NSUM];
    int cnt[TG_TEX_SCALES];
#pragma unroll
    for (int s = 0; s < TG_TEX_SCALES; ++s) {
        cnt[s] = 0;
#pragma unroll
        for (int q = 0; q < TG_TEX_NSUM; ++q) acc[s][q] = 0.0;
    }

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = ty * TX_TY, x0 = tx * TX_TX;
        // the thread's eight sel bytes, bit k = row w * 8 + k of column lane
        const int64_t x = (int64_t)x0 + lane;
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t y = (int64_t)y0 + w * 8 + k;
            if (y < H && x < W) mine |= (sel[y * W + x] != 0 ? 1u : 0u) << k;
        }
        // uniform over the workgroup, and the barrier after which the previous tile's readers are done
        if (!__syncthreads_or((int)mine)) continue;
        for (int j = threadIdx.x; j < TX_RY * TX_RX; j += 256) {
            const int r = j / TX_RX, c = j - r * TX_RX;
            const int64_t y = (int64_t)y0 - TX_HALO + r, xx = (int64_t)x0 - TX_HALO + c;
            float zv = 0.f, pv = 0.f;
            uint8_t f = 0;
            if (y >= 0 && y < H && xx >= 0 && xx < W) {
                const int64_t i = y * W + xx;
                zv = z[i];
                pv = p[i];
                f = known[i] != 0;
            }
            sz[r][c] = zv;
            sp[r][c] = pv;
            sk[r][c] = f;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const int ly = TX_HALO + w * 8 + k, lx = TX_HALO + lane;
            if (!((mine >> k) & 1u) || !sk[ly][lx]) continue;
            const double zc = sz[ly][lx], pc = sp[ly][lx];
#pragma unroll
            for (int o = 0; o < TG_TEX_OCTAVES; ++o) {
                if (o < octaves) {
                    const int h = 1 << o;
                    TX_TRIPLE(0, h, cnt[2 * o], acc[2 * o][0], acc[2 * o][1], acc[2 * o][2]);
                    TX_TRIPLE(h, 0, cnt[2 * o], acc[2 * o][0], acc[2 * o][1], acc[2 * o][2]);
                    TX_TRIPLE(h, h, cnt[2 * o + 1], acc[2 * o + 1][0], acc[2 * o + 1][1], acc[2 * o + 1][2]);
                    TX_TRIPLE(h, -h, cnt[2 * o + 1], acc[2 * o + 1][0], acc[2 * o + 1][1], acc[2 * o + 1][2]);
                }
            }
        }
    }

    // workgroup reduction in a fixed order: xor butterflies inside the waves, then waves 0..3
#pragma unroll
    for (int s = 0; s < TG_TEX_SCALES; ++s) {
#pragma unroll
        for (int q = 0; q < TG_TEX_NSUM; ++q) {
            const double v = wave_sum_d(acc[s][q]);
            if (lane == 0) dred[w][s * TG_TEX_NSUM + q] = v;
        }
        int v = cnt[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) ired[w][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < TX_ROW) {
        const int s = threadIdx.x;
        partials[(int64_t)blockIdx.x * TX_ROW + s] = ((dred[0][s] + dred[1][s]) + dred[2][s]) + dred[3][s];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + TG_TEX_SCALES) {
        const int s = threadIdx.x - 64;
        const int64_t v = (int64_t)ired[0][s] + ired[1][s] + ired[2][s] + ired[3][s];
        if (v) atomicAdd(&counts[s], (ull)v);
    }
}

// thread (chunk, col) adds rows chunk, chunk + 8, ... of column col in that order; then column col adds its chunks 0..7
__global__ __launch_bounds__(256) void texture_finish_kernel(const double* __restrict__ partials, int nwg,
                                                             double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double red[TX_FIN_CHUNKS][32];
    const int col = threadIdx.x & 31, chunk = threadIdx.x >> 5;
    double v = 0.0;
    if (col < TX_ROW)
        for (int g = chunk; g < nwg; g += TX_FIN_CHUNKS) v = v + partials[(int64_t)g * TX_ROW + col];
    red[chunk][col] = v;
    __syncthreads();
    if (threadIdx.x < TX_ROW) {
        double s = red[0][col];
#pragma unroll
        for (int c = 1; c < TX_FIN_CHUNKS; ++c) s = s + red[c][col];
        sums[col] = s;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" size_t tg_texture_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return (size_t)tx_grid(H, W) * TX_ROW * sizeof(double);
}

extern "C" int tg_texture_compare(const float* z, const float* p, const uint8_t* sel, const uint8_t* known, int H, int W,
                                  int octaves, int64_t* counts, double* sums, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_texture_compare", H, W)) return rc;
    const void* const ptr[] = {z, p, sel, known, counts, sums, ws};
    const char* const name[] = {"z", "p", "sel", "known", "counts", "sums", "ws"};
    for (int i = 0; i < 7; ++i) TG_REQUIRE(ptr[i], "tg_texture_compare: null pointer %s", name[i]);
    TG_REQUIRE(octaves >= 1 && octaves <= TG_TEX_OCTAVES, "tg_texture_compare: octaves %d must lie in [1, %d]", octaves,
               TG_TEX_OCTAVES);
    const size_t need = tg_texture_ws_bytes(H, W);
    TG_REQUIRE(ws_bytes >= need, "tg_texture_compare: workspace ws_bytes %zu < %zu", ws_bytes, need);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_TEX_SCALES * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_texture_compare: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int tiles_x = tx_tiles_x(W), ntiles = tx_tiles(H, W), grid = tx_grid(H, W);
    hipLaunchKernelGGL(texture_kernel, dim3(grid), dim3(256), 0, s, z, p, sel, known, H, W, octaves, tiles_x, ntiles,
                       reinterpret_cast<ull*>(counts), (double*)ws);
    TG_CHECK_LAUNCH("texture_kernel");
    hipLaunchKernelGGL(texture_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grid, sums);
    TG_CHECK_LAUNCH("texture_finish_kernel");
    return TG_OK;
}
