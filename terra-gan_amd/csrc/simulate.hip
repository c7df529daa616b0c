// Conditional simulation of voids: the unconditional random field, the conditioning step and the ensemble statistics
// (mvp_gan/src/simulate.py).
//
//   tg_sim_field    sim_field_kernel: u(x, y) = sum_k a_k cos(2 pi t_k(x, y)) + nugget_amp * g(x, y).  One workgroup per 1024 px of
//                   one row; the wave table goes to LDS once per workgroup with the row's share of the phase folded in, a lane owns
//                   the four pixels x, x + 256, x + 512, x + 768 and reads each wave once for all four (one broadcast 16-byte LDS
//                   read).  No atomics, no scratch.
//   tg_sim_combine  one thread per pixel: d = (double)u - (double)uk; out = known ? z : (float)((double)zk + d), an fp32 value
//                   rounded once; optionally d and d * d are added to two fp64 planes of running sums.
//   tg_sim_stats    one thread per pixel: the ensemble mean and standard deviation from those planes.
//
// Every operation of tg_sim_field has a numpy counterpart (tests/simulate_oracle.py reproduces u to the last bit):
//   phase    p = fx * X + fy * Y + phase in uint32, wrapping: 2^32 = one turn.  X, Y are the global coordinates mod 2^32.
//   cosine   q = p >> 30 (the quadrant); m = (p >> 6) & 0xffffff (24 bits of the quarter turn, truncated); an odd quadrant takes
//            m' = 2^24 - m, an even one m' = m; t = (float)m' * 2^-24 in [0, 1] (exact); s = t * t;
//            c = ((((((C7 s + C6) s + C5) s + C4) s + C3) s + C2) s + C1) s + C0 in fp32, every product and every sum rounded once
//            (no contraction), C_j = (float)((-1)^j (pi/2)^(2j) / (2j)!): cos(pi/2 t) on [0, 1].  Quadrants 1 and 2 take -c.
//   sum      acc = acc + (double)a_k * (double)c for k = 0 .. n_waves - 1, in fp64, starting from 0.
//   hash     mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16 (uint32).
//            key = mix(mix(mix(mix(seed + 0x9e3779b9) ^ realisation) ^ Y) ^ X); word j = mix(key + j * 0x9e3779b9), j = 1 .. 6:
//            three 64-bit hash words as six 32-bit halves, twelve 16-bit lanes.
//   nugget   S = the integer sum of the twelve lanes; g = (double)(S - 393210) * 2^-16 (Irwin-Hall: mean 0, variance
//            1 - 2^-32); acc = acc + (double)nugget_amp * g.  Skipped when nugget_amp == 0.
//   u = (float)acc.
#include <math.h>

#include "raster_sweep.h"

// the mirror does not fuse: no multiply-add contraction in this file
#pragma clang fp contract(off)

constexpr int SIM_T = 256;                     // threads of a workgroup
constexpr int SIM_PX = 4;                      // pixels of a lane, SIM_T apart
constexpr int SIM_SPAN = SIM_T * SIM_PX;       // pixels of a workgroup along its row
static_assert(sizeof(int4) * TG_SIM_MAX_WAVES <= 8 * 1024, "the wave table takes 8 KiB of LDS");

__device__ __forceinline__ uint32_t sim_mix(uint32_t v) {
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

// cos(2 pi p / 2^32) from the integer phase
__device__ __forceinline__ float sim_cos(uint32_t p) {
    const uint32_t q = p >> 30, m = (p >> 6) & 0xffffffu;
    const uint32_t mm = (q & 1u) ? 0x1000000u - m : m;
    const float t = (float)mm * 0x1p-24f;
    const float s = t * t;
    float c = -0x1.b6e250p-28f;
    c = c * s + 0x1.f9d38ap-22f;
    c = c * s + -0x1.a6d1f2p-16f;
    c = c * s + 0x1.e1f506p-11f;
    c = c * s + -0x1.55d3c8p-6f;
    c = c * s + 0x1.03c1f0p-2f;
    c = c * s + -0x1.3bd3ccp+0f;
    c = c * s + 1.0f;
    return ((q + 1u) & 2u) ? -c : c;
}

__global__ __launch_bounds__(SIM_T) void sim_field_kernel(float* __restrict__ u, int H, int W, uint32_t x0, uint32_t y0,
                                                          const int4* __restrict__ waves, int n_waves, float nugget_amp,
                                                          uint32_t seed, uint32_t realisation) {
    __shared__ int4 tab[TG_SIM_MAX_WAVES];     // fx, the phase at X = 0 of this row, unused, the bits of amp
    const int y = blockIdx.y;
    const uint32_t Y = y0 + (uint32_t)y;
    for (int k = threadIdx.x; k < n_waves; k += SIM_T) {
        int4 w = waves[k];
        w.y = (int)((uint32_t)w.y * Y + (uint32_t)w.z);
        tab[k] = w;
    }
    __syncthreads();
    const int xl = blockIdx.x * SIM_SPAN + threadIdx.x;
    if (xl >= W) return;                        // after the only barrier
    const uint32_t X = x0 + (uint32_t)xl;
    double acc[SIM_PX];
#pragma unroll
    for (int i = 0; i < SIM_PX; ++i) acc[i] = 0.0;
#pragma unroll 2
    for (int k = 0; k < n_waves; ++k) {
        const int4 w = tab[k];
        const uint32_t fx = (uint32_t)w.x;
        const double a = (double)__int_as_float(w.w);
        uint32_t p = fx * X + (uint32_t)w.y;
        const uint32_t step = fx * (uint32_t)SIM_T;
#pragma unroll
        for (int i = 0; i < SIM_PX; ++i) {
            acc[i] = acc[i] + a * (double)sim_cos(p);
            p += step;
        }
    }
    if (nugget_amp != 0.f) {
        const uint32_t row = sim_mix(sim_mix(sim_mix(seed + 0x9e3779b9u) ^ realisation) ^ Y);
        const double na = (double)nugget_amp;
#pragma unroll
        for (int i = 0; i < SIM_PX; ++i) {
            const uint32_t key = sim_mix(row ^ (X + (uint32_t)(i * SIM_T)));
            int32_t sum = 0;
#pragma unroll
            for (uint32_t j = 1; j <= 6; ++j) {
                const uint32_t h = sim_mix(key + j * 0x9e3779b9u);
                sum += (int32_t)(h & 0xffffu) + (int32_t)(h >> 16);
            }
            acc[i] = acc[i] + na * ((double)(sum - 393210) * 0x1p-16);
        }
    }
    float* row_u = u + (int64_t)y * W;
#pragma unroll
    for (int i = 0; i < SIM_PX; ++i) {
        const int x = xl + i * SIM_T;
        if (x < W) row_u[x] = (float)acc[i];
    }
}

__global__ __launch_bounds__(256) void sim_combine_kernel(float* __restrict__ out, const float* __restrict__ z,
                                                          const uint8_t* __restrict__ known, const float* __restrict__ zk,
                                                          const float* __restrict__ u, const float* __restrict__ uk,
                                                          double* __restrict__ s1, double* __restrict__ s2, int64_t n) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (known[p]) {
            out[p] = z[p];
            continue;
        }
        const double d = (double)u[p] - (double)uk[p];
        out[p] = (float)((double)zk[p] + d);       // one rounding to fp32: within half an ulp of zk + (u - uk)
        if (s1) {
            s1[p] = s1[p] + d;
            s2[p] = s2[p] + d * d;
        }
    }
}

__global__ __launch_bounds__(256) void sim_stats_kernel(float* __restrict__ mean, float* __restrict__ sd,
                                                        const float* __restrict__ zk, const double* __restrict__ s1,
                                                        const double* __restrict__ s2, int count, int64_t n) {
    const double dn = (double)count, dn1 = (double)(count - 1);
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const float k = zk[p];
        const double a = s1[p], b = s2[p];
        mean[p] = (float)((double)k + a / dn);
        const double v = (b - (a * a) / dn) / dn1;
        sd[p] = k != k ? k : (float)sqrt(v > 0.0 ? v : 0.0);       // an unfilled pixel stays NaN; a known one has a = b = 0
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
extern "C" int tg_sim_field(float* u, int H, int W, int64_t x0, int64_t y0, const void* waves, int n_waves, float nugget_amp,
                            uint32_t seed, uint32_t realisation, tg_stream_t stream) {
    TG_REQUIRE(H >= 1 && W >= 1 && H <= TG_EDT_MAX_SIDE && W <= TG_EDT_MAX_SIDE,
               "tg_sim_field: raster %dx%d: both sides must lie in [1, %d]", H, W, (int)TG_EDT_MAX_SIDE);
    TG_REQUIRE(u && waves, "tg_sim_field: null pointer");
    TG_REQUIRE(((uintptr_t)waves & 15) == 0, "tg_sim_field: waves must be 16-byte aligned");
    TG_REQUIRE(n_waves >= 1 && n_waves <= TG_SIM_MAX_WAVES, "tg_sim_field: n_waves %d must lie in [1, %d]", n_waves,
               TG_SIM_MAX_WAVES);
    TG_REQUIRE(x0 >= 0 && y0 >= 0 && x0 <= 0xffffffffll && y0 <= 0xffffffffll,
               "tg_sim_field: origin (%lld, %lld) must lie in [0, 2^32)", (long long)x0, (long long)y0);
    TG_REQUIRE(isfinite(nugget_amp) && nugget_amp >= 0.f, "tg_sim_field: nugget_amp %g must be finite and >= 0", (double)nugget_amp);
    const dim3 grid(cdiv(W, SIM_SPAN), H);
    hipLaunchKernelGGL(sim_field_kernel, grid, dim3(SIM_T), 0, S(stream), u, H, W, (uint32_t)x0, (uint32_t)y0,
                       (const int4*)waves, n_waves, nugget_amp, seed, realisation);
    TG_CHECK_LAUNCH("sim_field_kernel");
    return TG_OK;
}

extern "C" int tg_sim_combine(float* out, const float* z, const uint8_t* known, const float* zk, const float* u, const float* uk,
                              double* s1, double* s2, int H, int W, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_sim_combine", H, W)) return rc;
    TG_REQUIRE(out && z && known && zk && u && uk, "tg_sim_combine: null pointer");
    TG_REQUIRE(!s1 == !s2, "tg_sim_combine: s1 and s2 go together (both NULL: no running sums)");
    TG_REQUIRE(!s1 || s1 != s2, "tg_sim_combine: s1 and s2 must be distinct");
    TG_REQUIRE(out != z && out != zk && out != u && out != uk, "tg_sim_combine: out must not alias an input");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(sim_combine_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, S(stream), out, z, known, zk, u, uk, s1, s2, n);
    TG_CHECK_LAUNCH("sim_combine_kernel");
    return TG_OK;
}

extern "C" int tg_sim_stats(float* mean, float* sd, const float* zk, const double* s1, const double* s2, int n, int H, int W,
                            tg_stream_t stream) {
    if (int rc = raster_size_check("tg_sim_stats", H, W)) return rc;
    TG_REQUIRE(mean && sd && zk && s1 && s2, "tg_sim_stats: null pointer");
    TG_REQUIRE(n >= 2, "tg_sim_stats: n %d must be >= 2 (the deviation of one realisation is undefined)", n);
    TG_REQUIRE(mean != sd && mean != zk && sd != zk, "tg_sim_stats: mean, sd and zk must be distinct");
    const int64_t px = (int64_t)H * W;
    hipLaunchKernelGGL(sim_stats_kernel, dim3(ew_grid(px, 256)), dim3(256), 0, S(stream), mean, sd, zk, s1, s2, n, px);
    TG_CHECK_LAUNCH("sim_stats_kernel");
    return TG_OK;
}
