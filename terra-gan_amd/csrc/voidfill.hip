// Harmonic (Laplace) void fill of a DSM by masked multigrid (mvp_gan/src/fill_voids.py).
//
//   tg_vfill_setup   known map, count, min / max (integer atomics on order-preserving keys), offset c = (min + max) / 2, the
//                    initial guess u = z - c at known pixels and 0 elsewhere, the fixed flags of every coarse level (a coarse
//                    cell is fixed when any of its children is) and per level the list of 32 x 64 tiles that hold an unknown
//   tg_vfill_cycle   one V-cycle: per level a down pass (2 red-black Gauss-Seidel sweeps staged in LDS with a 5-px halo, the
//                    residual and its restriction to the next level in the same pass), the coarsest level (at most 16 x 16)
//                    by red-black SOR in one workgroup, per level an up pass (bilinear prolongation of the coarse correction,
//                    2 sweeps); the largest change of u over the unknowns goes to change_bits
//   tg_vfill_finish  known pixels copied bit for bit, u + c at the unknowns, NaN everywhere when nothing is known
//   tg_vfill_pcg_*   the same cycle as the preconditioner of flexible conjugate gradients (section 8n): start after setup,
//                    then one iteration per call in place of tg_vfill_cycle; the solution ends every iteration in level 0's u0
//   tg_vfill_bih_*   the biharmonic (thin-plate) fill (section 8q): conjugate gradients on D(D(u)) = 0 in fp64, preconditioned by
//                    two approximate Laplace solves made of the same cycle; kernels and host code at the end of this file
//
// Level 0 holds v = u - c (known values fixed); coarse levels hold the correction e (0 at fixed cells) with right-hand side f.
// Every unknown cell p solves f_p + sum_{q in N4(p), inside} (v_q - v_p) = 0; the sums run over neighbour DIFFERENCES, which
// fp32 keeps accurate for smooth fields, so the cycle converges below the rounding of v itself.  Restriction sums the four
// children (the unscaled 5-point operator grows by 4 per level), so no level carries an h^2; on a level one cell high or wide a
// coarse cell has two children and their sum is doubled.
//
// Determinism: every value is computed by one thread in a fixed order; tiles are independent (the down and up passes read one
// buffer and write the other); the change is a maximum on the bits of a non-negative float (integer atomic).  Results are
// bitwise reproducible.  No kernel uses scratch.
//
// Rounding: this file is compiled with the default contraction, and __fmul_rn / __fadd_rn are a plain product and sum to the
// compiler, so a product that feeds a sum is one fused multiply-add: the prolongation's 9 a + 3 b (fma(3, b, 9 a)), the SOR
// update u + omega q, and every x + alpha p, e + alpha p and z + beta p below.  The lines marked "fused" are these sites;
// tests/vfill_pcg_mirror.py (fma=True) rounds the same way and tests/test_hip_vfill_stages.py compares with it, so a change of
// the contraction (a pragma, a flag, a compiler) must be made in both places.
#include <math.h>
#include <stddef.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

constexpr int VF_TY = 32, VF_TX = 64;              // output tile of the level kernels
constexpr int VF_HS = 4;                           // half-sweeps per pass (2 red-black sweeps)
constexpr int VF_HALO = VF_HS + 1;                 // + 1: the residual after the last half-sweep
constexpr int VF_SY = VF_TY + 2 * VF_HALO, VF_SX = VF_TX + 2 * VF_HALO;
constexpr int VF_SXP = VF_SX + 2;                  // LDS row stride
constexpr int VF_CY = VF_TY / 2 + 8, VF_CX = VF_TX / 2 + 8;    // coarse patch of the prolongation (origin y0/2 - 4, x0/2 - 4)
constexpr int VF_MAX_GRID = 2048;
constexpr int VF_CMAX = 16;                        // coarsest level: longer side at most 16 (one cell per thread)
constexpr int VF_ALIGN = 256;
enum { VF_IN = 1, VF_FIX = 2 };

struct VfHdr {
    uint32_t lo_key, hi_key;                       // order-preserving keys of min / max z over K
    unsigned long long known;
    float c;                                       // offset (min + max) / 2
    int32_t _pad;
    int32_t ntiles[TG_VFILL_MAX_LEVELS];           // active tiles per level
};
static_assert(sizeof(VfHdr) <= VF_ALIGN, "header fits its slot");
// the layout VFILL_HDR of mvp_gan/src/fill_voids.py reads
static_assert(offsetof(VfHdr, lo_key) == 0 && offsetof(VfHdr, hi_key) == 4 && offsetof(VfHdr, known) == 8, "VFILL_HDR");
static_assert(offsetof(VfHdr, c) == 16 && offsetof(VfHdr, ntiles) == 24 && TG_VFILL_MAX_LEVELS == 32, "VFILL_HDR");
static_assert(sizeof(VfHdr) == 24 + 4 * 32, "VFILL_HDR");

// ---- host-side plan (mirrored by vfill_levels / vfill_layout in mvp_gan/src/fill_voids.py) ---------------------------
struct VfLevel {
    int H, W, tiles_x, tiles;
    size_t flags, list, u0, u1, f;                 // byte offsets; level 0 has no f
};
struct VfPlan {
    int L;
    VfLevel lv[TG_VFILL_MAX_LEVELS];
    size_t bytes;
};

static size_t al(size_t n) { return (n + VF_ALIGN - 1) / VF_ALIGN * VF_ALIGN; }

static void vf_plan(int H, int W, VfPlan* p) {
    int h = H, w = W, L = 0;
    size_t off = VF_ALIGN;                         // VfHdr
    for (;;) {
        VfLevel& v = p->lv[L];
        v.H = h; v.W = w;
        v.tiles_x = cdiv(w, VF_TX);
        v.tiles = cdiv(h, VF_TY) * v.tiles_x;
        const size_t n = (size_t)h * w;
        v.flags = off; off += al(n);
        v.list = off; off += al((size_t)v.tiles * 4);
        v.u0 = off; off += al(n * 4);
        v.u1 = off; off += al(n * 4);
        if (L > 0) { v.f = off; off += al(n * 4); } else { v.f = 0; }
        ++L;
        if ((h > w ? h : w) <= VF_CMAX) break;
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    p->L = L;
    p->bytes = off;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- setup --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vf_known_kernel(const float* __restrict__ dem, const float* __restrict__ mask,
                                                       int use_nodata, float nodata, int64_t n, uint8_t* __restrict__ flags,
                                                       VfHdr* hdr) {
    __shared__ uint32_t red[4][3];
    uint32_t cnt = 0, lo = 0xffffffffu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float z = dem[i];
        bool k = isfinite(z);
        if (mask) k = k && mask[i] != 0.f;
        if (use_nodata) k = k && z != nodata;
        flags[i] = k ? VF_FIX : 0;
        if (k) {
            ++cnt;
            const uint32_t q = f2key(z == 0.f ? 0.f : z);          // -0 and +0 share a key
            lo = q < lo ? q : lo;
            hi = q > hi ? q : hi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const uint32_t a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = cnt; red[w][1] = lo; red[w][2] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, l = 0xffffffffu, h = 0u;
        for (int q = 0; q < 4; ++q) {
            c += red[q][0];
            l = red[q][1] < l ? red[q][1] : l;
            h = red[q][2] > h ? red[q][2] : h;
        }
        if (c) {
            atomicAdd(&hdr->known, (unsigned long long)c);
            atomicMin(&hdr->lo_key, l);
            atomicMax(&hdr->hi_key, h);
        }
    }
}

// v = z - c at known pixels, 0 elsewhere, into both buffers; block 0 writes the statistics
__global__ __launch_bounds__(256) void vf_init_kernel(const float* __restrict__ dem, const uint8_t* __restrict__ flags,
                                                      int64_t n, VfHdr* hdr, float* __restrict__ u0, float* __restrict__ u1,
                                                      int64_t* __restrict__ stats) {
    const unsigned long long known = hdr->known;
    const float lo = key2f(hdr->lo_key), hi = key2f(hdr->hi_key);
    const float c = known ? __fadd_rn(__fmul_rn(lo, 0.5f), __fmul_rn(hi, 0.5f)) : 0.f;   // no overflow at +-FLT_MAX
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr->c = c;
        stats[TG_VFILL_KNOWN] = (int64_t)known;
        stats[TG_VFILL_UNKNOWN] = n - (int64_t)known;
        stats[TG_VFILL_MIN_BITS] = known ? (int64_t)__float_as_uint(lo) : 0;
        stats[TG_VFILL_MAX_BITS] = known ? (int64_t)__float_as_uint(hi) : 0;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = (flags[i] & VF_FIX) ? __fsub_rn(dem[i], c) : 0.f;
        u0[i] = v;
        u1[i] = v;
    }
}

// fixed flags of level l + 1: any fixed child
__global__ __launch_bounds__(256) void vf_coarsen_kernel(const uint8_t* __restrict__ fine, int Hf, int Wf,
                                                         uint8_t* __restrict__ coarse, int Hc, int Wc) {
    const int64_t n = (int64_t)Hc * Wc;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int Y = (int)(j / Wc), X = (int)(j - (int64_t)Y * Wc);
        uint8_t f = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * Y + dy, x = 2 * X + dx;
                if (y < Hf && x < Wf) f |= fine[(int64_t)y * Wf + x];
            }
        coarse[j] = f & VF_FIX;
    }
}

// tiles of a level holding an unknown cell -> list (order of the atomic counter; the passes do not depend on it)
__global__ __launch_bounds__(256) void vf_tiles_kernel(const uint8_t* __restrict__ flags, int H, int W, int tiles_x, int tiles,
                                                       int32_t* __restrict__ list, int32_t* __restrict__ count) {
    __shared__ int any[4];
    const int w = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        int a = 0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int y = y0 + j / VF_TX, x = x0 + (j & (VF_TX - 1));
            if (y < H && x < W && !(flags[(int64_t)y * W + x] & VF_FIX)) a = 1;
        }
        a = __any(a) ? 1 : 0;
        if ((threadIdx.x & 63) == 0) any[w] = a;
        __syncthreads();
        if (threadIdx.x == 0 && (any[0] | any[1] | any[2] | any[3])) list[atomicAdd(count, 1)] = t;
        __syncthreads();
    }
}

// ---- the level passes ---------------------------------------------------------------------------------------------------
struct VfPass {
    const float* in;          // level values read with the halo (nullptr: start from 0)
    float* out;               // the tile's values after the sweeps
    const float* rhs;         // f of this level (nullptr at level 0)
    const uint8_t* flags;
    const int32_t* list;
    const int32_t* count;
    int H, W, tiles_x;
    // down pass: residual restricted to the next level
    float* f_next;
    const uint8_t* flags_next;
    float rscale;             // 4 / children of an interior coarse cell: 1, or 2 on a level one cell high or wide
    // up pass: correction of the next level, prolongated
    const float* e_next;
    int Hn, Wn;
    uint32_t* change;         // level 0 up pass: max |out_new - out_old| bits over the unknowns
};

struct VfLds {
    float u[VF_SY][VF_SXP];
    float f[VF_SY][VF_SXP];
    uint8_t fl[VF_SY][VF_SXP];
    float r[VF_TY][VF_TX];
    float ec[VF_CY][VF_CX];
};

// one red-black half-sweep over the LDS cells at distance >= j + 1 from the staged border, colour (gy + gx) & 1 == col
__device__ __forceinline__ void vf_half_sweep(VfLds& s, int j, int col, int par0) {
    const int r0 = j + 1, r1 = VF_SY - j - 1, c0 = j + 1, c1 = VF_SX - j - 1;
    const int nr = r1 - r0, ncp = (c1 - c0 + 1) / 2;            // cells of one colour per row: at most ncp
    for (int k = threadIdx.x; k < nr * ncp; k += 256) {
        const int ly = r0 + k / ncp;
        int lx = c0 + 2 * (k - (k / ncp) * ncp);
        if (((ly + lx + par0) & 1) != col) ++lx;
        if (lx >= c1) continue;
        const uint8_t fl = s.fl[ly][lx];
        if ((fl & (VF_IN | VF_FIX)) != VF_IN) continue;
        const float up = s.u[ly][lx];
        float acc = s.f[ly][lx];
        int n = 0;
        if (s.fl[ly - 1][lx] & VF_IN) { acc += s.u[ly - 1][lx] - up; ++n; }
        if (s.fl[ly + 1][lx] & VF_IN) { acc += s.u[ly + 1][lx] - up; ++n; }
        if (s.fl[ly][lx - 1] & VF_IN) { acc += s.u[ly][lx - 1] - up; ++n; }
        if (s.fl[ly][lx + 1] & VF_IN) { acc += s.u[ly][lx + 1] - up; ++n; }
        if (n) s.u[ly][lx] = up + acc / (float)n;
    }
    __syncthreads();
}

// FINE: level 0, whose right-hand side is 0 (never read)
template <bool UP, bool FINE>
__global__ __launch_bounds__(256) void vf_pass_kernel(VfPass P) {
    __shared__ VfLds s;
    const int H = P.H, W = P.W;
    const int ntiles = *P.count;
    uint32_t mx = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list[t];
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        const int gy0 = y0 - VF_HALO, gx0 = x0 - VF_HALO;
        const int cy0 = y0 / 2 - 4, cx0 = x0 / 2 - 4;
        __syncthreads();                                          // the previous tile's readers are done
        if (UP) {
            for (int j = threadIdx.x; j < VF_CY * VF_CX; j += 256) {
                const int r = j / VF_CX, c = j - r * VF_CX;
                int Y = cy0 + r, X = cx0 + c;
                Y = Y < 0 ? 0 : (Y >= P.Hn ? P.Hn - 1 : Y);
                X = X < 0 ? 0 : (X >= P.Wn ? P.Wn - 1 : X);
                s.ec[r][c] = P.e_next[(int64_t)Y * P.Wn + X];
            }
            __syncthreads();
        }
        for (int j = threadIdx.x; j < VF_SY * VF_SX; j += 256) {
            const int r = j / VF_SX, c = j - r * VF_SX;
            const int y = gy0 + r, x = gx0 + c;
            float u = 0.f, f = 0.f;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                if (P.in) u = P.in[i];
                if (!FINE) f = P.rhs[i];
                if (UP && !(fl & VF_FIX)) {
                    const int Y = y >> 1, X = x >> 1;
                    const int ly = Y - cy0, lx = X - cx0;
                    const int ny = ly + ((y & 1) ? 1 : -1), nx = lx + ((x & 1) ? 1 : -1);
                    // fused: 9 a + 3 b is fma(3, b, 9 a)
                    const float e = (9.f * s.ec[ly][lx] + 3.f * s.ec[ny][lx] + 3.f * s.ec[ly][nx] + s.ec[ny][nx]) * 0.0625f;
                    u += e;
                }
            }
            s.u[r][c] = u;
            s.f[r][c] = f;
            s.fl[r][c] = fl;
        }
        __syncthreads();
        const int par0 = (gy0 + gx0) & 1;
#pragma unroll 1
        for (int j = 0; j < VF_HS; ++j) vf_half_sweep(s, j, j & 1, par0);

        if (!UP) {
            // residual at the tile's cells, then its restriction: the 2 x 2 children of a coarse cell lie in one tile
            for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
                const int r = j / VF_TX, c = j - r * VF_TX;
                const int ly = r + VF_HALO, lx = c + VF_HALO;
                const uint8_t fl = s.fl[ly][lx];
                float acc = 0.f;
                if ((fl & (VF_IN | VF_FIX)) == VF_IN) {
                    const float up = s.u[ly][lx];
                    acc = s.f[ly][lx];
                    if (s.fl[ly - 1][lx] & VF_IN) acc += s.u[ly - 1][lx] - up;
                    if (s.fl[ly + 1][lx] & VF_IN) acc += s.u[ly + 1][lx] - up;
                    if (s.fl[ly][lx - 1] & VF_IN) acc += s.u[ly][lx - 1] - up;
                    if (s.fl[ly][lx + 1] & VF_IN) acc += s.u[ly][lx + 1] - up;
                }
                s.r[r][c] = acc;
                const int y = y0 + r, x = x0 + c;
                if (y < H && x < W) P.out[(int64_t)y * W + x] = s.u[ly][lx];
            }
            __syncthreads();
            for (int j = threadIdx.x; j < (VF_TY / 2) * (VF_TX / 2); j += 256) {
                const int R = j / (VF_TX / 2), Cc = j - R * (VF_TX / 2);
                const int Y = y0 / 2 + R, X = x0 / 2 + Cc;
                if (Y >= P.Hn || X >= P.Wn) continue;
                const int64_t J = (int64_t)Y * P.Wn + X;
                const float v = (P.flags_next[J] & VF_FIX)
                                    ? 0.f
                                    : ((s.r[2 * R][2 * Cc] + s.r[2 * R][2 * Cc + 1]) + (s.r[2 * R + 1][2 * Cc] + s.r[2 * R + 1][2 * Cc + 1])) *
                                          P.rscale;
                P.f_next[J] = v;
            }
        } else {
            for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
                const int r = j / VF_TX, c = j - r * VF_TX;
                const int y = y0 + r, x = x0 + c;
                if (y >= H || x >= W) continue;
                const int ly = r + VF_HALO, lx = c + VF_HALO;
                const int64_t i = (int64_t)y * W + x;
                const float v = s.u[ly][lx];
                if (P.change && !(s.fl[ly][lx] & VF_FIX)) {
                    const uint32_t d = __float_as_uint(fabsf(v - P.out[i]));
                    mx = d > mx ? d : mx;
                }
                P.out[i] = v;
            }
        }
    }
    if (UP && P.change) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t u = __shfl_xor(mx, o, 64);
            mx = u > mx ? u : mx;
        }
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(P.change, mx);
    }
}

// ---- coarsest level: one workgroup, red-black SOR in LDS ----------------------------------------------------------------
struct VfCoarse {
    const float* in;          // level 0 only (the grid is the raster): v with the known values; else start from 0
    float* out;
    const float* rhs;         // nullptr at level 0
    const uint8_t* flags;
    int H, W, sweeps;
    float omega;
    uint32_t* change;         // level 0 only
};

__global__ __launch_bounds__(256) void vf_coarsest_kernel(VfCoarse P) {
    __shared__ float u[VF_CMAX + 2][VF_CMAX + 2];
    __shared__ float f[VF_CMAX][VF_CMAX];
    __shared__ uint8_t fl[VF_CMAX + 2][VF_CMAX + 2];
    __shared__ uint32_t red[4];
    const int H = P.H, W = P.W;
    for (int j = threadIdx.x; j < (VF_CMAX + 2) * (VF_CMAX + 2); j += 256) {
        const int r = j / (VF_CMAX + 2), c = j - r * (VF_CMAX + 2);
        const int y = r - 1, x = c - 1;
        float v = 0.f;
        uint8_t g = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int i = y * W + x;
            g = VF_IN | P.flags[i];
            if (P.in) v = P.in[i];
            f[y][x] = P.rhs ? P.rhs[i] : 0.f;
        }
        u[r][c] = v;
        fl[r][c] = g;
    }
    __syncthreads();
    const float om = P.omega;
    const int half = (W + 1) / 2;
#pragma unroll 1
    for (int sw = 0; sw < 2 * P.sweeps; ++sw) {
        const int col = sw & 1;
        for (int k = threadIdx.x; k < H * half; k += 256) {
            const int y = k / half;
            int x = 2 * (k - y * half);
            if (((y + x) & 1) != col) ++x;
            if (x >= W) continue;
            const int ly = y + 1, lx = x + 1;
            if ((fl[ly][lx] & (VF_IN | VF_FIX)) != VF_IN) continue;
            const float up = u[ly][lx];
            float acc = f[y][x];
            int n = 0;
            if (fl[ly - 1][lx] & VF_IN) { acc += u[ly - 1][lx] - up; ++n; }
            if (fl[ly + 1][lx] & VF_IN) { acc += u[ly + 1][lx] - up; ++n; }
            if (fl[ly][lx - 1] & VF_IN) { acc += u[ly][lx - 1] - up; ++n; }
            if (fl[ly][lx + 1] & VF_IN) { acc += u[ly][lx + 1] - up; ++n; }
            if (n) u[ly][lx] = up + om * (acc / (float)n);             // fused
        }
        __syncthreads();
    }
    uint32_t mx = 0;
    for (int k = threadIdx.x; k < H * W; k += 256) {
        const int y = k / W, x = k - y * W;
        const float v = u[y + 1][x + 1];
        if (P.change && !(fl[y + 1][x + 1] & VF_FIX)) {
            const uint32_t d = __float_as_uint(fabsf(v - P.out[k]));
            mx = d > mx ? d : mx;
        }
        P.out[k] = v;
    }
    if (P.change) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t t = __shfl_xor(mx, o, 64);
            mx = t > mx ? t : mx;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t m = 0;
            for (int q = 0; q < 4; ++q) m = red[q] > m ? red[q] : m;
            if (m) atomicMax(P.change, m);
        }
    }
}

// ---- conjugate gradients around the V-cycle (tg_vfill_pcg_*) --------------------------------------
// A x = b over the unknowns: A is the masked 5-point graph Laplacian, x the level-0 field v.  r = b - A x is the difference-form
// residual sum_q (x_q - x_p) with the known values in place; A p = -sum_q (p_q - p_p) with p = 0 at the fixed cells.  The
// vector work runs on level 0's active tiles with a 1-px halo.  Every partial dot product is stored by tile id and the slots
// are summed in tile-id order by one workgroup, in fp64: the tile list's order (an atomic counter) never reaches a result.
constexpr int VF_PY = VF_TY + 2, VF_PX = VF_TX + 2, VF_PXP = VF_PX + 1;

struct VfPcgScal {
    double rho, pap, rz_old, rz_new;               // r.z of the current direction, p.Ap, r'.z, r'.z'
    float alpha, beta;
    uint32_t restarts;                             // directions restarted from p = z
    uint32_t restart;                              // 1: the step is skipped (alpha = 0) and the next beta is 0
    uint32_t parity;                               // the current p is p[parity]
    uint32_t _pad;
};
static_assert(sizeof(VfPcgScal) <= VF_ALIGN, "scalars fit their slot");
// the layout VFILL_PCG_SCAL of mvp_gan/src/fill_voids.py reads (the biharmonic fill keeps two such blocks, sc_out and sc_in)
static_assert(offsetof(VfPcgScal, rho) == 0 && offsetof(VfPcgScal, pap) == 8, "VFILL_PCG_SCAL");
static_assert(offsetof(VfPcgScal, rz_old) == 16 && offsetof(VfPcgScal, rz_new) == 24, "VFILL_PCG_SCAL");
static_assert(offsetof(VfPcgScal, alpha) == 32 && offsetof(VfPcgScal, beta) == 36, "VFILL_PCG_SCAL");
static_assert(offsetof(VfPcgScal, restarts) == 40 && offsetof(VfPcgScal, restart) == 44, "VFILL_PCG_SCAL");
static_assert(offsetof(VfPcgScal, parity) == 48 && offsetof(VfPcgScal, _pad) == 52, "VFILL_PCG_SCAL");
static_assert(sizeof(VfPcgScal) == 56, "VFILL_PCG_SCAL");

struct VfPcg {
    const uint8_t* flags;
    const int32_t* list;      // nullptr on a one-level raster: the single tile 0
    const int32_t* count;
    int H, W, tiles_x;
    VfPcgScal* sc;
    const float* x_in;        // step: x (u0); dot: x' (u1)
    float* x_out;             // step: x' (u1); dot: u0
    float* r;
    const float* z;
    float* p0;
    float* p1;
    double* part;             // this launch's partials, by tile id
    uint32_t* change;
    int init;                 // step: alpha = 0 (the first residual)
};

// the sum of v over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double vf_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// x' = x + alpha p (halo included) -> x_out, r' = b - A x' -> r, the tile's r'.z_old and the largest |alpha p| over the unknowns
__global__ __launch_bounds__(256) void vf_pcg_step_kernel(VfPcg P) {
    __shared__ float sx[VF_PY][VF_PXP];
    __shared__ uint8_t sf[VF_PY][VF_PXP];
    __shared__ double red[4];
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const float alpha = P.init ? 0.f : P.sc->alpha;
    const float* pin = P.sc->parity ? P.p1 : P.p0;
    uint32_t mx = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();                                          // the previous tile's readers are done
        for (int j = threadIdx.x; j < VF_PY * VF_PX; j += 256) {
            const int r = j / VF_PX, c = j - r * VF_PX;
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float v = 0.f;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                v = P.x_in[i];
                const bool inner = r >= 1 && r <= VF_TY && c >= 1 && c <= VF_TX;
                if (!(fl & VF_FIX) && alpha != 0.f) {
                    const float d = __fmul_rn(alpha, pin[i]);
                    v = __fadd_rn(v, d);                           // fused: fma(alpha, p, v); d itself is the rounded product
                    if (inner) {
                        const uint32_t b = __float_as_uint(fabsf(d));
                        mx = b > mx ? b : mx;
                    }
                }
                if (inner) P.x_out[i] = v;
            }
            sx[r][c] = v;
            sf[r][c] = fl;
        }
        __syncthreads();
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int ly = r + 1, lx = c + 1;
            const int64_t i = (int64_t)y * W + x;
            float acc = 0.f;
            if (!(sf[ly][lx] & VF_FIX)) {
                const float up = sx[ly][lx];
                if (sf[ly - 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly - 1][lx], up));
                if (sf[ly + 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly + 1][lx], up));
                if (sf[ly][lx - 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly][lx - 1], up));
                if (sf[ly][lx + 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly][lx + 1], up));
                sum += (double)acc * (double)P.z[i];
            }
            P.r[i] = acc;
        }
        sum = vf_block_sum(sum, red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
    if (P.change) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t u = __shfl_xor(mx, o, 64);
            mx = u > mx ? u : mx;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0 && P.sc->restart) mx = 0x7f800000u;      // a skipped step is not convergence
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(P.change, mx);
    }
}

// the tile's r'.z'; x' moves from u1 back to u0
__global__ __launch_bounds__(256) void vf_pcg_dot_kernel(VfPcg P) {
    __shared__ double red[4];
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int64_t i = (int64_t)y * W + x;
            sum += (double)P.r[i] * (double)P.z[i];               // r is 0 at the fixed cells
            P.x_out[i] = P.x_in[i];
        }
        sum = vf_block_sum(sum, red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
}

// p = z + beta p (halo included) -> the other p buffer, A p in difference form, the tile's p.Ap
__global__ __launch_bounds__(256) void vf_pcg_dir_kernel(VfPcg P) {
    __shared__ float sp[VF_PY][VF_PXP];
    __shared__ uint8_t sf[VF_PY][VF_PXP];
    __shared__ double red[4];
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const float beta = P.sc->beta;
    const bool par = P.sc->parity != 0;
    const float* pin = par ? P.p1 : P.p0;
    float* pout = par ? P.p0 : P.p1;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();
        for (int j = threadIdx.x; j < VF_PY * VF_PX; j += 256) {
            const int r = j / VF_PX, c = j - r * VF_PX;
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float v = 0.f;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                if (!(fl & VF_FIX)) {
                    v = P.z[i];
                    if (beta != 0.f) v = __fadd_rn(v, __fmul_rn(beta, pin[i]));    // fused
                }
                if (r >= 1 && r <= VF_TY && c >= 1 && c <= VF_TX) pout[i] = v;
            }
            sp[r][c] = v;
            sf[r][c] = fl;
        }
        __syncthreads();
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int ly = r + 1, lx = c + 1;
            if (sf[ly][lx] & VF_FIX) continue;
            const float up = sp[ly][lx];
            float acc = 0.f;
            if (sf[ly - 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(up, sp[ly - 1][lx]));
            if (sf[ly + 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(up, sp[ly + 1][lx]));
            if (sf[ly][lx - 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(up, sp[ly][lx - 1]));
            if (sf[ly][lx + 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(up, sp[ly][lx + 1]));
            sum += (double)up * (double)acc;
        }
        sum = vf_block_sum(sum, red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
}

// One workgroup: the partials summed in tile-id order, then the scalars.
//   BETA:  rho' = sum pa (r'.z'), r'.z = sum pb; beta = (rho' - r'.z) / rho, or 0 at the start, after a restart and at rho = 0
//   !BETA: p.Ap = sum pa; alpha = rho / p.Ap, or 0 with the restart flag when that is no usable step; p's buffers swap
template <bool BETA>
__global__ __launch_bounds__(256) void vf_pcg_scalar_kernel(VfPcgScal* sc, const double* __restrict__ pa,
                                                            const double* __restrict__ pb, int tiles, int first,
                                                            uint32_t* restarts_out) {
    __shared__ double red[2][256];
    double a = 0.0, b = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) {
        a += pa[t];
        if (BETA) b += pb[t];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (BETA) {
        const double rzn = red[0][0], rzo = red[1][0];
        float beta = 0.f;
        if (!first) {
            if (sc->restart) {
                sc->restart = 0;
            } else if (sc->rho != 0.0) {                           // rho = 0: converged, alpha stays 0
                const float bf = (float)((rzn - rzo) / sc->rho);
                if (isfinite(bf)) beta = bf;
                else ++sc->restarts;
            }
        }
        sc->beta = beta;
        sc->rz_old = rzo;
        sc->rz_new = rzn;
        sc->rho = rzn;
    } else {
        const double pap = red[0][0], rho = sc->rho;
        float alpha = 0.f;
        uint32_t rs = 0;
        if (rho != 0.0) {                                          // rho = 0: converged, the step is 0
            const float af = (float)(rho / pap);
            if (pap > 0.0 && isfinite(af)) alpha = af;
            else { rs = 1; ++sc->restarts; }
        }
        sc->pap = pap;
        sc->alpha = alpha;
        sc->restart = rs;
        sc->parity ^= 1u;
        if (restarts_out) *restarts_out = sc->restarts;
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vf_finish_kernel(const float* __restrict__ dem, const uint8_t* __restrict__ flags,
                                                        const VfHdr* hdr, const float* __restrict__ u, int64_t n,
                                                        float* __restrict__ out) {
    const bool none = hdr->known == 0;
    const float c = hdr->c;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v;
        if (none) v = __int_as_float(0x7fc00000);
        else if (flags[i] & VF_FIX) v = dem[i];
        else v = __fadd_rn(u[i], c);
        out[i] = v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int vf_size_check(const char* who, int H, int W) {
    TG_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: raster %dx%d must be non-empty with H*W < 2^31", who,
               H, W);
    return TG_OK;
}

static int vf_ws_check(const char* who, int H, int W, const void* ws, size_t ws_bytes, VfPlan* p) {
    if (int rc = vf_size_check(who, H, W)) return rc;
    TG_REQUIRE(ws, "%s: null pointer", who);
    TG_REQUIRE(((uintptr_t)ws & (VF_ALIGN - 1)) == 0, "%s: workspace must be %d-byte aligned", who, VF_ALIGN);
    vf_plan(H, W, p);
    if (ws_bytes < p->bytes) {
        tg_set_error("%s: workspace %zu bytes < %zu", who, ws_bytes, p->bytes);
        return TG_ERR_WS;
    }
    return TG_OK;
}

static float vf_omega(int H, int W) {
    const int n = H > W ? H : W;
    return (float)(2.0 / (1.0 + sin(M_PI / (2.0 * n + 1.0))));
}
static int vf_sweeps(int H, int W) { return 8 * (H > W ? H : W) + 16; }

extern "C" size_t tg_vfill_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    VfPlan p;
    vf_plan(H, W, &p);
    return p.bytes;
}

extern "C" int tg_vfill_levels(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    VfPlan p;
    vf_plan(H, W, &p);
    return p.L;
}

extern "C" int tg_vfill_setup(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, void* ws,
                              size_t ws_bytes, int64_t* stats, tg_stream_t stream) {
    VfPlan p;
    if (int rc = vf_ws_check("tg_vfill_setup", H, W, ws, ws_bytes, &p)) return rc;
    TG_REQUIRE(dem && stats, "tg_vfill_setup: null pointer");
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    VfHdr* hdr = (VfHdr*)base;
    if (hipMemsetAsync(base, 0, p.bytes, s) != hipSuccess) {     // counters, coarse levels and tile counts start at 0
        tg_set_error("tg_vfill_setup: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const uint32_t lo_init = 0xffffffffu;
    if (hipMemsetD32Async((hipDeviceptr_t)&hdr->lo_key, (int)lo_init, 1, s) != hipSuccess) {
        tg_set_error("tg_vfill_setup: hipMemsetD32Async failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t n = (int64_t)H * W;
    const VfLevel& l0 = p.lv[0];
    uint8_t* fl0 = (uint8_t*)(base + l0.flags);
    hipLaunchKernelGGL(vf_known_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, dem, mask, use_nodata, nodata, n, fl0, hdr);
    TG_CHECK_LAUNCH("vf_known_kernel");
    hipLaunchKernelGGL(vf_init_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, dem, fl0, n, hdr, (float*)(base + l0.u0),
                       (float*)(base + l0.u1), stats);
    TG_CHECK_LAUNCH("vf_init_kernel");
    for (int l = 0; l < p.L; ++l) {
        const VfLevel& v = p.lv[l];
        if (l > 0) {
            const VfLevel& u = p.lv[l - 1];
            hipLaunchKernelGGL(vf_coarsen_kernel, dim3(ew_grid((int64_t)v.H * v.W, 256)), dim3(256), 0, s,
                               (const uint8_t*)(base + u.flags), u.H, u.W, (uint8_t*)(base + v.flags), v.H, v.W);
            TG_CHECK_LAUNCH("vf_coarsen_kernel");
        }
        if (l < p.L - 1) {
            hipLaunchKernelGGL(vf_tiles_kernel, dim3(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID), dim3(256), 0, s,
                               (const uint8_t*)(base + v.flags), v.H, v.W, v.tiles_x, v.tiles, (int32_t*)(base + v.list),
                               &hdr->ntiles[l]);
            TG_CHECK_LAUNCH("vf_tiles_kernel");
        }
    }
    return TG_OK;
}

// The launches of one V-cycle.  pre == nullptr: the plain cycle on level 0's u0 / u1.  With pre the cycle is the preconditioner
// of tg_vfill_pcg_*: level 0 is treated as a coarse level (start from 0, right-hand side pre->r, sweeps into pre->d, result
// in pre->z) and no change is taken.
struct VfPre {
    const float* r;
    float* d;
    float* z;
};

static int vf_launch_cycle(const VfPlan& p, char* base, const VfPre* pre, uint32_t* change_bits, hipStream_t s) {
    VfHdr* hdr = (VfHdr*)base;
    const int L = p.L;
    auto F = [&](size_t off) { return (float*)(base + off); };
    auto U8 = [&](size_t off) { return (const uint8_t*)(base + off); };
    auto pass = [&](int l) {
        const VfLevel& v = p.lv[l];
        VfPass a = {};
        a.flags = U8(v.flags);
        a.list = (const int32_t*)(base + v.list);
        a.count = &hdr->ntiles[l];
        a.H = v.H; a.W = v.W; a.tiles_x = v.tiles_x;
        a.rhs = l > 0 ? F(v.f) : (pre ? pre->r : nullptr);
        a.Hn = p.lv[l + 1].H; a.Wn = p.lv[l + 1].W;
        return a;
    };
    // down: level 0 reads u0 and writes u1; coarse levels start from 0 and write u1
    for (int l = 0; l < L - 1; ++l) {
        const VfLevel& v = p.lv[l];
        VfPass a = pass(l);
        a.in = l == 0 && !pre ? F(v.u0) : nullptr;
        a.out = l == 0 && pre ? pre->d : F(v.u1);
        a.f_next = F(p.lv[l + 1].f);
        a.flags_next = U8(p.lv[l + 1].flags);
        a.rscale = (v.H == 1 || v.W == 1) ? 2.f : 1.f;
        const dim3 g(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID);
        if (l == 0 && !pre) hipLaunchKernelGGL((vf_pass_kernel<false, true>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((vf_pass_kernel<false, false>), g, dim3(256), 0, s, a);
        TG_CHECK_LAUNCH("vf_pass_kernel<down>");
    }
    {
        const VfLevel& v = p.lv[L - 1];
        VfCoarse c;
        c.in = L == 1 && !pre ? F(v.u0) : nullptr;
        c.out = L == 1 && pre ? pre->z : F(v.u0);
        c.rhs = L == 1 ? (pre ? pre->r : nullptr) : F(v.f);
        c.flags = U8(v.flags);
        c.H = v.H; c.W = v.W;
        c.sweeps = vf_sweeps(v.H, v.W);
        c.omega = vf_omega(v.H, v.W);
        c.change = L == 1 && !pre ? change_bits : nullptr;
        hipLaunchKernelGGL(vf_coarsest_kernel, dim3(1), dim3(256), 0, s, c);
        TG_CHECK_LAUNCH("vf_coarsest_kernel");
    }
    // up: u1 + prolongated correction of level l + 1 (its u0) -> u0
    for (int l = L - 2; l >= 0; --l) {
        const VfLevel& v = p.lv[l];
        VfPass a = pass(l);
        a.in = l == 0 && pre ? pre->d : F(v.u1);
        a.out = l == 0 && pre ? pre->z : F(v.u0);
        a.e_next = F(p.lv[l + 1].u0);
        a.change = l == 0 && !pre ? change_bits : nullptr;
        const dim3 g(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID);
        if (l == 0 && !pre) hipLaunchKernelGGL((vf_pass_kernel<true, true>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((vf_pass_kernel<true, false>), g, dim3(256), 0, s, a);
        TG_CHECK_LAUNCH("vf_pass_kernel<up>");
    }
    return TG_OK;
}

extern "C" int tg_vfill_cycle(int H, int W, void* ws, size_t ws_bytes, uint32_t* change_bits, tg_stream_t stream) {
    VfPlan p;
    if (int rc = vf_ws_check("tg_vfill_cycle", H, W, ws, ws_bytes, &p)) return rc;
    TG_REQUIRE(change_bits, "tg_vfill_cycle: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(change_bits, 0, sizeof(uint32_t), s) != hipSuccess) {
        tg_set_error("tg_vfill_cycle: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    return vf_launch_cycle(p, (char*)ws, nullptr, change_bits, s);
}

extern "C" int tg_vfill_finish(const float* dem, int H, int W, const void* ws, size_t ws_bytes, float* out,
                               tg_stream_t stream) {
    VfPlan p;
    if (int rc = vf_ws_check("tg_vfill_finish", H, W, ws, ws_bytes, &p)) return rc;
    TG_REQUIRE(dem && out, "tg_vfill_finish: null pointer");
    const char* base = (const char*)ws;
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(vf_finish_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, S(stream), dem, (const uint8_t*)(base + p.lv[0].flags),
                       (const VfHdr*)base, (const float*)(base + p.lv[0].u0), n, out);
    TG_CHECK_LAUNCH("vf_finish_kernel");
    return TG_OK;
}

// ---- conjugate gradients: host side ----------------------------------------------------------------------------------------
// the second workspace (mirrored by vfill_pcg_layout in mvp_gan/src/fill_voids.py)
struct VfPcgPlan {
    size_t r, z, p0, p1, d, part[3];               // byte offsets; part: p.Ap, r'.z, r'.z' by tile id
    size_t bytes;
};

static void vf_pcg_plan(const VfPlan& p, VfPcgPlan* q) {
    const size_t n = (size_t)p.lv[0].H * p.lv[0].W;
    size_t off = VF_ALIGN;                         // VfPcgScal
    q->r = off; off += al(n * 4);
    q->z = off; off += al(n * 4);
    q->p0 = off; off += al(n * 4);
    q->p1 = off; off += al(n * 4);
    q->d = off; off += al(n * 4);
    for (int k = 0; k < 3; ++k) { q->part[k] = off; off += al((size_t)p.lv[0].tiles * 8); }
    q->bytes = off;
}

static int vf_pws_check(const char* who, const VfPlan& p, const void* pws, size_t pws_bytes, VfPcgPlan* q) {
    TG_REQUIRE(pws, "%s: null pointer", who);
    TG_REQUIRE(((uintptr_t)pws & (VF_ALIGN - 1)) == 0, "%s: pcg workspace must be %d-byte aligned", who, VF_ALIGN);
    vf_pcg_plan(p, q);
    if (pws_bytes < q->bytes) {
        tg_set_error("%s: pcg workspace %zu bytes < %zu", who, pws_bytes, q->bytes);
        return TG_ERR_WS;
    }
    return TG_OK;
}

extern "C" size_t tg_vfill_pcg_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    VfPlan p;
    VfPcgPlan q;
    vf_plan(H, W, &p);
    vf_pcg_plan(p, &q);
    return q.bytes;
}

// step (or the first residual), z = M r, r.z, beta, the new direction and p.Ap, alpha
static int vf_pcg_launch(const VfPlan& p, const VfPcgPlan& q, char* base, char* pb, bool first,
                         uint32_t* change_bits, uint32_t* restarts, hipStream_t s) {
    const VfLevel& v = p.lv[0];
    VfHdr* hdr = (VfHdr*)base;
    VfPcgScal* sc = (VfPcgScal*)pb;
    auto F = [&](size_t off) { return (float*)(pb + off); };
    auto D = [&](int k) { return (double*)(pb + q.part[k]); };
    VfPcg a = {};
    a.flags = (const uint8_t*)(base + v.flags);
    a.list = p.L > 1 ? (const int32_t*)(base + v.list) : nullptr;
    a.count = &hdr->ntiles[0];
    a.H = v.H; a.W = v.W; a.tiles_x = v.tiles_x;
    a.sc = sc;
    a.r = F(q.r); a.z = F(q.z); a.p0 = F(q.p0); a.p1 = F(q.p1);
    const dim3 g(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID);

    VfPcg st = a;
    st.x_in = (const float*)(base + v.u0);
    st.x_out = (float*)(base + v.u1);
    st.part = D(1);
    st.change = change_bits;
    st.init = first ? 1 : 0;
    hipLaunchKernelGGL(vf_pcg_step_kernel, g, dim3(256), 0, s, st);
    TG_CHECK_LAUNCH("vf_pcg_step_kernel");

    const VfPre pre = {F(q.r), F(q.d), F(q.z)};
    if (int rc = vf_launch_cycle(p, base, &pre, nullptr, s)) return rc;

    VfPcg dt = a;
    dt.x_in = (const float*)(base + v.u1);
    dt.x_out = (float*)(base + v.u0);
    dt.part = D(2);
    hipLaunchKernelGGL(vf_pcg_dot_kernel, g, dim3(256), 0, s, dt);
    TG_CHECK_LAUNCH("vf_pcg_dot_kernel");
    hipLaunchKernelGGL((vf_pcg_scalar_kernel<true>), dim3(1), dim3(256), 0, s, sc, (const double*)D(2), (const double*)D(1),
                       v.tiles, first ? 1 : 0, (uint32_t*)nullptr);
    TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<beta>");

    VfPcg dr = a;
    dr.part = D(0);
    hipLaunchKernelGGL(vf_pcg_dir_kernel, g, dim3(256), 0, s, dr);
    TG_CHECK_LAUNCH("vf_pcg_dir_kernel");
    hipLaunchKernelGGL((vf_pcg_scalar_kernel<false>), dim3(1), dim3(256), 0, s, sc, (const double*)D(0), (const double*)nullptr,
                       v.tiles, 0, restarts);
    TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<alpha>");
    return TG_OK;
}

extern "C" int tg_vfill_pcg_start(int H, int W, void* ws, size_t ws_bytes, void* pws, size_t pws_bytes, tg_stream_t stream) {
    VfPlan p;
    VfPcgPlan q;
    if (int rc = vf_ws_check("tg_vfill_pcg_start", H, W, ws, ws_bytes, &p)) return rc;
    if (int rc = vf_pws_check("tg_vfill_pcg_start", p, pws, pws_bytes, &q)) return rc;
    const hipStream_t s = S(stream);
    // scalars, partials of the inactive tiles, and r, z, p and the down-pass scratch outside the active tiles start at 0
    if (hipMemsetAsync(pws, 0, q.bytes, s) != hipSuccess) {
        tg_set_error("tg_vfill_pcg_start: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    return vf_pcg_launch(p, q, (char*)ws, (char*)pws, true, nullptr, nullptr, s);
}

extern "C" int tg_vfill_pcg_iter(int H, int W, void* ws, size_t ws_bytes, void* pws, size_t pws_bytes, uint32_t* change_bits,
                                 uint32_t* restarts, tg_stream_t stream) {
    VfPlan p;
    VfPcgPlan q;
    if (int rc = vf_ws_check("tg_vfill_pcg_iter", H, W, ws, ws_bytes, &p)) return rc;
    if (int rc = vf_pws_check("tg_vfill_pcg_iter", p, pws, pws_bytes, &q)) return rc;
    TG_REQUIRE(change_bits && restarts, "tg_vfill_pcg_iter: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(change_bits, 0, sizeof(uint32_t), s) != hipSuccess) {
        tg_set_error("tg_vfill_pcg_iter: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    return vf_pcg_launch(p, q, (char*)ws, (char*)pws, false, change_bits, restarts, s);
}

// ---- biharmonic (thin-plate) fill (tg_vfill_bih_*) -------------------------------------------------
// Minimise sum_{p in S} D(u)_p^2 over the unknowns, D the masked difference sum above and S the unknowns with their
// 4-neighbours: A x = b with A = D(D(.)) restricted to the unknowns, symmetric positive definite.  Outer loop: the flexible
// conjugate gradients of section 8n with x, D(x), the residual and every dot product in fp64 (in fp32 the loop stalls above the
// stop rule), the direction p in fp32.  Preconditioner M r = G(G(r)): G is `inner` iterations of the same conjugate gradients
// around the V-cycle on -D(e) = f (e = 0 at the fixed cells) from e = 0, all fp32; inner = 1 is one bare cycle.  The outer
// passes stage a 36 x 68 patch (2-px halo) in LDS, form w = D(.) on its 34 x 66 interior and D(w) on the tile's unknowns: w
// never goes to memory, and the ring of S that lies in a neighbouring tile without an unknown is covered by the halo.
constexpr int VF_BY = VF_TY + 4, VF_BX = VF_TX + 4, VF_BXP = VF_BX + 1;
constexpr int VF_WY = VF_TY + 2, VF_WX = VF_TX + 2, VF_WXP = VF_WX + 1;

struct VfBih {
    const uint8_t* flags;
    const int32_t* list;      // nullptr on a one-level raster: the single tile 0
    const int32_t* count;
    int H, W, tiles_x;
    VfPcgScal* sc;
    const double* x_in;       // step: x (xa); dot: x' (xb)
    double* x_out;            // step: x' (xb); dot: xa
    double* r;
    float* rf;                // the residual in fp32: the preconditioner's input
    const float* z;
    float* p0;
    float* p1;
    float* u;                 // dot: x' in fp32, the buffer tg_vfill_finish reads
    double* part;
    uint32_t* change;
    int init;                 // step: alpha = 0 (the first residual)
};

struct VfBihLds {
    double x[VF_BY][VF_BXP];
    double w[VF_WY][VF_WXP];
    uint8_t f[VF_BY][VF_BXP];
    double red[4];
};

// w = D(x) on the patch's 34 x 66 interior (0 outside the raster)
__device__ __forceinline__ void vf_bih_lap(VfBihLds& s) {
    for (int j = threadIdx.x; j < VF_WY * VF_WX; j += 256) {
        const int r = j / VF_WX, c = j - r * VF_WX;
        const int ly = r + 1, lx = c + 1;
        double acc = 0.0;
        if (s.f[ly][lx] & VF_IN) {
            const double up = s.x[ly][lx];
            if (s.f[ly - 1][lx] & VF_IN) acc += s.x[ly - 1][lx] - up;
            if (s.f[ly + 1][lx] & VF_IN) acc += s.x[ly + 1][lx] - up;
            if (s.f[ly][lx - 1] & VF_IN) acc += s.x[ly][lx - 1] - up;
            if (s.f[ly][lx + 1] & VF_IN) acc += s.x[ly][lx + 1] - up;
        }
        s.w[r][c] = acc;
    }
    __syncthreads();
}

// D(w) at the tile cell (r, c), which is not fixed
__device__ __forceinline__ double vf_bih_lap2(const VfBihLds& s, int r, int c) {
    const int ly = r + 2, lx = c + 2, wy = r + 1, wx = c + 1;
    const double wp = s.w[wy][wx];
    double acc = 0.0;
    if (s.f[ly - 1][lx] & VF_IN) acc += s.w[wy - 1][wx] - wp;
    if (s.f[ly + 1][lx] & VF_IN) acc += s.w[wy + 1][wx] - wp;
    if (s.f[ly][lx - 1] & VF_IN) acc += s.w[wy][wx - 1] - wp;
    if (s.f[ly][lx + 1] & VF_IN) acc += s.w[wy][wx + 1] - wp;
    return acc;
}

__global__ __launch_bounds__(256) void vf_bih_init_kernel(const float* __restrict__ u, int64_t n, double* __restrict__ xa,
                                                          double* __restrict__ xb) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = (double)u[i];
        xa[i] = v;
        xb[i] = v;
    }
}

// x' = x + alpha p (halo included) -> x_out, r' = b - A x' = -D(D(x')) -> r and rf, the tile's r'.z_old, the largest |alpha p|
__global__ __launch_bounds__(256) void vf_bih_step_kernel(VfBih P) {
    __shared__ VfBihLds s;
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const double alpha = P.init ? 0.0 : (double)P.sc->alpha;
    const float* pin = P.sc->parity ? P.p1 : P.p0;
    uint32_t mx = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();                                          // the previous tile's readers are done
        for (int j = threadIdx.x; j < VF_BY * VF_BX; j += 256) {
            const int r = j / VF_BX, c = j - r * VF_BX;
            const int y = y0 - 2 + r, x = x0 - 2 + c;
            double v = 0.0;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                v = P.x_in[i];
                const bool inner = r >= 2 && r < VF_TY + 2 && c >= 2 && c < VF_TX + 2;
                if (!(fl & VF_FIX) && alpha != 0.0) {
                    const double d = alpha * (double)pin[i];
                    v += d;
                    if (inner) {
                        const uint32_t b = __float_as_uint(fabsf((float)d));
                        mx = b > mx ? b : mx;
                    }
                }
                if (inner) P.x_out[i] = v;
            }
            s.x[r][c] = v;
            s.f[r][c] = fl;
        }
        __syncthreads();
        vf_bih_lap(s);
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int64_t i = (int64_t)y * W + x;
            double acc = 0.0;
            if (!(s.f[r + 2][c + 2] & VF_FIX)) {
                acc = -vf_bih_lap2(s, r, c);
                sum += acc * (double)P.z[i];
            }
            P.r[i] = acc;
            P.rf[i] = (float)acc;
        }
        sum = vf_block_sum(sum, s.red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
    if (P.change) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t u = __shfl_xor(mx, o, 64);
            mx = u > mx ? u : mx;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0 && P.sc->restart) mx = 0x7f800000u;      // a skipped step is not convergence
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(P.change, mx);
    }
}

// the tile's r'.z'; x' moves from xb back to xa, and in fp32 to level 0's u0
__global__ __launch_bounds__(256) void vf_bih_dot_kernel(VfBih P) {
    __shared__ double red[4];
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int64_t i = (int64_t)y * W + x;
            sum += P.r[i] * (double)P.z[i];                       // r is 0 at the fixed cells
            const double v = P.x_in[i];
            P.x_out[i] = v;
            P.u[i] = (float)v;
        }
        sum = vf_block_sum(sum, red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
}

// p = z + beta p (halo included) -> the other p buffer, A p = D(D(p)) with p = 0 at the fixed cells, the tile's p.Ap
__global__ __launch_bounds__(256) void vf_bih_dir_kernel(VfBih P) {
    __shared__ VfBihLds s;
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const float beta = P.sc->beta;
    const bool par = P.sc->parity != 0;
    const float* pin = par ? P.p1 : P.p0;
    float* pout = par ? P.p0 : P.p1;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();
        for (int j = threadIdx.x; j < VF_BY * VF_BX; j += 256) {
            const int r = j / VF_BX, c = j - r * VF_BX;
            const int y = y0 - 2 + r, x = x0 - 2 + c;
            float v = 0.f;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                if (!(fl & VF_FIX)) {
                    v = P.z[i];
                    if (beta != 0.f) v = __fadd_rn(v, __fmul_rn(beta, pin[i]));    // fused
                }
                if (r >= 2 && r < VF_TY + 2 && c >= 2 && c < VF_TX + 2) pout[i] = v;
            }
            s.x[r][c] = (double)v;
            s.f[r][c] = fl;
        }
        __syncthreads();
        vf_bih_lap(s);
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            if (s.f[r + 2][c + 2] & VF_FIX) continue;
            sum += s.x[r + 2][c + 2] * vf_bih_lap2(s, r, c);
        }
        sum = vf_block_sum(sum, s.red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
}

// The inner solve G: the passes of section 8n with a right-hand side from an array and 0 at the fixed cells.  Its dot and
// direction passes are vf_pcg_dot_kernel and vf_pcg_dir_kernel as they stand; the step and the last update are these two.
struct VfRhs {
    const uint8_t* flags;
    const int32_t* list;
    const int32_t* count;
    int H, W, tiles_x;
    const VfPcgScal* sc;
    const float* rhs;
    const float* e_in;        // nullptr: e = 0 (the first step of a solve)
    float* e_out;
    float* r;
    const float* z;
    const float* p0;
    const float* p1;
    double* part;
};

// e' = e + alpha p (halo included) -> e_out, r' = f + D(e') -> r, the tile's r'.z_old
__global__ __launch_bounds__(256) void vf_rhs_step_kernel(VfRhs P) {
    __shared__ float sx[VF_PY][VF_PXP];
    __shared__ uint8_t sf[VF_PY][VF_PXP];
    __shared__ double red[4];
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const float alpha = P.sc->alpha;
    const float* pin = P.sc->parity ? P.p1 : P.p0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        __syncthreads();                                          // the previous tile's readers are done
        for (int j = threadIdx.x; j < VF_PY * VF_PX; j += 256) {
            const int r = j / VF_PX, c = j - r * VF_PX;
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float v = 0.f;
            uint8_t fl = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                fl = VF_IN | P.flags[i];
                if (!(fl & VF_FIX)) {
                    if (P.e_in) v = P.e_in[i];
                    if (alpha != 0.f) v = __fadd_rn(v, __fmul_rn(alpha, pin[i]));    // fused
                }
                if (r >= 1 && r <= VF_TY && c >= 1 && c <= VF_TX) P.e_out[i] = v;
            }
            sx[r][c] = v;
            sf[r][c] = fl;
        }
        __syncthreads();
        double sum = 0.0;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int ly = r + 1, lx = c + 1;
            const int64_t i = (int64_t)y * W + x;
            float acc = 0.f;
            if (!(sf[ly][lx] & VF_FIX)) {
                const float up = sx[ly][lx];
                acc = P.rhs[i];
                if (sf[ly - 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly - 1][lx], up));
                if (sf[ly + 1][lx] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly + 1][lx], up));
                if (sf[ly][lx - 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly][lx - 1], up));
                if (sf[ly][lx + 1] & VF_IN) acc = __fadd_rn(acc, __fsub_rn(sx[ly][lx + 1], up));
                sum += (double)acc * (double)P.z[i];
            }
            P.r[i] = acc;
        }
        sum = vf_block_sum(sum, red);
        if (threadIdx.x == 0) P.part[tile] = sum;
    }
}

// the last update of a solve: e + alpha p -> e_out on the active tiles (no residual follows)
__global__ __launch_bounds__(256) void vf_rhs_final_kernel(VfRhs P) {
    const int H = P.H, W = P.W;
    const int ntiles = P.list ? *P.count : 1;
    const float alpha = P.sc->alpha;
    const float* pin = P.sc->parity ? P.p1 : P.p0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tile = P.list ? P.list[t] : 0;
        const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
        const int y0 = ty * VF_TY, x0 = tx * VF_TX;
        for (int j = threadIdx.x; j < VF_TY * VF_TX; j += 256) {
            const int r = j / VF_TX, c = j - r * VF_TX;
            const int y = y0 + r, x = x0 + c;
            if (y >= H || x >= W) continue;
            const int64_t i = (int64_t)y * W + x;
            float v = 0.f;
            if (!(P.flags[i] & VF_FIX)) {
                if (P.e_in) v = P.e_in[i];
                if (alpha != 0.f) v = __fadd_rn(v, __fmul_rn(alpha, pin[i]));    // fused
            }
            P.e_out[i] = v;
        }
    }
}

__global__ void vf_bih_restarts_kernel(const VfPcgScal* outer, const VfPcgScal* inner, uint32_t* restarts) {
    *restarts = outer->restarts + inner->restarts;
}

// the third workspace (mirrored by vfill_bih_layout in mvp_gan/src/fill_voids.py)
enum { VF_BIH_F64 = 3, VF_BIH_F32 = 12, VF_BIH_PARTS = 6 };
struct VfBihPlan {
    size_t sc_out, sc_in;
    size_t xa, xb, r;                              // fp64
    size_t rf, t, z, p0, p1;                       // fp32, outer
    size_t e0, e1, ri, zi, q0, q1, d;              // fp32, the inner solve
    size_t part[VF_BIH_PARTS];                     // outer p.Ap, r'.z, r'.z', then the inner solve's
    size_t bytes;
};

static void vf_bih_plan(const VfPlan& p, VfBihPlan* q) {
    const size_t n = (size_t)p.lv[0].H * p.lv[0].W;
    size_t off = 0;
    q->sc_out = off; off += VF_ALIGN;
    q->sc_in = off; off += VF_ALIGN;
    size_t* f64[VF_BIH_F64] = {&q->xa, &q->xb, &q->r};
    for (size_t* o : f64) { *o = off; off += al(n * 8); }
    size_t* f32[VF_BIH_F32] = {&q->rf, &q->t, &q->z, &q->p0, &q->p1, &q->e0, &q->e1, &q->ri, &q->zi, &q->q0, &q->q1, &q->d};
    for (size_t* o : f32) { *o = off; off += al(n * 4); }
    for (int k = 0; k < VF_BIH_PARTS; ++k) { q->part[k] = off; off += al((size_t)p.lv[0].tiles * 8); }
    q->bytes = off;
}

static int vf_bws_check(const char* who, const VfPlan& p, const void* bws, size_t bws_bytes, int inner, VfBihPlan* q) {
    TG_REQUIRE(bws, "%s: null pointer", who);
    TG_REQUIRE(((uintptr_t)bws & (VF_ALIGN - 1)) == 0, "%s: biharmonic workspace must be %d-byte aligned", who, VF_ALIGN);
    TG_REQUIRE(inner >= 1 && inner <= TG_VFILL_BIH_MAX_INNER, "%s: inner %d must be in 1..%d", who, inner, TG_VFILL_BIH_MAX_INNER);
    vf_bih_plan(p, q);
    if (bws_bytes < q->bytes) {
        tg_set_error("%s: biharmonic workspace %zu bytes < %zu", who, bws_bytes, q->bytes);
        return TG_ERR_WS;
    }
    return TG_OK;
}

extern "C" size_t tg_vfill_bih_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    VfPlan p;
    VfBihPlan q;
    vf_plan(H, W, &p);
    vf_bih_plan(p, &q);
    return q.bytes;
}

// out = G(f): `inner` cycles
static int vf_bih_solve(const VfPlan& p, const VfBihPlan& q, char* base, char* bb, const float* f, float* out, int inner,
                        hipStream_t s) {
    const VfLevel& v = p.lv[0];
    VfHdr* hdr = (VfHdr*)base;
    auto F = [&](size_t off) { return (float*)(bb + off); };
    auto D = [&](int k) { return (double*)(bb + q.part[3 + k]); };
    if (inner == 1) {
        const VfPre pre = {f, F(q.d), out};
        return vf_launch_cycle(p, base, &pre, nullptr, s);
    }
    VfPcgScal* sc = (VfPcgScal*)(bb + q.sc_in);
    const dim3 g(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID);
    VfPcg a = {};
    a.flags = (const uint8_t*)(base + v.flags);
    a.list = p.L > 1 ? (const int32_t*)(base + v.list) : nullptr;
    a.count = &hdr->ntiles[0];
    a.H = v.H; a.W = v.W; a.tiles_x = v.tiles_x;
    a.sc = sc;
    a.z = F(q.zi); a.p0 = F(q.q0); a.p1 = F(q.q1);
    VfRhs b = {};
    b.flags = a.flags; b.list = a.list; b.count = a.count;
    b.H = v.H; b.W = v.W; b.tiles_x = v.tiles_x;
    b.sc = sc;
    b.rhs = f;
    b.z = F(q.zi); b.p0 = F(q.q0); b.p1 = F(q.q1);
    for (int k = 0; k < inner; ++k) {
        const float* r = f;                                       // the residual of e = 0
        if (k > 0) {
            VfRhs st = b;
            st.e_in = k > 1 ? F(q.e0) : nullptr;
            st.e_out = F(q.e1);
            st.r = F(q.ri);
            st.part = D(1);
            hipLaunchKernelGGL(vf_rhs_step_kernel, g, dim3(256), 0, s, st);
            TG_CHECK_LAUNCH("vf_rhs_step_kernel");
            r = F(q.ri);
        }
        const VfPre pre = {r, F(q.d), F(q.zi)};
        if (int rc = vf_launch_cycle(p, base, &pre, nullptr, s)) return rc;
        VfPcg dt = a;
        dt.r = (float*)r;                                         // read only
        dt.x_in = k > 0 ? F(q.e1) : F(q.e0);                      // k = 0: e0 onto itself, whatever it holds
        dt.x_out = F(q.e0);
        dt.part = D(2);
        hipLaunchKernelGGL(vf_pcg_dot_kernel, g, dim3(256), 0, s, dt);
        TG_CHECK_LAUNCH("vf_pcg_dot_kernel");
        hipLaunchKernelGGL((vf_pcg_scalar_kernel<true>), dim3(1), dim3(256), 0, s, sc, (const double*)D(2), (const double*)D(1),
                           v.tiles, k == 0 ? 1 : 0, (uint32_t*)nullptr);
        TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<beta>");
        VfPcg dr = a;
        dr.part = D(0);
        hipLaunchKernelGGL(vf_pcg_dir_kernel, g, dim3(256), 0, s, dr);
        TG_CHECK_LAUNCH("vf_pcg_dir_kernel");
        hipLaunchKernelGGL((vf_pcg_scalar_kernel<false>), dim3(1), dim3(256), 0, s, sc, (const double*)D(0),
                           (const double*)nullptr, v.tiles, 0, (uint32_t*)nullptr);
        TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<alpha>");
    }
    VfRhs fn = b;
    fn.e_in = inner > 1 ? F(q.e0) : nullptr;
    fn.e_out = out;
    hipLaunchKernelGGL(vf_rhs_final_kernel, g, dim3(256), 0, s, fn);
    TG_CHECK_LAUNCH("vf_rhs_final_kernel");
    return TG_OK;
}

// step (or the first residual), z = G(G(r)), r.z, beta, the new direction and p.Ap, alpha
static int vf_bih_launch(const VfPlan& p, const VfBihPlan& q, char* base, char* bb, bool first, int inner,
                         uint32_t* change_bits, uint32_t* restarts, hipStream_t s) {
    const VfLevel& v = p.lv[0];
    VfHdr* hdr = (VfHdr*)base;
    VfPcgScal* sc = (VfPcgScal*)(bb + q.sc_out);
    auto F = [&](size_t off) { return (float*)(bb + off); };
    auto D = [&](int k) { return (double*)(bb + q.part[k]); };
    VfBih a = {};
    a.flags = (const uint8_t*)(base + v.flags);
    a.list = p.L > 1 ? (const int32_t*)(base + v.list) : nullptr;
    a.count = &hdr->ntiles[0];
    a.H = v.H; a.W = v.W; a.tiles_x = v.tiles_x;
    a.sc = sc;
    a.r = (double*)(bb + q.r); a.rf = F(q.rf); a.z = F(q.z); a.p0 = F(q.p0); a.p1 = F(q.p1);
    a.u = (float*)(base + v.u0);
    const dim3 g(v.tiles < VF_MAX_GRID ? v.tiles : VF_MAX_GRID);

    VfBih st = a;
    st.x_in = (const double*)(bb + q.xa);
    st.x_out = (double*)(bb + q.xb);
    st.part = D(1);
    st.change = change_bits;
    st.init = first ? 1 : 0;
    hipLaunchKernelGGL(vf_bih_step_kernel, g, dim3(256), 0, s, st);
    TG_CHECK_LAUNCH("vf_bih_step_kernel");

    if (int rc = vf_bih_solve(p, q, base, bb, F(q.rf), F(q.t), inner, s)) return rc;
    if (int rc = vf_bih_solve(p, q, base, bb, F(q.t), F(q.z), inner, s)) return rc;

    VfBih dt = a;
    dt.x_in = (const double*)(bb + q.xb);
    dt.x_out = (double*)(bb + q.xa);
    dt.part = D(2);
    hipLaunchKernelGGL(vf_bih_dot_kernel, g, dim3(256), 0, s, dt);
    TG_CHECK_LAUNCH("vf_bih_dot_kernel");
    hipLaunchKernelGGL((vf_pcg_scalar_kernel<true>), dim3(1), dim3(256), 0, s, sc, (const double*)D(2), (const double*)D(1),
                       v.tiles, first ? 1 : 0, (uint32_t*)nullptr);
    TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<beta>");

    VfBih dr = a;
    dr.part = D(0);
    hipLaunchKernelGGL(vf_bih_dir_kernel, g, dim3(256), 0, s, dr);
    TG_CHECK_LAUNCH("vf_bih_dir_kernel");
    hipLaunchKernelGGL((vf_pcg_scalar_kernel<false>), dim3(1), dim3(256), 0, s, sc, (const double*)D(0), (const double*)nullptr,
                       v.tiles, 0, (uint32_t*)nullptr);
    TG_CHECK_LAUNCH("vf_pcg_scalar_kernel<alpha>");
    if (restarts) {
        hipLaunchKernelGGL(vf_bih_restarts_kernel, dim3(1), dim3(1), 0, s, (const VfPcgScal*)sc,
                           (const VfPcgScal*)(bb + q.sc_in), restarts);
        TG_CHECK_LAUNCH("vf_bih_restarts_kernel");
    }
    return TG_OK;
}

extern "C" int tg_vfill_bih_start(int H, int W, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, int inner,
                                  tg_stream_t stream) {
    VfPlan p;
    VfBihPlan q;
    if (int rc = vf_ws_check("tg_vfill_bih_start", H, W, ws, ws_bytes, &p)) return rc;
    if (int rc = vf_bws_check("tg_vfill_bih_start", p, bws, bws_bytes, inner, &q)) return rc;
    const hipStream_t s = S(stream);
    // scalars, partials of the inactive tiles, and every fp32 vector outside the active tiles start at 0
    if (hipMemsetAsync(bws, 0, q.bytes, s) != hipSuccess) {
        tg_set_error("tg_vfill_bih_start: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t n = (int64_t)H * W;
    char* bb = (char*)bws;
    hipLaunchKernelGGL(vf_bih_init_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, (const float*)((char*)ws + p.lv[0].u0), n,
                       (double*)(bb + q.xa), (double*)(bb + q.xb));
    TG_CHECK_LAUNCH("vf_bih_init_kernel");
    return vf_bih_launch(p, q, (char*)ws, bb, true, inner, nullptr, nullptr, s);
}

extern "C" int tg_vfill_bih_iter(int H, int W, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, int inner,
                                 uint32_t* change_bits, uint32_t* restarts, tg_stream_t stream) {
    VfPlan p;
    VfBihPlan q;
    if (int rc = vf_ws_check("tg_vfill_bih_iter", H, W, ws, ws_bytes, &p)) return rc;
    if (int rc = vf_bws_check("tg_vfill_bih_iter", p, bws, bws_bytes, inner, &q)) return rc;
    TG_REQUIRE(change_bits && restarts, "tg_vfill_bih_iter: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(change_bits, 0, sizeof(uint32_t), s) != hipSuccess) {
        tg_set_error("tg_vfill_bih_iter: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    return vf_bih_launch(p, q, (char*)ws, (char*)bws, false, inner, change_bits, restarts, s);
}
