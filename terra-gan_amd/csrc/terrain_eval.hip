// Held-out terrain errors of an inpainted raster (mvp_gan/src/evaluate_raster.py).
//
//   tg_eval_holes             evaluation holes and keep mask of a band of cell rows: one thread per pixel, integer counters
//   tg_hole_table             one table row per hole (component root), slot map root -> row
//   tg_terrain_errors         one pass over 32 x 64 tiles of z and p staged in LDS with a 1-px halo: height, slope, gradient
//                             and Laplacian errors as per-workgroup fp64 partials, integer counters, per-hole integer atomics,
//                             and the two selection buffers
//   tg_terrain_errors_finish  one workgroup reduces the partials in a fixed order
//   tg_select_f32             exact k-th smallest by a radix select on the float bits (11 + 11 + 10), LDS histograms
//
// Determinism: no floating-point atomics.  Every thread accumulates its pixels in a fixed order (the grid is a function of the
// shape), the wave and workgroup reductions are fixed trees, and counts, maxima (on the bits of non-negative floats), bboxes
// and fixed-point per-hole sums use integer atomics.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

typedef unsigned long long ull;

// ---- evaluation holes ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_holes_kernel(const float* __restrict__ dem, const float* __restrict__ mask,
                                                         int use_nodata, float nodata, const uint8_t* __restrict__ objects,
                                                         const float* __restrict__ cell_masks, const int32_t* __restrict__ cell_of,
                                                         const uint8_t* __restrict__ hole_in, int H, int W, int tile, int row0,
                                                         int row1, uint8_t* __restrict__ holes, float* __restrict__ keep,
                                                         int64_t* __restrict__ counts) {
    __shared__ int red[4][3];
    const int ncx = (W + tile - 1) / tile;
    const int64_t base = (int64_t)row0 * W, n = (int64_t)(row1 - row0) * W;
    int nv = 0, nh = 0, no = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int64_t i = base + j;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        const float z = dem[i];
        bool v = isfinite(z);
        if (mask) v = v && mask[i] != 0.f;
        if (use_nodata) v = v && z != nodata;
        const bool o = objects && objects[i];
        bool h = hole_in && hole_in[i];
        if (cell_of) {
            const int cy = y / tile, cx = x / tile;
            const int k = cell_of[(int64_t)cy * ncx + cx];
            if (k >= 0) h = h || cell_masks[((int64_t)k * tile + (y - cy * tile)) * tile + (x - cx * tile)] == 0.f;
        }
        const bool hol = v && h && !o;
        holes[i] = hol;
        keep[i] = (v && !h && !o) ? 1.f : 0.f;
        nv += v;
        nh += hol;
        no += v && o;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        nv += __shfl_xor(nv, s, 64); nh += __shfl_xor(nh, s, 64); no += __shfl_xor(no, s, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = nv; red[w][1] = nh; red[w][2] = no; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<ull*>(&counts[threadIdx.x]), (ull)v);
    }
}

// ---- hole table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hole_table_kernel(const int32_t* __restrict__ labels, const int32_t* area, int H, int W,
                                                         int32_t* slot, int64_t* __restrict__ table, int cap,
                                                         int32_t* __restrict__ count) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (labels[i] != (int32_t)i) continue;
        const int64_t a = area[i];                  // read before slot[i] is written: the two may alias
        const int s = atomicAdd(count, 1);
        slot[i] = s;
        if (s >= cap) continue;
        const int64_t y = i / W, x = i - y * W;
        int64_t* r = table + (int64_t)s * TG_HOLE_COLS;
        r[0] = i; r[1] = a; r[2] = 0; r[3] = 0; r[4] = 0;
        r[5] = y; r[6] = x; r[7] = y; r[8] = x;
    }
}

// ---- terrain errors -----------------------------------------------------------------------------------------------------
constexpr int TE_TY = 32, TE_TX = 64;     // output tile: 4 waves x 8 rows, lane = column
constexpr int TE_SX = 72;                 // LDS row stride of the haloed tile (66 used; rows 8 banks apart)
constexpr int TE_SY = TE_TY + 2;
constexpr int TE_MAX_GRID = 2048;
constexpr double TE_FIX = 65536.0;        // 2^16: fixed-point scale of the per-hole sums
constexpr float TE_CLAMP = 32768.f;       // 2^15 m
enum { F_VALID = 1, F_KEEP = 2, F_PFIN = 4 };

static int te_grid(int H, int W) {
    const int64_t tiles = (int64_t)cdiv(H, TE_TY) * cdiv(W, TE_TX);
    return (int)(tiles < TE_MAX_GRID ? tiles : TE_MAX_GRID);
}

struct Horn {
    double gx, gy, lap;
};

// Horn's 3x3 gradient and the 5-point Laplacian at LDS (ly, lx), in fp64 from the fp32 values.  No contraction into fused
// multiply-adds: the two calls (z and p) must round alike, so that p == z gives errors of exactly 0.
__device__ __forceinline__ Horn horn(const float (*s)[TE_SX], int ly, int lx, double inv8c, double invc2) {
#pragma clang fp contract(off)
    const double a = s[ly - 1][lx - 1], b = s[ly - 1][lx], c = s[ly - 1][lx + 1];
    const double d = s[ly][lx - 1], e = s[ly][lx], f = s[ly][lx + 1];
    const double g = s[ly + 1][lx - 1], h = s[ly + 1][lx], k = s[ly + 1][lx + 1];
    Horn o;
    o.gx = ((c + 2.0 * f + k) - (a + 2.0 * d + g)) * inv8c;
    o.gy = ((g + 2.0 * h + k) - (a + 2.0 * b + c)) * inv8c;
    o.lap = (b + h + d + f - 4.0 * e) * invc2;
    return o;
}

struct TeArgs {
    const float* z;
    const float* p;
    const float* mask;
    int use_nodata;
    float nodata;
    const uint8_t* holes;
    const float* keep;
    const int32_t* labels;
    const int32_t* slot;
    int64_t* table;
    int nholes, H, W, tiles_x, ntiles;
    double inv8c, invc2;
    TgAreaClasses cls;
    int64_t* counts;
    float* sel_a;
    float* sel_s;
    double* partials;
};

__global__ __launch_bounds__(256) void terrain_errors_kernel(TeArgs A) {
    __shared__ float sz[TE_SY][TE_SX], sp[TE_SY][TE_SX];
    __shared__ uint8_t sf[TE_SY][TE_SX];
    __shared__ double dred[4][TG_TE_NSUM];
    __shared__ int64_t ired[4][TG_TE_NCOUNT];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int H = A.H, W = A.W;
    double acc[TG_TE_NSUM];
#pragma unroll
    for (int s = 0; s < TG_TE_NSUM; ++s) acc[s] = 0.0;
    int nv = 0, nh = 0, no = 0, ns = 0, nu = 0, nr = 0, nt = 0, nrt = 0, ncl = 0;
    uint32_t mx = 0;

    for (int t = blockIdx.x; t < A.ntiles; t += gridDim.x) {
        const int ty = t / A.tiles_x, tx = t - ty * A.tiles_x;
        const int y0 = ty * TE_TY, x0 = tx * TE_TX;
        __syncthreads();                                           // the previous tile's readers are done
        for (int j = threadIdx.x; j < TE_SY * (TE_TX + 2); j += 256) {
            const int r = j / (TE_TX + 2), c = j - r * (TE_TX + 2);
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float zv = 0.f, pv = 0.f;
            uint8_t f = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const int64_t i = (int64_t)y * W + x;
                zv = A.z[i];
                pv = A.p[i];
                bool v = isfinite(zv);
                if (A.mask) v = v && A.mask[i] != 0.f;
                if (A.use_nodata) v = v && zv != A.nodata;
                f = (v ? F_VALID : 0) | (A.keep[i] != 0.f ? F_KEEP : 0) | (isfinite(pv) ? F_PFIN : 0);
            }
            sz[r][c] = zv;
            sp[r][c] = pv;
            sf[r][c] = f;
        }
        __syncthreads();
        // a thread walks 8 rows of one column: per-hole atomics once per run of equal slots
        const int x = x0 + lane;
        int cur = -1;
        ull r_sc = 0, r_sum = 0;
        uint32_t r_mx = 0;
        int r_y1 = 0;
        auto flush = [&]() {
            if (cur < 0) return;
            ull* row = reinterpret_cast<ull*>(A.table + (int64_t)cur * TG_HOLE_COLS);
            if (r_sc) {
                atomicAdd(&row[2], r_sc);
                atomicAdd(&row[3], r_sum);
                atomicMax(&row[4], (ull)r_mx);
            }
            atomicMin(&row[6], (ull)x);
            atomicMax(&row[7], (ull)r_y1);
            atomicMax(&row[8], (ull)x);
        };
        for (int k = 0; k < 8; ++k) {
            const int r = w * 8 + k, y = y0 + r;
            if (y >= H || x >= W) continue;
            const int64_t i = (int64_t)y * W + x;
            const int ly = r + 1, lx = lane + 1;
            const uint8_t f = sf[ly][lx];
            const bool v = f & F_VALID, hol = A.holes[i] != 0;
            nv += v;
            float sa = __int_as_float(0x7fc00000), ss = __int_as_float(0x7fc00000);
            if (!hol) {
                no += v && !(f & F_KEEP);
            } else {
                ++nh;
                const int s = A.slot[A.labels[i]];
                const bool ok = s >= 0 && s < A.nholes;              // always, for a table built from these labels
                if (ok && s != cur) {
                    flush();
                    cur = s; r_sc = 0; r_sum = 0; r_mx = 0;
                }
                if (ok) r_y1 = y;
                if (!(f & F_PFIN)) {
                    ++nu;
                } else {
                    ++ns;
                    const float zc = sz[ly][lx], pc = sp[ly][lx];
                    const float e = __fsub_rn(pc, zc), a = fabsf(e);
                    sa = a;
                    const double ad = a, a2 = ad * ad;
                    acc[TG_TE_S_E] += (double)e;
                    acc[TG_TE_S_A] += ad;
                    acc[TG_TE_S_A2] += a2;
                    const uint32_t ab = __float_as_uint(a);
                    mx = ab > mx ? ab : mx;
                    if (ok) {
                        ++r_sc;
                        ncl += a > TE_CLAMP;
                        r_sum += (ull)__double2ll_rn((double)fminf(a, TE_CLAMP) * TE_FIX);
                        r_mx = ab > r_mx ? ab : r_mx;
                        const int64_t area = A.table[(int64_t)s * TG_HOLE_COLS + 1];
                        int c = 0;
                        for (int e2 = 0; e2 < A.cls.n_edges; ++e2) c += area >= A.cls.px[e2];
#pragma unroll
                        for (int q = 0; q < TG_EVAL_MAX_CLASSES; ++q) {
                            if (q == c) {
                                acc[TG_TE_CLASS + 2 * q] += ad;
                                acc[TG_TE_CLASS + 2 * q + 1] += a2;
                            }
                        }
                    }
                    uint8_t nb_and = 0xff, nb_or = 0;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const uint8_t g = sf[ly + dy][lx + dx];
                            nb_and &= g;
                            if (dy || dx) nb_or |= g;
                        }
                    const bool ring = nb_or & F_KEEP;
                    const bool slope = (nb_and & (F_VALID | F_PFIN)) == (F_VALID | F_PFIN);
                    if (ring) {
                        ++nr;
                        acc[TG_TE_R_A] += ad;
                        acc[TG_TE_R_A2] += a2;
                    }
                    if (slope) {
#pragma clang fp contract(off)
                        ++nt;
                        const Horn hz = horn(sz, ly, lx, A.inv8c, A.invc2), hp = horn(sp, ly, lx, A.inv8c, A.invc2);
                        const double rad2deg = 57.29577951308232;
                        const double sl_z = atan(hypot(hz.gx, hz.gy)) * rad2deg, sl_p = atan(hypot(hp.gx, hp.gy)) * rad2deg;
                        const double ds = sl_p - sl_z, dgx = hp.gx - hz.gx, dgy = hp.gy - hz.gy, dl = hp.lap - hz.lap;
                        const double dg2 = dgx * dgx + dgy * dgy;
                        acc[TG_TE_T_DS] += fabs(ds);
                        acc[TG_TE_T_DS2] += ds * ds;
                        acc[TG_TE_T_DG2] += dg2;
                        acc[TG_TE_T_DL2] += dl * dl;
                        ss = (float)fabs(ds);
                        if (ring) {
                            ++nrt;
                            acc[TG_TE_RT_DG2] += dg2;
                        }
                    }
                }
            }
            A.sel_a[i] = sa;
            A.sel_s[i] = ss;
        }
        flush();
    }

    // workgroup reduction in a fixed order: xor butterflies inside the waves, then waves 0..3
#pragma unroll
    for (int s = 0; s < TG_TE_NSUM; ++s) {
        const double v = wave_sum_d(acc[s]);
        if (lane == 0) dred[w][s] = v;
    }
    int64_t cnt[TG_TE_NCOUNT] = {nv, nh, no, ns, nu, nr, nt, nrt, ncl, 0};
#pragma unroll
    for (int s = 0; s < TG_TE_MAX_BITS; ++s) {
        int v = (int)cnt[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) ired[w][s] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(mx, o, 64);
        mx = u > mx ? u : mx;
    }
    if (lane == 0) ired[w][TG_TE_MAX_BITS] = mx;
    __syncthreads();
    if (threadIdx.x < TG_TE_NSUM) {
        const int s = threadIdx.x;
        A.partials[(int64_t)blockIdx.x * TG_TE_NSUM + s] = ((dred[0][s] + dred[1][s]) + dred[2][s]) + dred[3][s];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + TG_TE_NCOUNT) {
        const int s = threadIdx.x - 64;
        ull* c = reinterpret_cast<ull*>(A.counts);
        if (s == TG_TE_MAX_BITS) {
            ull m = 0;
            for (int q = 0; q < 4; ++q) m = (ull)ired[q][s] > m ? (ull)ired[q][s] : m;
            if (m) atomicMax(&c[s], m);
        } else {
            const ull v = (ull)(ired[0][s] + ired[1][s] + ired[2][s] + ired[3][s]);
            if (v) atomicAdd(&c[s], v);
        }
    }
}

__global__ __launch_bounds__(256) void terrain_errors_finish_kernel(const double* __restrict__ partials, int nwg,
                                                                    double* __restrict__ sums) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = 0; s < TG_TE_NSUM; ++s) {
        double v = 0.0;
        for (int g = threadIdx.x; g < nwg; g += 256) v += partials[(int64_t)g * TG_TE_NSUM + s];
        v = wave_sum_d(v);
        if (lane == 0) red[w] = v;
        __syncthreads();
        if (threadIdx.x == 0) sums[s] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// ---- exact selection ----------------------------------------------------------------------------------------------------
// Digits of the bits b <= 0x7f800000: pass 0 b >> 21, pass 1 (b >> 10) & 2047, pass 2 b & 1023.  Pass 0 builds one histogram
// for all k; passes 1 and 2 one per k over the values that share its prefix so far.
constexpr int SEL_BINS = 2048;
constexpr uint32_t SEL_MAX_BITS = 0x7f800000u;     // +inf; larger: NaN or negative (sign bit)

struct SelState {
    uint32_t prefix, rank, valid, _pad;
};

__device__ __forceinline__ int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }

__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ v, int64_t n, int pass, int nk,
                                                          const SelState* __restrict__ st, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t lh[];                    // [rows][SEL_BINS]
    const int rows = pass == 0 ? 1 : nk;
    for (int j = threadIdx.x; j < rows * SEL_BINS; j += 256) lh[j] = 0;
    const int sh = sel_shift(pass), hi = pass > 0 ? sel_shift(pass - 1) : 0;
    const uint32_t dmask = pass == 2 ? 1023u : 2047u;
    uint32_t pre[TG_SELECT_MAX_K];
    bool ok[TG_SELECT_MAX_K];
#pragma unroll
    for (int k = 0; k < TG_SELECT_MAX_K; ++k) {
        ok[k] = pass > 0 && k < nk && st[k].valid;
        pre[k] = ok[k] ? st[k].prefix >> hi : 0u;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t b = __float_as_uint(v[i]);
        if (b > SEL_MAX_BITS) continue;
        const uint32_t d = (b >> sh) & dmask;
        if (pass == 0) {
            atomicAdd(&lh[d], 1u);
        } else {
#pragma unroll
            for (int k = 0; k < TG_SELECT_MAX_K; ++k)
                if (ok[k] && (b >> hi) == pre[k]) atomicAdd(&lh[k * SEL_BINS + d], 1u);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < rows * SEL_BINS; j += 256)
        if (lh[j]) atomicAdd(&hist[j], lh[j]);
}

// one workgroup: per k, the digit whose cumulative count passes the rank; hist rows are left for the caller to clear
__global__ __launch_bounds__(256) void select_scan_kernel(int pass, int nk, const int64_t* __restrict__ ks,
                                                          SelState* __restrict__ st, const uint32_t* __restrict__ hist,
                                                          float* __restrict__ out) {
    __shared__ uint32_t wtot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int PER = SEL_BINS / 256;
    for (int k = 0; k < nk; ++k) {
        // the state of k is read before the first barrier and written after the second: no thread sees it half-updated
        SelState s = st[k];
        if (pass == 0) {
            const int64_t kk = ks[k];
            s.prefix = 0;
            s.rank = kk >= 0 && kk < ((int64_t)1 << 31) ? (uint32_t)kk : 0u;
            s.valid = kk >= 0 && kk < ((int64_t)1 << 31);
        }
        const uint32_t* h = hist + (pass == 0 ? 0 : k) * SEL_BINS;
        uint32_t loc[PER], sum = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) { loc[q] = h[threadIdx.x * PER + q]; sum += loc[q]; }
        uint32_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[w] = inc;
        __syncthreads();
        uint32_t before = 0;
        for (int q = 0; q < w; ++q) before += wtot[q];
        const uint32_t total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        if (pass == 0 && s.rank >= total) s.valid = 0;       // k past the number of values
        __syncthreads();                                      // every thread has read st[k] and wtot
        const uint32_t excl = before + inc - sum;
        if (!s.valid) {
            if (threadIdx.x == 0) {
                st[k] = s;
                if (pass == 2) out[k] = __uint_as_float(0x7fc00000u);
            }
        } else if (s.rank >= excl && s.rank < excl + sum) {  // exactly one thread
            uint32_t r = s.rank - excl;
            int d = threadIdx.x * PER;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                if (r >= loc[q] && d == threadIdx.x * PER + q) { r -= loc[q]; ++d; }
            }
            s.prefix |= (uint32_t)d << sel_shift(pass);
            s.rank = r;
            st[k] = s;
            if (pass == 2) out[k] = __uint_as_float(s.prefix);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int size_check(const char* who, int H, int W) {
    TG_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: raster %dx%d must be non-empty with H*W < 2^31", who,
               H, W);
    return TG_OK;
}

static int memset_async(void* p, size_t bytes, hipStream_t s, const char* who) {
    if (hipMemsetAsync(p, 0, bytes, s) != hipSuccess) {
        tg_set_error("%s: hipMemsetAsync failed", who);
        return TG_ERR_LAUNCH;
    }
    return TG_OK;
}

extern "C" int tg_eval_holes(const float* dem, const float* mask, int use_nodata, float nodata, const uint8_t* objects,
                             const float* cell_masks, const int32_t* cell_of, const uint8_t* hole_in, int H, int W, int tile,
                             int row0, int row1, uint8_t* holes, float* keep, int64_t* counts, tg_stream_t stream) {
    if (int rc = size_check("tg_eval_holes", H, W)) return rc;
    TG_REQUIRE(dem && holes && keep && counts, "tg_eval_holes: null pointer");
    TG_REQUIRE(tile >= 1 && tile <= 1024, "tg_eval_holes: tile %d out of range [1, 1024]", tile);
    TG_REQUIRE(!cell_of || cell_masks, "tg_eval_holes: cell_of without cell_masks");
    TG_REQUIRE(row0 >= 0 && row0 < row1 && row1 <= H && row0 % tile == 0,
               "tg_eval_holes: rows [%d, %d) must lie in [0, %d) and start at a multiple of the tile %d", row0, row1, H, tile);
    const int grid = ew_grid((int64_t)(row1 - row0) * W, 256);
    hipLaunchKernelGGL(eval_holes_kernel, dim3(grid), dim3(256), 0, S(stream), dem, mask, use_nodata, nodata, objects, cell_masks,
                       cell_of, hole_in, H, W, tile, row0, row1, holes, keep, counts);
    TG_CHECK_LAUNCH("eval_holes_kernel");
    return TG_OK;
}

extern "C" int tg_hole_table(const int32_t* labels, const int32_t* area, int H, int W, int32_t* slot, int64_t* table, int cap,
                             int32_t* count, tg_stream_t stream) {
    if (int rc = size_check("tg_hole_table", H, W)) return rc;
    TG_REQUIRE(labels && area && slot && count && (table || cap == 0), "tg_hole_table: null pointer");
    TG_REQUIRE(cap >= 0, "tg_hole_table: cap %d < 0", cap);
    if (int rc = memset_async(count, sizeof(int32_t), S(stream), "tg_hole_table")) return rc;
    hipLaunchKernelGGL(hole_table_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, S(stream), labels, area, H, W, slot,
                       table, cap, count);
    TG_CHECK_LAUNCH("hole_table_kernel");
    return TG_OK;
}

extern "C" size_t tg_terrain_errors_ws_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return (size_t)te_grid(H, W) * TG_TE_NSUM * sizeof(double);
}

extern "C" int tg_terrain_errors(const float* z, const float* p, const float* mask, int use_nodata, float nodata,
                                 const uint8_t* holes, const float* keep, const int32_t* labels, const int32_t* slot,
                                 int64_t* table, int nholes, int H, int W, double cellsize, const TgAreaClasses* classes,
                                 int64_t* counts, float* sel_a, float* sel_slope, void* ws, size_t ws_bytes,
                                 tg_stream_t stream) {
    if (int rc = size_check("tg_terrain_errors", H, W)) return rc;
    TG_REQUIRE(z && p && holes && keep && labels && slot && classes && counts && sel_a && sel_slope && ws && (table || !nholes),
               "tg_terrain_errors: null pointer");
    TG_REQUIRE(isfinite(cellsize) && cellsize > 0.0, "tg_terrain_errors: cellsize %g must be finite and > 0", cellsize);
    TG_REQUIRE(nholes >= 0, "tg_terrain_errors: nholes %d < 0", nholes);
    TG_REQUIRE(classes->n_edges >= 0 && classes->n_edges < TG_EVAL_MAX_CLASSES,
               "tg_terrain_errors: %d class edges out of range [0, %d]", classes->n_edges, TG_EVAL_MAX_CLASSES - 1);
    for (int e = 1; e < classes->n_edges; ++e)
        TG_REQUIRE(classes->px[e] >= classes->px[e - 1], "tg_terrain_errors: class edges must be nondecreasing");
    const size_t need = tg_terrain_errors_ws_bytes(H, W);
    if (ws_bytes < need) {
        tg_set_error("tg_terrain_errors: workspace %zu bytes < %zu", ws_bytes, need);
        return TG_ERR_WS;
    }
    if (int rc = memset_async(counts, TG_TE_NCOUNT * sizeof(int64_t), S(stream), "tg_terrain_errors")) return rc;
    TeArgs a;
    a.z = z; a.p = p; a.mask = mask; a.use_nodata = use_nodata; a.nodata = nodata; a.holes = holes; a.keep = keep;
    a.labels = labels; a.slot = slot; a.table = table; a.nholes = nholes; a.H = H; a.W = W;
    a.tiles_x = cdiv(W, TE_TX);
    a.ntiles = cdiv(H, TE_TY) * a.tiles_x;
    a.inv8c = 1.0 / (8.0 * cellsize);
    a.invc2 = 1.0 / (cellsize * cellsize);
    a.cls = *classes;
    a.counts = counts; a.sel_a = sel_a; a.sel_s = sel_slope; a.partials = (double*)ws;
    hipLaunchKernelGGL(terrain_errors_kernel, dim3(te_grid(H, W)), dim3(256), 0, S(stream), a);
    TG_CHECK_LAUNCH("terrain_errors_kernel");
    return TG_OK;
}

extern "C" int tg_terrain_errors_finish(int H, int W, const void* ws, size_t ws_bytes, double* sums, tg_stream_t stream) {
    if (int rc = size_check("tg_terrain_errors_finish", H, W)) return rc;
    TG_REQUIRE(ws && sums, "tg_terrain_errors_finish: null pointer");
    const size_t need = tg_terrain_errors_ws_bytes(H, W);
    if (ws_bytes < need) {
        tg_set_error("tg_terrain_errors_finish: workspace %zu bytes < %zu", ws_bytes, need);
        return TG_ERR_WS;
    }
    hipLaunchKernelGGL(terrain_errors_finish_kernel, dim3(1), dim3(256), 0, S(stream), (const double*)ws, te_grid(H, W), sums);
    TG_CHECK_LAUNCH("terrain_errors_finish_kernel");
    return TG_OK;
}

extern "C" size_t tg_select_f32_ws_bytes(int64_t n, int nk) {
    (void)n;
    if (nk < 1 || nk > TG_SELECT_MAX_K) return 0;
    return (size_t)nk * SEL_BINS * sizeof(uint32_t) + (size_t)nk * sizeof(SelState);
}

extern "C" int tg_select_f32(const float* v, int64_t n, const int64_t* ks, int nk, float* out, void* ws, size_t ws_bytes,
                             tg_stream_t stream) {
    TG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "tg_select_f32: n %lld out of range [1, 2^31)", (long long)n);
    TG_REQUIRE(nk >= 1 && nk <= TG_SELECT_MAX_K, "tg_select_f32: nk %d out of range [1, %d]", nk, TG_SELECT_MAX_K);
    TG_REQUIRE(v && ks && out && ws, "tg_select_f32: null pointer");
    const size_t need = tg_select_f32_ws_bytes(n, nk);
    if (ws_bytes < need) {
        tg_set_error("tg_select_f32: workspace %zu bytes < %zu", ws_bytes, need);
        return TG_ERR_WS;
    }
    const hipStream_t s = S(stream);
    uint32_t* hist = (uint32_t*)ws;
    SelState* st = (SelState*)(hist + (size_t)nk * SEL_BINS);
    int64_t g = cdiv64(n, 256 * 16);
    const int grid = (int)(g < 1024 ? (g < 1 ? 1 : g) : 1024);
    for (int pass = 0; pass < 3; ++pass) {
        const int rows = pass == 0 ? 1 : nk;
        if (int rc = memset_async(hist, (size_t)rows * SEL_BINS * sizeof(uint32_t), s, "tg_select_f32")) return rc;
        hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(256), (size_t)rows * SEL_BINS * sizeof(uint32_t), s, v, n, pass, nk,
                           st, hist);
        TG_CHECK_LAUNCH("select_hist_kernel");
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, pass, nk, ks, st, hist, out);
        TG_CHECK_LAUNCH("select_scan_kernel");
    }
    return TG_OK;
}
