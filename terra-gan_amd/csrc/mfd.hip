// Multiple-flow-direction (MFD) accumulation, slope and topographic wetness index of a raster (mvp_gan/src/flow_routing.py,
// DESIGN.md section 8aa).  Inputs are what the D8 routing of flow.hip leaves: the routed surface w, known, the direction grid.
//
// Neighbour k = 0..7 is code k + 1 of flow.hip (E, SE, S, SW, W, NW, N, NE).  For a known pixel q and a known neighbour n_j inside
// the raster: d_j = w(q) - w(n_j) (one fp32 subtract), valid iff d_j > 0; t_j = (double)d_j raised to the integer exponent e by
// e - 1 fp64 multiplies, times cdiag for odd j; S = the fp64 sum of the valid t_j in the order j = 0..7.  S > 0: q gives
// f_j = t_j / S (one fp64 divide) to n_j; else with a code 1..8 it gives 1.0 to its D8 receiver; else nothing.
// A(p) = 1.0, then for k = 0..7 in order, where neighbour k gives f > 0 to p: A(p) = A(p) + f * A(n_k), one fp64 multiply and one
// fp64 add, nothing fused.
//
//   mfd_s_kernel        S of every pixel into the workspace, A = -1.0 ("not final") on known pixels and 0.0 on unknown ones, the
//                       counts of dispersive (S > 0), single and sink pixels
//   mfd_mask_kernel     the donor byte of every pixel: bit k set iff neighbour k gives to it
//   mfd_left_kernel     one thread: the pixels that are not final = the three counts together
//   sweep_begin_kernel  (raster_sweep.h) one thread: advance the sweep counter by n (its parity picks the plane of wake marks)
//   mfd_sweep_kernel    one workgroup per marked 64x64 tile that still holds a pixel that is not final: A, S and w with a one-pixel halo
//                       and the donor bytes in LDS; a pixel that is not final and whose donors are all final computes its value,
//                       by the directional line scans of raster_sweep.h, until a round finalises nothing or a cap
//   mfd_finish_kernel   A -> fp32, the largest A, the fp64 sum of A over the sinks as per-workgroup partials
//   mfd_psum_kernel     the partials summed in their order
//   slope_kernel        Horn's 3x3 slope in fp32
//   wetness_kernel      logf(a / fmaxf(slope, min_slope))
//   wetness_cmp_kernel  the differences of two wetness planes inside a selection
//
// Every value of A is written exactly once, from final donor values, in a fixed neighbour order, so the plane does not depend on
// the order of the visits; a value that is not final is only ever waited for.  The sweep follows the tile-sweep protocol of
// raster_sweep.h with 64-bit halo loads and write-backs of A: a tile may read a neighbour tile's pixel as not final or as final, and
// either is right.
#include "raster_sweep.h"

#pragma clang fp contract(off)

constexpr int MF_T = SW_T, MF_R = SW_R, MF_S = SW_S;
constexpr int MF_ROUNDS = 128;           // cap on the inner rounds of one visit; the tile stays on the list anyway while open
constexpr int MF_PARTS = 2048;           // ew_grid's cap: workgroups of the reductions
constexpr int MF_PART_W = 4;             // doubles per workgroup

struct MfLayout : SweepLayout {
    size_t open, mask, s, part, total;
};

static MfLayout mf_layout(int H, int W) {
    MfLayout L;
    size_t o;
    static_cast<SweepLayout&>(L) = sweep_layout(H, W, o, 1);        // the open plane keeps its place before the marks
    L.open = SW_CTL_BYTES;
    const size_t px = (size_t)H * W;
    L.mask = o; o += al256(px);
    L.s = o; o += al256(px * 8);
    L.part = o; o += (size_t)MF_PARTS * MF_PART_W * 8;
    L.total = o;
    return L;
}

// t_j of a valid drop d towards neighbour j
__device__ __forceinline__ double mf_term(float d32, int j, int e, double cdiag) {
    const double d = (double)d32;
    double t = d;
    for (int i = 1; i < e; ++i) t = t * d;
    if (j & 1) t = t * cdiag;
    return t;
}

__device__ __forceinline__ void mf_count3(int a, int b, int c, ull* counts) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(counts, (ull)a);
        if (b) atomicAdd(counts + 1, (ull)b);
        if (c) atomicAdd(counts + 2, (ull)c);
    }
}

// ---- setup --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfd_s_kernel(const float* __restrict__ w, const uint8_t* __restrict__ known,
                                                    const uint8_t* __restrict__ dir, int H, int W, int e, double cdiag,
                                                    double* __restrict__ Sp, double* __restrict__ A, ull* __restrict__ counts) {
    const int64_t n = (int64_t)H * W;
    int nd = 0, ns = 0, nk = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!known[p]) {
            Sp[p] = 0.0;
            A[p] = 0.0;
            continue;
        }
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const float wp = w[p];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int yy = y + d8_dy(j), xx = x + d8_dx(j);
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const int64_t q = (int64_t)yy * W + xx;
            if (!known[q]) continue;
            const float d = wp - w[q];
            if (d > 0.f) s = s + mf_term(d, j, e, cdiag);
        }
        Sp[p] = s;
        A[p] = -1.0;
        const int code = dir[p];
        if (s > 0.0) ++nd;
        else if (code >= 1 && code <= 8) ++ns;
        else ++nk;
    }
    mf_count3(nd, ns, nk, counts);
}

__global__ __launch_bounds__(256) void mfd_mask_kernel(const float* __restrict__ w, const uint8_t* __restrict__ known,
                                                       const uint8_t* __restrict__ dir, const double* __restrict__ Sp, int H, int W,
                                                       int e, double cdiag, uint8_t* __restrict__ mask) {
    const int64_t n = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        uint32_t m = 0;
        if (known[p]) {
            const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
            const float wp = w[p];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int yy = y + d8_dy(k), xx = x + d8_dx(k);
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                const int64_t q = (int64_t)yy * W + xx;
                if (!known[q]) continue;
                const int back = (k + 4) & 7;                       // the direction from the neighbour to p
                const double sq = Sp[q];
                if (sq > 0.0) {
                    const float d = w[q] - wp;
                    if (d > 0.f && mf_term(d, back, e, cdiag) / sq > 0.0) m |= 1u << k;
                } else if (dir[q] == back + 1) {
                    m |= 1u << k;
                }
            }
        }
        mask[p] = (uint8_t)m;
    }
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mf_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const ull*>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void mf_store(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<ull*>(p), (ull)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wake marks (raster_sweep.h): a visit marks the tile itself for the next sweep when it stopped at the cap on the rounds, and its
// eight neighbours when it made a pixel on its rim final.  An open tile without a mark can make no pixel final.
__global__ __launch_bounds__(256) void mfd_sweep_kernel(const float* __restrict__ w, const double* __restrict__ Sp,
                                                        const uint8_t* __restrict__ mask, int H, int W, int tiles_y, int tiles_x,
                                                        int e, double cdiag, double* A, uint8_t* open, const int32_t* __restrict__ ctl,
                                                        int n, int j, uint8_t* plane0, uint8_t* plane1, ull* counts) {
    __shared__ double as[MF_R * MF_S];                              // < 0: not final
    __shared__ double ss[MF_R * MF_S];
    __shared__ float hs[MF_R * MF_S];
    __shared__ uint8_t ms[MF_T * MF_T];
    __shared__ int tot[3];
    SweepVisit v = sweep_visit_begin(ctl, n, j, plane0, plane1);
    if (!v.marked) return;                                          // uniform: nothing has changed for this tile
    const int t = threadIdx.x, tile = v.tile;
    if (!open[tile]) {                                              // uniform: every pixel of the tile is final; not a visit
        if (t == 0) v.cur[tile] = 0;
        return;
    }
    sweep_visit_place(v, tiles_x);
    const int y0 = v.y0, x0 = v.x0;
    if (t < 3) tot[t] = 0;

    // stage: positions outside the raster are final at 0, as unknown pixels are; no donor bit ever points at either
    for (int i = t; i < MF_R * MF_R; i += 256) {
        const SweepStage g = sweep_stage(i, y0, x0, H, W);
        double a = 0.0, s = 0.0;
        float h = 0.f;
        if (g.in_raster) {
            const int64_t p = (int64_t)g.gy * W + g.gx;
            a = g.on_tile ? A[p] : mf_load(A + p);         // the field: see SweepStage
            s = Sp[p];
            h = w[p];
        }
        as[g.ly * MF_S + g.lx] = a;
        ss[g.ly * MF_S + g.lx] = s;
        hs[g.ly * MF_S + g.lx] = h;
    }
    __syncthreads();
    uint32_t was = 0;                                               // bit q: pixel t + 256 q was not final at the start
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = t + 256 * q;
        const int ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        uint32_t m = 0;
        if (gy < H && gx < W) {
            m = mask[(int64_t)gy * W + gx];
            if (as[(ly + 1) * MF_S + lx + 1] < 0.0) was |= 1u << q;
        }
        ms[i] = (uint8_t)m;
    }
    if (!__syncthreads_or((int)was)) {
        if (t == 0) open[tile] = 0;
        sweep_visit_end(v, tiles_y, tiles_x, counts + 4, false, false);
        return;
    }

    // the line scans of raster_sweep.h.  A value read may be a neighbour thread's old one (not final: wait) or its new one (final
    // for good).  This needs 64-bit LDS accesses that do not tear: as[] holds 8-byte aligned doubles read and written by single
    // ds_read_b64 / ds_write_b64 operations, so the step from -1.0 to a value is never seen half written.  A layout that splits
    // them (packing, two 32-bit accesses) would break the rounds silently.
    const int line = t & 63, band = t >> 6;
    int live = 1;
    for (int round = 0; round < MF_ROUNDS && live; ++round) {
        const int dirn = round & 3;
        const int back = dirn & 1;
        const int c = band * 16 + (back ? 15 : 0);
        const int sgn = back ? -1 : 1;
        int step, idx, mstep, mi;
        if (dirn < 2) { step = sgn * MF_S; idx = (c + 1) * MF_S + line + 1; mstep = sgn * MF_T; mi = c * MF_T + line; }
        else          { step = sgn; idx = (line + 1) * MF_S + c + 1; mstep = sgn; mi = line * MF_T + c; }
        int done = 0;
        for (int k = 0; k < 16; ++k) {
            if (as[idx] < 0.0) {
                const uint32_t m = ms[mi];
                bool ready = true;
#pragma unroll
                for (int b = 0; b < 8; ++b)
                    if ((m >> b & 1) && as[idx + d8_dy(b) * MF_S + d8_dx(b)] < 0.0) ready = false;
                if (ready) {
                    const float hp = hs[idx];
                    double a = 1.0;
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        if (m >> b & 1) {
                            const int nb = idx + d8_dy(b) * MF_S + d8_dx(b);
                            const double sn = ss[nb];
                            double f = 1.0;
                            if (sn > 0.0) f = mf_term(hs[nb] - hp, (b + 4) & 7, e, cdiag) / sn;
                            a = a + f * as[nb];
                        }
                    }
                    as[idx] = a;
                    done = 1;
                }
            }
            idx += step;
            mi += mstep;
        }
        live = __syncthreads_or(done);
    }

    // write back what this visit made final
    int nf = 0, no = 0, rim = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (was >> q & 1) {
            const int i = t + 256 * q;
            const int ly = i >> 6, lx = i & 63;
            const double av = as[(ly + 1) * MF_S + lx + 1];
            if (av >= 0.0) {
                mf_store(A + (int64_t)(y0 + ly) * W + x0 + lx, av);
                ++nf;
                if (ly == 0 || ly == MF_T - 1 || lx == 0 || lx == MF_T - 1) rim = 1;
            } else {
                ++no;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o, 64);
        no += __shfl_xor(no, o, 64);
        rim += __shfl_xor(rim, o, 64);
    }
    if ((t & 63) == 0) {
        if (nf) atomicAdd(&tot[0], nf);
        if (no) atomicAdd(&tot[1], no);
        if (rim) atomicAdd(&tot[2], rim);
    }
    __syncthreads();
    if (t == 0) {
        if (tot[1] == 0) open[tile] = 0;
        if (tot[0]) atomicAdd(counts + 3, (ull)(-(long long)tot[0]));   // pixels that are not final yet
    }
    // marks: itself if the cap stopped it with pixels left, and after a final rim value its neighbours
    sweep_visit_end(v, tiles_y, tiles_x, counts + 4, live && tot[1] != 0, tot[2] != 0);
}

// ---- finish and reductions ----------------------------------------------------------------------------------------------
// the sums of one workgroup in a fixed order: the thread's own elements in order, the wave by shuffles, the four waves in order
template <int M>
__device__ __forceinline__ void mf_block_sums(double (&v)[M], double* __restrict__ part) {
    __shared__ double red[4][M];
#pragma unroll
    for (int j = 0; j < M; ++j) v[j] = wave_sum_d(v[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < M; ++j) red[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const int j = threadIdx.x;
        part[(size_t)blockIdx.x * MF_PART_W + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}

__global__ __launch_bounds__(256) void mfd_finish_kernel(const double* __restrict__ A, const double* __restrict__ Sp,
                                                         const uint8_t* __restrict__ dir, int64_t n, float* __restrict__ acc,
                                                         ull* __restrict__ amax, double* __restrict__ part) {
    double v[1] = {0.0};
    double m = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const double a = A[p];
        acc[p] = (float)a;
        if (a > m) m = a;
        if (a > 0.0 && !(Sp[p] > 0.0)) {
            const int code = dir[p];
            if (!(code >= 1 && code <= 8)) v[0] = v[0] + a;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(m, o, 64);
        m = m2 > m ? m2 : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(amax, (ull)__double_as_longlong(m));   // non-negative: the bits order
    mf_block_sums<1>(v, part);
}

__global__ void mfd_psum_kernel(const double* __restrict__ part, int nb, int m, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (blockIdx.x != 0 || j >= m) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s = s + part[(size_t)b * MF_PART_W + j];
    out[j] = s;
}

// ---- slope, wetness, comparison -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slope_kernel(const float* __restrict__ w, const uint8_t* __restrict__ known, int H, int W,
                                                    float den, float* __restrict__ slope) {
    const int64_t n = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!known[p]) {
            slope[p] = __uint_as_float(0x7fc00000u);
            continue;
        }
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const float e = w[p];
        float v[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int yy = y + i / 3 - 1, xx = x + i % 3 - 1;
            float h = e;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const int64_t q = (int64_t)yy * W + xx;
                if (known[q]) h = w[q];
            }
            v[i] = h;
        }
        // a b c / d . f / g h i = v[0..8]
        const float gx = ((v[2] - v[0]) + 2.f * (v[5] - v[3])) + (v[8] - v[6]);
        const float gy = ((v[6] - v[0]) + 2.f * (v[7] - v[1])) + (v[8] - v[2]);
        slope[p] = sqrtf(gx * gx + gy * gy) / den;
    }
}

__global__ __launch_bounds__(256) void wetness_kernel(const float* __restrict__ acc, const float* __restrict__ slope,
                                                      const uint8_t* __restrict__ known, int64_t n, float cellsize, float min_slope,
                                                      float* __restrict__ twi) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        float v = __uint_as_float(0x7fc00000u);
        if (known[p]) {
            const float a = acc[p] * cellsize;
            v = logf(a / fmaxf(slope[p], min_slope));
        }
        twi[p] = v;
    }
}

__global__ __launch_bounds__(256) void wetness_cmp_kernel(const uint8_t* __restrict__ sel, const float* __restrict__ tt,
                                                          const float* __restrict__ tp, int64_t n, ull* __restrict__ counts,
                                                          double* __restrict__ part) {
    double v[3] = {0.0, 0.0, 0.0};
    int cells = 0;
    float mx = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        if (!sel[p]) continue;
        const float a = tt[p], b = tp[p];
        if (!(fabsf(a) < __uint_as_float(0x7f800000u)) || !(fabsf(b) < __uint_as_float(0x7f800000u))) continue;
        const float d = b - a;
        const double dd = (double)d;
        ++cells;
        v[0] = v[0] + dd;
        v[1] = v[1] + fabs(dd);
        v[2] = v[2] + dd * dd;
        mx = fmaxf(mx, fabsf(d));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cells += __shfl_xor(cells, o, 64);
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (cells) atomicAdd(counts, (ull)cells);
        if (mx > 0.f) atomicMax(counts + 1, (ull)__float_as_uint(mx));
    }
    mf_block_sums<3>(v, part);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int mf_exp_check(const char* who, int e, double cdiag) {
    TG_REQUIRE(e >= 1 && e <= TG_MFD_MAX_EXPONENT, "%s: exponent %d must lie in [1, %d]", who, e, TG_MFD_MAX_EXPONENT);
    TG_REQUIRE(cdiag > 0.0 && cdiag <= 1.0, "%s: cdiag %g must lie in (0, 1]", who, cdiag);
    return TG_OK;
}

// every known pixel is not final at the start
__global__ void mfd_left_kernel(ull* __restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counts[3] = counts[0] + counts[1] + counts[2];
}

extern "C" size_t tg_mfd_ws_bytes(int H, int W) {
    if (!raster_size_ok(H, W)) return 0;
    return mf_layout(H, W).total;
}

extern "C" int tg_mfd_setup(const float* w, const uint8_t* known, const uint8_t* dir, int H, int W, int exponent, double cdiag,
                            double* A, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_mfd_setup", H, W)) return rc;
    if (int rc = mf_exp_check("tg_mfd_setup", exponent, cdiag)) return rc;
    TG_REQUIRE(w && known && dir && A && counts && ws, "tg_mfd_setup: null pointer");
    TG_REQUIRE((const void*)A != (const void*)w, "tg_mfd_setup: A must not alias w");
    const MfLayout L = mf_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_mfd_setup: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    if (!sweep_reset(L, ws, s) || hipMemsetAsync(base + L.open, 1, L.tiles(), s) != hipSuccess ||
        hipMemsetAsync(counts, 0, TG_MFD_COUNTS * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_mfd_setup: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const dim3 grid(ew_grid((int64_t)H * W, 256));
    double* Sp = (double*)(base + L.s);
    hipLaunchKernelGGL(mfd_s_kernel, grid, dim3(256), 0, s, w, known, dir, H, W, exponent, cdiag, Sp, A,
                       reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("mfd_s_kernel");
    hipLaunchKernelGGL(mfd_left_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<ull*>(counts));
    TG_CHECK_LAUNCH("mfd_left_kernel");
    hipLaunchKernelGGL(mfd_mask_kernel, grid, dim3(256), 0, s, w, known, dir, (const double*)Sp, H, W, exponent, cdiag,
                       (uint8_t*)(base + L.mask));
    TG_CHECK_LAUNCH("mfd_mask_kernel");
    return TG_OK;
}

extern "C" int tg_mfd_sweep(const float* w, int H, int W, int exponent, double cdiag, int n, double* A, int64_t* counts, void* ws,
                            size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_mfd_sweep", H, W)) return rc;
    if (int rc = mf_exp_check("tg_mfd_sweep", exponent, cdiag)) return rc;
    TG_REQUIRE(w && A && counts && ws, "tg_mfd_sweep: null pointer");
    TG_REQUIRE(n >= 1 && n <= (1 << 20), "tg_mfd_sweep: n = %d sweeps must lie in [1, 2^20]", n);
    TG_REQUIRE((const void*)A != (const void*)w, "tg_mfd_sweep: A must not alias w");
    const MfLayout L = mf_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_mfd_sweep: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    return sweep_run(L, ws, n, nullptr, s, "mfd_begin_kernel", "mfd_sweep_kernel",
                     [&](dim3 grid, const int32_t* ctl, int j, uint8_t* p0, uint8_t* p1) {
                         hipLaunchKernelGGL(mfd_sweep_kernel, grid, dim3(256), 0, s, w, (const double*)(base + L.s),
                                            (const uint8_t*)(base + L.mask), H, W, L.ty, L.tx, exponent, cdiag, A,
                                            (uint8_t*)(base + L.open), ctl, n, j, p0, p1, reinterpret_cast<ull*>(counts));
                     });
}

extern "C" int tg_mfd_finish(const double* A, const uint8_t* dir, int H, int W, float* acc, double* out, void* ws, size_t ws_bytes,
                             tg_stream_t stream) {
    if (int rc = raster_size_check("tg_mfd_finish", H, W)) return rc;
    TG_REQUIRE(A && dir && acc && out && ws, "tg_mfd_finish: null pointer");
    const MfLayout L = mf_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_mfd_finish: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    char* base = (char*)ws;
    if (hipMemsetAsync(out, 0, 2 * sizeof(double), s) != hipSuccess) {
        tg_set_error("tg_mfd_finish: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    const int nb = ew_grid(px, 256);
    double* part = (double*)(base + L.part);
    hipLaunchKernelGGL(mfd_finish_kernel, dim3(nb), dim3(256), 0, s, A, (const double*)(base + L.s), dir, px, acc,
                       reinterpret_cast<ull*>(out), part);
    TG_CHECK_LAUNCH("mfd_finish_kernel");
    hipLaunchKernelGGL(mfd_psum_kernel, dim3(1), dim3(64), 0, s, (const double*)part, nb, 1, out + 1);
    TG_CHECK_LAUNCH("mfd_psum_kernel");
    return TG_OK;
}

extern "C" int tg_terrain_slope(const float* w, const uint8_t* known, int H, int W, float den, float* slope, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_terrain_slope", H, W)) return rc;
    TG_REQUIRE(w && known && slope, "tg_terrain_slope: null pointer");
    TG_REQUIRE(den > 0.f && den < __builtin_inff(), "tg_terrain_slope: the divisor 8 * cellsize = %g must be finite and > 0",
               (double)den);
    TG_REQUIRE((const void*)slope != (const void*)w, "tg_terrain_slope: slope must not alias w");
    hipLaunchKernelGGL(slope_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, S(stream), w, known, H, W, den, slope);
    TG_CHECK_LAUNCH("slope_kernel");
    return TG_OK;
}

extern "C" int tg_wetness(const float* acc, const float* slope, const uint8_t* known, int H, int W, float cellsize, float min_slope,
                          float* twi, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_wetness", H, W)) return rc;
    TG_REQUIRE(acc && slope && known && twi, "tg_wetness: null pointer");
    TG_REQUIRE(cellsize > 0.f && cellsize < __builtin_inff(), "tg_wetness: cellsize %g must be finite and > 0", (double)cellsize);
    TG_REQUIRE(min_slope > 0.f && min_slope < __builtin_inff(), "tg_wetness: min_slope %g must be finite and > 0",
               (double)min_slope);
    hipLaunchKernelGGL(wetness_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, S(stream), acc, slope, known,
                       (int64_t)H * W, cellsize, min_slope, twi);
    TG_CHECK_LAUNCH("wetness_kernel");
    return TG_OK;
}

extern "C" int tg_wetness_compare(const uint8_t* sel, const float* twi_t, const float* twi_p, int H, int W, int64_t* counts,
                                  double* sums, void* ws, size_t ws_bytes, tg_stream_t stream) {
    if (int rc = raster_size_check("tg_wetness_compare", H, W)) return rc;
    TG_REQUIRE(sel && twi_t && twi_p && counts && sums && ws, "tg_wetness_compare: null pointer");
    const MfLayout L = mf_layout(H, W);
    TG_REQUIRE(ws_bytes >= L.total, "tg_wetness_compare: workspace %zu bytes < %zu", ws_bytes, L.total);
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        tg_set_error("tg_wetness_compare: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const int64_t px = (int64_t)H * W;
    const int nb = ew_grid(px, 256);
    double* part = (double*)((char*)ws + L.part);
    hipLaunchKernelGGL(wetness_cmp_kernel, dim3(nb), dim3(256), 0, s, sel, twi_t, twi_p, px, reinterpret_cast<ull*>(counts), part);
    TG_CHECK_LAUNCH("wetness_cmp_kernel");
    hipLaunchKernelGGL(mfd_psum_kernel, dim3(1), dim3(64), 0, s, (const double*)part, nb, 3, sums);
    TG_CHECK_LAUNCH("mfd_psum_kernel");
    return TG_OK;
}
