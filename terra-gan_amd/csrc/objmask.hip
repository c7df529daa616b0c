// Above-ground objects from the DSM alone (mvp_gan/src/object_mask.py): progressive morphological
// filter (Zhang et al. 2003) -> 8-connected components -> area filter -> buffer.
//
//   tg_objmask_known       known map [H][W] (mask != 0, finite, != nodata) and its transpose [W][H], uint8, LDS-tiled
//   tg_objmask_morph       clipped-window erosion / dilation over the known pixels: column pass, transpose, column pass,
//                          transpose
//   tg_objmask_pmf_step    one opening s -> open_r(s); its last column pass also sets flags where s - open_r(s) > dh
//   tg_objmask_components  union-find: tile-local merge in LDS, atomicMin hooking across tile borders, path compression;
//                          label = smallest linear index of the component, area at that index (integer atomics)
//   tg_objmask_filter      area threshold + buffer (separable max in an LDS tile) -> object map, keep mask, counters
//
// Column pass (morph_col_kernel): van Herk / Gil-Werman.  With k = 2r + 1, the padded rows -r .. H-1+r (identity outside the
// raster) are cut into blocks [b k - r, b k + r]; out(y) = min(suffix(y - r), prefix(y + r)), suffix / prefix taken inside
// the block of their argument.  One lane owns one column and one block: a backward scan of block b writes suffix(y - r) to
// out[y], a forward scan of block b + 1 folds prefix(y + r) in.  The 64 lanes of a wave own 64 adjacent columns, so every
// access is one 256-byte row segment; the cost per pixel is independent of r.  The row pass is the same kernel on the
// transpose (transpose_kernel: 64 x 64 LDS tiles).  Every kernel uses min / max, fp32 subtraction, comparisons and integer
// atomics only: results are bitwise deterministic.
#include <math.h>

#include "common.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }
__device__ __forceinline__ int64_t lmin(int64_t a, int64_t b) { return a < b ? a : b; }

constexpr int TT = 64;                  // transpose / known tile side
constexpr int CC_T = 32;                // component tile side (32 x 32 pixels, 256 threads x 4)
constexpr int FIL_TY = 32, FIL_TX = 64; // filter tile (rows x columns)

// ---- known map and its transpose --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void objmask_known_kernel(const float* __restrict__ dem, const float* __restrict__ mask,
                                                            int H, int W, int use_nodata, float nodata, int tiles_x,
                                                            uint8_t* __restrict__ known, uint8_t* __restrict__ known_t) {
    __shared__ uint8_t t[TT][TT + 4];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TT, x0 = tx * TT;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < TT; r += 4) {
        const int y = y0 + r, x = x0 + c;
        if (y < H && x < W) {
            const int64_t i = (int64_t)y * W + x;
            const float z = dem[i];
            bool k = isfinite(z);
            if (mask) k = k && mask[i] != 0.f;
            if (use_nodata) k = k && z != nodata;
            known[i] = k;
            t[r][c] = k;
        }
    }
    if (!known_t) return;
    __syncthreads();
    for (int r = r0; r < TT; r += 4) {                 // known_t[x][y]: lanes walk y (coalesced)
        const int x = x0 + r, y = y0 + c;
        if (x < W && y < H) known_t[(int64_t)x * H + y] = t[c][r];
    }
}

// ---- transpose: in [H][W] -> out [W][H] ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void objmask_transpose_kernel(const float* __restrict__ in, int H, int W, int tiles_x,
                                                                float* __restrict__ out) {
    __shared__ float t[TT][TT + 1];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TT, x0 = tx * TT;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < TT; r += 4) {
        const int y = y0 + r, x = x0 + c;
        if (y < H && x < W) t[r][c] = in[(int64_t)y * W + x];
    }
    __syncthreads();
    for (int r = r0; r < TT; r += 4) {
        const int x = x0 + r, y = y0 + c;
        if (x < W && y < H) out[(int64_t)x * H + y] = t[c][r];
    }
}

// ---- column pass ------------------------------------------------------------------------------------------------------
// out[y][c] = op over in[q][c], q in [y - r, y + r] clipped to [0, H), where known_in (if given) is nonzero; identity if none.
// EPI: out is the new surface s_next, and flags[y][c] = 1 where known_out and s_prev - s_next > dh (fp32).
template <bool MAX, bool EPI>
__global__ __launch_bounds__(256) void morph_col_kernel(const float* __restrict__ in, const uint8_t* __restrict__ known_in,
                                                        int H, int W, int r, int64_t nblk, int col_groups,
                                                        float* __restrict__ out, const float* __restrict__ s_prev,
                                                        const uint8_t* __restrict__ known_out, float dh,
                                                        uint8_t* __restrict__ flags) {
    const float I = MAX ? -INFINITY : INFINITY;
    const int lane = threadIdx.x & 63;
    const int64_t k = 2 * (int64_t)r + 1;
    const int64_t items = nblk * col_groups;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * 4) {
        const int64_t b = it / col_groups;
        const int c = (int)(it - b * col_groups) * 64 + lane;
        if (c >= W) continue;
        const int64_t bk = b * k;
        // backward: suffix minima of block b = [bk - r, bk + r] -> out[p + r]
        float run = I;
        for (int64_t p = lmin(bk + r, (int64_t)H - 1); p >= bk - r; --p) {
            if (p < 0) break;                   // the rest of the block is padding: run stays, its rows are < bk
            const int64_t i = p * W + c;
            const float v = in[i];
            if (!known_in || known_in[i]) run = MAX ? fmaxf(run, v) : fminf(run, v);
            const int64_t y = p + r;
            if (y < H) out[y * W + c] = run;
        }
        if (bk < r) {                           // block 0: rows y = p + r of the padding p < 0 take the whole suffix
            for (int64_t y = 0; y < lmin(r, H); ++y) out[y * W + c] = run;
        }
        // forward: prefix minima of block b + 1 folded into rows bk + 1 .. bk + k - 1
        run = I;
        const int64_t yend = lmin(bk + k, H);
        for (int64_t y = bk; y < yend; ++y) {
            const int64_t p = y + r;
            if (y > bk && p < H) {
                const int64_t i = p * W + c;
                const float v = in[i];
                if (!known_in || known_in[i]) run = MAX ? fmaxf(run, v) : fminf(run, v);
            }
            const int64_t o = y * W + c;
            const float a = out[o];
            const float s = MAX ? fmaxf(a, run) : fminf(a, run);
            out[o] = s;
            if (EPI && known_out[o] && __fsub_rn(s_prev[o], s) > dh) flags[o] = 1;
        }
    }
}

// ---- components -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int x) {
    int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return x;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[b], a);   // link the larger root under the smaller
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int g_find(int32_t* lab, int x) {
    int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

__device__ __forceinline__ void g_union(int32_t* lab, int a, int b) {
    for (;;) {
        a = g_find(lab, a);
        b = g_find(lab, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[b], a);
        if (old == b) return;
        b = old;
    }
}

// per 32 x 32 tile: union-find in LDS over the 8-neighbourhood inside the tile; lab = global index of the tile-local root
// (the smallest index of the tile-local component: local and global row-major orders agree inside a tile); area = 0
__global__ __launch_bounds__(256) void cc_local_kernel(const uint8_t* __restrict__ flags, int H, int W, int tiles_x,
                                                       int32_t* __restrict__ lab, int32_t* __restrict__ area) {
    __shared__ int par[CC_T * CC_T];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CC_T, x0 = tx * CC_T;
    for (int li = threadIdx.x; li < CC_T * CC_T; li += 256) {
        const int y = y0 + li / CC_T, x = x0 + li % CC_T;
        par[li] = (y < H && x < W && flags[(int64_t)y * W + x]) ? li : -1;
    }
    __syncthreads();
    for (int li = threadIdx.x; li < CC_T * CC_T; li += 256) {
        if (par[li] < 0) continue;
        const int ly = li / CC_T, lx = li % CC_T;
        if (lx > 0 && par[li - 1] >= 0) lds_union(par, li, li - 1);
        if (ly > 0) {
            if (par[li - CC_T] >= 0) lds_union(par, li, li - CC_T);
            if (lx > 0 && par[li - CC_T - 1] >= 0) lds_union(par, li, li - CC_T - 1);
            if (lx < CC_T - 1 && par[li - CC_T + 1] >= 0) lds_union(par, li, li - CC_T + 1);
        }
    }
    __syncthreads();
    for (int li = threadIdx.x; li < CC_T * CC_T; li += 256) {
        const int y = y0 + li / CC_T, x = x0 + li % CC_T;
        if (y >= H || x >= W) continue;
        const int64_t i = (int64_t)y * W + x;
        int root = -1;
        if (par[li] >= 0) {
            const int rl = lds_find(par, li);
            root = (y0 + rl / CC_T) * W + x0 + rl % CC_T;
        }
        lab[i] = root;
        area[i] = 0;
    }
}

// unions across tile borders: every flagged pixel with a flagged W / NW / N / NE neighbour in another tile
__global__ __launch_bounds__(256) void cc_border_kernel(int H, int W, int32_t* __restrict__ lab) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        const bool top = y % CC_T == 0 && y > 0, left = x % CC_T == 0 && x > 0, right = x % CC_T == CC_T - 1 && x < W - 1;
        if (!(top || left || right)) continue;
        if (lab[i] < 0) continue;
        const int a = (int)i;
        if (left && lab[i - 1] >= 0) g_union(lab, a, a - 1);
        if (y > 0) {
            const int64_t u = i - W;
            if (top && lab[u] >= 0) g_union(lab, a, (int)u);
            if (x > 0 && (top || left) && lab[u - 1] >= 0) g_union(lab, a, (int)u - 1);
            if (x < W - 1 && (top || right) && lab[u + 1] >= 0) g_union(lab, a, (int)u + 1);
        }
    }
}

// path compression and areas: one thread per run of 8 pixels of a row; one integer atomic per run of equal labels
constexpr int CC_RUN = 8;
__global__ __launch_bounds__(256) void cc_compress_kernel(int H, int W, int32_t* __restrict__ lab, int32_t* __restrict__ area) {
    const int runs_x = (W + CC_RUN - 1) / CC_RUN;
    const int64_t n = (int64_t)H * runs_x;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const int y = (int)(t / runs_x), x0 = (int)(t - (int64_t)y * runs_x) * CC_RUN;
        int cur = -1, cnt = 0;
        for (int x = x0; x < min(x0 + CC_RUN, W); ++x) {
            const int64_t i = (int64_t)y * W + x;
            if (lab[i] < 0) continue;
            const int root = g_find(lab, (int)i);
            lab[i] = root;
            if (root != cur) {
                if (cnt) atomicAdd(&area[cur], cnt);
                cur = root;
                cnt = 0;
            }
            ++cnt;
        }
        if (cnt) atomicAdd(&area[cur], cnt);
    }
}

// ---- area threshold + buffer -> object map, keep mask, counters -------------------------------------------------------
// counts: [0] flagged pixels, [1] components kept (objects), [2] components removed, [3] object pixels
__global__ __launch_bounds__(256) void objmask_filter_kernel(const uint8_t* __restrict__ known, const int32_t* __restrict__ lab,
                                                             const int32_t* __restrict__ area, int H, int W, int min_area,
                                                             int buf, int tiles_x, uint8_t* __restrict__ objects,
                                                             float* __restrict__ keep, int32_t* __restrict__ counts) {
    extern __shared__ uint8_t sm[];
    const int hy = FIL_TY + 2 * buf, hx = FIL_TX + 2 * buf;
    uint8_t* ob = sm;                   // [hy][hx]: surviving component pixels of the haloed tile
    uint8_t* rm = sm + hy * hx;         // [hy][FIL_TX]: their max along rows
    __shared__ int red[4][4];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * FIL_TY, x0 = tx * FIL_TX;
    for (int j = threadIdx.x; j < hy * hx; j += 256) {
        const int y = y0 - buf + j / hx, x = x0 - buf + j % hx;
        uint8_t o = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int l = lab[(int64_t)y * W + x];
            o = l >= 0 && area[l] >= min_area;
        }
        ob[j] = o;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < hy * FIL_TX; j += 256) {
        const int r = j / FIL_TX, c = j % FIL_TX;
        uint8_t o = 0;
        for (int d = 0; d <= 2 * buf; ++d) o |= ob[r * hx + c + d];
        rm[j] = o;
    }
    __syncthreads();
    int cf = 0, ck = 0, cr = 0, co = 0;
    for (int j = threadIdx.x; j < FIL_TY * FIL_TX; j += 256) {
        const int r = j / FIL_TX, c = j % FIL_TX;
        const int y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        uint8_t o = 0;
        for (int d = 0; d <= 2 * buf; ++d) o |= rm[(r + d) * FIL_TX + c];
        const int64_t i = (int64_t)y * W + x;
        objects[i] = o;
        keep[i] = (known[i] && !o) ? 1.f : 0.f;
        const int l = lab[i];
        cf += l >= 0;
        if (l == (int)i) {
            if (area[i] >= min_area) ++ck; else ++cr;
        }
        co += o;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        cf += __shfl_xor(cf, s, 64); ck += __shfl_xor(ck, s, 64);
        cr += __shfl_xor(cr, s, 64); co += __shfl_xor(co, s, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = cf; red[w][1] = ck; red[w][2] = cr; red[w][3] = co; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], v);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static int size_check(const char* who, int H, int W) {
    TG_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: raster %dx%d must be non-empty with H*W < 2^31", who,
               H, W);
    return TG_OK;
}

static int tiles(int H, int W, int ty, int tx, int& tiles_x) {
    tiles_x = cdiv(W, tx);
    return cdiv(H, ty) * tiles_x;      // < 2^31: H * W < 2^31
}

static int transpose(const float* in, int H, int W, float* out, hipStream_t s) {
    int tx;
    const int n = tiles(H, W, TT, TT, tx);
    hipLaunchKernelGGL(objmask_transpose_kernel, dim3(n), dim3(256), 0, s, in, H, W, tx, out);
    TG_CHECK_LAUNCH("objmask_transpose_kernel");
    return TG_OK;
}

template <bool MAX, bool EPI>
static int col_pass(const float* in, const uint8_t* known_in, int H, int W, int r, float* out, hipStream_t s,
                    const float* s_prev = nullptr, const uint8_t* known_out = nullptr, float dh = 0.f, uint8_t* flags = nullptr) {
    const int re = r < H - 1 ? r : H - 1;           // a window reaching past the raster is clipped to it
    const int64_t k = 2 * (int64_t)re + 1;
    const int64_t nblk = cdiv64(H, k);
    const int cg = cdiv(W, 64);
    const int64_t waves = nblk * cg;
    const int64_t g = cdiv64(waves, 4);
    const int grid = (int)(g < 8192 ? g : 8192);
    hipLaunchKernelGGL((morph_col_kernel<MAX, EPI>), dim3(grid), dim3(256), 0, s, in, known_in, H, W, re, nblk, cg, out, s_prev,
                       known_out, dh, flags);
    TG_CHECK_LAUNCH("morph_col_kernel");
    return TG_OK;
}

extern "C" int tg_objmask_known(const float* dem, const float* mask, int H, int W, int use_nodata, float nodata, uint8_t* known,
                                uint8_t* known_t, tg_stream_t stream) {
    if (int rc = size_check("tg_objmask_known", H, W)) return rc;
    TG_REQUIRE(dem && known, "tg_objmask_known: null pointer");
    int tx;
    const int n = tiles(H, W, TT, TT, tx);
    hipLaunchKernelGGL(objmask_known_kernel, dim3(n), dim3(256), 0, S(stream), dem, mask, H, W, use_nodata, nodata, tx, known,
                       known_t);
    TG_CHECK_LAUNCH("objmask_known_kernel");
    return TG_OK;
}

extern "C" int tg_objmask_morph(const float* in, const uint8_t* known, int H, int W, int radius, int op, float* tmp, float* out,
                                tg_stream_t stream) {
    if (int rc = size_check("tg_objmask_morph", H, W)) return rc;
    TG_REQUIRE(in && tmp && out, "tg_objmask_morph: null pointer");
    TG_REQUIRE(radius >= 0, "tg_objmask_morph: radius %d < 0", radius);
    TG_REQUIRE(op == TG_MORPH_ERODE || op == TG_MORPH_DILATE, "tg_objmask_morph: op %d is neither erode (0) nor dilate (1)", op);
    TG_REQUIRE(in != tmp && in != out && tmp != out, "tg_objmask_morph: in, tmp and out must be distinct buffers");
    const hipStream_t s = S(stream);
    int rc = op == TG_MORPH_DILATE ? col_pass<true, false>(in, known, H, W, radius, tmp, s)
                                   : col_pass<false, false>(in, known, H, W, radius, tmp, s);
    if (!rc) rc = transpose(tmp, H, W, out, s);                                   // out: [W][H]
    if (!rc) rc = op == TG_MORPH_DILATE ? col_pass<true, false>(out, nullptr, W, H, radius, tmp, s)
                                        : col_pass<false, false>(out, nullptr, W, H, radius, tmp, s);
    if (!rc) rc = transpose(tmp, W, H, out, s);
    return rc;
}

extern "C" int tg_objmask_pmf_step(const float* s_in, const uint8_t* known, const uint8_t* known_t, int H, int W, int radius,
                                   float dh, float* t0, float* t1, float* s_out, uint8_t* flags, tg_stream_t stream) {
    if (int rc = size_check("tg_objmask_pmf_step", H, W)) return rc;
    TG_REQUIRE(s_in && known && known_t && t0 && t1 && s_out && flags, "tg_objmask_pmf_step: null pointer");
    TG_REQUIRE(radius >= 0, "tg_objmask_pmf_step: radius %d < 0", radius);
    TG_REQUIRE(isfinite(dh) && dh >= 0.f, "tg_objmask_pmf_step: threshold %g must be finite and >= 0", (double)dh);
    TG_REQUIRE(s_in != t0 && s_in != t1 && s_in != s_out && t0 != t1 && t0 != s_out && t1 != s_out,
               "tg_objmask_pmf_step: s_in, t0, t1 and s_out must be distinct buffers");
    const hipStream_t s = S(stream);
    int rc = col_pass<false, false>(s_in, known, H, W, radius, t0, s);       // erode: columns, over the known pixels
    if (!rc) rc = transpose(t0, H, W, t1, s);
    if (!rc) rc = col_pass<false, false>(t1, nullptr, W, H, radius, t0, s);      //        rows (on the transpose)
    if (!rc) rc = col_pass<true, false>(t0, known_t, W, H, radius, t1, s);       // dilate: rows, eroded values at known pixels
    if (!rc) rc = transpose(t1, W, H, t0, s);
    if (!rc) rc = col_pass<true, true>(t0, nullptr, H, W, radius, s_out, s, s_in, known, dh, flags);   // columns + flags
    return rc;
}

extern "C" int tg_objmask_components(const uint8_t* flags, int H, int W, int32_t* labels, int32_t* area, tg_stream_t stream) {
    if (int rc = size_check("tg_objmask_components", H, W)) return rc;
    TG_REQUIRE(flags && labels && area, "tg_objmask_components: null pointer");
    int tx;
    const int n = tiles(H, W, CC_T, CC_T, tx);
    hipLaunchKernelGGL(cc_local_kernel, dim3(n), dim3(256), 0, S(stream), flags, H, W, tx, labels, area);
    TG_CHECK_LAUNCH("cc_local_kernel");
    hipLaunchKernelGGL(cc_border_kernel, dim3(ew_grid((int64_t)H * W, 256)), dim3(256), 0, S(stream), H, W, labels);
    TG_CHECK_LAUNCH("cc_border_kernel");
    hipLaunchKernelGGL(cc_compress_kernel, dim3(ew_grid((int64_t)H * cdiv(W, CC_RUN), 256)), dim3(256), 0, S(stream), H, W,
                       labels, area);
    TG_CHECK_LAUNCH("cc_compress_kernel");
    return TG_OK;
}

extern "C" int tg_objmask_filter(const uint8_t* known, const int32_t* labels, const int32_t* area, int H, int W, int min_area,
                                 int buffer_px, uint8_t* objects, float* keep, int32_t* counts, tg_stream_t stream) {
    if (int rc = size_check("tg_objmask_filter", H, W)) return rc;
    TG_REQUIRE(known && labels && area && objects && keep && counts, "tg_objmask_filter: null pointer");
    TG_REQUIRE(min_area >= 0, "tg_objmask_filter: min_area %d < 0", min_area);
    TG_REQUIRE(buffer_px >= 0 && buffer_px <= TG_OBJMASK_MAX_BUFFER, "tg_objmask_filter: buffer %d px out of range [0, %d]",
               buffer_px, TG_OBJMASK_MAX_BUFFER);
    if (hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), S(stream)) != hipSuccess) {
        tg_set_error("tg_objmask_filter: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    int tx;
    const int n = tiles(H, W, FIL_TY, FIL_TX, tx);
    const size_t lds = (size_t)(FIL_TY + 2 * buffer_px) * (FIL_TX + 2 * buffer_px) + (size_t)(FIL_TY + 2 * buffer_px) * FIL_TX;
    hipLaunchKernelGGL(objmask_filter_kernel, dim3(n), dim3(256), lds, S(stream), known, labels, area, H, W, min_area, buffer_px,
                       tx, objects, keep, counts);
    TG_CHECK_LAUNCH("objmask_filter_kernel");
    return TG_OK;
}
