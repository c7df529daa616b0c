// Winograd F(2x2,3x3) with bf16 MFMA operands (BASELINE config 3: bf16 mixed precision) -- included by igemm.hip after
// wino.inc, whose geometry (WinoGeom / WinoWeights), work decomposition and output transform it shares.
//
// Same algebra as wino_kernel: Y = At [ (G g Gt) (.) (Bt d B) ] A, 16 independent [tiles x Cin] x [Cin x Cout] products per
// 16x16-pixel x 64-channel work item.  What changes is the arithmetic of those products: BOTH TRANSFORMS STAY fp32 (input
// patch fp32 in LDS, Bt d B in fp32 registers; G g Gt in fp32 in wino_weights16_kernel) and the transformed operands are
// rounded to bf16 once, at the V / U store; the products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation and the
// output transform is fp32 again.  A K step is 16 channels: an image row is 16 bf16 = 32 bytes, i.e. the LDS images, the
// half-row swizzle and the ds_read_b128 fragment addressing are byte for byte those of the fp32 kernel -- but ONE MFMA
// (32 cycles) consumes the fragment that took four fp32 MFMAs (256 cycles).  The matrix pipe is then ~10 % busy and the
// kernel runs at the speed of its staging (LDS traffic + transform VALU), ~3x the fp32 Winograd kernel per channel: the
// full-resolution layers become HBM-bound, which is where a bf16 path belongs.  No hand-placed interleave here (there is
// nothing to hide the staging behind): plain double-buffered LDS, two barriers per step, compiler-scheduled.
#pragma once

constexpr int W16_IMG = 16 * 64 * 16;                 // bf16 elements of one V (or U) image: 32 KB
constexpr int W16_P = WINO_PPIX * 16;                 // floats of the fp32 patch: 18 x 18 pixels x 16 channels
constexpr size_t W16_LDS_BYTES = 4 * (size_t)W16_IMG * 2 + (size_t)W16_P * 4;      // 151,808 B
// wino16_pipe_kernel pads its patch: 16 floats behind every 2 pixels.  A pixel holds 16 channels = 16 banks and a Winograd tile
// starts every 2 pixels = 32 floats, so the eight lanes a ds_read_b128 serves per cycle (4 channel quads x 2 tiles) hit the
// same 16 banks twice; with 48 floats per pixel pair tile t + 1 lands on the other 16 banks.  The transform's patch reads are
// half of this kernel's LDS reads, and the LDS is what bounds its K step.
constexpr int W16_PP = WINO_PPIX * 24;
constexpr size_t W16_PIPE_LDS_BYTES = 4 * (size_t)W16_IMG * 2 + (size_t)W16_PP * 4;   // 162,176 B

__host__ __device__ __forceinline__ int w16_pos(int row, int c) { return ((((c >> 3) ^ (row >> 4)) & 1) << 3) + (c & 7); }

// U16[k/16][n/64][xi][n%64][k%16 (half-swizzled)] = bf16( (G g Gt)[xi] ); a thread owns two consecutive k (one 4-byte store)
__device__ void wino_weights16_body(const float* __restrict__ w, __bf16* __restrict__ U, int N, int K, const WinoWeights& ww) {
    const int NT = N / WINO_BN, K2 = K >> 1;
    const size_t total = (size_t)N * K2;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int n, k2;
        if (ww.k_fast) { k2 = (int)(idx % K2); n = (int)(idx / K2); }
        else { n = (int)(idx % N); k2 = (int)(idx / N); }
        float u[2][16];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* wp = w + (size_t)n * ww.sn + (size_t)(2 * k2 + h) * ww.sk;
            float g[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int v = 0; v < 3; ++v) g[a][v] = wp[(size_t)(ww.kyu[a] * 3 + ww.kxv[v]) * ww.stap];
            float tg[4][3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                tg[0][v] = g[0][v];
                tg[1][v] = 0.5f * (g[0][v] + g[1][v] + g[2][v]);
                tg[2][v] = 0.5f * (g[0][v] - g[1][v] + g[2][v]);
                tg[3][v] = g[2][v];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                u[h][a * 4 + 0] = tg[a][0];
                u[h][a * 4 + 1] = 0.5f * (tg[a][0] + tg[a][1] + tg[a][2]);
                u[h][a * 4 + 2] = 0.5f * (tg[a][0] - tg[a][1] + tg[a][2]);
                u[h][a * 4 + 3] = tg[a][2];
            }
        }
        const int k = 2 * k2, row = n % WINO_BN;
        __bf16* ub = U + ((size_t)(k >> 4) * NT + n / WINO_BN) * W16_IMG + row * 16 + w16_pos(row, k & 15);
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            bf16x2 v;
            v[0] = (__bf16)u[0][xi];
            v[1] = (__bf16)u[1][xi];
            *reinterpret_cast<bf16x2*>(ub + (size_t)xi * (WINO_BN * 16)) = v;
        }
    }
}
__global__ __launch_bounds__(256) void wino_weights16_kernel(const float* __restrict__ w, __bf16* __restrict__ U, int N, int K,
                                                             WinoWeights ww) {
    wino_weights16_body(w, U, N, K, ww);
}

// FAST: operands through buffer descriptors (scalar step offsets, padding through the bounds check), see wino_kernel
// GATED: a fused activation-backward gate, fetched ahead of the stores (see wino_kernel)
template <bool FAST, bool GATED>
__global__ __launch_bounds__(WINO_THREADS) void wino16_kernel(const IGemmParams p, const WinoGeom q, const __bf16* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* Vh = reinterpret_cast<__bf16*>(smem);              // [2][16][64][16]
    __bf16* Uh = Vh + 2 * W16_IMG;                              // [2][16][64][16]
    float* Ps = smem + (4 * W16_IMG) / 2;                       // [18*18][16] fp32

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    // persistent workgroups over (patch x N tile) work items, distributed exactly as in wino_kernel
    int item, item_end, istep;
    wino_distribute(q.total_work, q.interleave, item, item_end, istep);

    int n0, oy0, ox0, b;
    const __bf16* Ub;
    uint32_t poff[3];
    float pmul[3];
    int i_nt, i_tx, i_ty;
    auto locate = [&]() {
        i_nt = item % q.nt;
        int tile = item / q.nt;
        i_tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        i_ty = tile % q.tiles_y;
        b = tile / q.tiles_y;
    };
    constexpr int NSLOT = WINO_PPIX * 4;          // (pixel, channel quad) slots of the 16-channel patch: 1296
    auto decode = [&]() {
        n0 = i_nt * WINO_BN; oy0 = i_ty * 16; ox0 = i_tx * 16;
        Ub = U + (size_t)i_nt * W16_IMG;
        const int py0 = oy0 + q.sy_min, px0 = ox0 + q.sx_min;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int slot = tid + WINO_THREADS * i;
            const int pp = slot >> 2, spy = pp / 18, spx = pp - spy * 18;
            const int iy = py0 + spy, ix = px0 + spx;
            poff[i] = FAST ? 0x80000000u : 0u;
            pmul[i] = 0.f;
            if (slot < NSLOT && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) {
                const uint32_t pix = ((uint32_t)b * p.IH + iy) * p.IW + ix;
                poff[i] = pix * (uint32_t)p.C + 4 * (slot & 3);
                if constexpr (FAST) poff[i] *= 4u;
                else pmul[i] = p.amask ? p.amask[pix] : 1.f;
            }
        }
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src), 0, FAST ? (int)((size_t)p.B * p.IH * p.IW * p.C * 4) : 0,
                                                         0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(U), 0, FAST ? (int)((size_t)16 * p.N * p.C * 2) : 0, 0x00020000);
    const uint32_t u_voff = tid * 16;
    const bool p2_ok = tid + 2 * WINO_THREADS < NSLOT;
    const int c_begin = blockIdx.z * q.chunks_per_split;
    const int c_end = min(p.C >> 4, c_begin + q.chunks_per_split);
    const int c_last = c_end - 1;
    const size_t ustep = (size_t)q.nt * W16_IMG;        // bf16 elements between consecutive K steps of one N tile

    f32x4 ru[4], rp[3];
    auto pload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if constexpr (FAST) rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, poff[i], c * 64, 0));
            else rp[i] = *reinterpret_cast<const f32x4*>(p.src + poff[i] + c * 16);
        }
    };
    auto uload = [&](int c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (FAST)
                ru[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                    ursrc, u_voff, (int)(((size_t)i_nt * W16_IMG + (size_t)c * ustep) * 2) + 16 * WINO_THREADS * j, 0));
            else
                ru[j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(Ub + (size_t)c * ustep) + 16 * (tid + WINO_THREADS * j));
        }
    };
    auto pstore = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            f32x4 v = rp[i];
            if constexpr (!FAST) {
                v = v * pmul[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = pmul[i] != 0.f ? v[e] : 0.f;     // padding is 0 even next to inf/nan data
            }
            if (i < 2 || p2_ok) *reinterpret_cast<f32x4*>(Ps + 4 * (tid + WINO_THREADS * i)) = v;
        }
    };
    auto ustore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(Uh + buf * W16_IMG) + 16 * (tid + WINO_THREADS * j)) = ru[j];
    };

    // input transform: thread = (tile, channel quad) x rows a = 2*ah, 2*ah+1 of V = Bt d B (ah is wave-uniform)
    //   a = 0: d0 - d2   a = 1: d1 + d2   a = 2: d2 - d1   a = 3: d1 - d3
    const int t_pair = (wave & 3) * 64 + lane, t_quad = t_pair & 3, t_tile = t_pair >> 2, t_ah = wave >> 2;
    const int t_src = ((2 * (t_tile >> 3)) * 18 + 2 * (t_tile & 7)) * 16 + 4 * t_quad;       // + row * 18 * 16 + col * 16
    const int t_dst = t_tile * 16 + w16_pos(t_tile, 4 * t_quad);                                // + xi * 64 * 16
    auto transform = [&](int buf) {
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) {
            const int a = 2 * t_ah + aa;
            // rows ordered so that the first one enters with +1 (a = 2 reads d2 first): one fma per element
            const int r0 = a == 0 ? 0 : (a == 2 ? 2 : 1), r1 = a == 3 ? 3 : (a == 2 ? 1 : 2);
            const float s1 = a == 1 ? 1.f : -1.f;
            f32x4 tt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(Ps + t_src + (r0 * 18 + j) * 16);
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(Ps + t_src + (r1 * 18 + j) * 16);
                tt[j] = d0 + d1 * s1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 v = k == 0 ? tt[0] - tt[2] : k == 1 ? tt[1] + tt[2] : k == 2 ? tt[2] - tt[1] : tt[1] - tt[3];
                *reinterpret_cast<bf16x4*>(Vh + buf * W16_IMG + (a * 4 + k) * (64 * 16) + t_dst) = __builtin_convertvector(v, bf16x4);
            }
        }
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * (64 * 16) + arow * 16 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 3);
    const int b_off = (8 * xh) * (64 * 16) + brow * 16 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 3);

    if (item >= item_end || c_begin >= c_end) return;
    locate();
    decode();
    pload(c_begin);
    uload(c_begin);

    for (;;) {
        f32x16 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

        // step c_begin is staged synchronously while the operands of step c_begin+1 are in flight
        pstore();
        ustore(0);
        pload(min(c_begin + 1, c_last));
        uload(min(c_begin + 1, c_last));
        wino_barrier();
        transform(0);
        wino_barrier();
        int cur = 0;
        for (int c = c_begin; c < c_end; ++c) {
            const int nxt = cur ^ 1;
            // rp / ru hold the raw operands of step c+1.  The patch is single-buffered: every transform read of patch c
            // happened before the barrier that closed the previous step.
            pstore();
            ustore(nxt);
            const int c2 = min(c + 2, c_last);
            pload(c2);
            uload(c2);
            wino_barrier();                                   // patch c+1 visible
            const __bf16* Vc = Vh + cur * W16_IMG + a_off;
            const __bf16* Uc = Uh + cur * W16_IMG + b_off;
#pragma unroll
            for (int xi = 0; xi < 8; ++xi) {
                const bf16x8 fa = *reinterpret_cast<const bf16x8*>(Vc + xi * (64 * 16));
                const bf16x8 fb = *reinterpret_cast<const bf16x8*>(Uc + xi * (64 * 16));
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[xi], 0, 0, 0);
            }
            transform(nxt);                                   // V c+1 (the compiler interleaves it with the MFMAs above)
            wino_barrier();                                   // V / U images of step c+1 complete, images of step c released
            cur = nxt;
        }
        const int e_n0 = n0, e_oy0 = oy0, e_ox0 = ox0, e_b = b;      // output coordinates of the finished item
        const bool more_items = item + istep < item_end;

        // Output transform Y = At M A: as wino_kernel (the xi-halves exchange half of their row sums through LDS; the
        // exchange area and the store scratch overlay the V / U images, all of whose readers are behind the last barrier)
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
        if (more_items) {            // next item's first operands ahead of this item's stores (vmcnt retires in order)
            item += istep;
            locate();
            decode();
            pload(c_begin);
            uload(c_begin);
        }
        wino_barrier();
        // bias, row scales (and the gate) are fetched ahead of the stores: on gfx9 a load behind a store waits for its acknowledgement
        f32x4 bq = {0.f, 0.f, 0.f, 0.f};
        float rsq[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};
        if (p.splits == 1) {
            if (p.bias) bq = *reinterpret_cast<const f32x4*>(p.bias + e_n0 + 32 * nw + 4 * (lane & 7));
            if (p.rowscale) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4) {
                        const int t = 32 * mw + (lane >> 3) + 8 * t4;
                        const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                        rsq[j][t4] = p.rowscale[((size_t)e_b * p.DH + (oy * p.ds + p.dy0)) * p.DW + (ox * p.ds + p.dx0)];
                    }
            }
        }
        f32x4 gq[GATED ? 2 : 1][GATED ? 4 : 1];
        if constexpr (GATED) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int t = 32 * mw + (lane >> 3) + 8 * t4;
                    const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                    const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + p.dy0)) * p.DW + (ox * p.ds + p.dx0);
                    gq[j][t4] = *reinterpret_cast<const f32x4*>(p.gate + pix * p.N + e_n0 + 32 * nw + 4 * (lane & 7));
                }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
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
                    *reinterpret_cast<f32x4*>(p.dst + pix * p.N + nb) = epilogue4(p, v4, pix, nb, GATED ? &gq[GATED ? j : 0][GATED ? t4 : 0] : nullptr, &rsq[j][t4], &bq);
                }
            });
        }
        if (!more_items) break;
        wino_barrier();        // every wave is done with the exchange area / scratch before the next prologue stages into it
    }
}

// bf16 mode: stride-1 3x3, Cin % 16 == 0, Cout % 64 == 0, >= 16x16 outputs
// wino16_kernel<FAST> with the staging pipeline running across work items (see wino_pipe_kernel): the last two K steps of an
// item stage steps 0 and 1 of the workgroup's next item, only the first item has a synchronous prologue, and the output
// transform lives in the image buffers of the step just consumed plus the patch area (output halves one after the other).
// With 16-channel steps a 64-channel layer has FOUR steps per item: the prologue was a quarter of its time.
// POOL: the 2x2 max-pool of the activated output is written with it, exactly as in wino_pipe_kernel<.., POOL> (wino.inc)
// GBITS (with GATED): the ReLU gate as p.gate_bits, exactly as in wino_pipe_kernel<.., GBITS> (wino.inc)
template <bool GATED, bool POOL = false, bool GBITS = false>
__global__ __launch_bounds__(WINO_THREADS) void wino16_pipe_kernel(const IGemmParams p, const WinoGeom q, const __bf16* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* Vh = reinterpret_cast<__bf16*>(smem);              // [2][16][64][16]
    __bf16* Uh = Vh + 2 * W16_IMG;                              // [2][16][64][16]
    float* Ps = smem + (4 * W16_IMG) / 2;                       // [18*18 pixels][16] fp32, 16 floats of padding behind every pixel pair

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    int item, item_end, istep;
    wino_distribute(q.total_work, q.interleave, item, item_end, istep);

    constexpr int NSLOT = WINO_PPIX * 4;          // (pixel, channel quad) slots of the 16-channel patch: 1296
    struct Item { int nt, n0, oy0, ox0, b; uint32_t poff[3]; };
    auto decode_item = [&](int it) {
        Item r;
        r.nt = it % q.nt;
        int tile = it / q.nt;
        const int tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        const int ty = tile % q.tiles_y;
        r.b = tile / q.tiles_y;
        r.n0 = r.nt * WINO_BN; r.oy0 = ty * 16; r.ox0 = tx * 16;
        const int py0 = r.oy0 + q.sy_min, px0 = r.ox0 + q.sx_min;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int slot = tid + WINO_THREADS * i;
            const int pp = slot >> 2, spy = pp / 18, spx = pp - spy * 18;
            const int iy = py0 + spy, ix = px0 + spx;
            r.poff[i] = 0x80000000u;
            if (slot < NSLOT && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW)
                r.poff[i] = ((((uint32_t)r.b * p.IH + iy) * p.IW + ix) * (uint32_t)p.C + 4 * (slot & 3)) * 4u;
        }
        return r;
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src), 0, (int)((size_t)p.B * p.IH * p.IW * p.C * 4), 0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(U), 0, (int)((size_t)16 * p.N * p.C * 2), 0x00020000);
    const bool p2_ok = tid + 2 * WINO_THREADS < NSLOT;
    const int c_begin = blockIdx.z * q.chunks_per_split;
    const int c_end = min(p.C >> 4, c_begin + q.chunks_per_split);
    const size_t ustep = (size_t)q.nt * W16_IMG;        // bf16 elements between consecutive K steps of one N tile

    // B operand: the transformed weights are not staged through LDS -- the global U image has the layout of an LDS image, so a
    // wave fetches the 16 bytes of its own MFMA fragment (row 32 nw + lane % 32, k half lane / 32) of each of its 8 points
    // straight into registers, one K step ahead: 4 LDS writes and 8 of 32 LDS reads per wave and step less (the LDS bounds this
    // kernel's K step), for twice the U bytes through the vector-memory path (the two mw waves fetch the same fragments).
    f32x4 rp[3];
    bf16x8 fb[8];
    auto pload = [&](const Item& it, int c) {
#pragma unroll
        for (int i = 0; i < 3; ++i) rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, it.poff[i], c * 64, 0));
    };
    const uint32_t uf_voff = (uint32_t)(((8 * xh) * (64 * 16) + (32 * nw + (lane & 31)) * 16 +
                                         ((((lane >> 5) ^ ((32 * nw + (lane & 31)) >> 4)) & 1) << 3)) * 2);
    auto uload1 = [&](const Item& it, int c, int xi) {
        fb[xi] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
            ursrc, uf_voff, (int)(((size_t)it.nt * W16_IMG + (size_t)c * ustep + (size_t)xi * (64 * 16)) * 2), 0));
    };
    auto pstore = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < 2 || p2_ok) *reinterpret_cast<f32x4*>(Ps + 4 * tid + (tid >> 3) * 16 + i * (4 * WINO_THREADS + (WINO_THREADS >> 3) * 16)) = rp[i];   // slot s -> 4 s + 16 (s >> 3)
    };
    const int t_pair = (wave & 3) * 64 + lane, t_quad = t_pair & 3, t_tile = t_pair >> 2, t_ah = wave >> 2;
    const int t_src = ((2 * (t_tile >> 3)) * 18 + 2 * (t_tile & 7)) * 24 + 4 * t_quad;              // even pixel index x 24
    const int t_dst = t_tile * 16 + w16_pos(t_tile, 4 * t_quad);
    auto transform = [&](int buf) {
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) {
            const int a = 2 * t_ah + aa;
            const int r0 = a == 0 ? 0 : (a == 2 ? 2 : 1), r1 = a == 3 ? 3 : (a == 2 ? 1 : 2);
            const float s1 = a == 1 ? 1.f : -1.f;
            f32x4 tt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(Ps + t_src + (r0 * 18 + j) * 16 + (r0 * 9 + (j >> 1)) * 16);
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(Ps + t_src + (r1 * 18 + j) * 16 + (r1 * 9 + (j >> 1)) * 16);
                tt[j] = d0 + d1 * s1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 v = k == 0 ? tt[0] - tt[2] : k == 1 ? tt[1] + tt[2] : k == 2 ? tt[2] - tt[1] : tt[1] - tt[3];
                *reinterpret_cast<bf16x4*>(Vh + buf * W16_IMG + (a * 4 + k) * (64 * 16) + t_dst) = __builtin_convertvector(v, bf16x4);
            }
        }
    };
    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * (64 * 16) + arow * 16 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 3);
    const int b_off = (8 * xh) * (64 * 16) + brow * 16 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 3);

    if (item >= item_end || c_begin >= c_end) return;
    Item ci = decode_item(item);
    // prologue of the workgroup's first item
    pload(ci, c_begin);
#pragma unroll
    for (int xi = 0; xi < 8; ++xi) uload1(ci, c_begin, xi);
    pstore();
    pload(ci, c_begin + 1);
    wino_barrier();
    transform(0);
    wino_barrier();
    int cur = 0;

    for (;;) {
        f32x16 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        const bool more_items = item + istep < item_end;
        const Item ni = decode_item(more_items ? item + istep : item);       // the last item restages itself (unused)
        // one K step: the following step's raw operands (in rp / ru) are staged, step c2 of item `it` is requested
        // (uit, uc): the step FOLLOWING the one computed here -- its weight fragments replace those just consumed
        auto kstep = [&](const Item& it, int c2, const Item& uit, int uc) {
            const int nxt = cur ^ 1;
            pstore();
            pload(it, c2);
            wino_barrier();                                   // patch of the following step visible
            const __bf16* Vc = Vh + cur * W16_IMG + a_off;
            // A fragments one point ahead of their MFMA (the matrix instruction of point xi waits for nothing but its own operands)
            bf16x8 fa[2];
            fa[0] = *reinterpret_cast<const bf16x8*>(Vc);
#pragma unroll
            for (int xi = 0; xi < 8; ++xi) {
                if (xi < 7) fa[(xi + 1) & 1] = *reinterpret_cast<const bf16x8*>(Vc + (xi + 1) * (64 * 16));
                __builtin_amdgcn_sched_barrier(0);
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[xi & 1], fb[xi], acc[xi], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                uload1(uit, uc, xi);
            }
            transform(nxt);
            wino_barrier();                                   // images of the following step complete, those of this step released
            cur = nxt;
        };
        for (int c = c_begin; c < c_end - 2; ++c) kstep(ci, c + 2, ci, c + 1);
        kstep(ni, c_begin, ci, c_end - 1);
        kstep(ni, c_begin + 1, ni, c_begin);

        // output transform in the buffers of the step just consumed (cur ^ 1) and the patch area, one output half at a time
        const int fr = cur ^ 1;
        float* X = reinterpret_cast<float*>(Vh + fr * W16_IMG);               // [xh][nw][mw][16][64] floats = 32 KB
        float* scratch = wave < 7 ? reinterpret_cast<float*>(Uh + fr * W16_IMG) + wave * (32 * 36) : Ps;
        // Epilogue addresses as in wino_pipe_kernel (wino.inc): wave-uniform output row, lane-constant column -- buffer
        // instructions with one lane offset per half and scalar row offsets, out-of-range marker beyond the right edge, a scalar
        // branch beyond the bottom edge, activation without a switch per element.  With the bf16 pipe the K steps are short and
        // the per-item epilogue is most of a 64-channel item.
        const int e_wave = __builtin_amdgcn_readfirstlane(wave);
        const int e_mw = e_wave & 1, e_nw = (e_wave >> 1) & 1, e_xh = e_wave >> 2;
        const int e_row0 = ci.oy0 + 8 * e_mw + e_xh;                             // + 2 * t4
        const int e_pitch = p.DW * p.ds;
        const int e_pix0 = (ci.b * p.DH + p.dy0) * p.DW + p.dx0 + ci.ox0 * p.ds;
        const int e_nb0 = ci.n0 + 32 * e_nw;
        const uint32_t e_lane_px = 2 * (lane >> 3) * p.ds;
        const bool e_single = p.splits == 1;
        const float act_neg = p.act == TG_ACT_RELU ? 0.f : (p.act == TG_ACT_LEAKY ? p.slope : 1.f);
        const float gate_neg = p.gate_act == TG_ACT_LEAKY ? p.gate_slope : 0.f;
        const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(p.dst, 0, (int)((size_t)p.B * p.DH * p.DW * p.N * 4), 0x00020000);
        f32x4 bq = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && e_single) bq = *reinterpret_cast<const f32x4*>(p.bias + e_nb0 + 4 * (lane & 7));
        f32x4 pmx[POOL ? 4 : 1];
        uint32_t jbits = 0;            // POOL: bit (4 t4 + e) = the row maximum of that element sits in column j = 1
        if constexpr (POOL) {
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) pmx[t4] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float rsq[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};
        if (p.rowscale && e_single) {
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
                    const uint32_t soff = (uint32_t)(((e_pix0 + row * e_pitch) * p.N + e_nb0) * 4);
                    f32x4 o = (v4 + bq) * rsq[j][t4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f) + act_neg * fminf(o[e], 0.f);     // none / ReLU / leaky
                    if constexpr (GBITS) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] *= (gw[t4] >> e) & 1u ? 1.f : 0.f;
                    } else if constexpr (GATED) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] *= gq[t4][e] > 0.f ? 1.f : gate_neg;
                    }
                    if (p.accumulate) o += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, e_voff + soff, 0, 0));
                    if constexpr (POOL) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool gt = j == 1 && o[e] > pmx[t4][e];           // strictly greater: the first maximum wins
                            pmx[t4][e] = (j == 0 || gt) ? o[e] : pmx[t4][e];
                            jbits |= (gt ? 1u : 0u) << (4 * t4 + e);
                        }
                        if (p.pool_only) return;                                  // dst has no reader left: not written
                    }
                    // row offset in the VECTOR offset: see wino_pipe_kernel (scalar-offset stores and the data-register hazard)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), drsrc, e_voff + soff, 0, 0);
                } else {
                    const int t = 32 * mw + rr;
                    const int oy = ci.oy0 + 2 * (t >> 3) + xh, ox = ci.ox0 + 2 * (t & 7) + j;
                    if (oy >= p.OH || ox >= p.OW) return;
                    const size_t m = ((size_t)ci.b * p.OH + oy) * p.OW + ox;
                    *reinterpret_cast<f32x4*>(p.ws + ((size_t)blockIdx.z * p.M + m) * p.N + ci.n0 + 32 * nw + cc) = v4;
                }
            });
            if constexpr (POOL) {
                // row maxima of the odd rows -> the slot this wave read its partner's sums from (see wino_pipe_kernel)
                if (j == 1 && e_xh == 1) {
                    float* ps = X + ((0 * 2 + nw) * 2 + mw) * 1024 + lane;
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float v = pmx[t4][e];
                            ps[(t4 * 4 + e) * 64] = (p.pool_code && ((jbits >> (4 * t4 + e)) & 1u)) ? -v : v;      // column bit in the sign
                        }
                }
            }
            wino_barrier();                  // X and the scratch areas are free again
        }
        if constexpr (POOL) {
            // (the next item's transform writes X only behind the first barrier of its K step: these reads are ahead of it)
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
                    uint32_t code = 0;                                           // (see wino_pipe_kernel: position of the maximum + ReLU gate)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float raw = pr[(t4 * 4 + e) * 64];
                        const float r0 = pmx[t4][e], r1 = p.pool_code ? fabsf(raw) : raw;
                        const bool row1 = r1 > r0;
                        m[e] = row1 ? r1 : r0;
                        const uint32_t j0 = (jbits >> (4 * t4 + e)) & 1u, j1 = __float_as_uint(raw) >> 31;
                        code |= ((row1 ? 2u + j1 : j0) | (m[e] > 0.f ? 4u : 0u)) << (8 * e);
                    }
                    const int pix = (ci.b * PH + prow) * PW + (ci.ox0 >> 1);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m), prsrc, p_voff + (uint32_t)((pix * p.N + e_nb0) * 4), 0, 0);
                    if (p.pool_code) __builtin_amdgcn_raw_buffer_store_b32(code, crsrc, c_voff + (uint32_t)(pix * p.N + e_nb0), 0, 0);
                }
            }
        }
        if (!more_items) break;
        item += istep;
        ci = ni;
    }
}

// =================================================================================================
// Winograd wgrad F(3x3,2x2) with bf16 MFMA operands (bf16 mode):  dW = Gt [ sum_tiles (A dY At) (.) (Bt X B) ] G
// =================================================================================================
// The algebra, the (co tile, ci tile, split) work decomposition, the dU slabs and the reduce kernel are wino_wgrad_kernel's;
// both transforms stay fp32 and the transformed operands are rounded to bf16 once, at their LDS store.  A K step is a strip of
// SIXTEEN tiles (32 x 2 output pixels) -- the 16-deep v_mfma_f32_32x32x16_bf16 -- so one MFMA per transform point and step
// replaces the eight fp32 MFMAs of two 8-tile steps: the matrix pipe is idle most of the time and the kernel runs at the speed
// of its transform stage, which handles twice the tiles per instruction: a thread owns a PAIR of tiles (the two k-slots of one
// 4-byte image word), one channel quad and one row of the transform.  Images are single-buffered (2 x 32 KB) next to the raw
// fp32 strips (4 x 34 and 2 x 32 pixels x 64 channels, 72-float pitch): per step  barrier | transform | barrier | 8 MFMAs per
// wave + the next strip's raw store + the load of the strip after next.  The channel quads of a raw pixel are rotated by
// (pixel >> 2) so that the eight tile pairs of a wave read eight different 16-byte slots (a 72-float pitch alone puts
// pixels 4 apart on the same banks).
constexpr int W16G_XR = 4 * 34 * WG_PITCH;            // floats
constexpr int W16G_DR = 2 * 32 * WG_PITCH;
constexpr size_t W16G_LDS_BYTES = 2 * (size_t)W16_IMG * 2 + (size_t)(W16G_XR + W16G_DR) * 4;      // 123,136 B

__global__ __launch_bounds__(WINO_THREADS) void wino16_wgrad_kernel(const WgradParams p, const WinoWgradGeom q, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* Ah = reinterpret_cast<__bf16*>(smem);       // [16][64][16]   Yt, rows = co (permuted)
    __bf16* Bh = Ah + W16_IMG;                          // [16][64][16]   V,  rows = ci (permuted)
    float* Xr = smem + W16_IMG;                         // raw strip of x:  [4][34][WG_PITCH]   (2 * W16_IMG bf16 = W16_IMG floats)
    float* Dr = Xr + W16G_XR;                           // raw strip of dy: [2][32][WG_PITCH]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    const int work = xcd_remap(blockIdx.x, q.ntco * q.ntci * q.splits);
    const int tco = work % q.ntco, tci = (work / q.ntco) % q.ntci, split = work / (q.ntco * q.ntci);
    const int s_begin = split * q.steps_per_split;
    const int s_end = min(q.nstrips, s_begin + q.steps_per_split);

    // transform role: tile pair kp (tiles 2kp, 2kp+1 of the strip), channel quad qd, row a of the 4x4 transform (wave-uniform)
    const int kp = lane & 7, qd = (lane >> 3) + 8 * (wave & 1), a = wave >> 1;
    const int r0 = a == 0 ? 0 : (a == 2 ? 2 : 1), r1 = a == 3 ? 3 : (a == 2 ? 1 : 2);
    const float xs1 = a == 1 ? 1.f : -1.f;                                              // Bt row a = d[r0] + xs1*d[r1]
    int icol[4];          // bf16 element offset of channel e's image row (qd + 16 e) at k-slot 2kp, + xi * 1024
#pragma unroll
    for (int e = 0; e < 4; ++e) icol[e] = (4 * a) * 1024 + (qd + 16 * e) * 16 + w16_pos(qd + 16 * e, 2 * kp);
    // raw reads: pixel px of a strip row keeps its quads rotated by (px >> 2); this thread's pixels are 4kp + j
    auto rq = [&](int px) { return 4 * ((qd + (px >> 2)) & 15); };

    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((size_t)p.B * p.H * p.W * p.C * 4), 0x00020000);
    const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)((size_t)p.B * p.Ho * p.Wo * p.Cout * 4), 0x00020000);
    const uint32_t OOB = 0xFFFFFFF0u;

    // raw staging slots: (pixel slot, channel quad), a thread per 16 bytes: 4*34 = 136 pixels of x, 2*32 = 64 of dy
    int xs_r[5], xs_px[5], xs_lds[5];
    bool xs_on[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int idx = tid + WINO_THREADS * i;
        const int ps = idx >> 4;
        xs_on[i] = ps < 4 * 34;
        xs_r[i] = ps / 34;
        xs_px[i] = ps - xs_r[i] * 34;
        xs_lds[i] = ps * WG_PITCH + 4 * (((idx & 15) + (xs_px[i] >> 2)) & 15);
    }
    const uint32_t xs_ch = (uint32_t)(tci * 64 + 4 * (tid & 15)) * 4u;
    int ds_i[2], ds_px[2], ds_lds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + WINO_THREADS * i;
        const int ps = idx >> 4;
        ds_i[i] = ps >> 5;
        ds_px[i] = ps & 31;
        ds_lds[i] = ps * WG_PITCH + 4 * (((idx & 15) + (ds_px[i] >> 2)) & 15);
    }
    const uint32_t ds_ch = (uint32_t)(tco * 64 + 4 * (tid & 15)) * 4u;

    f32x4 rx[5], rd[2];
    int ls = s_begin, lsx = s_begin % q.strips_x, lty = (s_begin / q.strips_x) % q.tiles_y, lb = s_begin / (q.strips_x * q.tiles_y);
    auto raw_load = [&]() {      // raw pixels of strip ls -> rx / rd (out of range, or past this split's range: 0)
        const bool live = ls < s_end;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int py = 2 * lty - p.pad + xs_r[i], px = 32 * lsx - p.pad + xs_px[i];
            const bool ok = live && xs_on[i] && py >= 0 && py < p.H && px >= 0 && px < p.W;
            const uint32_t off = ok ? (((uint32_t)(lb * p.H + py) * p.W + px) * (uint32_t)p.C) * 4u + xs_ch : OOB;
            rx[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oy = 2 * lty + ds_i[i], ox = 32 * lsx + ds_px[i];
            const bool ok = live && oy < p.Ho && ox < p.Wo;
            const uint32_t off = ok ? (((uint32_t)(lb * p.Ho + oy) * p.Wo + ox) * (uint32_t)p.Cout) * 4u + ds_ch : OOB;
            rd[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, off, 0, 0));
        }
        ++ls;
        if (++lsx == q.strips_x) { lsx = 0; if (++lty == q.tiles_y) { lty = 0; ++lb; } }
    };
    auto raw_store = [&]() {
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (xs_on[i]) *reinterpret_cast<f32x4*>(Xr + xs_lds[i]) = rx[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(Dr + ds_lds[i]) = rd[i];
    };
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    auto put = [&](__bf16* img, int b, const f32x4& v0, const f32x4& v1) {      // point (a, b): tiles 2kp / 2kp+1 -> one word per channel
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bf16x2 w;
            w[0] = (__bf16)v0[e];
            w[1] = (__bf16)v1[e];
            *reinterpret_cast<bf16x2*>(img + b * 1024 + icol[e]) = w;
        }
    };
    auto transform = [&]() {
        {   // V = Bt X B: rows r0, r1 of the two tiles' 4 x 6 pixels -> row a, then the column pass per tile
            f32x4 tt[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int px = 4 * kp + j;
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(Xr + (r0 * 34 + px) * WG_PITCH + rq(px));
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(Xr + (r1 * 34 + px) * WG_PITCH + rq(px));
                tt[j] = d0 + d1 * xs1;
            }
            put(Bh, 0, tt[0] - tt[2], tt[2] - tt[4]);
            put(Bh, 1, tt[1] + tt[2], tt[3] + tt[4]);
            put(Bh, 2, tt[2] - tt[1], tt[4] - tt[3]);
            put(Bh, 3, tt[1] - tt[3], tt[3] - tt[5]);
        }
        {   // Yt = A dY At: rows D0, D1 of the two tiles' 2 x 4 pixels -> row a (D0, D0 + D1, D0 - D1, -D1), then columns
            f32x4 rr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = 4 * kp + j;
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(Dr + px * WG_PITCH + rq(px));
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(Dr + (32 + px) * WG_PITCH + rq(px));
                rr[j] = a == 0 ? d0 : a == 1 ? d0 + d1 : a == 2 ? d0 - d1 : -d1;
            }
            put(Ah, 0, rr[0], rr[2]);
            put(Ah, 1, rr[0] + rr[1], rr[2] + rr[3]);
            put(Ah, 2, rr[0] - rr[1], rr[2] - rr[3]);
            put(Ah, 3, -rr[1], -rr[3]);
        }
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = (8 * xh) * 1024 + arow * 16 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 3);
    const int b_off = (8 * xh) * 1024 + brow * 16 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 3);

    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    if (s_begin < s_end) {
        raw_load();                 // strip s_begin
        raw_store();
        raw_load();                 // strip s_begin + 1
        for (int s = s_begin; s < s_end; ++s) {
            wino_barrier();         // raw strip s visible; the MFMAs of step s-1 are done with the images
            transform();
            wino_barrier();         // images of strip s complete; the raw area is free
            raw_store();            // strip s+1
            raw_load();             // strip s+2
#pragma unroll
            for (int xi = 0; xi < 8; ++xi) {
                const bf16x8 fa = *reinterpret_cast<const bf16x8*>(Ah + a_off + xi * 1024);
                const bf16x8 fb = *reinterpret_cast<const bf16x8*>(Bh + b_off + xi * 1024);
                acc[xi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[xi], 0, 0, 0);
            }
        }
    }
    // dU slab of this (split, ci tile, co tile): [xi][row 64][col 64], raw accumulator layout (the fp32 kernel's)
    float* slab = slabs + ((size_t)work * 16 + 8 * xh) * 4096;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * mw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            slab[(size_t)i * 4096 + row * 64 + 32 * nw + (lane & 31)] = acc[i][r];
        }
}

static bool wino16_wgrad_ok(const TgConv* g, const float* in_mask) {
    static const bool off = getenv("TG_NO_WINO") != nullptr || getenv("TG_NO_WINO_WGRAD") != nullptr || getenv("TG_NO_WINO16") != nullptr ||
                            getenv("TG_NO_WINO16_WGRAD") != nullptr;
    if (off || in_mask != nullptr || g->precision != TG_PREC_BF16) return false;
    if (g->k != 3 || g->stride != 1 || (g->Cin % 64) != 0 || (g->Cout % 64) != 0 || g->Ho < 16 || g->Wo < 32) return false;
    if ((size_t)g->B * g->H * g->W * g->Cin * 4 >= ((size_t)1 << 31) || (size_t)g->B * g->Ho * g->Wo * g->Cout * 4 >= ((size_t)1 << 31))
        return false;         // 32-bit buffer offsets
    return true;
}
static WinoWgradGeom wino16_wgrad_plan(const TgConv* g) {
    WinoWgradGeom q = {};
    q.strips_x = cdiv(g->Wo, 32);
    q.tiles_y = cdiv(g->Ho, 2);
    q.nstrips = g->B * q.tiles_y * q.strips_x;
    q.ntco = g->Cout / 64;
    q.ntci = g->Cin / 64;
    const int tiles = q.ntco * q.ntci;
    int smax = q.nstrips / 4 < 512 ? q.nstrips / 4 : 512;      // at least 4 (16-tile) strips per split
    if (smax < 1) smax = 1;
    const int splits = choose_splits_k(tiles, smax, WINO_PLAN_CUS, q.nstrips, 0.03);
    q.steps_per_split = cdiv(q.nstrips, splits);
    q.splits = cdiv(q.nstrips, q.steps_per_split);
    return q;
}
static size_t wino16_wgrad_ws_floats(const TgConv* g) {
    if (!wino16_wgrad_ok(g, nullptr)) return 0;
    const WinoWgradGeom q = wino16_wgrad_plan(g);
    return (size_t)q.splits * q.ntco * q.ntci * 16 * 4096;
}
static int launch_wino16_wgrad(const TgConv* g, const WgradParams& p, float* dw, float* ws, hipStream_t s) {
    const WinoWgradGeom q = wino16_wgrad_plan(g);
    static LdsOptIn opt;
    if (int rc = lds_opt_in(opt, reinterpret_cast<const void*>(wino16_wgrad_kernel), W16G_LDS_BYTES, "wino16 wgrad")) return rc;
    {
        const double by = 4.0 * ((double)p.B * p.H * p.W * p.C + (double)p.Mpix * p.Cout + (double)p.Cout * p.Ktot);
        ProfScope ps(s, 3, 2.0 * p.Mpix * (double)p.Cout * p.Ktot * g_alg_scale, by, p.Cout, p.Ktot, p.Mpix, p.C, q.splits, 4116);
        ps.r.route = WR_WGRAD;
        hipLaunchKernelGGL(wino16_wgrad_kernel, dim3(q.ntco * q.ntci * q.splits), dim3(WINO_THREADS), W16G_LDS_BYTES, s, p, q, ws);
    }
    TG_CHECK_LAUNCH("wino16_wgrad_kernel");
    hipLaunchKernelGGL(wino_wgrad_reduce_kernel, dim3(ew_grid((int64_t)g->Cout * g->Cin, 256)), dim3(256), 0, s, ws, dw, g->Cout,
                       g->Cin, q.ntco, q.ntci, q.splits);
    TG_CHECK_LAUNCH("wino_wgrad_reduce_kernel");
    return TG_OK;
}
