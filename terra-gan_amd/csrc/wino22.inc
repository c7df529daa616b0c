// Winograd F(2x2,2x2) on the fp32 MFMA for the 4x4 / stride-2 / pad-1 convolutions (the PatchGAN discriminator,
// discriminator.py:17-23) -- included by igemm.hip after wino.inc, whose helpers it uses.
//
// Over the space-to-depth view shifted by the padding,  x2[b][yy][xx][(dy,dx,c)] = x[b][2yy+dy-1][2xx+dx-1][c]  (0 outside),
// a 4x4 / stride-2 / pad-1 convolution is EXACTLY a 2x2 / stride-1 "valid" convolution over 4*Cin channels with
// w2[co][ty][tx][(dy,dx,c)] = w[co][2ty+dy][2tx+dx][c].  Its input gradient splits into four parity classes
// dx[2yy'+1-dy][2xx'+1-dx][c] = sum_{ty,tx,co} w[co][2ty+dy][2tx+dx][c] * g[yy'+1-dy-ty][xx'+1-dx-tx][co], each again a
// 2x2 stride-1 convolution (now over the Cout channels of the output gradient, taps flipped).  For a 2x2 kernel
//     Y = At [ (G g Gt) (.) (Bt d B) ] A,   Bt = [[1,-1,0],[0,1,0],[0,-1,1]],  G = [[1,0],[1,1],[0,1]],  At = [[1,1,0],[0,1,1]]
// needs 9 products per 2x2 output tile instead of 16: 1.78x fewer multiplies, every transform coefficient +-1 (no rounding
// beyond the sums), on the layers the gathered-row / patch kernels ran at ~110 TF.
//
// Structure = wino_kernel: one 512-thread workgroup per CU owns 16x16 outputs (8x8 tiles) x 64 channels; K is walked in
// 8-channel steps through double-buffered LDS images V[9][64 tiles][8] / U[9][64 ch][8]; the input patch is 17x17 pixels.
// The 9 transform points are split 6 : 3 between the two waves of a SIMD (xh = 0: rows a = 0,1 of the 3x3 point grid,
// xh = 1: row a = 2) -- the matrix pipe is per SIMD, so the uneven split costs nothing -- and the output transform needs
// only ONE exchange: Y[0][.] = s0 + s1 is local to the xh = 0 waves, Y[1][.] = s1 + s2 takes s1 from them.
// The forward pass gathers its patch straight through the space-to-depth view (a K step lies inside one parity phase; the
// per-slot offsets and bounds are re-derived when the phase changes, every Cin/8 steps): no rearranged copy of x exists.
#pragma once

struct W22Geom {
    int tiles_x, tiles_y, total_work, chunks_per_split, nt;
    int sy_min, sx_min;
    int s2d;            // 1: the input is the shifted space-to-depth view of p.src = [B][XH][XW][XC]
    int XH, XW, XC;
    int interleave;     // work distribution, see wino_distribute
    int* qctr;          // work-stealing counter block of this launch (nullptr: static), see WinoWork (wino.inc)
    int ncls;           // 4: the parity classes of a dgrad in one launch -- class (cdy, cdx) reads from (-cdy, -cdx) and
                        // writes dst pixel (2*oy + 1 - cdy, 2*ox + 1 - cdx); 1: geometry from IGemmParams
};
// (struct W22Weights lives in wino.inc, next to the batched-preparation descriptor that embeds it)
constexpr int W22_PTS = 9;
constexpr int W22_V = W22_PTS * 64 * 8;        // floats of one V (or U) image: 4608
constexpr int W22_PPIX = 17 * 17;
constexpr int W22_P = W22_PPIX * 8;            // 2312
constexpr int W22_LDS_FLOATS = 4 * W22_V + W22_P + 8;     // 20752 floats = 83 KB

// U[class][k/8][n/64][xi][n%64][k%8 (half-swizzled)] = (G g Gt)[xi]
__device__ void wino22_weights_body(const float* __restrict__ w, float* __restrict__ U, int N, int K, const W22Weights& ww) {
    const int NT = N / WINO_BN;
    const size_t per = (size_t)N * K, total = per * ww.ncls;
    for (size_t idx0 = (size_t)blockIdx.x * 256 + threadIdx.x; idx0 < total; idx0 += (size_t)gridDim.x * 256) {
        const int cls = (int)(idx0 / per);
        const size_t idx = idx0 - cls * per;
        // thread order = the order of the U image (see wino_weights_body): 2 KB write runs
        const int blk = (int)(idx >> 9), KC = K >> 3;
        const int k = (blk % KC) * 8 + (int)(idx & 7), n = (blk / KC) * WINO_BN + (int)((idx >> 3) & 63);
        const int ph = ww.by_phase ? k / ww.cin : cls, kc = ww.by_phase ? k - ph * ww.cin : k;
        const int dy = ph >> 1, dx = ph & 1;
        const float* wp = w + (size_t)n * ww.sn + (size_t)kc * ww.sk;
        float g[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) g[u][v] = wp[(size_t)((2 * ww.tyu[u] + dy) * 4 + (2 * ww.txv[v] + dx)) * ww.cin];
        const int row = n % WINO_BN;
        float* ub = U + cls * (per * W22_PTS) + ((size_t)(k >> 3) * NT + n / WINO_BN) * W22_V + row * 8 + wino_swz(row, k & 7);
        const float r0[3] = {g[0][0], g[0][0] + g[0][1], g[0][1]};
        const float r2[3] = {g[1][0], g[1][0] + g[1][1], g[1][1]};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            ub[(0 * 3 + b) * (WINO_BN * 8)] = r0[b];
            ub[(1 * 3 + b) * (WINO_BN * 8)] = r0[b] + r2[b];
            ub[(2 * 3 + b) * (WINO_BN * 8)] = r2[b];
        }
    }
}
__global__ __launch_bounds__(256) void wino22_weights_kernel(const float* __restrict__ w, float* __restrict__ U, int N, int K,
                                                             W22Weights ww) {
    wino22_weights_body(w, U, N, K, ww);
}

// FAST (no source mask, source and U below 2 GB): operands through buffer descriptors, see wino_kernel
// GATED: a fused activation-backward gate, fetched ahead of each half's stores (see wino_kernel)
template <bool FAST, bool GATED, bool STEAL>
__global__ __launch_bounds__(WINO_THREADS) void wino22_kernel(const IGemmParams p, const W22Geom q, const float* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                            // [2][9][64][8]
    float* Us = smem + 2 * W22_V;                // [2][9][64][8]
    float* Ps = smem + 4 * W22_V;                // [17*17][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: role branches are s_cbranch
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    __shared__ int wq_slot[2];
    WinoWork<STEAL> wk;
    wk.init(q.total_work, q.interleave, q.qctr, wq_slot);

    int n0, oy0, ox0, b, cls;
    const float* Ub;
    // patch slots of this thread (pixel, channel quad): the pixel is fixed per item, offset / validity per parity phase
    int s_iy[2], s_ix[2];
    int32_t poff[2];
    float pmul[2];
    int i_nt, i_tx, i_ty;
    auto locate = [&]() {       // item = (image, patch y, patch x, class, N tile), N tile fastest: the four classes of a dgrad
        const int item = wk.item;
        i_nt = item % q.nt;     // read (nearly) the same patch of dy, so they sit next to each other
        int tile = item / q.nt;
        cls = tile % q.ncls;
        tile /= q.ncls;
        i_tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        i_ty = tile % q.tiles_y;
        b = tile / q.tiles_y;
    };
    const bool p1_ok = ((tid + WINO_THREADS) >> 1) < W22_PPIX;
    // offsets (floats, without the channel offset of the step) and 0/1 validity of the slots for parity phase ph
    auto set_phase = [&](int ph) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int iy = s_iy[i], ix = s_ix[i], H = p.IH, W = p.IW, Cc = p.C;
            if (q.s2d) {
                iy = 2 * iy + (ph >> 1) - 1;
                ix = 2 * ix + (ph & 1) - 1;
                H = q.XH; W = q.XW; Cc = q.XC;
            }
            const bool ok = (i == 0 || p1_ok) && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int32_t pix = ok ? (b * H + iy) * W + ix : 0;
            poff[i] = pix * Cc + 4 * (tid & 1);
            if constexpr (FAST) poff[i] = ok ? poff[i] * 4 : (int32_t)0x80000000u;      // byte offset; out of range = beyond 2 GB
            else pmul[i] = ok ? (p.amask ? p.amask[pix] : 1.f) : 0.f;
        }
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.src), 0, FAST ? (int)(q.s2d ? (size_t)p.B * q.XH * q.XW * q.XC * 4 : (size_t)p.B * p.IH * p.IW * p.C * 4) : 0, 0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U), 0, FAST ? (int)((size_t)q.ncls * W22_PTS * p.N * p.C * 4) : 0,
                                                         0x00020000);
    auto decode = [&]() {
        n0 = i_nt * WINO_BN; oy0 = i_ty * 16; ox0 = i_tx * 16;
        Ub = U + (size_t)cls * ((size_t)W22_PTS * p.N * p.C) + (size_t)i_nt * W22_V;
        const int py0 = oy0 + (q.ncls > 1 ? -(cls >> 1) : q.sy_min), px0 = ox0 + (q.ncls > 1 ? -(cls & 1) : q.sx_min);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (tid + WINO_THREADS * i) >> 1, spy = pp / 17, spx = pp - spy * 17;
            s_iy[i] = py0 + spy;
            s_ix[i] = px0 + spx;
        }
    };
    const int c_begin = blockIdx.z * q.chunks_per_split;
    const int c_end = min(p.C >> 3, c_begin + q.chunks_per_split);
    const int c_last = c_end - 1;
    const size_t ustep = (size_t)q.nt * W22_V;
    const int cpp = q.s2d ? (q.XC >> 3) : (p.C >> 3);       // K steps per parity phase
    const int ph_begin = c_begin / cpp;

    f32x4 ru[3], rp[2];
    int cur_ph, c_base, c_next;       // phase of the patch loads in flight, its first step, first step of the next phase
    auto start_phase = [&](int ph) { cur_ph = ph; c_base = ph * cpp; c_next = c_base + cpp; set_phase(ph); };
    auto pload1 = [&](int c, int i) {
        if constexpr (FAST) rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, poff[i], (c - c_base) * 32, 0));
        else rp[i] = *reinterpret_cast<const f32x4*>(p.src + poff[i] + (c - c_base) * 8);
    };
    // the third quarter of the U image is 128 float4 only: the other threads re-read their first one (no branch around a load)
    const int u_idx[3] = {tid, tid + WINO_THREADS, tid < 128 ? tid + 2 * WINO_THREADS : tid};
    const size_t u_base = (size_t)W22_PTS * p.N * p.C;       // floats of one class's U
    auto uload1 = [&](int c, int j) {
        if constexpr (FAST)
            ru[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                ursrc, 16 * u_idx[j], (int)(((size_t)cls * u_base + (size_t)i_nt * W22_V + (size_t)c * ustep) * 4), 0));
        else ru[j] = *reinterpret_cast<const f32x4*>(Ub + (size_t)c * ustep + 4 * u_idx[j]);
    };
    auto pstore1 = [&](int i) {
        f32x4 v = rp[i];
        if constexpr (!FAST) {
            v = v * pmul[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pmul[i] != 0.f ? v[e] : 0.f;
        }
        if (i == 0 || p1_ok) *reinterpret_cast<f32x4*>(Ps + 4 * (tid + WINO_THREADS * i)) = v;
    };
    auto ustore1 = [&](int buf, int j) {
        if (j < 2 || tid < 128) *reinterpret_cast<f32x4*>(Us + buf * W22_V + 4 * (tid + WINO_THREADS * j)) = ru[j];
    };

    // input transform: thread = (tile, channel quad, row a of V = Bt d B), a = wave >> 1 (waves 0..5; waves 6,7 have no role)
    //   a = 0: d0 - d1   a = 1: d1   a = 2: d2 - d1
    const int t_quad = lane & 1, t_tile = (lane >> 1) + 32 * (wave & 1), t_a = min(wave >> 1, 2);
    const bool t_on = wave < 6;
    const int t_src0 = ((2 * (t_tile >> 3) + t_a) * 17 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_src1 = ((2 * (t_tile >> 3) + 1) * 17 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_dst = (t_a * 3) * 512 + t_tile * 8 + (((t_quad ^ (t_tile >> 4)) & 1) << 2);
    f32x4 td[2][3], tt[3];
    auto t_read1 = [&](int k) {     // k = 0..5: (row k/3, column k%3)
        td[k / 3][k % 3] = *reinterpret_cast<const f32x4*>(Ps + ((k / 3) ? t_src1 : t_src0) + (k % 3) * 8);
    };
    auto t_row1 = [&](int j) {
        if (t_a == 1) tt[j] = td[0][j];
        else tt[j] = td[0][j] - td[1][j];
    };
    auto t_col1 = [&](int buf, int k) {
        const f32x4 v = k == 0 ? tt[0] - tt[1] : k == 1 ? tt[1] : tt[2] - tt[1];
        *reinterpret_cast<f32x4*>(Vs + buf * W22_V + t_dst + k * 512) = v;
    };

    const int pt0 = xh == 0 ? 0 : 6;
    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = pt0 * 512 + arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = pt0 * 512 + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    if (wk.item < 0 || c_begin >= c_end) { wk.done(q.qctr); return; }
    locate();
    decode();
    start_phase(ph_begin);
#pragma unroll
    for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) uload1(c_begin, j);

    for (;;) {
        f32x16 acc[6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        {
            // prologue: rp / ru hold step c_begin; it is staged synchronously while the operands of step c_begin+1 fly
#pragma unroll
            for (int i = 0; i < 2; ++i) pstore1(i);
#pragma unroll
            for (int j = 0; j < 3; ++j) ustore1(0, j);
            {
                const int c1 = min(c_begin + 1, c_last);
                if (c1 >= c_next) start_phase(cur_ph + 1);
#pragma unroll
                for (int i = 0; i < 2; ++i) pload1(c1, i);
#pragma unroll
                for (int j = 0; j < 3; ++j) uload1(c1, j);
            }
            wino_barrier();
            if (t_on) {
#pragma unroll
                for (int k = 0; k < 6; ++k) t_read1(k);
#pragma unroll
                for (int j = 0; j < 3; ++j) t_row1(j);
#pragma unroll
                for (int k = 0; k < 3; ++k) t_col1(0, k);
            }
            wino_barrier();
            f32x4 fa[2], fb[2];
            fa[0] = *reinterpret_cast<const f32x4*>(Vs + a_off);
            fb[0] = *reinterpret_cast<const f32x4*>(Us + b_off);
            int cur = 0;
            for (int c = c_begin; c < c_end; ++c) {
                const int nxt = cur ^ 1;
                const int c2 = min(c + 2, c_last);               // tail steps: redundant staging instead of branches
                const float* Vc = Vs + cur * W22_V + a_off;
                const float* Uc = Us + cur * W22_V + b_off;
                const float* Vn = Vs + nxt * W22_V + a_off;
                const float* Un = Us + nxt * W22_V + b_off;
                // 24 ticks: t = 4*xi + e.  The xh = 0 waves own 6 transform points (24 MFMAs), the xh = 1 waves 3 (12):
                // the two share a SIMD, i.e. one matrix pipe, so only the sum of 36 matters.
                wino_static_for(std::make_integer_sequence<int, 24>{}, [&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    constexpr int xi = t >> 2, e = t & 3;
                    if constexpr (t < 2) pstore1(t);                           // patch c+1 -> LDS (readers of patch c are done)
                    if constexpr (t == 2) {                                    // patch c+2 -> rp; new slot offsets on a phase change
                        if (c2 >= c_next) start_phase(cur_ph + 1);
                        pload1(c2, 0);
                    }
                    if constexpr (t == 3) pload1(c2, 1);
                    if constexpr (t == 4) wino_barrier();                      // patch c+1 visible
                    if constexpr (t >= 5 && t < 8) { if (t_on) { t_read1(t - 5); t_read1(3 + t - 5); } }
                    if constexpr (t >= 8 && t < 11) { if (t_on) t_row1(t - 8); }
                    if constexpr (t >= 12 && t < 15) { if (t_on) t_col1(nxt, t - 12); }
                    if constexpr (t >= 15 && t < 18) ustore1(nxt, t - 15);
                    if constexpr (t >= 18 && t < 21) uload1(c2, t - 18);       // U c+2 -> ru
                    if constexpr (t == 21) wino_barrier();                     // V / U images of step c+1 complete
                    if constexpr (e == 0 && xi < 5) {
                        if (xi + 1 < 3 || xh == 0) {
                            fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Vc + (xi + 1) * 512);
                            fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Uc + (xi + 1) * 512);
                        }
                    }
                    if constexpr (t == 22) {
                        fa[0] = *reinterpret_cast<const f32x4*>(Vn);
                        fb[0] = *reinterpret_cast<const f32x4*>(Un);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (xi < 3 || xh == 0) acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                });
                cur = nxt;
            }
        }
        const int e_n0 = n0, e_oy0 = oy0, e_ox0 = ox0, e_b = b, e_cls = cls;      // output coordinates of the finished item
        const int wq_next = wk.next(wq_slot);
        const bool more_items = wq_next >= 0;
        const int wq_pulled = wk.request(wq_next);
        wino_barrier();        // the exchange area and the epilogue scratch overlay V / U

        // Output transform Y = At M A over the 3x3 points M: row sums s[a][j] = M[a][j] + M[a][j+1].  The xh = 0 waves hold
        // a = 0,1: Y[0][j] = s0j + s1j is theirs and s1j goes to the partner; the xh = 1 waves hold a = 2: Y[1][j] = s1j + s2j.
        float* X = smem;                                         // [nw][mw][j][16][64]
        float* scratch = smem + 2 * W22_V + wave * (32 * 36);
        f32x16 own[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float* xs = X + ((nw * 2 + mw) * 2 + j) * 1024 + lane;
            if (xh == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s0 = acc[j][r] + acc[j + 1][r], s1 = acc[3 + j][r] + acc[4 + j][r];
                    own[j][r] = s0 + s1;
                    xs[r * 64] = s1;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) own[j][r] = acc[j][r] + acc[j + 1][r];
            }
        }
        // the accumulators are dead: switch the staging state to the next item and request its first operands ahead of the stores
        if (more_items) {
            wk.item = wq_next;
            locate();
            decode();
            start_phase(ph_begin);
#pragma unroll
            for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
            for (int j = 0; j < 3; ++j) uload1(c_begin, j);
        }
        wino_barrier();
        const int e_dy0 = q.ncls > 1 ? 1 - (e_cls >> 1) : p.dy0, e_dx0 = q.ncls > 1 ? 1 - (e_cls & 1) : p.dx0;
        // (this kernel has the registers to fetch the gate quads of BOTH halves before the first store)
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
                        rsq[j][t4] = p.rowscale[((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0)];
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
                    const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0);
                    gq[j][t4] = *reinterpret_cast<const f32x4*>(p.gate + pix * p.N + e_n0 + 32 * nw + 4 * (lane & 7));
                }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x16 y = own[j];
            if (xh == 1) {
                const float* xr = X + ((nw * 2 + mw) * 2 + j) * 1024 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) y[r] += xr[r * 64];
            }
            tile_rows4i(scratch, y, lane, [&](int t4, int rr, int cc, f32x4 v4) {
                const int t = 32 * mw + rr;
                const int oy = e_oy0 + 2 * (t >> 3) + xh, ox = e_ox0 + 2 * (t & 7) + j;
                const int nb = e_n0 + 32 * nw + cc;
                if (oy >= p.OH || ox >= p.OW) return;
                if (p.splits > 1) {      // slabs: [class][split][M][N]
                    const size_t m = ((size_t)e_b * p.OH + oy) * p.OW + ox;
                    *reinterpret_cast<f32x4*>(p.ws + (((size_t)e_cls * p.splits + blockIdx.z) * p.M + m) * p.N + nb) = v4;
                } else {
                    const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0);
                    *reinterpret_cast<f32x4*>(p.dst + pix * p.N + nb) = epilogue4(p, v4, pix, nb, GATED ? &gq[GATED ? j : 0][GATED ? t4 : 0] : nullptr, &rsq[j][t4], &bq);
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

// The wide form: item = (image, 16x16 output patch, class, 128-channel N tile).  Wave (mw, nw = 0..3) owns 32 tiles x 32 channels
// x ALL nine transform points (144 accumulator registers), so a K step stages the patch and the V image once for two of the
// narrow kernel's N tiles and carries 72 MFMAs per SIMD instead of 36; only the U copy doubles.  The U image of a step is two
// adjacent 64-channel blocks of the prepared layout (N tiles 2i, 2i+1 follow each other in U[k/8][n/64]), i.e. one contiguous
// run of 2 x W22_V floats: the prepared weights are the narrow kernel's.  K order, the 8-channel steps and the MFMA chain of a
// point are the narrow kernel's, and a wave holds all three point rows of its tiles, so the output transform needs no exchange
// and gives the same bits: Y[0][j] = s0j + s1j, Y[1][j] = s1j + s2j with s[a][j] = M[a][j] + M[a][j+1].
// Sources are read through buffer descriptors only (the narrow kernel's FAST form): masked sources stay on the narrow kernel,
// and so does every split-K launch (launch_wino22 has the rule).  The kernel sits close to the 256 registers a 512-thread
// workgroup has: DESIGN 8z lists what keeps it free of scratch (no values assigned under wave-role branches in the K loop,
// thread-index arithmetic re-derived behind opaque copies instead of being held across the loop, epilogue operands a tile at a time).
constexpr int W22W_U = 2 * W22_V;                                  // floats of one wide U image: 9216
constexpr int W22W_LDS_FLOATS = 2 * W22_V + 2 * W22W_U + W22_P + 8;    // 29968 floats = 120 KB

template <bool GATED, bool STEAL>
__global__ __launch_bounds__(WINO_THREADS) void wino22w_kernel(const IGemmParams p, const W22Geom q, const float* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                            // [2][9][64][8]
    float* Us = smem + 2 * W22_V;                // [2][2][9][64][8]
    float* Ps = smem + 2 * W22_V + 2 * W22W_U;   // [17*17][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mw = wave & 1, nw = wave >> 1;
    __shared__ int wq_slot[2];
    WinoWork<STEAL> wk;
    wk.init(q.total_work, q.interleave, q.qctr, wq_slot);

    int n0, oy0, ox0, b, cls;
    int py0, px0;               // patch origin of the item (scalars); the slots' pixel offsets are re-derived per parity phase
    int32_t poff[2];
    int i_nt, i_tx, i_ty;
    auto locate = [&]() {       // as wino22_kernel, q.nt = N / 128
        const int item = wk.item;
        i_nt = item % q.nt;
        int tile = item / q.nt;
        cls = tile % q.ncls;
        tile /= q.ncls;
        i_tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        i_ty = tile % q.tiles_y;
        b = tile / q.tiles_y;
    };
    const bool p1_ok = ((tid + WINO_THREADS) >> 1) < W22_PPIX;
    auto set_phase = [&](int ph) {
        // (an opaque thread index: the slot coordinates would otherwise be hoisted and held in registers across the K loop)
        int st = tid;
        asm volatile("" : "+v"(st));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (st + WINO_THREADS * i) >> 1, spy = pp / 17, spx = pp - spy * 17;
            int iy = py0 + spy, ix = px0 + spx, H = p.IH, W = p.IW, Cc = p.C;
            if (q.s2d) {
                iy = 2 * iy + (ph >> 1) - 1;
                ix = 2 * ix + (ph & 1) - 1;
                H = q.XH; W = q.XW; Cc = q.XC;
            }
            const bool ok = (i == 0 || p1_ok) && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int32_t pix = ok ? (b * H + iy) * W + ix : 0;
            poff[i] = ok ? (pix * Cc + 4 * (st & 1)) * 4 : (int32_t)0x80000000u;      // byte offset; out of range = beyond 2 GB
        }
    };
    const auto srsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.src), 0, (int)(q.s2d ? (size_t)p.B * q.XH * q.XW * q.XC * 4 : (size_t)p.B * p.IH * p.IW * p.C * 4), 0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U), 0, (int)((size_t)q.ncls * W22_PTS * p.N * p.C * 4), 0x00020000);
    auto decode = [&]() {
        n0 = i_nt * (2 * WINO_BN); oy0 = i_ty * 16; ox0 = i_tx * 16;
        py0 = oy0 + (q.ncls > 1 ? -(cls >> 1) : q.sy_min);
        px0 = ox0 + (q.ncls > 1 ? -(cls & 1) : q.sx_min);
    };
    const int c_begin = 0, c_end = p.C >> 3, c_last = c_end - 1;      // one split
    const size_t ustep = (size_t)(p.N / WINO_BN) * W22_V;
    const int cpp = q.s2d ? (q.XC >> 3) : (p.C >> 3);       // K steps per parity phase

    f32x4 ru[5], rp[2];
    int cur_ph, c_base, c_next;
    auto start_phase = [&](int ph) { cur_ph = ph; c_base = ph * cpp; c_next = c_base + cpp; set_phase(ph); };
    auto pload1 = [&](int c, int i) {
        rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, poff[i], (c - c_base) * 32, 0));
    };
    // the U image is 4.5 float4 per thread: in the fifth round the upper half of the threads re-reads its first one
    const size_t u_base = (size_t)W22_PTS * p.N * p.C;       // floats of one class's U
    const int u_last = tid < 256 ? tid + 4 * WINO_THREADS : tid;
    auto uload1 = [&](int c, int j) {
        ru[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            ursrc, 16 * (j < 4 ? tid + WINO_THREADS * j : u_last), (int)(((size_t)cls * u_base + (size_t)i_nt * W22W_U + (size_t)c * ustep) * 4), 0));
    };
    auto pstore1 = [&](int i) {
        if (i == 0 || p1_ok) *reinterpret_cast<f32x4*>(Ps + 4 * (tid + WINO_THREADS * i)) = rp[i];
    };
    auto ustore1 = [&](int buf, int j) {
        if (j < 4 || tid < 256) *reinterpret_cast<f32x4*>(Us + buf * W22W_U + 4 * (tid + WINO_THREADS * j)) = ru[j];
    };

    // input transform: the roles of wino22_kernel (waves 0..5), one patch column at a time -- column 1 first, it is in every
    // output: V[a][1] = r1, V[a][0] = r0 - r1, V[a][2] = r2 - r1 with r = row a of Bt d.  Every wave reads and computes (waves 6, 7
    // repeat row 2) and only the store is conditional: values assigned under `if (t_on)` would stay live around the whole K loop.
    const int t_quad = lane & 1, t_tile = (lane >> 1) + 32 * (wave & 1), t_a = min(wave >> 1, 2);
    const bool t_on = wave < 6;
    const int t_src0 = ((2 * (t_tile >> 3) + t_a) * 17 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_src1 = ((2 * (t_tile >> 3) + 1) * 17 + 2 * (t_tile & 7)) * 8 + 4 * t_quad;
    const int t_dst = (t_a * 3) * 512 + t_tile * 8 + (((t_quad ^ (t_tile >> 4)) & 1) << 2);
    f32x4 tp[2], tm;
    auto t_read1 = [&](int j) {
        tp[0] = *reinterpret_cast<const f32x4*>(Ps + t_src0 + j * 8);
        tp[1] = *reinterpret_cast<const f32x4*>(Ps + t_src1 + j * 8);
    };
    auto t_row1 = [&]() -> f32x4 { return t_a == 1 ? tp[0] : tp[0] - tp[1]; };
    auto t_col1 = [&](int buf, int k, f32x4 v) {
        if (t_on) *reinterpret_cast<f32x4*>(Vs + buf * W22_V + t_dst + k * 512) = v;
    };

    const int arow = 32 * mw + (lane & 31), brow = 32 * (nw & 1) + (lane & 31);
    const int a_off = arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = (nw >> 1) * W22_V + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    if (wk.item < 0 || c_begin >= c_end) { wk.done(q.qctr); return; }
    locate();
    decode();
    start_phase(0);
#pragma unroll
    for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
    for (int j = 0; j < 5; ++j) uload1(c_begin, j);

    for (;;) {
        f32x16 acc[W22_PTS];
#pragma unroll
        for (int i = 0; i < W22_PTS; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        {
            // prologue: as wino22_kernel
#pragma unroll
            for (int i = 0; i < 2; ++i) pstore1(i);
#pragma unroll
            for (int j = 0; j < 5; ++j) ustore1(0, j);
            {
                const int c1 = min(c_begin + 1, c_last);
                if (c1 >= c_next) start_phase(cur_ph + 1);
#pragma unroll
                for (int i = 0; i < 2; ++i) pload1(c1, i);
#pragma unroll
                for (int j = 0; j < 5; ++j) uload1(c1, j);
            }
            wino_barrier();
            t_read1(1);
            tm = t_row1();
            t_col1(0, 1, tm);
            t_read1(0);
            t_col1(0, 0, t_row1() - tm);
            t_read1(2);
            t_col1(0, 2, t_row1() - tm);
            wino_barrier();
            f32x4 fa[2], fb[2];
            fa[0] = *reinterpret_cast<const f32x4*>(Vs + a_off);
            fb[0] = *reinterpret_cast<const f32x4*>(Us + b_off);
            int cur = 0;
            for (int c = c_begin; c < c_end; ++c) {
                const int nxt = cur ^ 1;
                const int c2 = min(c + 2, c_last);               // tail steps: redundant staging instead of branches
                const float* Vc = Vs + cur * W22_V + a_off;
                const float* Uc = Us + cur * W22W_U + b_off;
                const float* Vn = Vs + nxt * W22_V + a_off;
                const float* Un = Us + nxt * W22W_U + b_off;
                // 36 ticks: t = 4*xi + e, an MFMA of every wave in each; point xi takes the fragment registers xi & 1
                wino_static_for(std::make_integer_sequence<int, 36>{}, [&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    constexpr int xi = t >> 2, e = t & 3;
                    if constexpr (t < 2) pstore1(t);                           // patch c+1 -> LDS (readers of patch c are done)
                    if constexpr (t == 2) {                                    // patch c+2 -> rp; new slot offsets on a phase change
                        if (c2 >= c_next) start_phase(cur_ph + 1);
                        pload1(c2, 0);
                    }
                    if constexpr (t == 3) pload1(c2, 1);
                    if constexpr (t == 4) wino_barrier();                      // patch c+1 visible
                    if constexpr (t == 5) t_read1(1);
                    if constexpr (t == 8) { tm = t_row1(); t_col1(nxt, 1, tm); t_read1(0); }
                    if constexpr (t == 11) { t_col1(nxt, 0, t_row1() - tm); t_read1(2); }
                    if constexpr (t == 14) t_col1(nxt, 2, t_row1() - tm);
                    if constexpr (t >= 17 && t < 22) ustore1(nxt, t - 17);
                    if constexpr (t >= 23 && t < 28) uload1(c2, t - 23);       // U c+2 -> ru
                    if constexpr (t == 32) wino_barrier();                     // V / U images of step c+1 complete
                    if constexpr (e == 0 && xi < 8) {
                        fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Vc + (xi + 1) * 512);
                        fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Uc + (xi + 1) * 512);
                    }
                    if constexpr (t == 33) {                                   // point 0 of step c+1 (point 7 is done with its registers)
                        fa[1] = *reinterpret_cast<const f32x4*>(Vn);
                        fb[1] = *reinterpret_cast<const f32x4*>(Un);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                });
                // nine points on two fragment registers: the next step starts in the other one -- moved, not renamed
                fa[0] = fa[1];
                fb[0] = fb[1];
                cur = nxt;
            }
        }
        const int e_n0 = n0, e_oy0 = oy0, e_ox0 = ox0, e_b = b, e_cls = cls;      // output coordinates of the finished item
        const int wq_next = wk.next(wq_slot);
        const bool more_items = wq_next >= 0;
        const int wq_pulled = wk.request(wq_next);
        wino_barrier();        // the epilogue scratch overlays U

        // row sums s[a][j] = M[a][j] + M[a][j+1] of the 3x3 points: the accumulators die here
        // the lane index of the epilogue is opaque to the compiler: the row / column offsets derived from it are otherwise hoisted
        // out of the item loop and held in registers across the K loop, where there are none to spare
        int el = lane;
        asm volatile("" : "+v"(el));
        float* scratch = smem + 2 * W22_V + wave * (32 * 36);
        f32x16 rs[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) rs[a][j][r] = acc[3 * a + j][r] + acc[3 * a + j + 1][r];
        const int e_dy0 = q.ncls > 1 ? 1 - (e_cls >> 1) : p.dy0, e_dx0 = q.ncls > 1 ? 1 - (e_cls & 1) : p.dx0;
        f32x4 bq = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bq = *reinterpret_cast<const f32x4*>(p.bias + e_n0 + 32 * nw + 4 * (el & 7));
#pragma unroll
        for (int xh = 0; xh < 2; ++xh) {
            // the staging state switches to the next item and its first operands are requested between the two output rows: ahead of
            // the second row's stores, once the first row's sums are dead (all of it does not fit beside three rows of sums)
            if (xh == 1 && more_items) {
                wk.item = wq_next;
                locate();
                decode();
                start_phase(0);
#pragma unroll
                for (int i = 0; i < 2; ++i) pload1(c_begin, i);
#pragma unroll
                for (int j = 0; j < 5; ++j) uload1(c_begin, j);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // row scales and gate quads of this tile are fetched ahead of its stores (a load behind a store waits for the store's
                // acknowledgement) -- a tile at a time, as wino_kernel does: the quads of two tiles do not fit beside the row sums
                float rsq[4] = {1.f, 1.f, 1.f, 1.f};
                if (p.rowscale) {
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4) {
                        const int t = 32 * mw + (el >> 3) + 8 * t4;
                        const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                        rsq[t4] = p.rowscale[((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0)];
                    }
                }
                f32x4 gq[GATED ? 4 : 1];
                if constexpr (GATED) {
#pragma unroll
                    for (int t4 = 0; t4 < 4; ++t4) {
                        const int t = 32 * mw + (el >> 3) + 8 * t4;
                        const int oy = min(e_oy0 + 2 * (t >> 3) + xh, p.OH - 1), ox = min(e_ox0 + 2 * (t & 7) + j, p.OW - 1);
                        const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0);
                        gq[t4] = *reinterpret_cast<const f32x4*>(p.gate + pix * p.N + e_n0 + 32 * nw + 4 * (el & 7));
                    }
                }
                f32x16 y;
#pragma unroll
                for (int r = 0; r < 16; ++r) y[r] = rs[xh][j][r] + rs[xh + 1][j][r];
                tile_rows4i(scratch, y, el, [&](int t4, int rr, int cc, f32x4 v4) {
                    const int t = 32 * mw + rr;
                    const int oy = e_oy0 + 2 * (t >> 3) + xh, ox = e_ox0 + 2 * (t & 7) + j;
                    const int nb = e_n0 + 32 * nw + cc;
                    if (oy >= p.OH || ox >= p.OW) return;
                    const size_t pix = ((size_t)e_b * p.DH + (oy * p.ds + e_dy0)) * p.DW + (ox * p.ds + e_dx0);
                    *reinterpret_cast<f32x4*>(p.dst + pix * p.N + nb) = epilogue4(p, v4, pix, nb, GATED ? &gq[GATED ? t4 : 0] : nullptr, &rsq[t4], &bq);
                });
            }
        }
        wk.publish(wq_pulled, wq_slot);
        if (!more_items) break;
        wino_barrier();        // every wave is done with the scratch before the next prologue stages into it
        wk.advance(wq_next);
    }
    wk.done(q.qctr);
}

static bool wino22_enabled() {
    static const bool off = getenv("TG_NO_WINO") != nullptr || getenv("TG_NO_WINO22") != nullptr;
    return !off;
}
// TG_WINO22_WIDE=0 keeps every launch on the 64-channel items.  Read at each launch: both forms can run in one process.
static bool wino22_wide_enabled() {
    const char* e = getenv("TG_WINO22_WIDE");
    return e == nullptr || atoi(e) != 0;
}
// 4x4 / stride 2 / pad 1, fp32, even input: forward needs Cout % 64 == 0 and Cin % 8 == 0, dgrad the mirror image
static bool wino22_fwd_geom_ok(const TgConv* g) {
    return wino22_enabled() && g->precision != TG_PREC_BF16 && g->k == 4 && g->stride == 2 && g->pad == 1 && (g->H % 2) == 0 &&
           (g->W % 2) == 0 && g->Ho == g->H / 2 && g->Wo == g->W / 2 && (g->Cin % 8) == 0 && (g->Cout % WINO_BN) == 0 && g->Ho >= 16 &&
           g->Wo >= 16;
}
static bool wino22_dgrad_geom_ok(const TgConv* g) {
    return wino22_enabled() && g->precision != TG_PREC_BF16 && g->k == 4 && g->stride == 2 && g->pad == 1 && (g->H % 2) == 0 &&
           (g->W % 2) == 0 && g->Ho == g->H / 2 && g->Wo == g->W / 2 && (g->Cout % 8) == 0 && (g->Cin % WINO_BN) == 0 && g->Ho >= 16 &&
           g->Wo >= 16;
}
// floats of the transformed weights (forward: one problem with K = 4 Cin; dgrad: four classes with K = Cout): 36 Cin Cout
static size_t wino22_u_floats(const TgConv* g) { return align_up((size_t)4 * W22_PTS * g->Cin * g->Cout, 64); }

// forward (dgrad == 0): y = conv(x), 2x2 taps over the shifted space-to-depth view of x.
// dgrad: dx = the four parity classes, each a 2x2 stride-1 correlation of dy, in ONE launch.
// p carries src / dst / epilogue fields, w_raw, wino_u, wino_ready, ws; the geometry is set here.
static int launch_wino22(const TgConv* g, IGemmParams& p, int dgrad, size_t ws_floats_avail, hipStream_t s) {
    W22Geom q = {};
    W22Weights ww = {};
    p.B = g->B;
    p.OH = g->Ho; p.OW = g->Wo;                  // the 2x2 problems live on the Ho x Wo grid, forward and every dgrad class
    p.M = g->B * g->Ho * g->Wo;
    ww.cin = g->Cin;
    if (!dgrad) {
        p.IH = g->Ho + 1; p.IW = g->Wo + 1; p.C = 4 * g->Cin; p.N = g->Cout;
        p.DH = g->Ho; p.DW = g->Wo; p.ds = 1; p.dy0 = 0; p.dx0 = 0;
        q.s2d = 1; q.XH = g->H; q.XW = g->W; q.XC = g->Cin; q.ncls = 1;
        q.sy_min = 0; q.sx_min = 0;
        ww.sn = 16L * g->Cin; ww.sk = 1; ww.by_phase = 1; ww.ncls = 1; ww.k_fast = 1;
        ww.tyu[0] = 0; ww.tyu[1] = 1; ww.txv[0] = 0; ww.txv[1] = 1;          // source row yy = oy + ty
    } else {
        p.IH = g->Ho; p.IW = g->Wo; p.C = g->Cout; p.N = g->Cin;
        p.DH = g->H; p.DW = g->W; p.ds = 2;
        q.s2d = 0; q.ncls = 4;
        ww.sn = 1; ww.sk = 16L * g->Cin; ww.by_phase = 0; ww.ncls = 4; ww.k_fast = 0;
        ww.tyu[0] = 1; ww.tyu[1] = 0; ww.txv[0] = 1; ww.txv[1] = 0;          // source row oy = yy' + (1 - dy) - ty, patch origin -dy
    }
    q.tiles_x = cdiv(p.OW, 16);
    q.tiles_y = cdiv(p.OH, 16);
    q.nt = p.N / WINO_BN;
    q.total_work = q.tiles_x * q.tiles_y * p.B * q.nt * q.ncls;
    // Sized by ONE class's U although the ~32 consecutive items an XCD works on in the interleaved walk cover all four classes of a
    // dgrad (N tile fastest, then class), i.e. 4x these bytes are in use at a time.  By wino_distribute's rule (the whole U in the
    // 4 MB L2) that would move the 256 <- 512 dgrad (4.7 MB per class, 18.9 MB in all) to contiguous ranges; measured on that layer,
    // both walks in fresh processes, twice: 115.7 / 116.5 against 115.6 / 114.6 us at 16 images, 171.7 / 172.1 against 167.9 / 170.3 us
    // at 32 -- inside the spread of the timings (profiles/r07_wino22_wide.txt), so the rule stays as it was.  The smaller dgrads
    // are below the limit either way (128 <- 256: 4.7 MB in all).
    q.interleave = wino_interleave_ok((size_t)W22_PTS * p.N * p.C * sizeof(float));
    const int nchunks = p.C / 8;
    int splits = 1;
    if (nchunks >= 16) {
        int smax = nchunks / 8 < 16 ? nchunks / 8 : 16;
        while (smax > 1 && (size_t)smax * p.M * p.N * q.ncls > ws_floats_avail) --smax;
        splits = choose_splits(q.total_work, smax, WINO_PLAN_CUS);
    }
    q.chunks_per_split = cdiv(nchunks, splits);
    p.splits = cdiv(nchunks, q.chunks_per_split);
    p.Ktot = 4 * p.C;
    TgWprepItem it = {};
    it.kind = 3; it.N = p.N; it.K = p.C; it.w = p.w_raw; it.out = p.wino_u; it.w22 = ww;
    int rc = TG_OK;
    const auto transform = [&]() -> int {
        hipLaunchKernelGGL(wino22_weights_kernel, dim3(ew_grid((int64_t)p.N * p.C * q.ncls, 256)), dim3(256), 0, s, p.w_raw, p.wino_u, p.N,
                           p.C, ww);
        TG_CHECK_LAUNCH("wino22_weights_kernel");
        return TG_OK;
    };
    if (wino_prep(p, it, transform, &rc)) return rc;
    static const bool no_fast = getenv("TG_WINO_NO_FAST") != nullptr;
    const size_t src_bytes = (size_t)g->B * (dgrad ? (size_t)g->Ho * g->Wo * g->Cout : (size_t)g->H * g->W * g->Cin) * 4;
    const bool fast = !no_fast && p.amask == nullptr && src_bytes < ((size_t)1 << 31) && wino22_u_floats(g) * 4 < ((size_t)1 << 31);
    const bool gated = p.gate != nullptr && p.splits == 1;
    typedef void (*W22Kern)(const IGemmParams, const W22Geom, const float*);
    static const W22Kern kerns[8] = {wino22_kernel<false, false, false>, wino22_kernel<false, true, false>, wino22_kernel<true, false, false>,
                                     wino22_kernel<true, true, false>, wino22_kernel<false, false, true>, wino22_kernel<false, true, true>,
                                     wino22_kernel<true, false, true>, wino22_kernel<true, true, true>};
    static LdsOptIn opts[8];
    // the wide form (wino22w_kernel): 128-channel items, where they still fill the chip -- one split (the split plan above is made
    // for the 64-channel items and is not touched), an unmasked source, and at least one item per planned CU.  Both forms read the
    // same prepared weights and give the same bits.
    const bool wide = wino22_wide_enabled() && fast && (p.N % (2 * WINO_BN)) == 0 && p.splits == 1 && q.total_work / 2 >= WINO_PLAN_CUS;
    if (wide) { q.nt /= 2; q.total_work /= 2; }
    static const W22Kern kernsw[4] = {wino22w_kernel<false, false>, wino22w_kernel<true, false>, wino22w_kernel<false, true>,
                                      wino22w_kernel<true, true>};
    static LdsOptIn optsw[4];
    q.qctr = wino_queue_block(s, p.splits, q.total_work);
    const int ki = (q.qctr ? 4 : 0) + (fast ? 2 : 0) + (gated ? 1 : 0);
    const double mtot = (double)p.M * q.ncls;
    const WinoProf pf = {0, 4022, (int)mtot, 2.0 * mtot * (double)p.N * p.Ktot,              // (direct form: 16 taps)
                         4.0 * ((double)g->B * (dgrad ? g->Ho * g->Wo * g->Cout : g->H * g->W * g->Cin) + 16.0 * g->Cin * g->Cout +
                                mtot * p.N + (p.rowscale ? mtot : 0.0)), WR_FIRST + (wide ? WR_W22_WIDE : 0) + ki};
    if (wide) {
        const int kw = (q.qctr ? 2 : 0) + (gated ? 1 : 0);
        return wino_launch(kernsw[kw], optsw[kw], (size_t)W22W_LDS_FLOATS * sizeof(float), "wino22w_kernel", p, q, pf, false, s);
    }
    // the split-K slabs of the ncls classes are reduced by one launch of the multi-class epilogue
    if ((rc = wino_launch(kerns[ki], opts[ki], (size_t)W22_LDS_FLOATS * sizeof(float), "wino22_kernel", p, q, pf, false, s))) return rc;
    if (p.splits > 1) {
        IGemmMulti pm = {};
        for (int c = 0; c < q.ncls; ++c) {
            pm.c[c] = p;
            pm.c[c].ws = p.ws + (size_t)c * p.splits * p.M * p.N;
            if (q.ncls > 1) { pm.c[c].dy0 = 1 - (c >> 1); pm.c[c].dx0 = 1 - (c & 1); }
        }
        hipLaunchKernelGGL(igemm_splitk_epilogue_multi, dim3(ew_grid((int64_t)p.M * p.N, 256), q.ncls), dim3(256), 0, s, pm);
        TG_CHECK_LAUNCH("igemm_splitk_epilogue_multi");
    }
    return TG_OK;
}

// =================================================================================================
// Winograd wgrad F(2x2,2x2) of the 4x4 / stride-2 / pad-1 convolutions:
//     dW2[ty][tx] = Gt [ sum_tiles (A dY At) (.) (Bt X2 B) ] G ,   dW[co][2ty+dy][2tx+dx][c] = dW2[co][ty][tx][(dy,dx,c)]
// =================================================================================================
// 9 products per 2x2 tile of dY instead of 16, contracted over the TILES as in wino_wgrad_kernel: per transform point
//     dU[xi][co][n] = sum_tiles Yt[xi][tile][co] * V[xi][tile][n],   n = (parity phase, c) over 4 Cin
// M = Cout, N = 4 Cin, K = tiles.  A 512-thread workgroup owns 64 co x 64 n x 9 points (the 6 : 3 MFMA split of
// wino22_kernel) and walks strips of 8 tiles (16 x 2 output pixels).  A 64-channel N tile lies inside ONE parity phase
// (Cin % 64 == 0), so the strip of the shifted space-to-depth view it needs is 3 rows x 17 pixels of x taken at every second
// row / column: fetched once, coalesced (256 B per pixel), into LDS; the transform roles (tile, channel quad, row a) read
// their 2x3 / 2x2 pixels from there and write the images K-contiguous.  Split-K over strips; slabs hold dU, the reduce
// kernel sums them in fixed order and applies Gt . G.
struct W22WgradGeom {
    int strips_x, tiles_y, nstrips, steps_per_split, splits, ntco, ntci, ctiles;     // ctiles = Cin / 64 (N tiles per phase)
};
constexpr int W22_XR = 3 * 17 * WG_PITCH;
constexpr int W22_DR = 2 * 16 * WG_PITCH;
constexpr int W22_WG_LDS_FLOATS = 4 * W22_V + W22_XR + W22_DR;

__global__ __launch_bounds__(WINO_THREADS) void wino22_wgrad_kernel(const WgradParams p, const W22WgradGeom q, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                    // [2][9][64][8]   Yt, rows = co (permuted)
    float* Bs = smem + 2 * W22_V;        // [2][9][64][8]   V,  rows = n (permuted)
    float* Xr = smem + 4 * W22_V;        // raw strip of x2: [3][17][WG_PITCH]
    float* Dr = Xr + W22_XR;             // raw strip of dy: [2][16][WG_PITCH]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mw = wave & 1, nw = (wave >> 1) & 1, xh = wave >> 2;
    const int work = xcd_remap(blockIdx.x, q.ntco * q.ntci * q.splits);
    const int tco = work % q.ntco, tci = (work / q.ntco) % q.ntci, split = work / (q.ntco * q.ntci);
    const int ph = tci / q.ctiles, ct = tci - ph * q.ctiles;          // parity phase (dy, dx) and channel tile of this N tile
    const int pdy = (ph >> 1) - 1, pdx = (ph & 1) - 1;                // x2[yy][xx] = x[2 yy + pdy][2 xx + pdx]
    const int s_begin = split * q.steps_per_split;
    const int s_end = min(q.nstrips, s_begin + q.steps_per_split);

    // transform role: tile k of the strip, channel quad qd, row a of the 3x3 transform (waves 0..5; 6 and 7 have none)
    const int k = lane & 7, qd = (lane >> 3) + 8 * (wave & 1), a = min(wave >> 1, 2);
    const bool t_on = wave < 6;
    int icol[4];          // image column of channel e of this thread's quad: row (qd + 16 e), k-slot swizzled
#pragma unroll
    for (int e = 0; e < 4; ++e) icol[e] = (3 * a) * 512 + (qd + 16 * e) * 8 + ((((k >> 2) ^ e) & 1) << 2) + (k & 3);
    const int xrd0 = (a * 17 + 2 * k) * WG_PITCH + 4 * qd, xrd1 = (17 + 2 * k) * WG_PITCH + 4 * qd;      // + j * WG_PITCH
    const int drd = (2 * k) * WG_PITCH + 4 * qd;                                                           // + (i*16 + j) * WG_PITCH

    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)((size_t)p.B * p.H * p.W * p.C * 4), 0x00020000);
    const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dy), 0, (int)((size_t)p.B * p.Ho * p.Wo * p.Cout * 4), 0x00020000);
    const uint32_t OOB = 0xFFFFFFF0u;

    // raw staging slots: (pixel slot, channel quad), a thread per 16 bytes
    int xs_r[2], xs_px[2], xs_lds[2];
    bool xs_on[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + WINO_THREADS * i;
        const int ps = idx >> 4;
        xs_on[i] = ps < 3 * 17;
        xs_r[i] = ps / 17;
        xs_px[i] = ps - xs_r[i] * 17;
        xs_lds[i] = ps * WG_PITCH + 4 * (idx & 15);
    }
    const uint32_t xs_ch = (uint32_t)(ct * 64 + 4 * (tid & 15)) * 4u;
    const int ds_i = tid >> 8, ds_px = (tid >> 4) & 15, ds_lds = (tid >> 4) * WG_PITCH + 4 * (tid & 15);
    const uint32_t ds_ch = (uint32_t)(tco * 64 + 4 * (tid & 15)) * 4u;

    // raw strips in flight: TWO register sets -- strip s+1 is stored from one while strip s+2 waits in the other and s+3 is being
    // requested (with one set the loads had a single K step, 1.6-2.4 us, to arrive: the kernel whose waves WAIT, 38 % of their cycles)
    f32x4 rx[2][2], rd[2];
    int ls = s_begin, lsx = s_begin % q.strips_x, lty = (s_begin / q.strips_x) % q.tiles_y, lb = s_begin / (q.strips_x * q.tiles_y);
    auto raw_load = [&](auto setc) {      // raw pixels of strip ls -> rx / rd of register set `setc` (out of range, or past this split's range: 0)
        constexpr int SET = decltype(setc)::value;
        const bool live = ls < s_end;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int py = 2 * (2 * lty + xs_r[i]) + pdy, px = 2 * (16 * lsx + xs_px[i]) + pdx;
            const bool ok = live && xs_on[i] && py >= 0 && py < p.H && px >= 0 && px < p.W;
            const uint32_t off = ok ? (((uint32_t)(lb * p.H + py) * p.W + px) * (uint32_t)p.C) * 4u + xs_ch : OOB;
            rx[SET][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0));
        }
        {
            const int oy = 2 * lty + ds_i, ox = 16 * lsx + ds_px;
            const bool ok = live && oy < p.Ho && ox < p.Wo;
            const uint32_t off = ok ? (((uint32_t)(lb * p.Ho + oy) * p.Wo + ox) * (uint32_t)p.Cout) * 4u + ds_ch : OOB;
            rd[SET] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, off, 0, 0));
        }
        ++ls;
        if (++lsx == q.strips_x) { lsx = 0; if (++lty == q.tiles_y) { lty = 0; ++lb; } }
    };
    auto raw_store = [&](auto setc) {
        constexpr int SET = decltype(setc)::value;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (xs_on[i]) *reinterpret_cast<f32x4*>(Xr + xs_lds[i]) = rx[SET][i];
        *reinterpret_cast<f32x4*>(Dr + ds_lds) = rd[SET];
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;
    f32x4 xr[2][3], dr[2][2], tt[3], rr[2];
    auto x_read = [&](int j) {      // column j of both rows
        xr[0][j] = *reinterpret_cast<const f32x4*>(Xr + xrd0 + j * WG_PITCH);
        xr[1][j] = *reinterpret_cast<const f32x4*>(Xr + xrd1 + j * WG_PITCH);
    };
    auto d_read = [&](int i) {      // row i, both columns
        dr[i][0] = *reinterpret_cast<const f32x4*>(Dr + drd + (i * 16) * WG_PITCH);
        dr[i][1] = *reinterpret_cast<const f32x4*>(Dr + drd + (i * 16 + 1) * WG_PITCH);
    };
    auto x_rows = [&]() {           // Bt rows: a = 0: x0 - x1, a = 1: x1, a = 2: x2 - x1
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (a == 1) tt[j] = xr[0][j];
            else tt[j] = xr[0][j] - xr[1][j];
        }
    };
    auto d_rows = [&]() {           // A rows: a = 0: D0, a = 1: D0 + D1, a = 2: D1
#pragma unroll
        for (int j = 0; j < 2; ++j) rr[j] = a == 0 ? dr[0][j] : (a == 1 ? dr[0][j] + dr[1][j] : dr[1][j]);
    };
    // output b (0..2) of the column transform; half h writes channels 2h, 2h+1
    auto x_out = [&](int buf, int b, int h) {
        const f32x4 v = b == 0 ? tt[0] - tt[1] : b == 1 ? tt[1] : tt[2] - tt[1];
        float* dst = Bs + buf * W22_V + b * 512;
        dst[icol[2 * h]] = v[2 * h];
        dst[icol[2 * h + 1]] = v[2 * h + 1];
    };
    auto d_out = [&](int buf, int b, int h) {
        const f32x4 v = b == 0 ? rr[0] : b == 1 ? rr[0] + rr[1] : rr[1];
        float* dst = As + buf * W22_V + b * 512;
        dst[icol[2 * h]] = v[2 * h];
        dst[icol[2 * h + 1]] = v[2 * h + 1];
    };

    const int pt0 = xh == 0 ? 0 : 6;
    const int arow = 32 * mw + (lane & 31), brow = 32 * nw + (lane & 31);
    const int a_off = pt0 * 512 + arow * 8 + ((((lane >> 5) ^ (arow >> 4)) & 1) << 2);
    const int b_off = pt0 * 512 + brow * 8 + ((((lane >> 5) ^ (brow >> 4)) & 1) << 2);

    f32x16 acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    if (s_begin < s_end) {
        raw_load(Set0{});           // strip s_begin
        raw_store(Set0{});
        raw_load(Set0{});           // strips s_begin + 1 and + 2: in flight while the first images are built
        raw_load(Set1{});
        wino_barrier();
        if (t_on) {
#pragma unroll
            for (int j = 0; j < 3; ++j) x_read(j);
            d_read(0);
            d_read(1);
            x_rows();
            d_rows();
#pragma unroll
            for (int b = 0; b < 3; ++b) { x_out(0, b, 0); x_out(0, b, 1); d_out(0, b, 0); d_out(0, b, 1); }
        }
        wino_barrier();
        f32x4 fa[2], fb[2];
        fa[0] = *reinterpret_cast<const f32x4*>(As + a_off);
        fb[0] = *reinterpret_cast<const f32x4*>(Bs + b_off);
        int cur = 0;
        auto kstep = [&](auto setc) {
            const int nxt = cur ^ 1;
            const float* Ac = As + cur * W22_V + a_off;
            const float* Bc = Bs + cur * W22_V + b_off;
            const float* An = As + nxt * W22_V + a_off;
            const float* Bn = Bs + nxt * W22_V + b_off;
            // register set `setc` holds the raw strip s+1: to LDS, transformed into the images of buffer nxt while the MFMAs consume
            // strip s; the set then takes strip s+3 (the other one holds s+2).  24 ticks, xh = 1 waves issue MFMAs in the first 12.
            wino_static_for(std::make_integer_sequence<int, 24>{}, [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int xi = t >> 2, e = t & 3;
                if constexpr (t == 0) raw_store(setc);
                if constexpr (t == 1) raw_load(setc);
                if constexpr (t == 2) wino_barrier();                      // raw strip visible
                if constexpr (t >= 3 && t < 6) { if (t_on) x_read(t - 3); }
                if constexpr (t == 6) { if (t_on) { d_read(0); d_read(1); } }
                if constexpr (t == 7) { if (t_on) x_rows(); }
                if constexpr (t >= 8 && t < 14) { if (t_on) x_out(nxt, (t - 8) >> 1, t & 1); }
                if constexpr (t == 13) { if (t_on) d_rows(); }
                if constexpr (t >= 14 && t < 20) { if (t_on) d_out(nxt, (t - 14) >> 1, t & 1); }
                if constexpr (t == 20) wino_barrier();                     // images of strip s+1 complete
                if constexpr (e == 0 && xi < 5) {
                    if (xi + 1 < 3 || xh == 0) {
                        fa[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Ac + (xi + 1) * 512);
                        fb[(xi + 1) & 1] = *reinterpret_cast<const f32x4*>(Bc + (xi + 1) * 512);
                    }
                }
                if constexpr (t == 22) {
                    fa[0] = *reinterpret_cast<const f32x4*>(An);
                    fb[0] = *reinterpret_cast<const f32x4*>(Bn);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (xi < 3 || xh == 0) acc[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[xi & 1][e], fb[xi & 1][e], acc[xi], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
            cur = nxt;
        };
        for (int s = s_begin; s < s_end; s += 2) {
            kstep(Set0{});
            if (s + 1 < s_end) kstep(Set1{});
        }
    }
    // dU slab of this (split, N tile, co tile): [xi][row 64][col 64], raw accumulator layout (permuted channels)
    float* slab = slabs + ((size_t)work * W22_PTS + pt0) * 4096;
    const int npts = xh == 0 ? 6 : 3;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (i < npts) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * mw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                slab[(size_t)i * 4096 + row * 64 + 32 * nw + (lane & 31)] = acc[i][r];
            }
        }
    }
}

// dW[co][2ty+dy][2tx+dx][c] = sum_{a in {ty,ty+1}} sum_{b in {tx,tx+1}} (sum_splits dU[a][b][co][(dy,dx,c)])
__global__ __launch_bounds__(256) void wino22_wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int Cout,
                                                                  int Cin, int ntco, int ntci, int splits) {
    const int total = Cout * 4 * Cin;
    const int ctiles = Cin / 64;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int col = idx & 63, row = (idx >> 6) & 63, tile = idx >> 12;       // tile = tci * ntco + tco
        const int tco = tile % ntco, tci = tile / ntco;
        float u[W22_PTS];
#pragma unroll
        for (int i = 0; i < W22_PTS; ++i) u[i] = 0.f;
        const size_t sstride = (size_t)ntci * ntco * W22_PTS * 4096;
        const float* sl = slabs + ((size_t)tile * W22_PTS) * 4096 + row * 64 + col;
        int sp = 0;
        for (; sp + 4 <= splits; sp += 4) {          // 36 independent loads per trip, summed in slab order
            float v[4][W22_PTS];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < W22_PTS; ++i) v[k][i] = sl[(size_t)(sp + k) * sstride + (size_t)i * 4096];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < W22_PTS; ++i) u[i] += v[k][i];
        }
        for (; sp < splits; ++sp)
#pragma unroll
            for (int i = 0; i < W22_PTS; ++i) u[i] += sl[(size_t)sp * sstride + (size_t)i * 4096];
        const int ph = tci / ctiles, ct = tci - ph * ctiles;
        const int co = tco * 64 + 4 * (row & 15) + (row >> 4), c = ct * 64 + 4 * (col & 15) + (col >> 4);
        const int dy = ph >> 1, dx = ph & 1;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty)
#pragma unroll
            for (int tx = 0; tx < 2; ++tx)
                dw[((size_t)(co * 4 + 2 * ty + dy) * 4 + 2 * tx + dx) * Cin + c] =
                    (u[ty * 3 + tx] + u[ty * 3 + tx + 1]) + (u[(ty + 1) * 3 + tx] + u[(ty + 1) * 3 + tx + 1]);
    }
}

static bool wino22_wgrad_ok(const TgConv* g, const float* in_mask) {
    static const bool off = getenv("TG_NO_WINO22_WGRAD") != nullptr;
    if (off || !wino22_enabled() || in_mask != nullptr || g->precision == TG_PREC_BF16) return false;
    if (g->k != 4 || g->stride != 2 || g->pad != 1 || (g->H % 2) || (g->W % 2) || g->Ho != g->H / 2 || g->Wo != g->W / 2) return false;
    if ((g->Cin % 64) != 0 || (g->Cout % 64) != 0 || g->Ho < 16 || g->Wo < 16) return false;
    if ((size_t)g->B * g->H * g->W * g->Cin * 4 >= ((size_t)1 << 31) || (size_t)g->B * g->Ho * g->Wo * g->Cout * 4 >= ((size_t)1 << 31))
        return false;         // 32-bit buffer offsets
    return true;
}
static W22WgradGeom wino22_wgrad_plan(const TgConv* g) {
    W22WgradGeom q = {};
    q.strips_x = cdiv(g->Wo, 16);
    q.tiles_y = cdiv(g->Ho, 2);
    q.nstrips = g->B * q.tiles_y * q.strips_x;
    q.ntco = g->Cout / 64;
    q.ctiles = g->Cin / 64;
    q.ntci = 4 * q.ctiles;
    const int tiles = q.ntco * q.ntci;
    // at least 8 strips per split (small batches: 32 left three quarters of the chip idle -- 48-64 workgroups of 32 strips)
    int smax = q.nstrips / 8 < 512 ? q.nstrips / 8 : 512;
    if (smax < 1) smax = 1;
    const int splits = choose_splits_k(tiles, smax, WINO_PLAN_CUS, q.nstrips, 0.03);
    q.steps_per_split = cdiv(q.nstrips, splits);
    q.splits = cdiv(q.nstrips, q.steps_per_split);
    return q;
}
static size_t wino22_wgrad_ws_floats(const TgConv* g) {
    if (!wino22_wgrad_ok(g, nullptr)) return 0;
    const W22WgradGeom q = wino22_wgrad_plan(g);
    return (size_t)q.splits * q.ntco * q.ntci * W22_PTS * 4096;
}
static int launch_wino22_wgrad(const TgConv* g, const WgradParams& p, float* dw, float* ws, hipStream_t s) {
    const W22WgradGeom q = wino22_wgrad_plan(g);
    const size_t lds = (size_t)W22_WG_LDS_FLOATS * sizeof(float);
    static LdsOptIn opt;
    if (int rc = lds_opt_in(opt, reinterpret_cast<const void*>(wino22_wgrad_kernel), lds, "wino22 wgrad")) return rc;
    {
        const double by = 4.0 * ((double)p.B * p.H * p.W * p.C + (double)p.Mpix * p.Cout + (double)p.Cout * p.Ktot);
        ProfScope ps(s, 1, 2.0 * p.Mpix * (double)p.Cout * p.Ktot, by, p.Cout, p.Ktot, p.Mpix, p.C, q.splits, 4122);
        ps.r.route = WR_WGRAD;
        hipLaunchKernelGGL(wino22_wgrad_kernel, dim3(q.ntco * q.ntci * q.splits), dim3(WINO_THREADS), lds, s, p, q, ws);
    }
    TG_CHECK_LAUNCH("wino22_wgrad_kernel");
    hipLaunchKernelGGL(wino22_wgrad_reduce_kernel, dim3(ew_grid((int64_t)g->Cout * 4 * g->Cin, 256)), dim3(256), 0, s, ws, dw, g->Cout,
                       g->Cin, q.ntco, q.ntci, q.splits);
    TG_CHECK_LAUNCH("wino22_wgrad_reduce_kernel");
    return TG_OK;
}
