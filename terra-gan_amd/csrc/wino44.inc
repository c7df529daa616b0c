// Winograd F(4x4,3x3) on the fp32 MFMA -- included by igemm.hip after wino.inc (uses WinoWeights, wino_distribute,
// wino_barrier, wino_static_for, tile_rows4i, epilogue4, ProfScope).
//
// The frozen VGG16 trunk of the perceptual loss (losses.py:31-34,79-90: six stride-1 3x3 convolutions forward over 2B images
// and their dgrads over B) is 27 % of the train step on the F(2x2,3x3) kernel, which is bound by the matrix pipe.  The only
// lever left there is fewer multiplies:  Y = At [ (G g Gt) (.) (Bt d B) ] A  over 4x4 output tiles needs 36 products per 16
// outputs (2.25 per output) against 16 per 4 (4 per output) -- 1.78x fewer MFMAs.  The price is numerical: the transforms have
// coefficients up to 8 and 1/24, so one layer's rounding error on random data is 6-7x (rms) / ~20x (maximum: 1e-5 of the
// tensor's largest value, tools/conv_fuzz.py) that of F(2x2,3x3); on the trunk's feature map, averaged by its ReLUs and pools:
// 6e-7 of max|f| against 4e-7 for a direct fp32 convolution, perceptual loss 2.5e-6 relative -- inside the stated fp32 tolerances
// for the perceptual term and its gradient, which is all this trunk feeds; the generator and discriminator stay on F(2x2,...).
// Selected per call (TgConv.precision = TG_PREC_F32_WINO4), never by default.
//
// Workgroup = 512 threads = 8 waves (2 per SIMD), one per CU (130 KB LDS), persistent over work items (image, 16 x 32 output
// pixels = 4 x 8 tiles, 64 output channels).  The 36 transform points are a 6x6 grid; wave (pg, nh) owns one 3x3 QUADRANT of
// it (pg = 2*ah + bh) for all 32 tiles x 32 channels (nh): 9 accumulator tiles of the 32x32x2 fp32 MFMA = 144 registers.
//   * A operand (transformed input V): the 18 x 34 pixel x 8 channel patch of a K step is staged in LDS, transformed in two
//     separable passes -- columns once per patch column (shared by horizontally adjacent tiles), then rows per tile -- into
//     V[point][k half][tile][4]: a lane's MFMA fragment (4 k values) is one conflict-free ds_read_b128.
//   * B operand (transformed weights U, 36 x Cin x Cout floats): NOT staged through LDS -- 74 KB per K step would not fit twice
//     next to V.  wino44_weights_kernel lays U out in MFMA-fragment order ([k step][N tile][point][n half][lane][4]) and every
//     wave streams its own 1 KB per point straight from L2 into registers, two points ahead of its use.
//   * A K step is 36 MFMAs per wave (2304 cycles; 4608 per SIMD for 512 output pixels: 9 cycles per pixel and 8 channels against
//     16 on F(2x2,3x3)); the staging of the next step is cut into one-instruction pieces between them (sched_barrier).
//   * Output transform: a wave turns its 3x3 points into partial 4x4 outputs (two 3 -> 4 passes), keeps the 2x2 block it
//     finalises and sends the other three quadrants' blocks through LDS (4 rounds of 96 KB), then bias / activation / gate
//     and 16-byte stores through the usual LDS transposition.
#pragma once

constexpr int W4_PTS = 36;
constexpr int W4_BW = 32, W4_BH = 16;
constexpr int W4_PW = W4_BW + 2, W4_PH = W4_BH + 2;        // 34 x 18 patch
constexpr int W4_PPIX = W4_PW * W4_PH;                     // 612 pixels
constexpr int W4_V = W4_PTS * 2 * 32 * 4;                  // floats of one V image: [pt][k half][tile][4]
constexpr int W4_T = 4 * 6 * 2 * W4_PW * 4;                // column-transformed patch [tile row][a][quad][x][4]
constexpr int W4_P = 2 * W4_PPIX * 4;                      // patch [quad][pixel][4]
constexpr int W4_LDS_FLOATS = 2 * W4_V + 9216 + W4_P;      // 9216 >= W4_T: also the 8 x 1152-float store scratch
constexpr int W4_U_STEP = W4_PTS * 2 * 64 * 4;             // floats of U per (k step, N tile)
static_assert(W4_T <= 9216, "T area");
static_assert(4 * 4 * 3 * 2 * 64 * 4 <= W4_LDS_FLOATS, "exchange area");

struct Wino44Geom {
    int tiles_x, tiles_y, total_work, nt;
    int sy_min, sx_min;
    int interleave;
};

// 1D input transform Bt d (6 -> 6) of F(4,3):  rows [4 0 -5 0 1 0], [0 -4 -4 1 1 0], [0 4 -4 -1 1 0], [0 -2 -1 2 1 0],
// [0 2 -1 -2 1 0], [0 4 0 -5 0 1]
// (one output row at a time, computed right before its store: holding all six outputs next to the six inputs costs 24 registers
//  this kernel does not have; the shared sub-expressions are recomputed, +3 vector operations per pass)
template <int A>
__device__ __forceinline__ f32x4 w44_bt1(const f32x4 (&d)[6]) {
    if constexpr (A == 0) return 4.f * d[0] + (d[4] - 5.f * d[2]);
    else if constexpr (A == 1) return (d[4] - 4.f * d[2]) + (d[3] - 4.f * d[1]);
    else if constexpr (A == 2) return (d[4] - 4.f * d[2]) - (d[3] - 4.f * d[1]);
    else if constexpr (A == 3) return (d[4] - d[2]) + 2.f * (d[3] - d[1]);
    else if constexpr (A == 4) return (d[4] - d[2]) - 2.f * (d[3] - d[1]);
    else return 4.f * d[1] + (d[5] - 5.f * d[3]);
}
// half of the output transform At (4 x 6):  rows [1 1 1 1 1 0], [0 1 -1 2 -2 0], [0 1 1 4 4 0], [0 1 -1 8 -8 1]; h selects the
// columns 0..2 (h = 0) or 3..5 (h = 1): the contribution of three points to the four outputs
template <int h>
__device__ __forceinline__ void w44_at3(float x0, float x1, float x2, float (&o)[4]) {
    if constexpr (h == 0) {
        const float sm = x1 + x2, df = x1 - x2;
        o[0] = x0 + sm; o[1] = df; o[2] = sm; o[3] = df;
    } else {
        const float sm = x0 + x1, df = x0 - x1;
        o[0] = sm; o[1] = 2.f * df; o[2] = 4.f * sm; o[3] = 8.f * df + x2;
    }
}

// U[k/8][n/64][pt][(n%64)/32][lane = n%32 + 32*((k%8)/4)][k%4] = (G g Gt)[pt] -- the B fragment of MFMA j = k%4 of point pt for
// lane (n%32, k half): G = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
__device__ __forceinline__ void w44_g(float g0, float g1, float g2, float (&o)[6]) {
    o[0] = 0.25f * g0;
    o[1] = (-1.f / 6.f) * (g0 + g1 + g2);
    o[2] = (-1.f / 6.f) * (g0 - g1 + g2);
    o[3] = (1.f / 24.f) * g0 + (1.f / 12.f) * g1 + (1.f / 6.f) * g2;
    o[4] = (1.f / 24.f) * g0 - (1.f / 12.f) * g1 + (1.f / 6.f) * g2;
    o[5] = g2;
}
__device__ __forceinline__ void wino44_weights_body(const float* __restrict__ w, float* __restrict__ U, int N, int K, const WinoWeights& ww) {
    const int NT = N / 64;
    const size_t total = (size_t)N * K;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int blk = (int)(idx >> 9), e = (int)(idx & 511);
        const int kc = blk / NT, nt = blk - kc * NT;
        const int nh = e >> 8, lane = (e >> 2) & 63, j = e & 3;
        const int n = nt * 64 + nh * 32 + (lane & 31), k = kc * 8 + 4 * (lane >> 5) + j;
        const float* wp = w + (size_t)n * ww.sn + (size_t)k * ww.sk;
        float tg[6][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            float col[6];
            w44_g(wp[(size_t)(ww.kyu[0] * 3 + ww.kxv[v]) * ww.stap], wp[(size_t)(ww.kyu[1] * 3 + ww.kxv[v]) * ww.stap],
                  wp[(size_t)(ww.kyu[2] * 3 + ww.kxv[v]) * ww.stap], col);
#pragma unroll
            for (int a = 0; a < 6; ++a) tg[a][v] = col[a];
        }
        float* ub = U + (size_t)blk * W4_U_STEP + e;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            float row[6];
            w44_g(tg[a][0], tg[a][1], tg[a][2], row);
#pragma unroll
            for (int b = 0; b < 6; ++b) ub[(a * 6 + b) * 512] = row[b];
        }
    }
}
__global__ __launch_bounds__(256) void wino44_weights_kernel(const float* __restrict__ w, float* __restrict__ U, int N, int K, WinoWeights ww) {
    wino44_weights_body(w, U, N, K, ww);
}

// GBITS (with GATED): the ReLU gate as p.gate_bits, one dword per pixel and 32-channel group (e_nb0 = n0 + 32 nh, n0 a multiple
// of 64), each lane of a row of tile_rows4i taking its nibble -- as in wino_pipe_kernel<.., GBITS> (wino.inc)
template <bool GATED, bool GBITS = false>
__global__ __launch_bounds__(WINO_THREADS) void wino44_kernel(const IGemmParams p, const Wino44Geom q, const float* __restrict__ U) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                          // [2][36][2][32][4]
    float* Ts = smem + 2 * W4_V;               // [4][6][2][34][4]
    float* Ps = smem + 2 * W4_V + 9216;        // [2][612][4]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // provably wave-uniform: it feeds scalar buffer offsets
    const int pg = wave & 3, nh = wave >> 2, ah = pg >> 1, bh = pg & 1;
    int item, item_end, istep;
    wino_distribute(q.total_work, q.interleave, item, item_end, istep);
    if (item >= item_end) return;

    const int nchunks = p.C >> 3;
    const int img_bytes = p.IH * p.IW * p.C * 4;                     // one image per descriptor: any batch size stays below 2 GB
    auto srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src), 0, img_bytes, 0x00020000);
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U), 0, (int)((size_t)W4_PTS * p.N * p.C * 4), 0x00020000);

    // patch slots of this thread: slot = pixel * 2 + quad, 1224 slots on 512 threads
    int n0, oy0, ox0, b, i_nt;
    uint32_t poff[3];
    const bool p2_ok = tid + 2 * WINO_THREADS < 2 * W4_PPIX;
    auto decode = [&]() {
        i_nt = item % q.nt;
        int tile = item / q.nt;
        const int tx = tile % q.tiles_x;
        tile /= q.tiles_x;
        const int ty = tile % q.tiles_y;
        b = tile / q.tiles_y;
        n0 = i_nt * 64; oy0 = ty * W4_BH; ox0 = tx * W4_BW;
        srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.src) + (size_t)b * p.IH * p.IW * p.C, 0, img_bytes, 0x00020000);
        const int py0 = oy0 + q.sy_min, px0 = ox0 + q.sx_min;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int slot = tid + WINO_THREADS * i, pp = slot >> 1, spy = pp / W4_PW, spx = pp - spy * W4_PW;
            const int iy = py0 + spy, ix = px0 + spx;
            poff[i] = 0x80000000u;                      // beyond the descriptor's range: reads 0 (zero padding)
            if (pp < W4_PPIX && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW)
                poff[i] = (((uint32_t)iy * p.IW + ix) * (uint32_t)p.C + 4 * (slot & 1)) * 4u;
        }
    };
    f32x4 rp[3];
    auto pload1 = [&](int c, int i) { rp[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, poff[i], c * 32, 0)); };
    auto pstore1 = [&](int i) {
        const int slot = tid + WINO_THREADS * i;
        if (i < 2 || p2_ok) *reinterpret_cast<f32x4*>(Ps + ((slot & 1) * W4_PPIX + (slot >> 1)) * 4) = rp[i];
    };

    // pass 1 (columns): thread = (patch column x, quad, tile row ty): 6 patch rows -> 6 transform rows a
    const bool t1_on = tid < 2 * 4 * W4_PW;
    const int t1_x = tid % W4_PW, t1_q = (tid / W4_PW) & 1, t1_ty = (tid / W4_PW) >> 1;
    const int t1_src = (t1_q * W4_PPIX + (4 * (t1_on ? t1_ty : 0)) * W4_PW + t1_x) * 4;
    const int t1_dst = ((((t1_on ? t1_ty : 0) * 6) * 2 + t1_q) * W4_PW + t1_x) * 4;
    // pass 2 (rows): thread = (quad, tile, transform row a): 6 columns of row a -> points (a, 0..5)
    const bool t2_on = tid < 384;
    const int t2_q = tid & 1, t2_tile = (tid >> 1) & 31, t2_a = t2_on ? tid >> 6 : 0;
    const int t2_src = ((((t2_tile >> 3) * 6 + t2_a) * 2 + t2_q) * W4_PW + 4 * (t2_tile & 7)) * 4;
    const int t2_dst = ((t2_a * 6 * 2 + t2_q) * 32 + t2_tile) * 4;
    f32x4 td[6];
    auto t1_read = [&](int r) { td[r] = *reinterpret_cast<const f32x4*>(Ps + t1_src + r * (W4_PW * 4)); };
    auto t1_write = [&](auto ac) {
        constexpr int a = decltype(ac)::value;
        const f32x4 o = w44_bt1<a>(td);
        if (t1_on) *reinterpret_cast<f32x4*>(Ts + t1_dst + a * (2 * W4_PW * 4)) = o;
    };
    auto t2_read = [&](int j) { td[j] = *reinterpret_cast<const f32x4*>(Ts + t2_src + j * 4); };
    auto t2_write = [&](int buf, auto bc) {
        constexpr int bb = decltype(bc)::value;
        const f32x4 o = w44_bt1<bb>(td);
        if (t2_on) *reinterpret_cast<f32x4*>(Vs + buf * W4_V + t2_dst + bb * (2 * 32 * 4)) = o;
    };

    // MFMA operands: A fragment of point pt for lane (tile = lane & 31, k half = lane >> 5); B fragment straight from global
    const int a_off = ((lane >> 5) * 32 + (lane & 31)) * 4;
    auto pt_of = [&](int lp) { return (3 * ah + lp / 3) * 6 + 3 * bh + lp % 3; };
    const uint32_t u_voff = (uint32_t)((nh * 64 + lane) * 16);
    f32x4 fa[3], fb[3];
    auto uload = [&](int c, int lp, int slot) {
        fb[slot] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            ursrc, u_voff, (int)((((size_t)c * q.nt + i_nt) * W4_U_STEP + (size_t)pt_of(lp) * 512) * 4), 0));
    };

    for (;;) {
        decode();
        f32x16 acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

        // prologue: step 0 staged synchronously, step 1's patch in flight
#pragma unroll
        for (int i = 0; i < 3; ++i) pload1(0, i);
        uload(0, 0, 0);
        uload(0, 1, 1);
#pragma unroll
        for (int i = 0; i < 3; ++i) pstore1(i);
#pragma unroll
        for (int i = 0; i < 3; ++i) pload1(min(1, nchunks - 1), i);
        wino_barrier();
#pragma unroll
        for (int r = 0; r < 6; ++r) t1_read(r);
        wino_static_for(std::make_integer_sequence<int, 6>{}, [&](auto ac) { t1_write(ac); });
        wino_barrier();
#pragma unroll
        for (int j = 0; j < 6; ++j) t2_read(j);
        wino_static_for(std::make_integer_sequence<int, 6>{}, [&](auto bc) { t2_write(0, bc); });
        wino_barrier();
        fa[0] = *reinterpret_cast<const f32x4*>(Vs + pt_of(0) * 256 + a_off);

        int cur = 0;
        for (int c = 0; c < nchunks; ++c) {
            const int nxt = cur ^ 1;
            const int c1 = min(c + 1, nchunks - 1), c2 = min(c + 2, nchunks - 1);
            const float* Vc = Vs + cur * W4_V + a_off;
            const float* Vn = Vs + nxt * W4_V + a_off;
            // 36 MFMA ticks: t = 4 * lp + e (local point lp of this wave's quadrant, k pair e).  Between them, one piece per
            // tick, the staging of step c + 1:  patch -> LDS | barrier | column pass -> T | barrier | row pass -> V[nxt] | barrier
            wino_static_for(std::make_integer_sequence<int, 36>{}, [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int lp = t >> 2, e = t & 3;
                if constexpr (t < 3) pstore1(t);                                  // rp = patch of step c + 1
                if constexpr (t == 3) wino_barrier();
                if constexpr (t >= 3 && t < 6) pload1(c2, t - 3);                 // patch of step c + 2
                if constexpr (t >= 4 && t < 10) t1_read(t - 4);
                if constexpr (t >= 11 && t < 17) t1_write(std::integral_constant<int, (t >= 11 && t < 17) ? t - 11 : 0>{});
                if constexpr (t == 17) wino_barrier();
                if constexpr (t >= 18 && t < 24) t2_read(t - 18);
                if constexpr (t >= 25 && t < 31) t2_write(nxt, std::integral_constant<int, (t >= 25 && t < 31) ? t - 25 : 0>{});
                if constexpr (t == 31) wino_barrier();
                if constexpr (e == 0) {
                    // operands two / one point(s) ahead: U of point lp + 2 from L2, the V fragment of point lp + 1 from LDS
                    if constexpr (lp < 7) uload(c, lp + 2, (lp + 2) % 3);
                    else uload(c1, lp - 7, (lp + 2) % 3);
                    if constexpr (lp < 8) fa[(lp + 1) % 3] = *reinterpret_cast<const f32x4*>(Vc + pt_of(lp + 1) * 256);
                    else fa[0] = *reinterpret_cast<const f32x4*>(Vn + pt_of(0) * 256);      // behind barrier t = 31
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[lp] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[lp % 3][e], fb[lp % 3][e], acc[lp], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
            cur = nxt;
        }
        const bool more_items = item + istep < item_end;
        wino_barrier();        // every wave is past its last V read: the whole LDS becomes the exchange area

        // ---- output transform: partial 4x4 outputs of this quadrant's 3x3 points; 2x2 blocks exchanged between the quadrants ----
        float* X = smem;       // [el 4][dst quadrant 4][source rank 3][nh 2][lane 64][4]
        float y[4][16];        // the 2x2 output block (di, dj) this wave finalises, MFMA-tile shaped (scalars: they take over the
                               // registers of the accumulator elements already consumed)
        // one specialisation per quadrant (the transform halves and the exchange slots become compile-time)
        auto out_xform = [&](auto ahc, auto bhc) {
            constexpr int AH = decltype(ahc)::value, BH = decltype(bhc)::value, PG = 2 * AH + BH;
#pragma unroll
            for (int rd = 0; rd < 4; ++rd) {
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int el = 4 * rd + k4;
                    float T[3][4], P[4][4];
#pragma unroll
                    for (int al = 0; al < 3; ++al) w44_at3<BH>(acc[3 * al][el], acc[3 * al + 1][el], acc[3 * al + 2][el], T[al]);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float col[4];
                        w44_at3<AH>(T[0][jj], T[1][jj], T[2][jj], col);
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii) P[ii][jj] = col[ii];
                    }
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int di = 2 * (d >> 1), dj = 2 * (d & 1);
                        const f32x4 v = {P[di][dj], P[di][dj + 1], P[di + 1][dj], P[di + 1][dj + 1]};
                        if (d == PG) {
#pragma unroll
                            for (int px = 0; px < 4; ++px) y[px][el] = v[px];
                        } else {
                            const int sr = PG < d ? PG : PG - 1;
                            *reinterpret_cast<f32x4*>(X + ((((k4 * 4 + d) * 3 + sr) * 2 + nh) * 64 + lane) * 4) = v;
                        }
                    }
                }
                wino_barrier();
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int el = 4 * rd + k4;
#pragma unroll
                    for (int sr = 0; sr < 3; ++sr) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(X + ((((k4 * 4 + PG) * 3 + sr) * 2 + nh) * 64 + lane) * 4);
#pragma unroll
                        for (int px = 0; px < 4; ++px) y[px][el] += v[px];
                    }
                }
                wino_barrier();
            }
        };
        if (pg == 0) out_xform(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        else if (pg == 1) out_xform(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        else if (pg == 2) out_xform(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
        else out_xform(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
        // ---- epilogue: bias / activation / gate, 16-byte stores (rows of the MFMA tile = the 32 tiles of the block) ----
        // Addresses as in wino_pipe_kernel: the output row  oy0 + 4 t4 + 2 ah + di  is wave-uniform (t4 = row group of
        // tile_rows4i), the column  ox0 + 4 (lane >> 3) + 2 bh + dj  a lane constant plus uniform terms -- buffer instructions
        // with one lane offset per pixel position and scalar row offsets; lanes beyond the right edge carry the out-of-range
        // marker, rows beyond the bottom edge are a scalar branch; activation without a switch per element.  (The generic
        // form -- 64-bit pixel arithmetic and the act / bias / row-scale / accumulate switches for each of 16 stores -- was
        // 11 of the 22 us an item costs on top of its K steps, tools/wino44_item_overhead.py; wino44_ok keeps row scales
        // and tensors of 2 GB and more on the F(2x2,3x3) kernels.)
        const int e_n0 = n0, e_oy0 = oy0, e_ox0 = ox0, e_b = b;
        float* scratch = Ts + wave * (32 * 36);
        const int e_nb0 = e_n0 + 32 * nh;
        const int e_pitch = p.DW * p.ds;
        const int e_pix0 = (e_b * p.DH + p.dy0) * p.DW + p.dx0 + (e_ox0 + 2 * bh) * p.ds;     // + row * e_pitch + dj * ds (+ lane part)
        const uint32_t e_lane = (uint32_t)(4 * (lane >> 3) * p.ds * p.N + 4 * (lane & 7)) * 4u;
        const int e_lane_ox = e_ox0 + 4 * (lane >> 3) + 2 * bh;
        const float act_neg = p.act == TG_ACT_RELU ? 0.f : (p.act == TG_ACT_LEAKY ? p.slope : 1.f);
        const float gate_neg = p.gate_act == TG_ACT_LEAKY ? p.gate_slope : 0.f;
        const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(p.dst, 0, (int)((size_t)p.B * p.DH * p.DW * p.N * 4), 0x00020000);
        f32x4 bq = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bq = *reinterpret_cast<const f32x4*>(p.bias + e_nb0 + 4 * (lane & 7));
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int di = px >> 1, dj = px & 1;
            const uint32_t e_voff = e_lane_ox + dj < p.OW ? e_lane : 0x80000000u;
            const int e_row0 = e_oy0 + 2 * ah + di;                              // + 4 * t4
            f32x4 gq[GATED && !GBITS ? 4 : 1];
            uint32_t gw[GBITS ? 4 : 1];
            if constexpr (GBITS) {       // the gate words of this pixel position ahead of its stores
                const int nw32 = p.N >> 5;
                const auto brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(p.gate_bits), 0, (int)((size_t)p.B * p.DH * p.DW * nw32 * 4), 0x00020000);
                const uint32_t b_voff = e_lane_ox + dj < p.OW ? (uint32_t)(4 * (lane >> 3) * p.ds * nw32) * 4u : 0x80000000u;
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int row = min(e_row0 + 4 * t4, p.OH - 1);
                    gw[t4] = __builtin_amdgcn_raw_buffer_load_b32(brsrc, b_voff, ((e_pix0 + row * e_pitch + dj * p.ds) * nw32 + (e_nb0 >> 5)) * 4, 0)
                             >> (4 * (lane & 7));
                }
            } else if constexpr (GATED) {       // the gate quads of this pixel position ahead of its stores (vmcnt counts stores too)
                const auto grsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gate), 0, (int)((size_t)p.B * p.DH * p.DW * p.N * 4), 0x00020000);
#pragma unroll
                for (int t4 = 0; t4 < 4; ++t4) {
                    const int row = min(e_row0 + 4 * t4, p.OH - 1);
                    gq[t4] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                        grsrc, e_voff, ((e_pix0 + row * e_pitch + dj * p.ds) * p.N + e_nb0) * 4, 0));
                }
            }
            f32x16 yv;
#pragma unroll
            for (int r = 0; r < 16; ++r) yv[r] = y[px][r];
            tile_rows4i(scratch, yv, lane, [&](int t4, int rr, int cc, f32x4 v4) {
                const int row = e_row0 + 4 * t4;
                if (row >= p.OH) return;                                         // wave-uniform
                const uint32_t soff = (uint32_t)(((e_pix0 + row * e_pitch + dj * p.ds) * p.N + e_nb0) * 4);
                f32x4 o = v4 + bq;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f) + act_neg * fminf(o[e], 0.f);         // none / ReLU / leaky
                if constexpr (GBITS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] *= (gw[t4] >> e) & 1u ? 1.f : 0.f;
                } else if constexpr (GATED) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] *= gq[t4][e] > 0.f ? 1.f : gate_neg;
                }
                if (p.accumulate) o += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, e_voff + soff, 0, 0));
                // row offset in the VECTOR offset: see wino_pipe_kernel (scalar-offset stores and the data-register hazard)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), drsrc, e_voff + soff, 0, 0);
            });
        }
        if (!more_items) break;
        item += istep;
        wino_barrier();        // the store scratch (T area) is free again before the next item's column pass writes it
    }
}

static bool wino44_enabled() {
    static const bool off = getenv("TG_NO_WINO") != nullptr || getenv("TG_NO_WINO44") != nullptr;
    return !off;
}
// geometry of the IMPLICIT problem (p.C = contraction channels, p.N = output channels, p.OH x p.OW = output grid)
// Two predicates, because the prepared weights outlive the call that made them (tg_conv_wprep + the caller's cache):
//  * wino44_geom_ok: what decides the LAYOUT of a prepared buffer -- channels, taps, image size, precision: exactly the
//    fields a caller's cache key holds (tg_hip.ops._prepared), nothing that varies from launch to launch;
//  * wino44_runtime_ok: what only a launch knows -- batch size (dst < 2 GB), row scales, an input mask.  A launch that fails
//    it while holding an F(4x4) buffer transforms F(2x2) weights into its workspace instead (conv_fwd_impl / conv_dgrad_impl).
static bool wino44_geom_ok(const IGemmParams& p) {
    if (!wino44_enabled() || p.wino_u == nullptr || p.bf16 || !p.wino4) return false;
    if (p.TH != 3 || p.TW != 3 || p.ss != 1 || (p.tstep != 1 && p.tstep != -1) || (p.kstep != 1 && p.kstep != -1)) return false;
    if ((p.C % 8) != 0 || (p.N % 64) != 0 || p.OH < 16 || p.OW < 32) return false;
    if ((size_t)p.IH * p.IW * p.C * 4 >= ((size_t)1 << 31) || (size_t)W4_PTS * p.N * p.C * 4 >= ((size_t)1 << 31)) return false;
    return true;
}
static bool wino44_runtime_ok(const IGemmParams& p) {
    // the epilogue addresses dst / gate through buffer descriptors and knows bias, activation, gate and accumulate only
    return p.amask == nullptr && p.rowscale == nullptr && (size_t)p.B * p.DH * p.DW * p.N * 4 < ((size_t)1 << 31);
}
static bool wino44_ok(const IGemmParams& p) {
    return wino44_geom_ok(p) && (p.wino_ready < 0 || wino44_runtime_ok(p));
}
// a prepared buffer in the F(4x4) layout met a launch that cannot run on wino44_kernel
static bool wino44_prepared_unusable(const IGemmParams& p) { return p.wino_ready > 0 && wino44_geom_ok(p) && !wino44_runtime_ok(p); }
static size_t wino44_u_floats(int N, int C) { return (size_t)W4_PTS * N * C; }

static int launch_wino44(IGemmParams& p, hipStream_t s) {
    Wino44Geom q = {};
    q.tiles_x = cdiv(p.OW, W4_BW);
    q.tiles_y = cdiv(p.OH, W4_BH);
    q.nt = p.N / 64;
    q.total_work = q.tiles_x * q.tiles_y * p.B * q.nt;
    q.interleave = wino_interleave_ok(wino44_u_floats(p.N, p.C) * sizeof(float));
    const int sy_b = p.sy0 + 2 * p.tstep, sx_b = p.sx0 + 2 * p.tstep;
    q.sy_min = p.sy0 < sy_b ? p.sy0 : sy_b;
    q.sx_min = p.sx0 < sx_b ? p.sx0 : sx_b;
    const WinoWeights ww = wino_weights_map(p, q.sy_min, q.sx_min);
    p.splits = 1;
    p.Ktot = 9 * p.C;
    const TgWprepItem it = {};        // (kind 0: not batched -- prepared once, for the frozen trunk)
    int rc = TG_OK;
    const auto transform = [&]() -> int {
        hipLaunchKernelGGL(wino44_weights_kernel, dim3(ew_grid((int64_t)p.N * p.C, 256)), dim3(256), 0, s, p.w_raw, p.wino_u, p.N, p.C, ww);
        TG_CHECK_LAUNCH("wino44_weights_kernel");
        return TG_OK;
    };
    if (wino_prep(p, it, transform, &rc)) return rc;
    const bool gated = p.gate != nullptr;
    const bool gbits = p.gate_bits != nullptr;      // (one split always: the bits are read here)
    if (gbits) p.gate_bits_done = 1;
    const int ki = gbits ? 2 : gated ? 1 : 0;
    typedef void (*Kern)(const IGemmParams, const Wino44Geom, const float*);
    static const Kern kerns[3] = {wino44_kernel<false>, wino44_kernel<true>, wino44_kernel<true, true>};
    static LdsOptIn opts[3];
    const WinoProf pf = {0, 4044, p.M, 2.0 * p.M * (double)p.N * p.Ktot * g_alg_scale,
                         4.0 * ((double)p.B * p.IH * p.IW * p.C + (double)p.N * p.Ktot + (double)p.M * p.N), WR_FIRST + ki};
    return wino_launch(kerns[ki], opts[ki], (size_t)W4_LDS_FLOATS * sizeof(float), "wino44_kernel", p, q, pf, false, s);
}
