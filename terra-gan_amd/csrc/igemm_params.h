// Parameter blocks shared by the MFMA conv kernels (igemm.hip) and the small-channel kernels (smallconv.hip).
#pragma once
#include "common.h"

// BatchNorm + activation applied to the SOURCE tensor as it is staged (tg_conv_fwd_bnin / tg_conv_wgrad_bnin): the layer's input
// is act(BN(src)) without that tensor ever being written.  mean == nullptr: none.
struct BnIn {
    const float *mean, *rstd, *gamma, *beta;
    int act;
    float slope;
};
struct IGemmParams {
    const float* src;       // A source, NHWC [B][IH][IW][C]
    const float* amask;     // optional [B][IH][IW]: A row scale at the SOURCE pixel (x (.) mask)
    const float* wmat;      // B matrix [N][Kfull], K-contiguous, K index = tapidx*C + c
    const float* bias;      // optional [N]
    const float* rowscale;  // optional, indexed by DESTINATION pixel (ratio / dgrad mask)
    float* dst;             // NHWC [B][DH][DW][N]
    float* ws;              // split-K slabs [splits][M][N] when splits > 1
    int B, IH, IW, C;
    int OH, OW, N, M;       // output grid of this launch, M = B*OH*OW
    int DH, DW, ds, dy0, dx0;           // grid point (oy,ox) -> dst pixel (oy*ds+dy0, ox*ds+dx0)
    int TH, TW, ss, tstep, sy0, sx0;    // tap (ty,tx) -> src pixel (oy*ss+sy0+ty*tstep, ...)
    int KW, kstep, ky0, kx0;            // tap (ty,tx) -> weight tap (ky0+ty*kstep)*KW + kx0+tx*kstep
    int Kfull, Ktot;        // wmat row length; K elements walked by this launch (TH*TW*C)
    int nchunks, T;         // ceil(C/32); number of 32-deep K steps
    int splits, steps_per_split;
    int act;
    float slope;
    int accumulate;
    int bf16;               // operands rounded to bf16 at LDS staging, v_mfma_f32_32x32x16_bf16 (patch kernel only)
    const float* gate;      // optional [dst pixels][N]: result *= act'(gate) (fused activation backward)
    int gate_act;
    float gate_slope;
    // Winograd path (wino.inc): raw weights with the element strides of (output row n, contraction k, tap), and room
    // for the transformed weights; wino_u == nullptr disables it
    const float* w_raw;
    long w_sn, w_sk, w_stap;
    float* wino_u;
    int wino4;              // TG_PREC_F32_WINO4: Winograd F(4x4,3x3) where the geometry allows (wino44.inc)
    int wino_ready;         // wino_u already holds the transformed weights (prepared by tg_conv_wprep): skip the transform
    // 2x2 / stride-2 max-pool of the (activated) output, written next to dst from the output transform (tg_conv_fwd_pool):
    // [B][OH/2][OW/2][N].  A launcher that writes it sets pool_done; otherwise the caller runs the pool kernel on dst.
    float* pool_dst;
    int pool_done;
    // tg_conv_fwd_pool_code: with the pooled tensor a BYTE per pooled element and channel -- bits 0-1 the window position of the
    // maximum (2*row + column, first maximum wins as in ATen), bit 2 "maximum > 0" (the ReLU gate) -- which is all the pool's
    // backward needs; pool_only: dst itself is NOT written (its only readers were the pool and that backward)
    unsigned char* pool_code;
    int pool_only;
    BnIn in_bn;             // (the 64 -> 1 channel LDS-patch kernel only: `final`, smallconv.hip)
    // optional [dst pixels][N/32] words, bit c % 32 of word c / 32 = (ReLU output > 0) (tg_relu_gate_pack): a ReLU gate in one
    // bit per element, exclusive with `gate`.  Read natively by the GBITS instantiations of the pipelined Winograd kernels (which
    // set gate_bits_done); every other launch runs ungated and tg_conv_dgrad_gbits applies the bits afterwards (gate_bits_apply).
    const uint32_t* gate_bits;
    int gate_bits_done;
    // tg_conv_fwd_sparse: prediction-half tile map of a [pred; target] batch (host side; launch_wino decides whether it applies)
    // tg_conv_dgrad_sparse: the map of a batch of sparse->nb images.  The 64 -> 1 channel LDS-patch launch that honours it and
    // zeroes every pixel outside sparse->pix sets sparse_pix_done; otherwise the caller zeroes them (pix_zero_launch)
    const TgSparseMap* sparse;
    int sparse_pix_done;
};
__device__ __forceinline__ float gate_factor(const IGemmParams& p, size_t idx) {
    const float gv = p.gate[idx];
    return gv > 0.f ? 1.f : (p.gate_act == TG_ACT_LEAKY ? p.gate_slope : 0.f);
}

// dx[row][c] *= bit c of the row's words: the multiply of gate_factor (ReLU) as a pass of its own (pointwise.hip)
int gate_bits_apply_launch(float* dx, const uint32_t* bits, int64_t rows, int C, hipStream_t s);

// Up to 4 independent problems in ONE launch (the parity classes of a stride-2 dgrad)
struct IGemmMulti {
    IGemmParams c[4];
    int zbeg[5];            // igemm_multi_kernel: class i owns blockIdx.z in [zbeg[i], zbeg[i + 1]) -- its own split count (c[i].splits)
};

struct WgradParams {
    const float* x;
    const float* amask;
    const float* dy;
    float* out;  // [splits][Cout][Ktot]
    int B, H, W, C, Ho, Wo, Cout, k, stride, pad;
    int Mpix, Ktot, T, splits, steps_per_split;
    int nx, ny;   // N' tiles, Cout tiles (grid is launched flat: nx*ny*splits workgroups)
    int rowseg;   // Wo % 32 == 0: every 32-pixel K step lies inside one output row (cheap gather addressing)
    BnIn in_bn;   // (to1wgrad64_lds_kernel only)
};

// Which kernel a small-channel launch runs (smallconv.hip).  The three launchers choose it in one function each and switch on it,
// and the launch records carry it (ProfRec::route, column `route` of tg_prof_dump), so a test can pin the kernel that ran: the
// records' cfg is 2000 / 2001 / 2004 for all of them.  0 = not a small-channel launch.
enum SmallRoute {
    SR_NONE = 0,
    SR_C1MFMA = 100,                // + taps per side (7 | 4 | 3): c1mfma_kernel<k, k>
    SR_C1CONV = 110,                // + 7 | 4 | 3, + 0 = the runtime-tap instantiation: c1conv_kernel<k, k>
    SR_TO1CONVW = 200,              // + 10 k + CQ (k = 3 | 4, CQ = C / 256): to1convw_kernel<k, k, CQ>
    SR_TO1_LDS = 300,               // to1conv64_lds_kernel<false>
    SR_TO1_LDS_BNIN = 301,          // to1conv64_lds_kernel<true>: BatchNorm-on-load
    SR_TO1_LDS_MAP = 302,           // to1conv64_lds_kernel<false, true>: tile map
    SR_TO1CONV64 = 400,             // + 10 TH + TW: to1conv64_kernel<TH, TW>
    SR_MULTI22_LDS = 500,           // to1conv64_multi22_lds_kernel
    SR_MULTI22 = 501,               // to1conv64_multi22_kernel
    SR_C1WGRAD_MFMA = 600,          // + k (7 | 4 | 3): c1wgrad_mfma_kernel<k> without bias partials
    SR_C1WGRAD_MFMA_BIAS = 610,     // + k: ... with bias partials
    SR_C1WGRAD = 620,               // + k: c1wgrad_kernel<k>
    SR_TO1WGRADW = 700,             // + k (3 | 4): to1wgradw_kernel<k>
    SR_TO1WGRAD_LDS = 800,          // to1wgrad64_lds_kernel<false>
    SR_TO1WGRAD_LDS_BNIN = 801,     // to1wgrad64_lds_kernel<true>
    SR_TO1WGRAD64 = 900,            // + k (3 | 4): to1wgrad64_kernel<k>
};

// Which instantiation a Winograd launch runs: the same column of the launch records.  The records' cfg names the family (4064 /
// 4016 F(2x2,3x3) in fp32 / bf16, 4022 F(2x2,2x2), 4044 F(4x4,3x3), 4164 / 4116 / 4122 their weight gradients); the route is
// WR_FIRST + the index into the launcher's kernel table, so 0 stays "not recorded".
//   4064 (launch_wino, WinoPlan::kernel):  1 wino_kernel  2 + gate  3 fast  4 fast + gate  5 wino_pipe_kernel  6 + gate  7 + pool
//                                          8 + bit gate;  9-16 the same eight with a work-stealing queue;  17 tile map  18 tile map
//                                          + pool;  19-21 the list-only tile map: plain, gate, bit gate
//   4016 (launch_wino, bf16):              1-8 as 4064's first eight (wino16_kernel / wino16_pipe_kernel)
//   4022 (launch_wino22):                  1 + (queue ? 4 : 0) + (fast ? 2 : 0) + gate;  + 8: the wide form, wino22w_kernel (fast only)
//   4044 (launch_wino44):                  1 plain  2 gate  3 bit gate
//   4164 / 4116 / 4122:                    1 (one kernel each)
enum WinoRoute {
    WR_NONE = 0,
    WR_FIRST = 1,                   // + kernel-table index
    WR_PIPE = WR_FIRST + 4,         // wino_pipe_kernel / wino16_pipe_kernel: + gate; + 2 pool; + 3 bit gate
    WR_QUEUED = WR_FIRST + 8,       // 4064: + the static walk's index
    WR_MAP = WR_FIRST + 16,         // 4064: + pool
    WR_MAP_LIST = WR_FIRST + 18,    // 4064: + gate; + 2 bit gate
    WR_W22_FAST = 2, WR_W22_QUEUED = 4,         // 4022: WR_FIRST + these + gate
    WR_W22_WIDE = 8,                // 4022: + the narrow form's index (128-channel items)
    WR_WGRAD = WR_FIRST,
};

// smallconv.hip: bandwidth-bound special cases that would waste >95% of an MFMA tile.  The launchers report the route they took
// through `route` (a SmallRoute value).
bool smallconv_fwd_applies(const IGemmParams& p);             // C == 1 -> N%64 == 0, or N == 1 <- C%64 == 0
int smallconv_fwd_launch(const IGemmParams& p, hipStream_t s, int* route = nullptr);
bool smallconv_to1_map_ok(const IGemmParams& p);              // smallconv_fwd_launch will honour p.sparse (64 -> 1, LDS patch)
// dx[b][y][x] = 0 where bit x of pix[b][y] is clear (pointwise.hip)
int pix_zero_launch(float* dx, const uint64_t* pix, int B, int H, int W, hipStream_t s);
bool smallconv_to1_multi_applies(const IGemmParams* cls, int ncls);   // 64 -> 1 channel, the four 2x2-tap classes of a 4x4 stride-2 dgrad
int smallconv_to1_multi_launch(const IGemmParams* cls, int ncls, hipStream_t s, int* route = nullptr);
bool smallconv_wgrad_applies(const WgradParams& p);
bool smallconv_bnin_fwd_ok(const IGemmParams& p);             // launches that can take IGemmParams::in_bn / WgradParams::in_bn
bool smallconv_bnin_wgrad_ok(const WgradParams& p);
size_t smallconv_wgrad_ws_floats(const WgradParams& p);
int smallconv_wgrad_launch(const WgradParams& p, float* dw, float* ws, size_t ws_floats, hipStream_t s, float* db = nullptr,
                           int* db_done = nullptr, int* route = nullptr);
