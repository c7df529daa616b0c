/*
 * terragan_hip.h -- C ABI of libterragan_hip.so: the MI355X (gfx950) kernels behind TERRA-GAN's
 * partial-convolution inpainting train step.
 *
 * The reference (/root/reference) is pure Python on stock ATen ops and has no native interface;
 * each entry point below names the reference arithmetic it replaces (file:line) and is what a
 * maintainer would bind (ctypes stub in INTEGRATION.md) from mvp_gan/src/models/{pconv,generator,discriminator}.py,
 * mvp_gan/src/utils/losses.py and mvp_gan/src/train.py.
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are DEVICE pointers (fp32 unless noted);
 *   - activations are NHWC ("channels-last"): [B][H][W][C]; masks are [B][H][W] fp32 {0,1},
 *     1 = valid pixel, 0 = hole (dataset.py:37, generator.py:60-62);
 *   - conv weights are [Cout][kh][kw][Cin] (= the channels_last storage of an OIHW tensor);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates,
 *     never synchronises; scratch memory is supplied by the caller (`ws`, sized by the matching
 *     tg_*_ws_bytes query);
 *   - return 0 on success, negative TG_ERR_* otherwise; tg_last_error() gives the thread-local
 *     message.  Invalid shapes are rejected on the host before any launch.
 */
#ifndef TERRAGAN_HIP_H
#define TERRAGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tg_stream_t; /* hipStream_t */

enum { TG_OK = 0, TG_ERR_ARG = -1, TG_ERR_LAUNCH = -2, TG_ERR_WS = -3 };
enum { TG_ACT_NONE = 0, TG_ACT_RELU = 1, TG_ACT_LEAKY = 2 };
/* Arithmetic of the conv inner product.  TG_PREC_BF16: operands are rounded to bf16 inside the kernel and multiplied
 * on the bf16 MFMA with fp32 accumulation; tensors in memory, bias, mask ratio and epilogue stay fp32
 * (BASELINE config 3: bf16 compute, fp32 master weights).  Kernels without a bf16 variant ignore it. */
enum { TG_PREC_F32 = 0, TG_PREC_BF16 = 1, TG_PREC_F32_WINO4 = 2 };
/* TG_PREC_F32_WINO4: fp32 arithmetic as TG_PREC_F32, but stride-1 3x3 convolutions (forward and dgrad) with Cin % 8 == 0,
 * Cout % 64 == 0, >= 16 x 32 outputs, no input mask / row scale and tensors below 2 GB run as Winograd F(4x4,3x3) (36 multiplies per 16 outputs instead of 16 per 4): faster,
 * with 6-7x the rms (~20x the maximum: 1e-5 of the tensor's largest value) rounding error of the default F(2x2,3x3) per layer.  The train step requests it for the frozen VGG16 trunk of
 * the perceptual loss only (losses.py:31-34,79-90), whose stated tolerances it keeps; everything else ignores the hint. */

/* Geometry of one 2-D convolution (square kernel, symmetric padding). */
typedef struct TgConv {
    int32_t B, H, W, Cin;   /* input  [B][H][W][Cin]   */
    int32_t Ho, Wo, Cout;   /* output [B][Ho][Wo][Cout] */
    int32_t k, stride, pad;
    int32_t precision;      /* TG_PREC_* */
} TgConv;

int tg_version(void);
const char* tg_last_error(void);

/* ---- partial / plain convolution: implicit-GEMM on fp32 MFMA ------------------------------- */

/* y = act( (conv(x (.) in_mask, w) + bias) * ratio )
 * Replaces PConv2d.forward's input*mask -> input_conv -> output*mask_ratio (pconv.py:27-30,43)
 * when in_mask/ratio are given, and nn.Conv2d (+LeakyReLU/ReLU) otherwise
 * (generator.py:29,56; discriminator.py:11,15,22; losses.py:32 VGG trunk).
 * in_mask [B][H][W], bias [Cout], ratio [B][Ho][Wo] may be NULL.
 * ws >= tg_conv_fwd_ws_bytes: weight-transform room + split-K room of 64 output slabs (at most 64 Mi floats).  The split-K
 * planners use no more than that, so the result is the same bit for bit for any larger workspace. */
size_t tg_conv_fwd_ws_bytes(const TgConv* g);
int tg_conv_fwd(const TgConv* g, const float* x, const float* in_mask, const float* w,
                const float* bias, const float* ratio, int act, float slope, float* y,
                float* ws, size_t ws_bytes, tg_stream_t stream);

/* dx (+)= conv_transpose(dy, w) (.) in_mask   -- autograd of the conv above w.r.t. x.
 * dy must already carry the ratio factor.  accumulate!=0 adds into dx (skip connections).
 * ws >= tg_conv_dgrad_ws_bytes (holds the [Cin][kh][kw][Cout] transposed weights + split-K room of 64 slabs of dx, at most
 * 64 Mi floats; as for the forward, a larger workspace gives the same bits). */
size_t tg_conv_dgrad_ws_bytes(const TgConv* g);
int tg_conv_dgrad(const TgConv* g, const float* dy, const float* w, const float* in_mask,
                  float* dx, int accumulate, float* ws, size_t ws_bytes, tg_stream_t stream);
/* Same, with the backward of the activation that PRODUCED x fused into the epilogue:
 * dx = (convT(dy, w) (.) in_mask) * act'(x_act), x_act = that activation's output [B][H][W][Cin]
 * (ReLU of the VGG trunk, LeakyReLU of the discriminator's first block). */
int tg_conv_dgrad_gated(const TgConv* g, const float* dy, const float* w, const float* in_mask,
                        const float* x_act, int act, float slope, float* dx, float* ws,
                        size_t ws_bytes, tg_stream_t stream);

/* Prepared weights.  The weight rearrangements inside tg_conv_fwd / tg_conv_dgrad (Winograd transform of the stride-1 3x3
 * layers, the [Cin][kh][kw][Cout] transpose of the gather dgrads, the 3x3 x 4C regrouping of 5x5 stride-2 layers) depend
 * on the weights only: a caller that keeps them once per optimiser step (once ever for the frozen VGG trunk of
 * losses.py:31-34) saves ~45 small launches per train step.  tg_conv_wprep_bytes == 0: that (geometry, mode) runs on the
 * raw weights.  The *_p entry points equal tg_conv_fwd / tg_conv_dgrad / tg_conv_dgrad_gated (x_act != NULL) when
 * wprep == NULL; with wprep they skip the preparation and need no workspace room for it.  A prepared buffer is valid for
 * the geometry (all TgConv fields but B) and mode it was made for, until the weights change. */
enum { TG_WPREP_FWD = 0, TG_WPREP_DGRAD = 1 };
size_t tg_conv_wprep_bytes(const TgConv* g, int mode);
int tg_conv_wprep(const TgConv* g, int mode, const float* w, float* wprep, tg_stream_t stream);
/* Batched form: tg_conv_wprep_item writes a POD descriptor (tg_conv_wprep_item_bytes() bytes, HOST memory) of what
 * tg_conv_wprep(g, mode, w, wprep) would launch and returns 1 -- or returns 0 when that preparation cannot be batched (it
 * stays with tg_conv_wprep).  The caller copies the descriptors of all its layers into one DEVICE array once and has them
 * executed by ONE launch per optimiser step: tg_conv_wprep_run(items_dev, n).  The descriptors hold the w / wprep pointers:
 * they stay valid while those allocations live. */
size_t tg_conv_wprep_item_bytes(void);
int tg_conv_wprep_item(const TgConv* g, int mode, const float* w, float* wprep, void* item_out);
int tg_conv_wprep_run(const void* items_dev, int n, tg_stream_t stream);
int tg_conv_fwd_p(const TgConv* g, const float* x, const float* in_mask, const float* w, const float* wprep,
                  const float* bias, const float* ratio, int act, float slope, float* y, float* ws,
                  size_t ws_bytes, tg_stream_t stream);
/* tg_conv_fwd_p plus the 2x2 / stride-2 max-pool of its (activated) output: y [B][Ho][Wo][Cout] AND pool_y [B][Ho/2][Wo/2][Cout]
 * (Ho, Wo even).  Replaces  features[i](x) -> ReLU -> MaxPool2d(2)  of the frozen VGG16 trunk
 * (/root/reference/mvp_gan/src/utils/losses.py:31-34,79-90: torchvision vgg16().features[:16], layers 2-4 and 7-9) in one call:
 * the stride-1 3x3 fp32 Winograd kernel writes the pooled tensor from its output transform (a 2x2 output tile is a pooling
 * window); every other geometry runs tg_maxpool2_fwd on y.  Same values either way. */
int tg_conv_fwd_pool(const TgConv* g, const float* x, const float* in_mask, const float* w, const float* wprep,
                     const float* bias, const float* ratio, int act, float slope, float* y, float* pool_y, float* ws,
                     size_t ws_bytes, tg_stream_t stream);
/* conv -> ReLU -> MaxPool2d(2) where the full-resolution conv output has no other reader than the pool and the pool's backward
 * (torchvision vgg16().features[2..4] and [7..9], losses.py:31-34,79-90): writes the pooled tensor [B][Ho/2][Wo/2][Cout] and one
 * CODE byte per pooled element and channel (bits 0-1: window position 2*row + column of the maximum, the first one as in ATen;
 * bit 2: maximum > 0, i.e. the ReLU gate) -- the conv output itself is never written.  tg_maxpool2_bwd_code turns the pooled
 * gradient + code into the full-resolution gradient in front of the ReLU.  Only where the fp32 Winograd kernel takes the
 * launch in one K split: tg_conv_pool_code_supported (callers fall back to tg_conv_fwd_pool / tg_maxpool2_bwd). */
int tg_conv_pool_code_supported(const TgConv* g);
int tg_conv_fwd_pool_code(const TgConv* g, const float* x, const float* w, const float* wprep, const float* bias,
                          float* pool_y, unsigned char* code, float* ws, size_t ws_bytes, tg_stream_t stream);
int tg_maxpool2_bwd_code(const float* dout, const unsigned char* code, int B, int Ho, int Wo, int C, float* dx,
                         tg_stream_t stream);
/* Prediction-half tile maps of the frozen VGG trunk.  The trunk runs on [pred; target] stacked along the batch (2 nb images).
 * Where the receptive field of a 16x16 output tile of a layer holds no pixel whose 32-bit pattern differs between pred[b] and
 * target[b], the layer's output tile of image b equals that of image nb + b bit for bit (every kernel on the route computes a
 * pixel from its input patch and the weights alone, in a fixed order).  tg_vgg_sparse_map builds, in ONE launch and from the
 * data alone, for every conv of `plan` (a string of 'C' = 3x3 / stride-1 / pad-1 conv and 'M' = 2x2 / stride-2 max-pool, in the
 * trunk's order; x is the trunk's 1-channel input [2 nb][H][W]):
 *   bits   bit (b * tiles + t) of the word array: tile t (row-major over cdiv(Ho,16) x cdiv(Wo,16)) of prediction image b
 *          may differ from the target's;
 *   list   the set tiles as entries b * tiles + t, ascending; count = their number.  All three live on the device.
 * tg_vgg_sparse_map_bytes is the size of `buf` (0: the map cannot be built for this geometry -- run the trunk dense);
 * `ticket` is nb + 1 ints of device memory that are zero at the call and zero again behind the launch (the kernel's last
 * workgroups reset them).  maps[i] (out, one per 'C') point into `buf`.  tg_conv_fwd_sparse is tg_conv_fwd_p (pool_y == code == NULL),
 * tg_conv_fwd_pool (pool_y only) or tg_conv_fwd_pool_code (both; y unused) of the batch [pred; target]: with sp != NULL the
 * launcher computes only the prediction tiles `sp` marks and copies the target's results into the others -- wherever its
 * planner can honour the map (the fp32 F(2x2,3x3) pipelined kernel in one K split, static walk); any other route runs dense.
 * The results are the same bit for bit either way.
 *
 * The same maps serve the trunk's BACKWARD where the gradient at the trunk's input is read only at "needed" pixels.  With
 * mask != NULL ([nb][H][W]) tg_vgg_sparse_map marks a pixel where the patterns differ OR mask != 1 (the forward then computes those
 * tiles as well: still exact) and every map carries `pix`, those pixel bits ([nb][H][cdiv(W, 64)] 64-bit words, bit x % 64 of word
 * x / 64).  Only gradient positions whose feature depends on a needed pixel can reach one, so maps[i] -- the map of conv i's
 * OUTPUT -- is a superset of what is needed of conv i's input gradient, on the same tile grid:
 *   tg_conv_dgrad_sparse      tg_conv_dgrad_p (gate_bits == NULL) or tg_conv_dgrad_gbits (x_act == NULL) of a batch of sp->nb
 *                             images that writes only the tiles `sp` lists, wherever its planner can (the fp32 F(2x2,3x3)
 *                             pipelined kernel in one K split, static walk); any other route writes every tile.  Listed tiles
 *                             hold the dense call's values bit for bit provided dy is valid inside the map of the layer above;
 *                             other tiles may be left UNWRITTEN.  The caller must not ask for F(4x4,3x3) with a partly written
 *                             dy: there every output mixes the whole input patch.  Cin == 1 (the trunk's first conv; needs
 *                             sp->pix): EVERY pixel of dx is written -- the dense value where its pix bit is set, exactly 0.0f
 *                             elsewhere -- so nothing unwritten or non-finite upstream reaches a consumer of dx.
 *   tg_maxpool2_bwd_code_sparse  tg_maxpool2_bwd_code writing only the full-resolution tiles `sp` lists (the map of the pooled
 *                             conv); it reads dout only under those tiles. */
typedef struct TgSparseMap {
    const uint32_t* bits;
    const int32_t* list;
    const int32_t* count;
    const uint64_t* pix;        /* needed-pixel bits of the trunk's input (NULL: built without a mask) */
    int32_t nb, tiles_y, tiles_x, _pad;
} TgSparseMap;
size_t tg_vgg_sparse_map_bytes(int nb, int H, int W, const char* plan);
int tg_vgg_sparse_map(const float* x, const float* mask, int nb, int H, int W, const char* plan, void* buf, size_t buf_bytes,
                      int* ticket, TgSparseMap* maps, tg_stream_t stream);
int tg_conv_dgrad_sparse(const TgConv* g, const float* dy, const float* w, const float* wprep, const float* x_act, int act,
                         float slope, const uint32_t* gate_bits, float* dx, const TgSparseMap* sp, float* ws, size_t ws_bytes,
                         tg_stream_t stream);
/* 1: tg_conv_dgrad_sparse writes only the listed tiles for this geometry and gate (0 none, 1 x_act, 2 gate_bits); 0: every tile. */
int tg_conv_dgrad_sparse_planned(const TgConv* g, int gate, const TgSparseMap* sp);
int tg_maxpool2_bwd_code_sparse(const float* dout, const unsigned char* code, int B, int Ho, int Wo, int C, float* dx,
                                const TgSparseMap* sp, tg_stream_t stream);
int tg_conv_fwd_sparse(const TgConv* g, const float* x, const float* w, const float* wprep, const float* bias, int act,
                       float slope, float* y, float* pool_y, unsigned char* code, const TgSparseMap* sp, float* ws,
                       size_t ws_bytes, tg_stream_t stream);
/* BatchNorm + activation on load: the layer's input is act(BN(x)) -- x the PRE-BatchNorm output of the layer below, statistics
 * and affine parameters in `bn` -- and that tensor is never written.  For `final` (generator.py:29,56: Conv2d(64, 1, 3, 1, 1) over
 * dec1's ReLU(BN(.)) output, pconv.py:43-48): saves dec1's BatchNorm-apply pass (one read + one write of the widest activation).
 * Same rounding sequence as tg_bn_act_fwd, so results equal the two-call form bit for bit.  tg_conv_bnin_supported(g, wgrad)
 * says whether the geometry has the kernel (64 -> 1 channels, 3x3, stride 1, pad 1, W % 4 == 0, at least 4 x 16 pixels);
 * the two calls fail otherwise (the caller then materialises the activation with tg_bn_act_fwd). */
typedef struct TgBnAct {
    const float *mean, *rstd, *gamma, *beta;   /* [Cin] each */
    int32_t act;                               /* TG_ACT_* */
    float slope;
} TgBnAct;
int tg_conv_bnin_supported(const TgConv* g, int wgrad);
int tg_conv_fwd_bnin(const TgConv* g, const float* x, const TgBnAct* bn, const float* w, const float* bias, int act,
                     float slope, float* y, float* ws, size_t ws_bytes, tg_stream_t stream);
int tg_conv_wgrad_bnin(const TgConv* g, const float* x, const TgBnAct* bn, const float* dy, float* dw, float* db, float* ws,
                       size_t ws_bytes, tg_stream_t stream);
int tg_conv_dgrad_p(const TgConv* g, const float* dy, const float* w, const float* wprep, const float* in_mask,
                    const float* x_act, int act, float slope, float* dx, int accumulate, float* ws,
                    size_t ws_bytes, tg_stream_t stream);
/* ReLU gates in one bit per element, for backward passes that need only act'(x) of a ReLU output (the frozen VGG trunk under
 * activation checkpointing): a [rows][C] fp32 tensor -> bits [rows][C/32] uint32, bit c % 32 of word c / 32 = (a > 0) -- the
 * predicate of the fused fp32 gate (-0.0 and NaN give 0).  C % 32 == 0; pointers 16-byte aligned. */
int tg_relu_gate_pack(const float* a, int64_t rows, int C, uint32_t* bits, tg_stream_t stream);
/* tg_conv_dgrad_p gated by such bits (gate_bits [B][H][W][Cin/32], Cin % 32 == 0) in place of x_act / act / slope: the same
 * result bit for bit as the fp32 ReLU gate.  accumulate must be 0. */
int tg_conv_dgrad_gbits(const TgConv* g, const float* dy, const float* w, const float* wprep, const float* in_mask,
                        const uint32_t* gate_bits, float* dx, int accumulate, float* ws, size_t ws_bytes, tg_stream_t stream);

/* Leave `cus` of the 256 CUs free in the launches that otherwise occupy every CU with one long-running workgroup (the
 * Winograd kernels): data-parallel runs set this so that RCCL's kernels on the communication stream can be scheduled
 * while a convolution is running (0 = default, single-GPU). */
int tg_set_cu_reserve(int cus);
/* mode 1: the persistent Winograd launches with two or more work items per workgroup hand out the items behind each
 * workgroup's first one from per-XCD queues (one atomic per item) instead of walking a fixed list, so that a workgroup whose
 * CU is held by another stream's long-running kernel (RCCL's reductions in a data-parallel run) delays one item, not its
 * whole list (profiles/r03_ws_contention.txt: +90 % -> +8 % with 4-16 CUs held).  mode 2: every such launch (tests).
 * mode 0 (default, single GPU): static lists -- 1 % faster on an uncontended chip.  Results are bitwise equal in all modes. */
int tg_set_work_stealing(int mode);

/* dw[Cout][k][k][Cin] = sum_pixels dy (x) (x (.) in_mask);  db[Cout] = sum_pixels dy (db may be NULL).
 * Deterministic: split-K partial slabs in ws, reduced in a fixed order.  The query sizes the slabs, bias partials and column
 * sum from the launch's own parameters; a smaller ws is rejected (TG_ERR_ARG) before any launch. */
size_t tg_conv_wgrad_ws_bytes(const TgConv* g);
int tg_conv_wgrad(const TgConv* g, const float* x, const float* in_mask, const float* dy,
                  float* dw, float* db, float* ws, size_t ws_bytes, tg_stream_t stream);

/* w3 [Cout][k][k][Cin] -> w1 [Cout][k][k][1] = sum over Cin: the VGG first conv sees the grey
 * image repeated x3 (losses.py:79-80), i.e. a 1-channel conv with the channel-summed kernel. */
int tg_fold_cin(const float* w3, int cout, int taps, int cin, float* w1, tg_stream_t stream);

/* ---- mask path (exact integer arithmetic in fp32 storage) ---------------------------------- */

/* S = window sum of mask; mask_out = [S>0]; ratio = k*k/(S+1e-8)*[S>0]   (pconv.py:33-40). */
int tg_mask_update(const float* mask, int B, int H, int W, int k, int stride, int pad, int Ho,
                   int Wo, float* mask_out, float* ratio, tg_stream_t stream);
/* out = max(nearest_up2(up_mask) zero-padded to [H][W], skip_mask)  (generator.py:51-54,68-74). */
int tg_mask_up_merge(const float* up_mask, const float* skip_mask, int B, int h, int w, int H,
                     int W, float* out, tg_stream_t stream);

/* The whole mask pyramid of one generator forward (14 x tg_mask_update + 7 x tg_mask_up_merge, which depend on the input
 * mask only) as ONE launch: `op[i]` is applied to every image after op[i-1] (one workgroup per image walks the levels).
 * kind 0 = tg_mask_update(in[B][H][W]; k, stride, pad) -> out (mask) [B][Ho][Wo], out2 (ratio);
 * kind 1 = tg_mask_up_merge(in = up_mask [B][H][W], in2 = skip_mask [B][Ho][Wo]) -> out [B][Ho][Wo].
 * Results are bit-identical to the per-level entry points. */
#define TG_MASK_PYRAMID_MAX 24
typedef struct TgMaskOp {
    int kind, H, W, Ho, Wo, k, stride, pad;
    const float* in;
    const float* in2;
    float* out;
    float* out2;
} TgMaskOp;
typedef struct TgMaskPyramid {
    int nops, _pad;
    TgMaskOp op[TG_MASK_PYRAMID_MAX];
} TgMaskPyramid;
int tg_mask_pyramid(const TgMaskPyramid* pm, int B, tg_stream_t stream);

/* ---- BatchNorm (+ReLU / LeakyReLU) ---------------------------------------------------------- */

/* Training-mode batch statistics of y[rows][C] (biased var, eps inside rstd) and the running
 * update with `momentum` (unbiased var) -- nn.BatchNorm2d, pconv.py:21,47; discriminator.py:13.
 * running_* and num_batches_tracked (int64) may be NULL.  ws >= tg_bn_ws_bytes(rows, C). */
size_t tg_bn_ws_bytes(int64_t rows, int C);
int tg_bn_stats(const float* y, int64_t rows, int C, float eps, float momentum, float* save_mean,
                float* save_rstd, float* running_mean, float* running_var,
                int64_t* num_batches_tracked, float* ws, size_t ws_bytes, tg_stream_t stream);
/* tg_bn_stats followed (when out != NULL) by tg_bn_act_fwd as one call: one launch for small maps (few rows: the bottleneck
 * levels of the U-Net, where the separate launches are pure latency), the same kernels as the two calls otherwise.
 * ws as for tg_bn_stats. */
int tg_bn_fwd(const float* y, int64_t rows, int C, float eps, float momentum, const float* gamma,
              const float* beta, int act, float slope, float* save_mean, float* save_rstd,
              float* running_mean, float* running_var, int64_t* num_batches_tracked, float* out,
              float* ws, size_t ws_bytes, tg_stream_t stream);
/* eval mode: mean = running_mean, rstd = 1/sqrt(running_var + eps). */
int tg_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps,
                     float* mean, float* rstd, tg_stream_t stream);
/* out = act( (y-mean)*rstd*gamma + beta )   (pconv.py:47-48; discriminator.py:13-14). */
int tg_bn_act_fwd(const float* y, int64_t rows, int C, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, int act, float slope, float* out,
                  tg_stream_t stream);
/* Backward of bn_act_fwd in training mode.  dy = dBN(dout (.) act'(.)) [* ratio[row]], dgamma,
 * dbeta.  ratio may be NULL.  dy may alias dout.  dbias (may be NULL) receives sum_rows dy, i.e. the
 * gradient of the bias of the convolution feeding this BatchNorm, obtained in closed form from the
 * same reduction pass (no extra read of dy). */
int tg_bn_act_bwd(const float* dout, const float* y, int64_t rows, int C, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, int act, float slope,
                  const float* ratio, float* dy, float* dgamma, float* dbeta, float* dbias, float* ws,
                  size_t ws_bytes, tg_stream_t stream);
/* The same when the incoming gradient is the INPUT gradient of a C -> 1 channel 3x3 / stride-1 / pad-1 convolution (dec1's
 * BatchNorm under `final`, generator.py:29,56 + pconv.py:43-48):  dout[b][y][x][c] = sum_{ky,kx} dz[b][y+1-ky][x+1-kx] * w[ky][kx][c]
 * (w = that convolution's weight, [1][3][3][C]) is recomputed from the 1-channel dz inside both passes instead of being written by
 * tg_conv_dgrad and read twice.  dy [B][H][W][C] is written (nothing is consumed in place).  tg_bn_bwd_conv1_supported(rows, C):
 * C % 4 == 0 and more rows than the one-launch small-map form takes. */
int tg_bn_bwd_conv1_supported(int64_t rows, int C);
size_t tg_bn_conv1_ws_bytes(int64_t rows, int C);
int tg_bn_act_bwd_conv1(const float* dz, const float* w, int B, int H, int W, const float* y, int C, const float* mean,
                        const float* rstd, const float* gamma, const float* beta, int act, float slope, const float* ratio,
                        float* dy, float* dgamma, float* dbeta, float* dbias, float* ws, size_t ws_bytes, tg_stream_t stream);
/* din = dout * act'(out) [* ratio[row]] for a conv epilogue activation (out = post-activation).
 * din may alias dout. */
int tg_act_bwd(const float* dout, const float* out, int64_t rows, int C, int act, float slope,
               const float* ratio, float* din, tg_stream_t stream);

/* ---- decoder plumbing: bilinear x2 upsample (+) channel concat ------------------------------- */

/* out[B][H][W][Cu+Cs] = cat( pad(bilinear_up2(up[B][h][w][Cu])), skip[B][H][W][Cs] ) (.) out_mask
 * (generator.py:50,52,67,70,73; align_corners=False; skip may be NULL with Cs=0).  out_mask
 * [B][H][W] (NULL = 1) is the merged decoder mask: writing the concat already multiplied by it is the
 * `input * mask` of the consuming PConv2d (pconv.py:27), so that conv and its wgrad read it unmasked. */
int tg_upcat_fwd(const float* up, const float* skip, const float* out_mask, int B, int h, int w,
                 int Cu, int H, int W, int Cs, float* out, tg_stream_t stream);
/* The same with `up` = the PRE-BatchNorm output of the decoder layer below: the interpolation runs over act(BN(up)) formed on
 * load (TgBnAct: see tg_conv_fwd_bnin above), so that layer's activation -- read by nothing else
 * (generator.py:66-76 consumes it once, through F.interpolate) -- is never written.  Exact x2 geometries only
 * (H == 2h, W == 2w, Cu % 4 == 0, Cs % 4 == 0): tg_upcat_bn_supported; same bits as tg_bn_act_fwd + tg_upcat_fwd. */
int tg_upcat_bn_supported(int B, int h, int w, int Cu, int H, int W, int Cs);
int tg_upcat_fwd_bn(const float* up, const TgBnAct* bn, const float* skip, const float* out_mask, int B, int h, int w,
                    int Cu, int H, int W, int Cs, float* out, tg_stream_t stream);
/* adjoint: dup[B][h][w][Cu] = bilinear_up2^T(dout[..., :Cu]);  dskip = dout[..., Cu:]. */
int tg_upcat_bwd(const float* dout, int B, int h, int w, int Cu, int H, int W, int Cs, float* dup,
                 float* dskip, tg_stream_t stream);

/* ---- generator head --------------------------------------------------------------------------- */

/* out = sigmoid(logits)*(1-mask) + x*mask   (generator.py:57-62), n = B*H*W. */
int tg_sigmoid_composite_fwd(const float* logits, const float* x, const float* mask, int64_t n,
                             float* out, tg_stream_t stream);
/* dlogits = dout*(1-mask)*s*(1-s);  dx (may be NULL) = dout*mask. */
int tg_sigmoid_composite_bwd(const float* dout, const float* logits, const float* mask, int64_t n,
                             float* dlogits, float* dx, tg_stream_t stream);

/* ---- VGG trunk helpers (losses.py:31-34,79-90) ------------------------------------------------ */
int tg_maxpool2_fwd(const float* x, int B, int H, int W, int C, float* out, tg_stream_t stream);
/* relu_gate != 0: x is a ReLU output and its backward is fused (no gradient where the max is 0). */
int tg_maxpool2_bwd(const float* dout, const float* x, int B, int H, int W, int C, int relu_gate,
                    float* dx, tg_stream_t stream);

/* ---- losses ------------------------------------------------------------------------------------ */

/* Pixel-space part of InpaintingLoss.forward (losses.py:73,98-100,118-127,404-416) in one pass
 * family over (pred, target, mask) [B][H][W]:
 *   out[0] = L1 mean, out[1] = TV(pred*(1-mask)) (B divided twice, as the reference),
 *   out[2] = boundary loss (3x3 morphological-gradient band; 0 if the band is empty or the value
 *            is NaN/Inf), out[3] = sum(band), out[4] = l1 + w_tv*tv + w_bnd*boundary.
 * l1_weight (NULL = 1) weights |pred-target| inside the L1 mean: HumanGuidedLoss's human term
 * L1(pred*h, target*h) with h in {0,1} (losses.py:173-176).
 * If dpred != NULL also writes d out[4] / d pred * (*gscale) (gscale NULL = 1), accumulating into
 * dpred when accumulate != 0.  No host synchronisation.  ws >= tg_pixel_loss_ws_bytes(). */
size_t tg_pixel_loss_ws_bytes(int B, int H, int W);
int tg_pixel_losses(const float* pred, const float* target, const float* mask,
                    const float* l1_weight, int B, int H, int W,
                    float w_l1, float w_tv, float w_bnd, float bnd_eps, const float* gscale,
                    float* out5, float* dpred, int accumulate, float* ws, size_t ws_bytes,
                    tg_stream_t stream);

/* out[0] = mean |a-b| over n;  if da != NULL: da = coef * (*gscale) * sign(a-b)/n
 * (nn.L1Loss on VGG features, losses.py:86-89). */
size_t tg_reduce_ws_bytes(int64_t n);
int tg_l1_mean(const float* a, const float* b, int64_t n, float coef, const float* gscale,
               float* out1, float* da, float* ws, size_t ws_bytes, tg_stream_t stream);
/* The same with `a` a ReLU OUTPUT and the gradient taken in front of that ReLU: da = (a > 0) ? coef*g*sign(a-b)/n : 0 -- the
 * perceptual term's L1 over relu3_3 features (losses.py:86-89) and the backward of features[15] = ReLU(inplace) in one pass. */
int tg_l1_mean_relu(const float* a, const float* b, int64_t n, float coef, const float* gscale, float* out1, float* da,
                    float* ws, size_t ws_bytes, tg_stream_t stream);

/* nn.BCEWithLogitsLoss (mean) against the constant `target` (train.py:115,203,215-216):
 * out[0] = loss; if dz != NULL: dz = coef * (*gscale) * (sigmoid(z)-target)/n. */
int tg_bce_logits(const float* z, int64_t n, float target, float coef, const float* gscale,
                  float* out1, float* dz, float* ws, size_t ws_bytes, tg_stream_t stream);

/* ---- optimiser / misc ---------------------------------------------------------------------------- */

/* torch.optim.Adam defaults (main_pipeline.py:214-221; train.py:139-147): in-place update of
 * p, m (exp_avg), v (exp_avg_sq) from g*grad_scale with bias correction for `step` (1-based). */
/* lr/betas/eps are doubles: they are rounded to fp32 exactly where torch.optim.Adam rounds its Python floats. */
int tg_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
            double beta2, double eps, int step, float grad_scale, tg_stream_t stream);

/* Multi-tensor form: ONE launch over a device-resident table of segments (whole parameter tensors) and a
 * device-resident work list of int32 pairs (segment index, chunk index); chunk c of a segment covers elements
 * [c*chunk_elems, min(n, (c+1)*chunk_elems)).  All segments share lr/betas/eps/step.  chunk_elems must be a positive
 * multiple of 4 (a segment whose four pointers are 16-byte aligned is walked with 16-byte accesses from each chunk's first
 * element); any other value is refused.  Segments need no alignment: an unaligned one takes the scalar path. */
typedef struct TgAdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
} TgAdamSeg;
int tg_adam_multi(const TgAdamSeg* segs_dev, const int32_t* work_dev, int nwork, int chunk_elems,
                  double lr, double beta1, double beta2, double eps, int step, float grad_scale,
                  tg_stream_t stream);

/* The same launch with the two per-step scalars read from DEVICE memory -- scal_dev[0] = lr / (1 - beta1^step),
 * scal_dev[1] = sqrt(1 - beta2^step), exactly the two floats tg_adam_multi derives from (lr, betas, step) and which
 * tg_adam_scalars writes to HOST memory -- so that a train step captured in a hipGraph can be replayed: the host refreshes
 * the two floats (one small copy) before each replay, every other kernel argument of a step is step-invariant. */
int tg_adam_scalars(double lr, double beta1, double beta2, int step, float* out2_host);
/* dst_dev[0..n) = vals_host[0..n), n <= 16; the values travel as kernel arguments, so vals_host may be reused at once. */
int tg_write_floats(float* dst_dev, int n, const float* vals_host, tg_stream_t stream);
int tg_adam_multi_s(const TgAdamSeg* segs_dev, const int32_t* work_dev, int nwork, int chunk_elems,
                    double beta1, double beta2, double eps, const float* scal_dev, float grad_scale,
                    tg_stream_t stream);

/* y = a*x + b*y elementwise (gradient accumulation / scaling glue). */
int tg_axpby(const float* x, float a, float b, float* y, int64_t n, tg_stream_t stream);
/* out = a*x + b*y of two device scalars/vectors into a third (loss totals). */
int tg_lincomb(const float* x, float a, const float* y, float b, float* out, int64_t n,
               tg_stream_t stream);
/* out = a*b elementwise (masked_imgs = real_imgs * masks, train.py:181). */
int tg_mul(const float* a, const float* b, float* out, int64_t n, tg_stream_t stream);
/* out = a*b and a_copy = a from one read of a: masked_imgs (train.py:181) plus real_imgs placed behind the generated batch
 * in the stacked [gen; real] buffer the loss trunk (losses.py:79-88) and the discriminator passes (train.py:202,211) read. */
int tg_mul_keep(const float* a, const float* b, float* out, float* a_copy, int64_t n, tg_stream_t stream);
/* Re-apply the BatchNorm running-stat momentum update from saved batch statistics
 * (mean, rstd as written by tg_bn_stats): used when a forward pass is provably identical to one
 * already computed (D(gen) and D(gen.detach()), train.py:202,212) and only its running-stat side
 * effect remains to be reproduced. */
/* ---- BatchNorm over `groups` passes stacked along the rows: statistics PER PASS, one set of launches -------------------------
 * The train step stacks D(fake) and D(real) (train.py:202,211) into one forward / one backward; each pass keeps its own batch
 * statistics (discriminator.py:13: nn.BatchNorm2d in train mode, once per call).  y / out / dout / dy: [groups*rows_per_group][C],
 * mean / rstd: [groups][C].  Bit-identical to `groups` separate tg_bn_stats + tg_bn_act_fwd (resp. tg_bn_act_bwd) calls whose
 * parameter gradients are added in pass order.  C % 4 == 0.  No running-statistics side effect: tg_bn_running_update_multi. */
size_t tg_bn_grouped_ws_bytes(int64_t rows_per_group, int groups, int C);
int tg_bn_fwd_grouped(const float* y, int64_t rows_per_group, int groups, int C, float eps, const float* gamma,
                      const float* beta, int act, float slope, float* save_mean, float* save_rstd, float* out,
                      float* ws, size_t ws_bytes, tg_stream_t stream);
int tg_bn_act_bwd_grouped(const float* dout, const float* y, int64_t rows_per_group, int groups, int C,
                          const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                          float slope, float* dy, float* dgamma, float* dbeta, float* dbias, float* ws,
                          size_t ws_bytes, tg_stream_t stream);
/* tg_bn_running_update for passes order[0], order[1], ... (indices into mean / rstd [groups][C]) applied one after the other:
 * the reference updates model.N's buffers in the order D(fake), D(real), D(fake.detach()) (train.py:202,211,212). */
int tg_bn_running_update_multi(const float* save_mean, const float* save_rstd, int64_t rows_per_group, int C,
                               float eps, float momentum, const int* order, int norder, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, tg_stream_t stream);
int tg_bn_running_update(const float* save_mean, const float* save_rstd, int64_t rows, int C,
                         float eps, float momentum, float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, tg_stream_t stream);
/* [B][C][H][W] <-> [B][H][W][C] transposes (API boundary only; C==1 tensors need none). */
int tg_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float* y, tg_stream_t stream);
int tg_nhwc_to_nchw(const float* x, int B, int C, int H, int W, float* y, tg_stream_t stream);

/* ---- measurement hooks (bench.py roofline figures; no reference counterpart) ------------------- */

/* Quality metrics the reference logs per batch / validation pass, in ONE pass over [imgs][H][W] fp32 tensors
 * (imgs = B*C) with no host synchronisation:
 *   out[0] mse   out[1] psnr = 20 log10(1/sqrt(mse)) (inf when mse == 0)   out[2] ssim (11x11 avg_pool2d windows, zero
 *   padding, divisor 121, C1 = 0.01^2, C2 = 0.03^2)   out[3] l1   out[4] l2 = sqrt(mse)
 *     -- utils/experiment_tracking.py:176-231 (= MaskEvaluator._calculate_psnr/_ssim, evaluation/metrics.py:47-76)
 *   out[5] boundary_mse = mean over ALL elements of ((pred-target)*band)^2, band = clamp(maxpool3(m) - (1 - maxpool3(1-m)))
 *   out[6] boundary_psnr = 10 log10(1 / (boundary_mse + 1e-6))
 *   out[7] boundary_gradient_diff = | (mean|dy pred| + mean|dx pred|) - (mean|dy target| + mean|dx target|) |
 *   out[8] sum(band); out[5..7] are 0 when sum(band) < 1e-6
 *     -- calculate_boundary_quality, mvp_gan/src/evaluation/metrics.py:79-133
 * ws: 8-byte aligned, >= tg_quality_metrics_ws_bytes(). */
size_t tg_quality_metrics_ws_bytes(int64_t imgs, int H, int W);
int tg_quality_metrics(const float* pred, const float* target, const float* mask, int64_t imgs, int H, int W,
                       float* out9, float* ws, size_t ws_bytes, tg_stream_t stream);

/* Pre-decoded uint8 tile shards -> fp32 tiles on the device: img_f32 = img_u8 / 255 (IEEE fp32 division),
 * mask_f32 = mask_u8 > 0 -- mvp_gan/src/utils/dataset.py:35-37 (ToTensor scaling, binarise AFTER the resize).
 * Either input may be NULL.  n elements; pointers 16-byte aligned. */
int tg_u8_to_tiles(const uint8_t* img_u8, const uint8_t* mask_u8, int64_t n, float* img_f32, float* mask_f32,
                   tg_stream_t stream);

/* ---- whole-raster inpainting (mvp_gan/src/inpaint_raster.py; no reference counterpart: the reference quantises each source
 * grid to a uint8 512^2 PNG and never reassembles the tiles, utils/data_extraction.py:60-115, main_pipeline.py:497-530) ----
 * A float32 DSM [H][W] in metres is cut into overlapping windows of wh x ww.  Per axis the window starts are min(i*s, N-w),
 * i = 0..n-1, with s = w - overlap and n = ceil((N - w) / s) + 1; window index = iy * nx + ix.  A pixel is KNOWN when
 * mask != 0 (mask may be NULL), it is finite, and (use_nodata) it differs from nodata. */
typedef struct TgRasterPlan {
    int32_t H, W;           /* raster */
    int32_t wh, ww;         /* window sides, 1 <= wh <= H, 1 <= ww <= W */
    int32_t overlap;        /* 0 <= overlap < min(wh, ww) */
    int32_t ny, nx;         /* window grid; must equal the formula above */
} TgRasterPlan;

/* Per window: lo / hi = min / max over its known pixels (0 / 0 when it has none; a -0 extreme is stored as +0),
 * counts[2*win] = known pixels, counts[2*win+1] = holes.  lo, hi: [ny*nx]; counts: [ny*nx][2].  Deterministic. */
int tg_raster_window_stats(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                           float* lo, float* hi, int32_t* counts, tg_stream_t stream);
/* Network input of the windows win_idx[0..n) (device int32, 1 <= n <= 65535): x[j] = known ? (z - lo) / (hi - lo) : 0 (IEEE
 * fp32; 0 when hi == lo), m[j] = known; x, m: [n][wh][ww]. */
int tg_raster_gather(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                     const float* lo, const float* hi, const int32_t* win_idx, int n, float* x, float* m, tg_stream_t stream);
/* Composite raster out [H][W]: known pixels are copied bit for bit; a hole gets sum_j w_j * (lo_j + o_j * (hi_j - lo_j)) /
 * sum_j w_j over the covering windows j with run_of_window[j] = k >= 0 (their generator output o_j = wout[k], wout:
 * [n_run][wh][ww]), summed window row ascending, then column.  w = r_y * r_x, r(t) = min(1, (t+0.5)/overlap,
 * (w-t-0.5)/overlap) (1 when overlap == 0) with the ramp of a side on the raster border replaced by 1.  A hole no running
 * window covers is NaN and counted in *unfilled (device int32, zeroed by the call).  No float atomics: bitwise deterministic. */
int tg_raster_blend(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                    const float* lo, const float* hi, const int32_t* run_of_window, const float* wout, int n_run, float* out,
                    int32_t* unfilled, tg_stream_t stream);
/* Test-time augmentation (inpaint_raster(tta=...)).  A transform op in [0, 7] is tg_raster_sample's: member
 * pixel (i, j) reads window pixel (a, b) = op & 4 ? (j, i) : (i, j), then a = wh-1-a if op & 2, b = ww-1-b if op & 1.  Ops 4..7
 * transpose and are refused unless wh == ww, so a member frame is always [wh][ww].
 * tg_raster_gather with a transform per list item: item k (1 <= n <= 65535) is window win_idx[k] (device int32) under op_idx[k]
 * (HOST int32 [n], read and checked before any launch), written in the member's frame; x, m: [n][wh][ww].  Every value is the
 * one tg_raster_gather computes for the source pixel; with op 0 the result is bitwise tg_raster_gather's. */
int tg_raster_gather_ops(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                         const float* lo, const float* hi, const int32_t* win_idx, const int32_t* op_idx, int n, float* x, float* m,
                         tg_stream_t stream);
/* gout [n][T][wh][ww]: the generator outputs of n windows under ops[0..T) (HOST int32 [T]; T = 2, 4 or 8), each in its member
 * frame.  Per window pixel, in the window's frame, with o_t the member values there: mean = (o_0 + ... + o_{T-1}) * (1 / T) and
 * var = sum_t (o_t - mean)^2 / (T - 1), both added in member order in IEEE fp32 without contraction (a float32 mirror reproduces
 * them bit for bit).  mean, var: [n][wh][ww]. */
int tg_raster_tta_reduce(const float* gout, const int32_t* ops, int T, int n, int wh, int ww, float* mean, float* var,
                         tg_stream_t stream);
/* tg_raster_blend of the window means (out and *unfilled bitwise those of tg_raster_blend(..., wout = wmean)) plus the spread
 * in metres: with d_j = hi_j - lo_j and dn_j = fma(mean_j, d_j, lo_j) over the running covering windows j,
 * spread = sqrt(sum_j w_j (var_j d_j^2 + (dn_j - out)^2) / sum_j w_j): the law of total variance over the mixture of windows.
 * A known pixel gets 0, a hole no running window covers NaN.  wmean, wvar: [n_run][wh][ww].  Bitwise deterministic. */
int tg_raster_blend_tta(const float* dem, const float* mask, const TgRasterPlan* plan, int use_nodata, float nodata,
                        const float* lo, const float* hi, const int32_t* run_of_window, const float* wmean, const float* wvar,
                        int n_run, float* out, float* spread, int32_t* unfilled, tg_stream_t stream);

/* ---- training windows from a whole raster (mvp_gan/src/utils/raster_dataset.py; no reference counterpart: the reference
 * trains on uint8 PNG tiles min-max scaled over all pixels, utils/data_extraction.py:96-100) ----
 * Hole masks: window i (0 <= i < n) is the union of the primitives prims[offsets[i] .. offsets[i+1]) (at most 32 are read;
 * offsets [n+1] nondecreasing, in range of prims), each 8 int32, in the window's pixel coordinates (row, column):
 *   TG_HOLE_RECT    {0, cy, cx, a, b, u, v, 0}: with dy = i - cy, dx = j - cx, p = dx u + dy v, q = dy u - dx v,
 *                   L2 = u^2 + v^2, a hole when p^2 <= a^2 L2 and q^2 <= b^2 L2
 *   TG_HOLE_ELLIPSE {1, cy, cx, a, b, u, v, 0}: a hole when p^2 b^2 + q^2 a^2 <= a^2 b^2 L2
 *   TG_HOLE_STROKE  {2, y0, x0, y1, x1, r, 0, 0}: a hole when the point-to-segment distance is <= r (exact integer test)
 * Ranges for exactness (int64 throughout): coordinates in [-side, 2 side], 0 <= a, b, r <= 2 side, |u|, |v| <= 16.  A direction
 * (0, 0), an ellipse with a = 0 or b = 0 (its inequality would be a line or the whole plane) or an unknown kind covers nothing.  mask: [n][side][side], 1 = keep, 0 = hole.  Bit-exact. */
enum { TG_HOLE_RECT = 0, TG_HOLE_ELLIPSE = 1, TG_HOLE_STROKE = 2 };
int tg_hole_masks(const int32_t* prims, const int32_t* offsets, int n, int side, float* mask, tg_stream_t stream);
/* Windows cut from dem [H][W] (float32): draws int32 [n][3] = (y0, x0, op).  Output pixel (i, j) reads
 * dem[y0 + a][x0 + b] with (a, b) = op & 4 ? (j, i) : (i, j), then a = side-1-a if op & 2, b = side-1-b if op & 1.
 * lo / hi [n]: min / max of the window over the pixels with mask != 0 (norm_known) or over all pixels; a -0 extreme is stored
 * as +0; +inf / -inf when no pixel counts.  x [n][side][side] = (z - lo) / (hi - lo) at EVERY pixel, holes included (IEEE
 * fp32; with norm_known hole values may leave [0, 1]); 0 when hi == lo or no pixel counts.  A draw whose window leaves the
 * raster or whose op is outside [0, 7] gets NaN in its x, lo and hi.  Order-independent integer atomics: deterministic. */
int tg_raster_sample(const float* dem, int64_t H, int64_t W, const int32_t* draws, int n, int side, const float* mask,
                     int norm_known, float* x, float* lo, float* hi, tg_stream_t stream);

/* ---- above-ground objects from the DSM alone (mvp_gan/src/object_mask.py; no reference counterpart: the reference draws its
 * masks from aerial imagery with OpenCV heuristics, utils/mask_processing/core.py) ----
 * Progressive morphological filter, 8-connected components, area filter and buffer.  Rasters are
 * row-major [H][W] with 1 <= H, W and H * W < 2^31.  The morphology window of p with radius r is the square (2r+1)^2 centred on
 * p, clipped at the raster border; a radius past the raster is the whole raster.  Buffers come from the caller, no call
 * allocates or synchronises, and every result is bitwise deterministic (min / max, fp32 subtraction, integer atomics). */
enum { TG_MORPH_ERODE = 0, TG_MORPH_DILATE = 1 };
enum { TG_OBJMASK_MAX_BUFFER = 64 };
/* known [H][W] uint8 = mask != 0 (mask may be NULL), finite, and (use_nodata) != nodata; known_t [W][H] its transpose
 * (may be NULL). */
int tg_objmask_known(const float* dem, const float* mask, int H, int W, int use_nodata, float nodata, uint8_t* known,
                     uint8_t* known_t, tg_stream_t stream);
/* out [H][W] = min (op TG_MORPH_ERODE) / max (TG_MORPH_DILATE) of in over the pixels q of the window of p with known[q] != 0
 * (known may be NULL: every pixel counts); +inf / -inf where the window has none.  radius >= 0; tmp: [H*W] floats;
 * in, tmp and out distinct. */
int tg_objmask_morph(const float* in, const uint8_t* known, int H, int W, int radius, int op, float* tmp, float* out,
                     tg_stream_t stream);
/* One filter step: s_out = dilate_r(erode_r(s_in)), the erosion reading s_in and the dilation reading the eroded values at
 * known pixels only (known [H][W], known_t [W][H] from tg_objmask_known); s_out has a value at every pixel.  flags [H][W]
 * uint8 is set to 1 where known and s_in - s_out > dh in fp32 (dh finite, >= 0), and left alone elsewhere.  t0, t1: [H*W]
 * floats; s_in, t0, t1, s_out distinct. */
int tg_objmask_pmf_step(const float* s_in, const uint8_t* known, const uint8_t* known_t, int H, int W, int radius, float dh,
                        float* t0, float* t1, float* s_out, uint8_t* flags, tg_stream_t stream);
/* 8-connected components of flags != 0: labels [H][W] int32 = the smallest linear index y*W + x in the pixel's component,
 * -1 where not flagged; area [H*W] int32 = the component's pixel count at that index, 0 elsewhere. */
int tg_objmask_components(const uint8_t* flags, int H, int W, int32_t* labels, int32_t* area, tg_stream_t stream);
/* Components with area >= min_area are objects; objects [H][W] uint8 = 1 within the clipped square of radius buffer_px
 * (0 .. TG_OBJMASK_MAX_BUFFER) of an object pixel; keep [H][W] float = known && !objects.  counts [4] int32 (zeroed by the
 * call): flagged pixels, components kept, components removed, object pixels. */
int tg_objmask_filter(const uint8_t* known, const int32_t* labels, const int32_t* area, int H, int W, int min_area,
                      int buffer_px, uint8_t* objects, float* keep, int32_t* counts, tg_stream_t stream);

/* ---- held-out terrain errors of an inpainted raster (mvp_gan/src/evaluate_raster.py; no reference
 * counterpart: the reference scores 8-bit tiles only) ----
 * Rasters are row-major [H][W] with 1 <= H, W and H * W < 2^31.  valid: mask != 0 (mask may be NULL), finite, and
 * (use_nodata) != nodata.  No call allocates or synchronises; every result is bitwise deterministic (integer atomics only,
 * fp64 sums from per-workgroup partials reduced in a fixed order). */
/* Evaluation holes of raster rows [row0, row1) (row0 a multiple of tile, row1 <= H): pixel (y, x) lies in cell
 * (y / tile, x / tile) of a grid of ncy x ncx = ceil(H / tile) x ceil(W / tile) cells; k = cell_of[cy][cx] >= 0 names its
 * hole mask cell_masks[k][tile][tile] (float, 0 = hole, as tg_hole_masks writes it) read at (y % tile, x % tile); -1 = no
 * hole.  hole_in [H][W] uint8 (may be NULL) adds the pixels where it is nonzero.  objects [H][W] uint8 may be NULL.
 * holes [H][W] uint8 = valid && hole && !objects; keep [H][W] float = valid && !hole && !objects.  counts [3] int64 are
 * ADDED to (the caller zeroes them): valid pixels, holes, valid object pixels. */
int tg_eval_holes(const float* dem, const float* mask, int use_nodata, float nodata, const uint8_t* objects,
                  const float* cell_masks, const int32_t* cell_of, const uint8_t* hole_in, int H, int W, int tile, int row0,
                  int row1, uint8_t* holes, float* keep, int64_t* counts, tg_stream_t stream);
/* Per-hole table: every root i of labels (labels[i] == i, from tg_objmask_components on the holes) gets a row
 * s = slot[i] (atomic counter order: the caller sorts by label) of table [cap][TG_HOLE_COLS] int64 =
 * {label, area, scored 0, fixed-point sum 0, max bits 0, y0, x0, y1, x1}, the bbox set to the root pixel; tg_terrain_errors
 * adds the rest.  slot [H*W] int32 is written at the roots only and may alias area.  count [1] int32 (zeroed by the call) =
 * the number of roots; rows past cap are not written. */
enum { TG_HOLE_COLS = 9 };
int tg_hole_table(const int32_t* labels, const int32_t* area, int H, int W, int32_t* slot, int64_t* table, int cap,
                  int32_t* count, tg_stream_t stream);
/* Area classes of tg_terrain_errors: a hole of area A px is in class c = #{e < n_edges : A >= px[e]} (px nondecreasing). */
enum { TG_EVAL_MAX_CLASSES = 8 };
typedef struct {
    int32_t n_edges, _pad;
    int64_t px[TG_EVAL_MAX_CLASSES - 1];
} TgAreaClasses;
/* fp64 sums (tg_terrain_errors_finish), e = p - z (fp32), a = |e|; S = hole && finite(p); T = S pixels whose 3x3 neighbourhood
 * lies inside the raster, is valid and has finite p; R = S pixels with an 8-neighbour in keep; dg2 = |grad p - grad z|^2 (Horn,
 * fp64), ds = slope_p - slope_z in degrees, dl = laplacian_p - laplacian_z: */
enum {
    TG_TE_S_E = 0, TG_TE_S_A, TG_TE_S_A2, TG_TE_T_DS, TG_TE_T_DS2, TG_TE_T_DG2, TG_TE_T_DL2, TG_TE_R_A, TG_TE_R_A2,
    TG_TE_RT_DG2, TG_TE_CLASS /* + 2c: sum a, + 2c + 1: sum a^2 over S pixels of class c */,
    TG_TE_NSUM = TG_TE_CLASS + 2 * TG_EVAL_MAX_CLASSES
};
/* int64 counters (zeroed by tg_terrain_errors): */
enum {
    TG_TE_N_VALID = 0, TG_TE_N_HOLES, TG_TE_N_OBJECTS, TG_TE_N_SCORED, TG_TE_N_UNFILLED, TG_TE_N_RING, TG_TE_N_SLOPE,
    TG_TE_N_RING_SLOPE, TG_TE_N_CLAMPED, TG_TE_MAX_BITS, TG_TE_NCOUNT
};
size_t tg_terrain_errors_ws_bytes(int H, int W);
/* z, p [H][W] float; holes [H][W] uint8 (nonzero = evaluation hole); keep [H][W] float (nonzero = known to the model); labels,
 * slot, table, nholes from tg_objmask_components + tg_hole_table (nholes <= cap rows).  Per hole (integer atomics at
 * row slot[labels[i]]): scored += 1, sum += rint(min(a, 2^15) * 2^16), max bits, bbox over all its pixels.  counts
 * [TG_TE_NCOUNT] int64; sel_a [H*W] = a on S, NaN elsewhere; sel_slope [H*W] = (float)|ds| on T, NaN elsewhere;
 * ws >= tg_terrain_errors_ws_bytes: per-workgroup partials for tg_terrain_errors_finish. */
int tg_terrain_errors(const float* z, const float* p, const float* mask, int use_nodata, float nodata, const uint8_t* holes,
                      const float* keep, const int32_t* labels, const int32_t* slot, int64_t* table, int nholes, int H, int W,
                      double cellsize, const TgAreaClasses* classes, int64_t* counts, float* sel_a, float* sel_slope,
                      void* ws, size_t ws_bytes, tg_stream_t stream);
/* sums [TG_TE_NSUM] double = the partials of the last tg_terrain_errors call of this shape on ws, reduced in a fixed order. */
int tg_terrain_errors_finish(int H, int W, const void* ws, size_t ws_bytes, double* sums, tg_stream_t stream);
/* out[j] = the ks[j]-th smallest (0-based) of the values v[0 .. n) whose bits are <= 0x7f800000 (neither NaN nor negative,
 * -0 included); NaN when ks[j] is out of range.  Exact (radix select on the bits: 11 + 11 + 10), so bitwise equal to
 * np.sort(v[v >= +0 bits])[k].  ks [nk] int64 device, 1 <= nk <= TG_SELECT_MAX_K, n < 2^31; ws >= tg_select_f32_ws_bytes. */
enum { TG_SELECT_MAX_K = 8 };
size_t tg_select_f32_ws_bytes(int64_t n, int nk);
int tg_select_f32(const float* v, int64_t n, const int64_t* ks, int nk, float* out, void* ws, size_t ws_bytes,
                  tg_stream_t stream);

/* ---- harmonic void fill of a DSM (mvp_gan/src/fill_voids.py; no reference counterpart) ----
 * Rasters are row-major [H][W] with 1 <= H, W and H * W < 2^31.  Known K: mask != 0 (mask may be NULL), finite, and
 * (use_nodata) != nodata; every other pixel is unknown and solves sum_{q in N4(p) inside the raster} (u_q - u_p) = 0 with
 * u = z on K.  Masked multigrid: levels halve with ceil until the longer side is at most 16 (tg_vfill_levels); a coarse
 * cell is fixed when any of its children is.  ws: 256-byte aligned, >= tg_vfill_ws_bytes(H, W), kept between the calls of
 * one fill.  No call allocates or synchronises; results are bitwise deterministic (integer atomics only). */
enum { TG_VFILL_MAX_LEVELS = 32 };
/* stats [TG_VFILL_NSTATS] int64 written by tg_vfill_setup: known and unknown pixels, the float bits of min and max z over K
 * (0 when K is empty). */
enum { TG_VFILL_KNOWN = 0, TG_VFILL_UNKNOWN, TG_VFILL_MIN_BITS, TG_VFILL_MAX_BITS, TG_VFILL_NSTATS };
size_t tg_vfill_ws_bytes(int H, int W);
int tg_vfill_levels(int H, int W);
/* Known map, statistics, offset c = (min + max) / 2, initial guess (z - c on K, 0 elsewhere), coarse fixed flags and the
 * per-level lists of 32 x 64 tiles that hold an unknown cell. */
int tg_vfill_setup(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, void* ws, size_t ws_bytes,
                   int64_t* stats, tg_stream_t stream);
/* One V-cycle over all levels; change_bits [1] (device, zeroed by the call) = float bits of the largest |change| of u over
 * the unknown pixels during the cycle. */
int tg_vfill_cycle(int H, int W, void* ws, size_t ws_bytes, uint32_t* change_bits, tg_stream_t stream);
/* out [H][W] = dem at known pixels (bit for bit), the solution at the unknowns; NaN everywhere when K is empty. */
int tg_vfill_finish(const float* dem, int H, int W, const void* ws, size_t ws_bytes, float* out, tg_stream_t stream);
/* Conjugate gradients preconditioned by the V-cycle (fill_voids(solver="pcg")): for the large and the
 * tile-aligned voids on which the plain cycle stalls.  pws: a second workspace, 256-byte aligned, >= tg_vfill_pcg_ws_bytes(H, W)
 * (0 for the sizes tg_vfill_ws_bytes rejects), kept between the calls of one fill; the layout of ws is unchanged.
 * tg_vfill_pcg_start runs once after tg_vfill_setup (residual, z = M r, first direction); each tg_vfill_pcg_iter is one
 * iteration = one V-cycle and stands in for tg_vfill_cycle: change_bits [1] (device, zeroed by the call) = float bits of the
 * largest |alpha p| over the unknown pixels (+inf when the step was skipped and the direction restarted from p = z),
 * restarts [1] (device) = directions restarted so far.  The solution ends every iteration in the buffer tg_vfill_finish reads.
 * Dot products are fp64 sums of per-tile partials in tile order: results are bitwise deterministic. */
size_t tg_vfill_pcg_ws_bytes(int H, int W);
int tg_vfill_pcg_start(int H, int W, void* ws, size_t ws_bytes, void* pws, size_t pws_bytes, tg_stream_t stream);
int tg_vfill_pcg_iter(int H, int W, void* ws, size_t ws_bytes, void* pws, size_t pws_bytes, uint32_t* change_bits,
                      uint32_t* restarts, tg_stream_t stream);
/* Biharmonic (thin-plate) fill (fill_voids(method="biharmonic")): the unknowns minimise the sum of
 * D(u)^2 over themselves and their 4-neighbours, D the masked difference sum above; the normal equations D(D(u)) = 0 at the
 * unknowns are solved by flexible conjugate gradients (x, residual and dots fp64) preconditioned by G(G(r)), G being `inner`
 * (1..TG_VFILL_BIH_MAX_INNER) conjugate-gradient iterations around the V-cycle (1: one bare cycle).  bws: a third workspace,
 * 256-byte aligned, >= tg_vfill_bih_ws_bytes(H, W) (0 for the sizes tg_vfill_ws_bytes rejects), kept between the calls of one
 * fill; the layouts of ws and pws are unchanged and pws is not needed.  tg_vfill_bih_start runs once after tg_vfill_setup;
 * each tg_vfill_bih_iter is one outer iteration = 2 * inner V-cycles, with the same `inner` as the start.  change_bits and
 * restarts as for tg_vfill_pcg_iter (restarts counts the inner solves' too); the solution ends every iteration, in fp32, in
 * the buffer tg_vfill_finish reads.  Bitwise deterministic. */
enum { TG_VFILL_BIH_MAX_INNER = 8 };
size_t tg_vfill_bih_ws_bytes(int H, int W);
int tg_vfill_bih_start(int H, int W, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, int inner, tg_stream_t stream);
int tg_vfill_bih_iter(int H, int W, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, int inner, uint32_t* change_bits,
                      uint32_t* restarts, tg_stream_t stream);

/* ---- seam correction of a filled DSM by a harmonic delta surface (mvp_gan/src/seam_correct.py; no
 * reference counterpart) ----
 * Rasters are row-major [H][W] with 1 <= H, W and H * W < 2^31.  Known K as above (mask may be NULL).  A hole pixel is filled
 * when `filled` is finite there; `filled` at known pixels is never read.  Ring I: filled holes with a known 4-neighbour inside
 * the raster; interior U': the other filled holes.  No call allocates or synchronises; integer atomics only. */
enum { TG_SEAM_RING = 0, TG_SEAM_INTERIOR, TG_SEAM_UNFILLED, TG_SEAM_MAX_BITS, TG_SEAM_NCOUNTS };
/* delta [H][W]: on I the ring target minus the fill, d_p = (sum_dir (e_dir - g_p)) / n over the directions up, left, right,
 * down whose neighbour q is known, summed in that order in fp32, with e_dir = fma(2, z_q, -z_q2) when order == 1 and
 * q2 = p + 2 dir is inside and known, else z_q; 0 on K and on unfilled holes; NaN on U'.  counts [TG_SEAM_NCOUNTS] (device
 * int32, zeroed by the call): pixels of I, of U', unfilled holes, and the float bits of max |d_p|. */
int tg_seam_delta(const float* dem, const float* mask, int use_nodata, float nodata, const float* filled, int H, int W, int order,
                  float* delta, int32_t* counts, tg_stream_t stream);
/* out [H][W] = dem at known pixels (bit for bit), filled + delta_filled (one fp32 add) at filled holes, NaN at unfilled holes. */
int tg_seam_apply(const float* dem, const float* mask, int use_nodata, float nodata, const float* filled,
                  const float* delta_filled, int H, int W, float* out, tg_stream_t stream);

/* ---- raster resampling between cell sizes (mvp_gan/src/resample.py; no reference counterpart) ----
 * The scale p / q is the output cell size over the source cell size.  Per axis, in units of 1/q source pixel: source pixel i
 * covers [i q, (i+1) q), output pixel I covers [I p, (I+1) p) clipped to [0, N q), and No = ceil(N q / p); Ho and Wo are
 * those sizes, or smaller ones for the top-left crop of that grid.  1 <= p, q <= 1024, N q + 2 p < 2^30 per axis.  Known K as
 * above (mask may be NULL).  out [Ho][Wo] (may be NULL) gets the value, NaN where the output pixel is unknown; out_mask
 * [Ho][Wo] (may be NULL) 1 / 0; n_nan [1] (device int32, zeroed by the call) the number of unknown output pixels, the NaN
 * pixels of out; with out and out_mask NULL the call only counts (at p = q = 1: the unknown pixels of dem).  keep_dem / keep_mask [Ho][Wo] (may be NULL): where that pixel is known
 * under (keep_mask, keep_use_nodata, keep_nodata), out gets its bits and out_mask 1.  No workspace, no allocation, no
 * synchronisation; bitwise deterministic (one integer atomic per workgroup). */
/* To a coarser grid, 1 <= p / q <= 16.  The weight of source pixel (i, j) in output pixel (I, J) is the integer overlap of their
 * intervals along y times that along x.  The output is known iff cov_known > 0 and cov_known * cov_den >= cov_num * cov_total
 * (int64), the weight sums over the known taps and over all taps of the clipped footprint; 0 <= cov_num <= cov_den <= 1000.
 * Its value is z0 + (sum w (z - z0)) / cov_known in fp32 over the known taps in row-major order, z0 the first of them (z0
 * itself when the sum is 0: a footprint of one repeated value returns its bits). */
int tg_resample_area(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, int p, int q, int cov_num,
                     int cov_den, const float* keep_dem, const float* keep_mask, int keep_use_nodata, float keep_nodata, int Ho,
                     int Wo, float* out, float* out_mask, int32_t* n_nan, tg_stream_t stream);
/* To a finer grid, 1/16 <= p / q <= 1 (the return trip of every area scale).  The centre of output pixel I lies at source
 * coordinate ((2 I + 1) p - q) / (2 q) = f + t, f its integer floor; tap indices are clamped to the raster.  The output is known iff the source pixel containing the centre
 * (f when t < 1/2, else f + 1, clamped) is known; that pixel's value zc is the pivot.  Value: zc + sum w (z - zc) with the
 * Catmull-Rom (Keys a = -0.5) weights of taps f - 1 .. f + 2 when all 16 are known, else the bilinear weights of taps f, f + 1
 * renormalised over the known ones (zc itself when the sum is 0). */
int tg_resample_interp(const float* dem, const float* mask, int use_nodata, float nodata, int H, int W, int p, int q,
                       const float* keep_dem, const float* keep_mask, int keep_use_nodata, float keep_nodata, int Ho, int Wo,
                       float* out, float* out_mask, int32_t* n_nan, tg_stream_t stream);

/* ---- Distance to the nearest known pixel; terrain errors by depth (csrc/edt.hip) ---------------- */
/* Exact Euclidean distance transform.  2 * 32767^2 < 2^31: an int32 holds every squared distance of an admitted raster. */
enum { TG_EDT_FAR = 0x7fffffff, TG_EDT_MAX_SIDE = 32767 };
size_t tg_edt_ws_bytes(int H, int W);
/* seed [H][W] uint8, nonzero = distance 0.  d2 [H][W] int32 = min(exact squared Euclidean distance in pixels to the
 * nearest seed, cap2); cap2 <= 0: no cap, TG_EDT_FAR where the raster has no seed at all.  dist_m (may be NULL) [H][W] float
 * = (float)(cellsize * sqrt((double)d2)), +inf at TG_EDT_FAR; cellsize is read only with dist_m.  Integer arithmetic up to
 * dist_m: bit-exact and deterministic.  ws >= tg_edt_ws_bytes (the band words, the carried rows and the uint16 column
 * distances); 0 from the query and TG_ERR_ARG from the call for a side outside [1, TG_EDT_MAX_SIDE]. */
int tg_edt(const uint8_t* seed, int H, int W, int32_t cap2, double cellsize, int32_t* d2, float* dist_m,
           void* ws, size_t ws_bytes, tg_stream_t stream);
/* Depth classes of tg_depth_errors: a pixel of squared distance D is in class c = #{e < n_edges : D >= d2[e]}. */
enum { TG_DEPTH_MAX_CLASSES = 8 };
typedef struct { int32_t n_edges, _pad; int32_t d2[TG_DEPTH_MAX_CLASSES - 1]; } TgDepthClasses;   /* nondecreasing */
size_t tg_depth_errors_ws_bytes(int H, int W);
/* a [H*W]: |error| on the scored pixels, NaN elsewhere (tg_terrain_errors' sel_a, read only).  Pixel i with a[i] not NaN is in
 * class c = #{e < n_edges : d2[i] >= cls->d2[e]}.  counts [TG_DEPTH_MAX_CLASSES] int64 (zeroed here), max_bits
 * [TG_DEPTH_MAX_CLASSES] uint32 (zeroed here) = largest a per class as float bits; hole_d2 [nholes] int32 (zeroed here) = max
 * d2 over ALL pixels of the hole (labels >= 0), at row slot[labels[i]].  Per-workgroup fp64 partials of sum a and sum a*a per
 * class go to ws (>= tg_depth_errors_ws_bytes); the grid is a function of the shape. */
int tg_depth_errors(const float* a, const int32_t* d2, const int32_t* labels, const int32_t* slot, int nholes, int H, int W,
                    const TgDepthClasses* cls, int64_t* counts, uint32_t* max_bits, int32_t* hole_d2,
                    void* ws, size_t ws_bytes, tg_stream_t stream);
/* sums [2 * TG_DEPTH_MAX_CLASSES] double: sums[2c] = sum a, sums[2c + 1] = sum a*a over class c, from the partials of the last
 * tg_depth_errors call of this shape on ws, reduced in a fixed order. */
int tg_depth_errors_finish(int H, int W, const void* ws, size_t ws_bytes, double* sums /* [2*TG_DEPTH_MAX_CLASSES] */,
                           tg_stream_t stream);

/* ---- Feature transform; directional IDW and nearest-neighbour void fills (csrc/edt.hip, csrc/idw.hip) ------ */
size_t tg_edt_nearest_ws_bytes(int H, int W);
/* The feature transform of tg_edt: d2 [H][W] int32 is bit for bit what tg_edt writes for the same seed and cap2; idx [H][W]
 * int32 = y * W + x of the nearest seed, -1 where d2 is TG_EDT_FAR or, with a cap, d2 >= cap2.  Tie rule (part of the
 * interface): among the seeds at the smallest squared distance the smallest row, among those the smallest column.  Integer
 * arithmetic only, no data-dependent order.  Sides, rejections and workspace (>= tg_edt_nearest_ws_bytes) as tg_edt. */
int tg_edt_nearest(const uint8_t* seed, int H, int W, int32_t cap2, int32_t* d2, int32_t* idx, void* ws, size_t ws_bytes,
                   tg_stream_t stream);
size_t tg_rayfill_ws_bytes(int H, int W);
/* Eight-direction inverse-distance fill.  Directions in this order: N, NE, E, SE, S, SW, W, NW, (dy, dx) = (-1,0), (-1,1),
 * (0,1), (1,1), (1,0), (1,-1), (0,-1), (-1,-1); s_j = 1 on the axes, 2 on the diagonals.  For an unknown pixel p (known[p] == 0)
 * k_j is the smallest k >= 1 with p + k d_j inside the raster and known; no hit when the ray leaves the raster first or
 * k_j^2 s_j > lim2 (lim2 <= 0: no limit).  out[p] = (float)((sum_j w_j z[p + k_j d_j]) / (sum_j w_j)) over the hits in that
 * order, both sums in fp64 from 0.0 without multiply-add contraction, one fp64 division, one rounding to fp32;
 * w_j = 1.0 / (double)(k_j^2 s_j) for power == 2, 1.0 / sqrt((double)(k_j^2 s_j)) for power == 1 (every operation correctly
 * rounded), pow((double)(k_j^2 s_j), -power / 2) for any other power in (0, 8].  Known pixels are copied bit for bit.  An
 * unknown pixel without a hit takes z[idx[p]] when d2 and idx (tg_edt_nearest's; both or neither) are given, idx[p] >= 0 and
 * 0 <= d2[p] <= lim2 (no distance condition without a limit); else NaN.  hits (may be NULL) [8][H][W] uint16: k_j, 0 = no
 * hit, 0 on known pixels.  counts [3] int64 (zeroed here): unknown pixels filled by rays, by the nearest pixel, left NaN.
 * ws >= tg_rayfill_ws_bytes: per family of lines (columns, rows, both diagonals) a 64-bit word and two int32 carried
 * positions per 64 pixels of a line.  out must not alias z.  Sides in [1, TG_EDT_MAX_SIDE]. */
int tg_rayfill(const float* z, const uint8_t* known, int H, int W, int32_t lim2, double power, const int32_t* d2,
               const int32_t* idx, float* out, uint16_t* hits, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream);
/* out[p] = known[p] ? z[p] : (idx[p] >= 0 ? z[idx[p]] : NaN); counts [2] int64 (zeroed here): filled, left NaN. */
int tg_gather_fill(const float* z, const uint8_t* known, const int32_t* idx, int H, int W, float* out, int64_t* counts,
                   tg_stream_t stream);
/* One Jacobi step of a 3x3 mean on the filled pixels: an unknown, non-NaN pixel becomes the fp64 sum, in row-major order, of
 * the non-NaN pixels of its 3x3 neighbourhood (itself included, clipped at the raster edge) divided by their count and
 * rounded to fp32 once; known and NaN pixels are copied.  in and out are distinct. */
int tg_void_smooth(const float* in, const uint8_t* known, int H, int W, float* out, tg_stream_t stream);

/* ---- Natural-neighbour (discrete Sibson) void fill (csrc/natural.hip) ------------------------------------------
 * Sites are the known pixels (known[q] != 0, tg_objmask_known's map).  d2 [H][W] int32: the UNCAPPED feature transform of the
 * known map (tg_edt_nearest with cap2 = 0; its tie rule is part of this definition); nn [H][W] float: the nearest fill
 * tg_gather_fill writes from it, nn(q) = known(q) ? z(q) : z[idx(q)], NaN where idx(q) < 0.  radius r in [1, 32];
 * c(q) = min(d2(q), r^2).  For a void pixel p (known[p] == 0) the raster pixel q contributes iff |p - q|^2 < c(q), in integers,
 * strictly: a known q (c = 0) never does, q = p always does, and every contributor lies within r - 1 pixels of p on each axis.
 * out[p] = (float)(sum nn(q) / n(p)): the sum over the contributors in row-major order of q (row, then column, ascending) in
 * fp64 from 0.0, n(p) their number, one fp64 division, one rounding to fp32.  No atomics on the sums, no data-dependent order:
 * two calls agree bit for bit.  support (may be NULL) [H][W] int32 = n(p), 0 on known pixels: the discrete area of the Voronoi
 * cell p would claim.  Known pixels: out[p] = nn[p] bit for bit.  A void pixel with d2[p] == TG_EDT_FAR (no known pixel at
 * all) is NaN; with lim2 > 0 a void pixel with d2[p] > lim2 is NaN too, while q beyond the limit still contribute to the
 * pixels within it (the limit masks the output only).  counts [2] int64 (zeroed here): void pixels filled, left NaN.  With
 * r = 1 out is nn on the void pixels; a constant nn comes back constant.
 * ws >= tg_natural_fill_ws_bytes(H, W): one uint16 per 4 x 64 tile, the tile's largest c (tg_natural_tile_maxima writes the same
 * words and nothing else; tg_natural_fill does not need it called first).  Rejected on the host: null pointers, sides outside
 * [1, TG_EDT_MAX_SIDE] (0 from the query), radius outside [1, 32], a short workspace, out aliasing nn. */
size_t tg_natural_fill_ws_bytes(int H, int W);
int tg_natural_tile_maxima(const int32_t* d2, int H, int W, int radius, void* ws, size_t ws_bytes, tg_stream_t stream);
int tg_natural_fill(const float* nn, const int32_t* d2, const uint8_t* known, int H, int W, int radius, int32_t lim2, float* out,
                    int32_t* support /* may be NULL */, int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream);

/* ---- Depression filling (pit removal) (csrc/depfill.hip) ------------------------------------------------------
 * Known pixels: known[p] != 0 (tg_objmask_known's map).  Connectivity conn = 8 or 4.  An outlet is a known pixel on the raster's
 * edge or with an unknown conn-neighbour.  For a known pixel p, W(p) = min over conn-connected paths of known pixels from p to
 * an outlet of the max of z along the path: exact (comparisons, fminf and fmaxf only), independent of the order of the sweeps.
 * Sides as tg_objmask_known (H, W >= 1, H * W < 2^31).  One workspace ws >= tg_depfill_ws_bytes(H, W) serves all calls: 256
 * control bytes, two dirty planes of one byte per 64x64 tile (each rounded up to 256 bytes), then 40 bytes per workgroup of the
 * statistics, min(1024, ceil(H * W / 4096)) of them (rounded up to 256 bytes).  0 for sides out of range. */
size_t tg_depfill_ws_bytes(int H, int W);
/* w [H][W] = z at outlets, +inf at the other known pixels, NaN at unknown ones; every tile of ws is marked dirty. */
int tg_depfill_init(const float* z, const uint8_t* known, int H, int W, int conn, float* w, void* ws, size_t ws_bytes,
                    tg_stream_t stream);
/* Enqueues n sweeps, 1 <= n <= 2^20, of w (after tg_depfill_init on the same z, known, conn, w and ws): every dirty tile is relaxed,
 * W(p) <- max(z(p), min(W(p), min over the neighbours W)), to a fixed point against its one-pixel halo (or to a cap on the inner
 * rounds; it stays dirty then); a tile is dirty in a sweep when it changed in the one before or a neighbour tile lowered a
 * value on its rim.  changed [1] int32 (zeroed here): the workgroup visits of the LAST of the n sweeps that lowered a value; 0
 * means w is the answer.  visits [1] int64 is added to (the caller zeroes it): tiles visited.  Every value of w is at all times
 * an upper bound of the answer and the bits of some known z, or +inf (not reached yet).  The raster at the fixed point does not
 * depend on the order of the visits; the number of sweeps to it may. */
int tg_depfill_sweep(const float* z, const uint8_t* known, int H, int W, int conn, int n, float* w, int32_t* changed,
                     int64_t* visits, void* ws, size_t ws_bytes, tg_stream_t stream);
/* Over the known pixels, with sel (uint8 [H][W], may be NULL) only those with sel != 0: counts [3] int64 = pixels with w > z,
 * pixels with w == +inf (among the former), pixels counted; sums [2] double = the sum of (double)w - (double)z over the pixels
 * with z < w < +inf, in a fixed order (per-workgroup partials, then one ordered pass: two calls agree bitwise), and the largest
 * such difference (exact).  Uses only the statistics part of ws: the state of the sweeps is kept. */
int tg_depfill_stats(const float* z, const float* w, const uint8_t* known, const uint8_t* sel, int H, int W, int64_t* counts,
                     double* sums, void* ws, size_t ws_bytes, tg_stream_t stream);
/* out [H][W] = w where z < w < +inf, z's own bits where w <= z, NaN at unknown pixels and where w == +inf.  depth (may be
 * NULL) = out - z in fp32: 0 where not raised, NaN where out is.  flags (uint8, may be NULL) = 1 on the known pixels with
 * w > z, else 0 (tg_objmask_components' input). */
int tg_depfill_finish(const float* z, const float* w, const uint8_t* known, int H, int W, float* out, float* depth,
                      uint8_t* flags, tg_stream_t stream);

/* ---- D8 flow directions, flat resolution, flow accumulation (csrc/flow.hip) -----------------------------------
 * Known pixels: known[p] != 0 (tg_objmask_known's map); w [H][W] is any fp32 surface, usually tg_depfill_finish's out at
 * connectivity 8.  Sides as tg_objmask_known (H, W >= 1, H * W < 2^31).  A direction code is one uint8: 0 unknown; 1..8 the
 * receiver E, SE, S, SW, W, NW, N, NE (the ESRI code is 1 << (code - 1)); TG_FLOW_OUT, an outlet that drains off the raster or
 * into a void; TG_FLOW_PIT, no receiver; TG_FLOW_UNDECIDED only between tg_flow_slope and tg_flow_flat_dir.  Equal candidates
 * are taken in the order of preference E, S, W, N, SE, SW, NW, NE.  An outlet is a known pixel on the raster's edge or with an
 * unknown 8-neighbour.
 * One workspace ws >= tg_flow_ws_bytes(H, W) serves all calls: 256 control bytes, two dirty planes of one byte per 64x64 tile
 * (each rounded up to 256 bytes), then four int32 planes of H * W words (each rounded up to 256 bytes): the pointers and the sums
 * of the accumulation, both double-buffered, 16 bytes per pixel.  0 for sides out of range. */
#define TG_FLOW_OUT 9
#define TG_FLOW_UNDECIDED 254
#define TG_FLOW_PIT 255
#define TG_FLOW_FAR 0x7fffffff
#define TG_FLOW_MAX_ROUNDS 32
size_t tg_flow_ws_bytes(int H, int W);
/* The slope step.  For a known pixel p and a known 8-neighbour n: d = w(p) - w(n) in fp32, s = d for a cardinal n and
 * d * 0x1.6a09e6p-1f (one fp32 multiply, nothing fused) for a diagonal one.  If some s > 0, dir(p) is the neighbour with the
 * largest s; otherwise TG_FLOW_OUT if p is an outlet, else TG_FLOW_UNDECIDED.  D [H][W] int32 = 0 where decided, TG_FLOW_FAR
 * where undecided, -1 at unknown pixels.  counts [2] int64 (zeroed here) = known pixels, outlets.  Every tile of ws is marked
 * dirty and its sweep counter zeroed. */
int tg_flow_slope(const float* w, const uint8_t* known, int H, int W, uint8_t* dir, int32_t* D, int64_t* counts, void* ws,
                  size_t ws_bytes, tg_stream_t stream);
/* Enqueues n sweeps, 1 <= n <= 2^20, of D (after tg_flow_slope on the same w, D and ws): every dirty tile is relaxed,
 * D(p) <- min(D(p), 1 + min over the known 8-neighbours n with w(n) == w(p) of D(n)), to a fixed point against its one-pixel halo
 * (or to a cap on the inner rounds; it stays dirty then).  The fixed point is, for an undecided pixel, the smallest number of
 * 8-connected steps through pixels of its own height to a decided pixel of that height, TG_FLOW_FAR if there is none.  changed,
 * visits and the dirty tiles as tg_depfill_sweep.  Every value of D is at all times the length of such a path or TG_FLOW_FAR;
 * the plane at the fixed point does not depend on the order of the visits. */
int tg_flow_flat_sweep(const float* w, int H, int W, int n, int32_t* D, int32_t* changed, int64_t* visits, void* ws,
                       size_t ws_bytes, tg_stream_t stream);
/* Every TG_FLOW_UNDECIDED pixel of dir gets its code: with 0 < D(p) < TG_FLOW_FAR the known neighbour n with w(n) == w(p) and the
 * smallest D(n) < D(p) (at the fixed point of the sweeps that is D(p) - 1), else TG_FLOW_PIT.  counts [2] int64 (zeroed here) =
 * pixels that got a flat code, pits.  Along every edge (w, D) decreases lexicographically, converged or not: a forest. */
int tg_flow_flat_dir(const float* w, const int32_t* D, int H, int W, uint8_t* dir, int64_t* counts, tg_stream_t stream);
/* Flow accumulation A(p) = 1 + sum of A(q) over the pixels q whose receiver is p, int32, 0 at unknown pixels, by pointer
 * doubling in ws.  _init: next(p) = the receiver's linear index (-1 for every other code), S = 1 on the pixels with dir != 0.
 * tg_flow_accum enqueues rounds k0 .. k0 + n - 1 (k0 = the rounds enqueued before, k0 + n <= TG_FLOW_MAX_ROUNDS): in round k
 * every pixel adds its S to itself and to S[next(p)] in the other plane by integer atomics (exact in any order) and takes
 * next(next(p)); a round that finds no pointer left does nothing.  state [2] int32 = pointers left after these rounds (0: done),
 * rounds that ran.  _finish(rounds = state[1]) copies the sums to acc [H][W] and writes their maximum to amax [1]. */
int tg_flow_accum_init(const uint8_t* dir, int H, int W, void* ws, size_t ws_bytes, tg_stream_t stream);
int tg_flow_accum(int H, int W, int k0, int n, int32_t* state, void* ws, size_t ws_bytes, tg_stream_t stream);
int tg_flow_accum_finish(int H, int W, int rounds, int32_t* acc, int32_t* amax, void* ws, size_t ws_bytes, tg_stream_t stream);

/* ---- Watersheds, flow length, drainage comparison (csrc/drainage.hip) ------------------------------------------
 * dir [H][W] uint8 is a direction grid of the section above without TG_FLOW_UNDECIDED (the caller's to check: it needs a read of
 * the grid).  next0(p) = the receiver's linear index for the codes 1..8, else -1.  pour (may be NULL) [H][W] uint8, nonzero = pour
 * point: a pixel with pour != 0 and dir != 0 is a terminal whatever its code (next0 = -1); a pour point on a pixel with dir == 0
 * is ignored.  T(p) is the last pixel of p's path (T(p) = p for a terminal), nc(p) and nd(p) the cardinal and diagonal steps
 * from p to T(p); pixels with dir == 0 have T = -1, nc = nd = 0.  Sides as tg_objmask_known (H, W >= 1, H * W < 2^31).
 * Gather-only pointer doubling: a pixel's state is one 16-byte record (next, last, nc, nd), start (next0, p, c0, d0) with
 * (c0, d0) = (1, 0) for a cardinal code, (0, 1) for a diagonal one, else (0, 0); in round k a pixel with q = next(p) >= 0 takes
 * (next(q), last(q), nc(p) + nc(q), nd(p) + nd(q)), every word of q from the state before the round; any other pixel copies its
 * record.  No atomics on the rasters: exact, bitwise reproducible.
 * One workspace ws >= tg_flow_basin_ws_bytes(H, W) serves the three calls: 256 control bytes, then two planes of H * W records
 * of 16 bytes (each rounded up to 256 bytes), 32 bytes per pixel; round k reads plane k & 1 and writes the other.  ws is aligned
 * to 16 bytes.  0 for sides out of range. */
#define TG_FLOW_BASIN_COUNTS 3
#define TG_FLOW_COMPARE_COUNTS 19
size_t tg_flow_basin_ws_bytes(int H, int W);
/* The start state in plane 0, live[0].  counts [2] int64 (zeroed here) = pour points that became terminals, pour points ignored. */
int tg_flow_basin_init(const uint8_t* dir, const uint8_t* pour /* may be NULL */, int H, int W, int64_t* counts, void* ws,
                       size_t ws_bytes, tg_stream_t stream);
/* Enqueues rounds k0 .. k0 + n - 1 (k0 = the rounds enqueued before, k0 + n <= TG_FLOW_MAX_ROUNDS); a round that finds no pointer
 * left does nothing.  state [2] int32 = pointers left after these rounds (0: done), rounds that ran. */
int tg_flow_basin(int H, int W, int k0, int n, int32_t* state, void* ws, size_t ws_bytes, tg_stream_t stream);
/* From the plane of `rounds` (= state[1]) rounds: basin [H][W] int32 = last (T at the end, -1 where dir == 0); nc, nd (int32,
 * may be NULL); length_m (may be NULL) = (float)(cellsize * ((double)nc + 1.4142135623730951 * (double)nd)): one fp64 multiply,
 * one add, one multiply, nothing fused, one rounding to fp32.  counts [TG_FLOW_BASIN_COUNTS] int64 (zeroed here) = terminals
 * (pixels with last == p), the largest nc + nd, the bits of the largest length_m (computed with or without the plane; a
 * non-negative float's bits order as integers).  cellsize finite and > 0. */
int tg_flow_basin_finish(int H, int W, int rounds, double cellsize, int32_t* basin, int32_t* nc, int32_t* nd, float* length_m,
                         int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream);
/* Two routings of one raster compared in integers, over the pixels with sel != 0, dir_t != 0 and dir_p != 0 (t = truth, p = the
 * fill).  basin_*: tg_flow_basin_finish's; acc_*: tg_flow_accum_finish's; a pixel is a stream of a side when acc >= stream_cells
 * (>= 1); d2_t, d2_p: tg_edt's squared distances to the truth's and the fill's stream masks, so sides in [1, TG_EDT_MAX_SIDE];
 * 0 <= tol2 < TG_EDT_FAR.  counts [TG_FLOW_COMPARE_COUNTS] int64 (zeroed here), exact in any order (per-wave shuffles, one 64-bit integer
 * atomic per wave and counter):
 *   0 cells; 1 dir_equal (the codes are equal); 2 dir_routed (both codes in 1..8); 3 dir_within_45 (both in 1..8 and their
 *   cyclic difference <= 1); 4 same_outlet (basin_t == basin_p); 5 outlet_d2_sum, 6 outlet_d2_max: the squared pixel distance
 *   between the two terminals (0 where a basin is negative); 7 area_octave_sum: sum of |floor(log2 acc_t) - floor(log2 acc_p)|
 *   (an acc < 1 counts as 1); 8 streams_truth, 9 streams_pred, 10 streams_both; over the fill's stream pixels: 11 matched
 *   (d2_t <= tol2), 12 far (d2_t == TG_EDT_FAR; not in the next two), 13 d2_sum, 14 d2_max; over the truth's stream pixels the
 *   same four from d2_p: 15, 16, 17, 18. */
int tg_flow_compare(const uint8_t* sel, const uint8_t* dir_t, const uint8_t* dir_p, const int32_t* basin_t, const int32_t* basin_p,
                    const int32_t* acc_t, const int32_t* acc_p, const int32_t* d2_t, const int32_t* d2_p, int H, int W,
                    int32_t stream_cells, int32_t tol2, int64_t* counts, tg_stream_t stream);

/* ---- Stream classes, links, Strahler order, height above the nearest drainage, flood comparison (csrc/drainage.hip, DESIGN.md
 * 8x) ------------------------------------------------------------------------------------------------------------------------
 * dir [H][W] uint8 as in the section above; acc [H][W] int32 is any accumulation plane (it need not belong to dir).  A stream
 * pixel has dir != 0 and acc >= min_cells (>= 1).  A stream donor of p is a stream pixel with a code 1..8 whose receiver is p; sd(p)
 * is their number.  Class (uint8): 0 not a stream, TG_STREAM_HEAD (sd = 0), TG_STREAM_INTERIOR (sd = 1), TG_STREAM_JUNCTION
 * (sd >= 2).  up(p) is the one stream donor of an interior pixel, -1 elsewhere; top(p) is the end of p's up chain (top(p) = p for
 * heads and junctions): the upstream end of p's link.  Strahler order: 1 for a head, the donor's for an interior pixel, for a
 * junction max(m1, m2 + 1) with m1 >= m2 the two largest orders among its stream donors; constant along a link.
 * Sides as tg_objmask_known (H, W >= 1, H * W < 2^31). */
#define TG_STREAM_HEAD 1
#define TG_STREAM_INTERIOR 2
#define TG_STREAM_JUNCTION 3
#define TG_STREAM_ORDER_BINS 15
#define TG_STREAM_ORDER_COUNTS (1 + 2 * TG_STREAM_ORDER_BINS)
#define TG_FLOOD_MAX_STAGES 8
#define TG_FLOOD_COUNTS (6 + 3 * TG_FLOOD_MAX_STAGES)
typedef struct {
    float s[TG_FLOOD_MAX_STAGES];
} tg_flood_stages;
/* One pass: cls [H][W] uint8; order [H][W] int32 = 1 on stream pixels, 0 elsewhere (the start of tg_stream_order); and the start
 * records of the upstream doubling in plane 0 of a tg_flow_basin workspace (ws >= tg_flow_basin_ws_bytes(H, W), aligned to 16
 * bytes) with live[0]: (up, p, c, d) for an interior pixel, (c, d) = (1, 0) for a cardinal code of the donor and (0, 1) for a
 * diagonal one; (-1, p, 0, 0) for heads and junctions; (-1, -1, 0, 0) off the streams.  After it tg_flow_basin's rounds and
 * tg_flow_basin_finish give top (as basin; -1 off the streams), the cardinal and diagonal steps from top(p) down to p and their
 * length.  counts [4] int64 (zeroed here) = stream pixels, heads, junctions, stream terminals (stream pixels whose receiver is
 * not a stream pixel). */
int tg_stream_class(const uint8_t* dir, const int32_t* acc, int H, int W, int32_t min_cells, uint8_t* cls, int32_t* order,
                    int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream);
/* Enqueues n >= 1 rounds over the junctions [nj] int32 (the linear indices of the pixels of class TG_STREAM_JUNCTION, in any
 * order; nj = 0 launches nothing).  In a round junction j reads order[top(q)] of its stream donors q (the neighbours with
 * cls != 0 whose code points at j) and raises order[j] to max(m1, m2 + 1) if that is larger: in place, relaxed atomic loads at
 * agent scope and atomicMax, so a round may see values of its own; the update is monotone and every iterate is a lower bound of
 * the order, so any schedule ends at the same plane.  changed [1] int32 (zeroed here) = raises of the last of the n rounds (0: a
 * fixed point).  An index junctions[i] or top[q] outside [0, H * W) is skipped. */
int tg_stream_order(const uint8_t* dir, const uint8_t* cls, const int32_t* top, const int32_t* junctions, int nj, int H, int W,
                    int n, int32_t* order, int32_t* changed, tg_stream_t stream);
/* out [H][W] uint8 = order[top(p)] on stream pixels (at most 255), 0 elsewhere.  counts [TG_STREAM_ORDER_COUNTS] int64 (zeroed
 * here) = the largest order; cells of order 1 .. TG_STREAM_ORDER_BINS; links (heads and junctions) of order 1 ..
 * TG_STREAM_ORDER_BINS; higher orders go into the last bin. */
int tg_stream_order_finish(const uint8_t* cls, const int32_t* top, const int32_t* order, int H, int W, uint8_t* out,
                           int64_t* counts, tg_stream_t stream);
/* Height above the nearest drainage.  w [H][W] fp32 is the routed surface, basin [H][W] int32 tg_flow_basin_finish's terminals
 * with the drainage mask smask [H][W] uint8 as pour points.  p is drained when T = basin(p) lies in [0, H * W) and smask(T) != 0:
 * hand(p) = w(p) - w(T), one fp32 subtract; NaN (0x7fc00000) elsewhere.  With length_m and distance_m (both or neither NULL)
 * distance_m(p) = length_m(p) where drained, NaN elsewhere.  counts [4] int64 (zeroed here) = drained pixels, undrained pixels
 * (basin >= 0, not drained), drainage pixels (smask != 0 and basin >= 0), the bits of the largest hand > 0. */
int tg_hand(const float* w, const int32_t* basin, const uint8_t* smask, const float* length_m, int H, int W, float* hand,
            float* distance_m, int64_t* counts, tg_stream_t stream);
/* Two HAND planes compared over the pixels with sel != 0 (t = truth, p = the fill), stages s[0] < ... < s[k - 1], 1 <= k <=
 * TG_FLOOD_MAX_STAGES, each finite and > 0.  counts [TG_FLOOD_COUNTS] int64 (zeroed here), exact in any order (per-wave shuffles,
 * one 64-bit integer atomic per wave and non-zero counter):
 *   0 cells (neither hand NaN); 1 undrained_t, 2 undrained_p (that side's hand NaN); over the cells: 3 abs_q10 = sum of
 *   rint((double)|hp - ht| * 1024) with the difference and the absolute value in fp32 and the rounding half-to-even, 4 bias_q10 =
 *   the same of hp - ht, signed; 5 abs_max_bits, the bits of the largest |hp - ht|; for stage i: 6 + 3 i wet_t (ht <= s[i]),
 *   7 + 3 i wet_p, 8 + 3 i wet_both. */
int tg_flood_compare(const uint8_t* sel, const float* hand_t, const float* hand_p, int H, int W, tg_flood_stages stages, int k,
                     int64_t* counts, tg_stream_t stream);

/* ---- Multiple-flow-direction accumulation, slope, topographic wetness index (csrc/mfd.hip) ---------------------
 * w, known and dir [H][W] are a routed surface, its known map and its direction grid as the sections above leave them (dir
 * without TG_FLOW_UNDECIDED).  Neighbour k = 0..7 is code k + 1.  For a known pixel q and a known neighbour n_j inside the raster:
 * d_j = w(q) - w(n_j), one fp32 subtract, valid iff d_j > 0 (a NaN never is); t_j = (double)d_j raised to the integer exponent
 * e (1 .. TG_MFD_MAX_EXPONENT) by e - 1 fp64 multiplies t = t * d, times cdiag for odd j (a diagonal); S = the fp64 sum of the
 * valid t_j in the order j = 0..7.  S > 0 ("dispersive"): q gives the fraction f_j = t_j / S, one fp64 divide, to n_j; otherwise
 * with dir(q) in 1..8 ("single") it gives 1.0 to its D8 receiver; otherwise (a "sink": TG_FLOW_OUT, TG_FLOW_PIT) nothing.  cdiag
 * in (0, 1] is the caller's 2^(-(e + 1) / 2).  A(p) = 1.0 for a known p, then for k = 0..7 in order, where neighbour k gives a
 * fraction f > 0 to p, A(p) = A(p) + f * A(n_k): one fp64 multiply, one fp64 add, nothing fused; 0 at unknown pixels.  Every A(p) is
 * computed once, from final values, so the plane does not depend on the order of the visits.  Sides as tg_objmask_known.
 * One workspace ws >= tg_mfd_ws_bytes(H, W) serves all calls: 256 control bytes, three planes of one byte per 64x64 tile (open,
 * and the wake marks of two sweeps), one donor byte per pixel, one fp64 S per pixel (each rounded up to 256 bytes) and 64 KiB of
 * partial sums.  0 for sides out of range. */
#define TG_MFD_MAX_EXPONENT 8
#define TG_MFD_COUNTS 5
size_t tg_mfd_ws_bytes(int H, int W);
/* S and the donor bytes into ws, every tile on the work list; A [H][W] fp64 = -1.0 ("not final") at known pixels, 0.0 at unknown
 * ones.  counts [TG_MFD_COUNTS] int64 (zeroed here) = dispersive, single, sink pixels, pixels that are not final (their sum), tile
 * visits (0). */
int tg_mfd_setup(const float* w, const uint8_t* known, const uint8_t* dir, int H, int W, int exponent, double cdiag, double* A,
                 int64_t* counts, void* ws, size_t ws_bytes, tg_stream_t stream);
/* Enqueues n sweeps, 1 <= n <= 2^20 (after tg_mfd_setup with the same w, exponent, cdiag, A, counts and ws): every marked tile
 * that holds a pixel that is not final is visited; in it a pixel that is not final and whose donors are all final gets its value,
 * until nothing more can (or a cap on the inner rounds).  A tile is marked for a sweep when the sweep before stopped it at the cap
 * or made a pixel on a neighbour tile's rim final; for the first sweep every tile is.  The marks decide which visits happen, never
 * what a visit computes.  counts[3] goes down by the pixels made final, counts[4] up by the tiles visited.  A block of sweeps in
 * which counts[3] stays above 0 and unchanged would mean a cycle; the graph has none. */
int tg_mfd_sweep(const float* w, int H, int W, int exponent, double cdiag, int n, double* A, int64_t* counts, void* ws,
                 size_t ws_bytes, tg_stream_t stream);
/* acc [H][W] fp32 = A rounded once; out [2] double (zeroed here) = the largest A, and the sum of A over the sinks in a fixed order
 * (per-workgroup partials, then one ordered pass: two calls agree bitwise).  With every pixel final that sum is the number of
 * known pixels up to rounding. */
int tg_mfd_finish(const double* A, const uint8_t* dir, int H, int W, float* acc, double* out, void* ws, size_t ws_bytes,
                  tg_stream_t stream);
/* Horn's slope tan(beta) in fp32, nothing fused: with the 3x3 neighbourhood a b c / d . f / g h i (rows top to bottom), a neighbour
 * outside the raster or unknown replaced by the centre, gx = ((c - a) + 2 (f - d)) + (i - g), gy = ((g - a) + 2 (h - b)) + (i - c),
 * slope = sqrtf(gx gx + gy gy) / den with den = (float)(8 * cellsize) from the caller; NaN (0x7fc00000) at unknown pixels. */
int tg_terrain_slope(const float* w, const uint8_t* known, int H, int W, float den, float* slope, tg_stream_t stream);
/* twi = logf((acc * cellsize) / fmaxf(slope, min_slope)) at known pixels, NaN (0x7fc00000) at unknown ones; cellsize and min_slope
 * finite and > 0. */
int tg_wetness(const float* acc, const float* slope, const uint8_t* known, int H, int W, float cellsize, float min_slope,
               float* twi, tg_stream_t stream);
/* Two wetness planes over the pixels with sel != 0 where both are finite (t = truth, p = the fill), d = twi_p - twi_t in fp32:
 * counts [2] int64 (zeroed here) = cells, the bits of the largest |d|; sums [3] double = the sums of d, |d| and d * d in fp64 in a
 * fixed order (as tg_mfd_finish's).  ws >= tg_mfd_ws_bytes(H, W); only its partial sums are used. */
int tg_wetness_compare(const uint8_t* sel, const float* twi_t, const float* twi_p, int H, int W, int64_t* counts, double* sums,
                       void* ws, size_t ws_bytes, tg_stream_t stream);

/* ---- Second-difference spectrum of a fill against the truth (csrc/texture.hip) ----------------------------------
 * z (truth) and p (the fill) fp32 [H][W]; sel uint8 [H][W], nonzero = scored; known uint8 [H][W], nonzero = known in both surfaces.
 * Octave j = 0 .. octaves - 1 (octaves in 1 .. TG_TEX_OCTAVES) has the lag h = 2^j px; class 0 (axial) has the unit steps
 * u = (dy, dx) in {(0, 1), (1, 0)}, class 1 (diagonal) {(1, 1), (1, -1)}; scale s = 2 j + class.  A triple (centre x, step u of
 * the class) counts when sel[x] and known[x] are nonzero and both arms x - h u and x + h u lie inside the raster and are known;
 * the arms may lie outside sel.  Per triple, in fp64 from the fp32 values and nothing fused:
 * d_s = (s(x - h u) + s(x + h u)) - 2 s(x) for s in {z, p}.  counts [TG_TEX_SCALES] int64 (zeroed here) = the triples per scale,
 * exact (integer atomics); sums [TG_TEX_SCALES][TG_TEX_NSUM] double = the sums of d_z d_z, d_p d_p and d_z d_p per scale in a
 * fixed order (per-workgroup rows of partials in ws, then one workgroup adds the rows in index order: two calls agree bitwise).
 * The entries of octaves that were not requested come back zero.  p may alias z (the spectrum of one surface); neither is written.
 * ws >= tg_texture_ws_bytes(H, W), 8-byte aligned, contents arbitrary; 0 for sides out of range. */
#define TG_TEX_OCTAVES 5
#define TG_TEX_SCALES 10
#define TG_TEX_NSUM 3
size_t tg_texture_ws_bytes(int H, int W);
int tg_texture_compare(const float* z, const float* p, const uint8_t* sel, const uint8_t* known, int H, int W, int octaves,
                       int64_t* counts, double* sums, void* ws, size_t ws_bytes, tg_stream_t stream);

/* ---- Empirical semivariogram; ordinary kriging over the eight ray hits (csrc/kriging.hip) -------------------------
 * z fp32 [H][W]; known uint8 [H][W], nonzero = known.  Octave j = 0 .. octaves - 1 (octaves in 1 .. TG_VGM_OCTAVES) has the lag
 * L = 2^j px; class 0 (axial) has the unit steps u = (dy, dx) in {(0, 1), (1, 0)}, class 1 (diagonal) {(1, 1), (1, -1)}; scale
 * s = 2 j + class.  A pair is (x, x + L u) with both pixels inside the raster and known: every unordered pair of a scale counts
 * once.  Per pair, in fp64 from the fp32 values and nothing fused: d = (double)z(x) - (double)z(x + L u).  counts
 * [TG_VGM_SCALES] int64 (zeroed here) = the pairs per scale, exact (integer atomics); sums [TG_VGM_SCALES] double = the sums of
 * d * d per scale in a fixed order (per-workgroup rows of partials in ws, then one workgroup adds the rows in index order: two
 * calls agree bitwise); the semivariance of a scale is sums / (2 counts).  The entries of octaves that were not requested come
 * back zero.  ws >= tg_variogram_ws_bytes(H, W), 8-byte aligned, contents arbitrary; 0 for sides out of range. */
#define TG_VGM_OCTAVES 6
#define TG_VGM_SCALES 12
size_t tg_variogram_ws_bytes(int H, int W);
int tg_variogram(const float* z, const uint8_t* known, int H, int W, int octaves, int64_t* counts, double* sums, void* ws,
                 size_t ws_bytes, tg_stream_t stream);
/* Variogram models gamma(h), h > 0 in metres; gamma(0) = 0.  power: nugget + scale * h^shape, 0 < shape < 2, with
 * h^shape taken as exp2(shape * log2(h)); exponential:
 * nugget + scale * (1 - exp(-h / shape)), shape > 0; spherical: nugget + scale * (1.5 r - 0.5 r^3), r = min(h / shape, 1),
 * shape > 0.  nugget >= 0 and scale > 0, all finite. */
enum { TG_VGM_POWER = 0, TG_VGM_EXPONENTIAL = 1, TG_VGM_SPHERICAL = 2 };
/* Ordinary kriging of the unknown pixels (known[p] == 0) from at most eight samples each: hits uint16 [8][H][W] as tg_rayfill
 * writes it (k_j steps along N, NE, E, SE, S, SW, W, NW to the first known pixel, 0 = no sample; a k_j that leaves the raster
 * counts as 0), sample j at p + k_j d_j.  Distances are h = cellsize * sqrt((double)n) with n the exact squared pixel distance.
 * With n >= 1 samples the weights solve sum_j w_j gamma(h_ij) + mu = gamma(h_i0), sum w = 1, in fp64.  r is the nearest sample,
 * the first in ray order among equals; out = (float)(z_r + sum_{i != r} w_i (z_i - z_r)), so a constant field comes back exactly
 * constant, and var = (float)max(0, sum w_i gamma(h_i0) + mu) in m^2; one sample gives out = z_r and var = 2 gamma(h_r0).  The
 * system is reduced against r (M_ij = gamma_ir + gamma_jr - gamma_ij, b_i = gamma_ir + gamma_r0 - gamma_i0, var = 2 gamma_r0 -
 * b^T M^-1 b) and factorised by Cholesky without pivoting.  An unknown pixel without a sample takes z[idx[p]] and var =
 * (float)(2 gamma(cellsize * sqrt(d2[p]))) when d2 and idx (tg_edt_nearest's; both or neither) are given and idx[p] >= 0; else
 * out and var are NaN.  Known pixels: out = z bit for bit, var = 0.  counts [3] int64 (zeroed here): unknown pixels filled from
 * ray samples, from the nearest pixel, left NaN.  out, var and z are distinct.  Sides in [1, TG_EDT_MAX_SIDE]. */
int tg_krige(const float* z, const uint8_t* known, const uint16_t* hits, int H, int W, double cellsize, int model, double nugget,
             double scale, double shape, const int32_t* d2, const int32_t* idx, float* out, float* var, int64_t* counts,
             tg_stream_t stream);

/* ---- Conditional simulation of voids (csrc/simulate.hip) ---------------------------------------------------------
 * tg_sim_field: u fp32 [H][W] = sum_k a_k cos(2 pi t_k) + nugget_amp * g, an unconditional random field.  waves: n_waves (1 ..
 * TG_SIM_MAX_WAVES) records of 16 bytes {int32 fx, int32 fy, uint32 phase, float amp}, 16-byte aligned; fx, fy are the frequency
 * in turns per pixel as Q32 fixed point.  The phase t_k = fx * X + fy * Y + phase is taken in wrapping uint32 arithmetic (2^32 =
 * one turn) at the global pixel X = x0 + x, Y = y0 + y (mod 2^32; x0, y0 in [0, 2^32)), so a tile with its origin set gets the
 * bits of the whole raster.  The cosine is a fixed fp32 polynomial of the top 26 bits of the phase, the sum over k runs in fp64
 * in index order, g is an Irwin-Hall sum of twelve 16-bit lanes of a counter hash of (seed, realisation, X, Y) with mean 0 and
 * variance 1 - 2^-32, skipped when nugget_amp == 0; the head of csrc/simulate.hip states every operation.  nugget_amp finite, >= 0.
 * Sides in [1, TG_EDT_MAX_SIDE]. */
#define TG_SIM_MAX_WAVES 512
int tg_sim_field(float* u, int H, int W, int64_t x0, int64_t y0, const void* waves, int n_waves, float nugget_amp, uint32_t seed,
                 uint32_t realisation, tg_stream_t stream);
/* Conditioning by kriging, one pixel at a time: out = z bit for bit where known != 0, else the fp32 value zk + (u - uk), taken as
 * (float)((double)zk + d), d = (double)u - (double)uk: one rounding (zk, uk: tg_krige of z and of u over the same hits; NaN where zk
 * is NaN).  With s1 and s2 (fp64 [H][W]; both or neither) an unknown pixel also adds d to s1 and d * d to s2: running sums over
 * realisations, zeroed by the caller.  out aliases no input. */
int tg_sim_combine(float* out, const float* z, const uint8_t* known, const float* zk, const float* u, const float* uk, double* s1,
                   double* s2, int H, int W, tg_stream_t stream);
/* The ensemble of n >= 2 realisations from the running sums: mean = (float)(zk + s1 / n), sd = (float)sqrt(max(0, (s2 - s1 * s1 /
 * n) / (n - 1))) in fp64; sd = 0 on known pixels (their sums are zero) and NaN where zk is NaN.  mean, sd and zk are distinct. */
int tg_sim_stats(float* mean, float* sd, const float* zk, const double* s1, const double* s2, int n, int H, int W,
                 tg_stream_t stream);

/* When enabled, every launch of the MFMA conv kernels is bracketed by hipEvents on its own launch
 * stream and tagged with its algorithmic FLOPs and bytes.  kind: 0 = fwd/dgrad implicit GEMM,
 * 1 = wgrad.  tg_prof_summary synchronises those events (host-blocking: call it outside any timed
 * region), returns the totals for `kind` and consumes its records. */
int tg_prof_enable(int on);
int tg_prof_summary(int kind, double* total_ms, int64_t* launches, double* flops, double* bytes);
/* One CSV row per recorded launch (kind,cfg,M,N,K,C,splits,ms,gflop,alg_mb,tag,route); records are kept.
 * route: which small-channel kernel a launch of cfg 2000 / 2001 / 2004 ran (SmallRoute, csrc/igemm_params.h),
 * 0 for every other kernel.  Read the file by column name: new columns are added at the end. */
int tg_prof_dump(const char* path);
/* Label (<= 31 chars, e.g. "dec1.fwd") attached to the launches recorded after it on the calling thread. */
int tg_prof_tag(const char* tag);

#ifdef __cplusplus
}
#endif
#endif /* TERRAGAN_HIP_H */
