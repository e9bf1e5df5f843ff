/*
 * corenet_hip.h -- C ABI of libcorenet_hip.so, the MI355X (gfx950) native
 * implementation of the CoReNet forward/backward hot path.
 *
 * Plain C: raw device pointers, explicit sizes/strides, a hipStream_t passed as
 * void*.  No torch types.  Every entry point returns 0 on success, a negative
 * CRN_E* code on bad arguments, or a positive hipError_t.
 *
 * Each entry point names the reference (google-research/corenet, paths relative
 * to src/corenet/) interface it replaces.  The Python host in corenet_amd/
 * mirrors the reference's module API on top of these.
 */
#ifndef CORENET_HIP_H_
#define CORENET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRN_OK 0
#define CRN_EINVAL (-1)   /* bad argument (shape / alignment / unsupported mode) */
#define CRN_ENOMEM (-2)   /* workspace too small */
#define CRN_ENOCONV (-3)  /* iterative kernel did not converge within max rounds */

typedef void* crnStream;  /* hipStream_t */

/* Logical NCDHW view of an fp32 tensor.  element(b,c,d,h,w) lives at
 *   base + b*sB + (chan_off ? chan_off[c] : c*sC) + d*sD + h*sH + w*sW
 * chan_off (device int32 table) expresses space-to-depth / depth-to-space
 * (pixel-shuffle) channel layouts without materialising them.              */
typedef struct {
  float* base;
  int32_t B, C, D, H, W;
  int64_t sB, sC;
  const int32_t* chan_off;
  int32_t sD, sH, sW;
} crnView;

/* Per-channel affine(+ReLU) applied to the INPUT of a conv while it is staged
 * into LDS: v = x; if(pre_relu) v=max(v,0); v = v*scale[c]+shift[c];
 * if(post_relu) v=max(v,0).  Zero padding is applied AFTER the transform
 * (reference: BatchRenorm/ReLU modules precede the padded conv,
 * reconstruction_decoder.py:56-60, resnet50.py:62-69).  scale==NULL => identity. */
typedef struct {
  const float* scale;
  const float* shift;
  int32_t pre_relu, post_relu;
} crnInTransform;

/* Structural zeros of the packed weights (transposed convolutions written as window correlations:
 * each of the 8 output/input parities only uses a sub-box of the window, 343 of 8*64 taps for k=7).
 * The logical OUTPUT channels [0, y->C) form n_groups equal contiguous groups, the logical INPUT
 * channels [0, x->C) c_groups groups; for group g every weight with a tap outside the half-open box
 * (d0,d1,h0,h1,w0,w1) is zero, and the kernels skip those taps.  0 groups = no information.  Host memory. */
typedef struct {
  int32_t n_groups, c_groups;          /* 0..8 */
  int8_t n_box[8][6];
  int8_t c_box[8][6];
} crnTapBoxes;

/* ---------------- convolutions (MFMA fp32 implicit GEMM) -------------------
 * One stride-1 window correlation covers Conv2d / Conv3d / ConvTranspose3d
 * forward and data-gradient of the reference (resnet50.py:62-69,95-107,124;
 * reconstruction_decoder.py:49-95; ray_traced_skip_connection.py:38) through
 * views + packed weights (corenet_amd/model/conv_geometry.py):
 *   y[b,n,o] = bias[b*bias_sB+n] + sum_{c,t} T(x)[b,c,o - pad_lo + t] * w[(c*T+t)*Npad + n]
 * w: packed [Cin][kd*kh*kw][Npad] fp32, Npad multiple of 16.
 * splits>1 splits the Cin reduction over blocks (atomic accumulate; y is
 * zeroed first by the call).                                                 */
int crn_conv_fwd(const crnView* x, const crnInTransform* tr, const float* w, int Npad,
                 const float* bias, int bias_sB, const crnView* y,
                 int kd, int kh, int kw, int pd, int ph, int pw,
                 int splits, int accumulate /* y += result instead of y = result */,
                 const crnTapBoxes* boxes /* may be NULL */, crnStream stream);

/* Two 1x1x1 convolutions onto one output in ONE launch of the pointwise kernel:
 *   y[b,n,o] (+)= sum_{c < C1} x1[b,c,o] * w1[c*Npad + n] + sum_{c < C2} x2[b,c,o] * w2[c*Npad + n]
 * (the data gradients of op_a and of the shortcut of a down-sampling bottleneck, resnet50.py:94-107, are such a pair).
 * The reduction runs over the channels of x1, then those of x2, so the result differs from two crn_conv_fwd calls (the
 * second accumulating) by fp32 summation order only.  No input transform, no bias.
 * Covered: x1, x2 and y plain views (every sample a dense [C][D][H][W] block, 16-byte aligned base, batch stride a
 * multiple of 4) of the same B and the same S = D*H*W, S % 4 == 0, x1->C % 64 == 0, one Npad (multiple of 16, >= y->C)
 * for both weight matrices, 16-byte aligned weights; CRN_EINVAL otherwise, before anything is written or launched and
 * without consuming the arming of crn_splitk_defer.
 * splits: 0 = the rule of crn_conv_fwd's 1x1 path on C1 + C2 channels, 1 = none, n = at most n.  A split launch follows
 * the split-K protocol of crn_conv_fwd (crn_splitk_defer below): one pending sum or one reduction launch.          */
int crn_conv1x1_fwd_pair(const crnView* x1, const float* w1, const crnView* x2, const float* w2, int Npad,
                         const crnView* y, int splits, int accumulate /* y += result */, crnStream stream);

/* Which kernel a crn_conv_fwd / crn_conv_wgrad call with these arguments gets: the selection the launch itself runs,
 * as host arithmetic on extents, strides and alignment.  No HIP call is made and no pointer is followed except the view,
 * transform and box structs themselves (base, chan_off, w, dw, scale are only tested for NULL and alignment), so a
 * query needs no GPU.  Returns what the launch would return for a rejected call (CRN_EINVAL), CRN_OK otherwise.
 * The arguments are those of the launch, the stream replaced by the plan.                                        */
#define CRN_PLAN_DENSE_COLS 1   /* one position, many columns */
#define CRN_PLAN_DENSE_ROWS 2   /* one position, long reduction onto few columns */
#define CRN_PLAN_DENSE_WGRAD 3  /* weight gradient of the dense layer */
#define CRN_PLAN_POINTWISE 4    /* 1x1x1 window on plain views */
#define CRN_PLAN_GENERIC 5      /* tile engine: msub x nsub configuration */
typedef struct {
  int32_t path;             /* CRN_PLAN_* */
  int32_t msub, nsub;       /* 16-row (forward: MSUB; weight gradient: RSUB) and 16-column MFMA blocks per wave */
  int32_t xstage, dystage;  /* staging of x / dy: 0 scalars, 1 float4 units, 2 position pairs */
  int32_t forced;           /* forward: scalar staging because no 16-byte configuration fits */
  int32_t cc;               /* input channels per chunk */
  int32_t td, th, tw;       /* position tile */
  int32_t mw;               /* forward: width of the 16-position sub-tile */
  int32_t splits;           /* splits the launch asks for (whether the scratch can be had is only known there) */
  int32_t chunks;           /* what they divide: channel chunks (forward), position tiles (weight gradient) */
  int32_t vec_store;        /* forward: float4 epilogue (a split launch writes the dense scratch) */
  int32_t balanced;         /* weight gradient: per-group splits from the tap boxes */
  int32_t lds_bytes, lds_budget;
} crnConvPlan;
int crn_conv_fwd_plan(const crnView* x, const crnInTransform* tr, const float* w, int Npad,
                      const float* bias, int bias_sB, const crnView* y,
                      int kd, int kh, int kw, int pd, int ph, int pw,
                      int splits, int accumulate, const crnTapBoxes* boxes, crnConvPlan* out);

/* The same operation on the split-bf16 ("bf16x3") MFMA engine (csrc/conv_bf3.hip): every fp32 operand is
 * split into two bf16 terms and a product is three v_mfma_f32_16x16x32_bf16 with fp32 accumulation
 * (hi*hi + hi*lo + lo*hi; ~2^-16 relative per product instead of fp32's 2^-24).  A throughput mode for
 * the big decoder layers (reconstruction_decoder.py:72-95), selected per layer by the host; the fp32
 * engine above stays the parity default.  Returns CRN_EINVAL, before anything is written and without consuming the arming
 * of crn_splitk_defer, for calls it does not cover.  Covered:
 *   window  kd <= 8 and kh*kw in 13..16 (four tap groups) or 25..28 (seven): 4x4 and 5x5 planes, but also 2x7, 3x5, ...;
 *           at most 1024 staging units per patch (rules out 5x5 planes with kd = 8 on 8^3 tiles and the like)
 *   y       W a multiple of 16 with H >= 8, D >= 4 (tiles of 4 x 8 x 16 positions), or W == 8 with H even and >= 8,
 *           D >= 8 (tiles of 8 x 8 x 8); D and H need not be whole tiles; any strides; y->C <= Npad, Npad % 16 == 0
 *   x       unit W stride without channel table, every extent and stride even, 8-byte aligned base -- or a stride-2
 *           view with channel table and even W (4x4 planes only); x->C <= 512; x->C * taps * Npad < 2^29
 *   pads    any (an odd pw costs one leading patch column)                                                        */
int crn_conv_fwd_bf3(const crnView* x, const crnInTransform* tr, const float* w, int Npad,
                     const float* bias, int bias_sB, const crnView* y,
                     int kd, int kh, int kw, int pd, int ph, int pw,
                     int accumulate, const crnTapBoxes* boxes /* may be NULL */, crnStream stream);

/* crn_conv_fwd_bf3 with the weights pre-split and pre-arranged by crn_bf3_operands (slab order): the kernel copies
 * its weight slabs instead of gathering and splitting them at every staging step.  Same results bit for bit.     */
int crn_conv_fwd_bf3_slabs(const crnView* x, const crnInTransform* tr, const void* wslab, int Npad,
                           const float* bias, int bias_sB, const crnView* y,
                           int kd, int kh, int kw, int pd, int ph, int pw,
                           int accumulate, const crnTapBoxes* boxes /* may be NULL */, crnStream stream);

/* crn_conv_fwd_bf3_slabs as the DATA GRADIENT in front of a BatchRenorm's backward (reconstruction_decoder.py:56-60: a decoder
 * block is ReLU -> BatchRenorm -> conv, so the data gradient of the conv is the output gradient dy of the norm, and
 * batch_renorm.py:41-47's autograd needs sum(dy) and sum(dy * xn) over the tensor before it can form dx).  The launch that
 * writes dy = y also accumulates those two sums per channel from its accumulators, reading the norm's input x once, and
 * stores them per workgroup in `ws` ([C][nparts][2] doubles, the layout of crn_batch_renorm_bwd's own first pass), so that
 * crn_batch_renorm_bwd_apply can run without that pass: one full read of dy and of x less per norm.  The order of the sums is
 * fixed (lane, wave, workgroup slot): results do not depend on scheduling.
 * fuse->nparts is set to 0 when the launch could not produce the sums (split reduction, strided / non-dense y or x, more
 * workgroups than `ws` holds): the caller then runs crn_batch_renorm_bwd; y is written either way.  dsum (may be NULL) is
 * zeroed by the launch as crn_batch_renorm_bwd's first pass would.                                                       */
typedef struct crnBnBwdFuse {
  const float* x;      /* input of the norm: dense [B][C][D*H*W] inside each sample, D, H, W, C of y */
  int64_t sB_x;
  const float* saved;  /* [4][C] of crn_batch_renorm_stats: mu, rstd, r, d */
  int pre_relu;        /* the norm sees max(x, 0) */
  double* ws; size_t ws_bytes;
  float* dsum; int ndsum;
  int nparts;          /* out */
} crnBnBwdFuse;
int crn_conv_fwd_bf3_slabs_bnbwd(const crnView* x, const crnInTransform* tr, const void* wslab, int Npad,
                                 const float* bias, int bias_sB, const crnView* y,
                                 int kd, int kh, int kw, int pd, int ph, int pw,
                                 int accumulate, const crnTapBoxes* boxes /* may be NULL */, crnBnBwdFuse* fuse,
                                 crnStream stream);

/* ... or the partial sums of the BatchRenorm BEHIND the convolution (reconstruction_decoder.py:56-60): sum(y'), sum(y'^2) per
 * channel and workgroup, y' = max(y, 0) with pre_relu, in ws[(n * *nparts + i) * 2 + {0,1}] for crn_batch_renorm_finalize.
 * *nparts = 0 when the launch could not produce them (as above): the caller runs crn_batch_renorm_stats.          */
int crn_conv_fwd_bf3_slabs_stats(const crnView* x, const crnInTransform* tr, const void* wslab, int Npad,
                                 const float* bias, int bias_sB, const crnView* y,
                                 int kd, int kh, int kw, int pd, int ph, int pw,
                                 int accumulate, const crnTapBoxes* boxes /* may be NULL */, int pre_relu,
                                 double* ws, size_t ws_bytes, int* nparts, crnStream stream);

/* A convolution that splits its reduction writes partial sums to the library's scratch and adds them up in a
 * second launch.  crn_splitk_defer(1) arms, for the NEXT convolution call of this host thread (crn_conv2d_bf3, or
 * the 1x1 path of crn_conv_fwd), the following shortcut: if that call splits and does not accumulate, the sum is
 * left pending (recorded per host thread, together with the stream and device the convolution ran on) and a
 * crn_batch_renorm_stats (x = the conv's output) or crn_batch_renorm_bwd (dy = the conv's output) that follows ON THE
 * SAME STREAM adds the partial sums up while it loads them (stats also stores the sum to x; bwd is dy's only reader: its
 * register-resident form does not write dy, its two-pass form stores the sum to dy in the first pass for the second; the
 * one-workgroup-per-channel forms that read their input twice get the sum from a reduction launch first).  Results are
 * bit-identical to reduction + call: the splits are added in the reduction's order.  EVERY other entry point of this
 * library that takes a stream -- and a BatchRenorm call on another tensor or another stream -- first completes a
 * pending sum with an ordinary reduction launch on the convolution's own stream, so arming is always safe for callers that reach the tensor through this library on that
 * host thread; it only pays when the BatchRenorm call follows directly (resnet50.py:62-69: every conv of the encoder is
 * followed by its norm; in backward every data gradient feeds the norm's backward).  A caller that hands y to code
 * OUTSIDE the library (a torch op, a memcpy) or to another host thread while a sum may be pending must not arm.   */
int crn_splitk_defer(int on);
/* Split-K scratch is kept per (device, stream) and grown on demand -- which a stream under HIP-graph capture cannot do.
 * Call this BEFORE the capture: reserves `floats` (or, with 0, as much as any stream of the device has needed so far).  */
int crn_splitk_reserve(int64_t floats, crnStream stream);
/* Releases the scratch of `stream` (call before destroying a stream that was given one; waits for the device).  The table of
 * per-stream scratch buffers holds 64 entries per process and is guarded by a mutex.                                      */
int crn_splitk_release(crnStream stream);

/* Weight gradient in the same packed layout:
 *   dw[(c*T+t)*Npad+n] = sum_{b,o} T(x)[b,c,o-pad_lo+t] * dy[b,n,o]
 * dw must be zeroed by the caller or zero_first!=0.  Replaces autograd of the
 * modules above.                                                             */
int crn_conv_wgrad(const crnView* x, const crnInTransform* tr, const crnView* dy,
                   float* dw, int Npad, int kd, int kh, int kw, int pd, int ph, int pw,
                   int zero_first, const crnTapBoxes* boxes /* may be NULL; entries of dw at structural zeros may be left untouched */,
                   crnStream stream);

int crn_conv_wgrad_plan(const crnView* x, const crnInTransform* tr, const crnView* dy,
                        float* dw, int Npad, int kd, int kh, int kw, int pd, int ph, int pw,
                        int zero_first, const crnTapBoxes* boxes, crnConvPlan* out);

/* The weight gradient on the split-bf16 MFMA engine (csrc/conv_bf3.hip; see crn_conv_fwd_bf3): same packed
 * dw, same zero_first contract; CRN_EINVAL, before anything is written (the zero_first memset included), for calls it
 * does not cover.  Covered: windows of 57..64 tap pairs (5^3, 2x8x8, ...: 8 pairs per wave) on a unit-stride dy, or of
 * 25..32 pairs (4^3, 6x3x3, 2x5x5, 1x7x8, ...: 4 per wave) on a stride-2 space-to-depth dy or a unit-stride dy whose W is a
 * multiple of 16 (pairs = ceil(kd*kh*kw / 2)); dy W a multiple of 16 (D >= 4) or of 8 (D >= 8), H >= 8; unit-stride even x
 * as above; at most 1024 staging units per patch.  Channel counts are free (dy->C may be smaller than Npad).     */
int crn_conv_wgrad_bf3(const crnView* x, const crnInTransform* tr, const crnView* dy,
                       float* dw, int Npad, int kd, int kh, int kw, int pd, int ph, int pw,
                       int zero_first, crnStream stream);
/* ... with the tap boxes of the output columns (transposed convolutions): window rows that are structural zeros for all
 * columns of a workgroup are not multiplied (4^3 windows; their dw entries are not touched).                        */
int crn_conv_wgrad_bf3_boxes(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                             int kd, int kh, int kw, int pd, int ph, int pw, int zero_first,
                             const crnTapBoxes* boxes /* may be NULL */, crnStream stream);

/* Which kernel a call of the split-bf16 engine gets, as crn_conv_fwd_plan says it for the fp32 engine: the selection the
 * launches themselves run, host arithmetic only (no GPU needed), CRN_EINVAL where the launch returns it.
 * Forward query: exactly one of w / wslab as for crn_conv_fwd_bf3 / _slabs; fuse NULL, or the request of
 * crn_conv_fwd_bf3_slabs_bnbwd (fuse->x NULL: of crn_conv_fwd_bf3_slabs_stats, which reads pre_relu, ws, ws_bytes only).
 * A launch that wants to split is described as it runs when the split-K scratch can be had.                       */
#define CRN_BF3_PLAIN 0   /* conv_bf3_kernel */
#define CRN_BF3_HALF 1    /* conv_bf3_half_kernel: last chunk of <= 4 channels as 8 taps x 4 channels */
#define CRN_BF3_WS 2      /* conv_bf3_ws_kernel: wave-specialised */
typedef struct {
  int32_t kind;                /* forward: CRN_BF3_* */
  int32_t nsub;                /* N block = nsub x 16 columns */
  int32_t xmode;               /* forward: staging of x, 1 unit stride, 2 stride 2 */
  int32_t ng;                  /* forward: groups of 4 in-plane taps (4 or 7) */
  int32_t slabs;               /* forward: weights as pre-arranged slabs */
  int32_t td, th, tw;          /* position tile: 4 x 8 x 16 or 8 x 8 x 8 */
  int32_t splits;              /* over channel chunks (forward) / position tiles (weight gradient) */
  int32_t chunks;              /* what they divide */
  int32_t per_split;           /* chunks_per_split / tiles_per_split */
  int32_t vec_store, mode;     /* forward: float4 epilogue; 0 store, 1 accumulate, 3 partial sums to the scratch */
  int32_t rowskip, half_last;  /* forward */
  int32_t lead;                /* leading patch column of an odd pw */
  int32_t n_groups, c_groups;  /* tap-box groups applied (0: given none, or ignored) */
  int32_t nparts;              /* forward, fuse request: parts the launch would leave (0: it declines) */
  int32_t dmode, tpw, twt;     /* weight gradient: staging of dy (1 / 2), tap pairs per wave (8 / 4), tile width (16 / 8) */
  int32_t pipe, inherit, boxskip; /* weight gradient */
  int32_t lds_bytes;
} crnBf3Plan;
int crn_conv_fwd_bf3_plan(const crnView* x, const crnInTransform* tr, const float* w, const void* wslab, int Npad,
                          const float* bias, int bias_sB, const crnView* y,
                          int kd, int kh, int kw, int pd, int ph, int pw,
                          int accumulate, const crnTapBoxes* boxes, const crnBnBwdFuse* fuse, crnBf3Plan* out);
int crn_conv_wgrad_bf3_plan(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                            int kd, int kh, int kw, int pd, int ph, int pw, int zero_first,
                            const crnTapBoxes* boxes, crnBf3Plan* out);

/* Encoder engine (csrc/conv_e2d.hip): the ResNet-50 encoder's stride-1 Conv2d 1x1 / 3x3 layers (resnet50.py:49-115;
 * the stride of a down-sampling block is applied by crn_stride2_gather before its first 1x1) at batch sizes where
 * a layer is 1 GFLOP: split-bf16 MFMA like crn_conv_fwd_bf3, with the weights pre-arranged in MFMA operand order.
 *
 * crn_bf3_operands: packed fp32 weights [Cin][T][Npad] (the layout crn_conv_fwd reads) -> operand blocks, for
 * `nlayers` layers in one launch.  desc (DEVICE, int64 [nlayers][7]) = (first float of the layer in `packed`,
 * first 32-byte entry of the layer in `out`, Cin, T taps, Npad (multiple of 16), first workgroup of the layer,
 * KHW); ceil(entries/256) workgroups per layer, total_blocks = their sum.  An entry is 8 bf16 hi terms followed by
 * 8 bf16 lo terms of 8 consecutive input channels (w = hi + lo, hi = bf16(w)).
 * KHW == 0, encoder engine (Cin % 32 == 0): (Cin/32)*T*(Npad/16)*64 entries, entry ((cb*T + t)*(Npad/16) + ntile)*64
 *   + kk*16 + i = output column 16*ntile + i, tap t, channels 32*cb + 8*kk .. +7.
 * KHW == kh*kw, decoder engine (crn_conv_fwd_bf3_slabs): ceil(Cin/8)*kd*TP*Npad entries, TP = KHW rounded up to 4,
 *   entry ((chunk*kd + zd)*TP + tp)*Npad + n = output column n, tap zd*KHW + tp (zeros for tp >= KHW), channels
 *   8*chunk .. +7 (zeros past Cin).                                                                              */
int crn_bf3_operands(const float* packed, const int64_t* desc, int nlayers, int64_t total_blocks, void* out,
                     crnStream stream);
/* y = bias + window correlation of T(x) with the operand blocks `wop` of one layer (same operation, transform and
 * bias contract as crn_conv_fwd; forward pass, or data gradient with the packed data-gradient weights).
 * Covers: window 1x1 (pads 0) or 3x3, dense NC(D)HW views (unit W stride, rows and planes back to back), x and y of
 * the same extent, Cin % 32 == 0, Cout % 64 == 0 (= Npad), H*W a multiple of 64 (3x3: W % 8 == 0 and tiles of
 * 4x16 / 8x8 positions divide the image), 3x3 pads 0..2 per axis, one sample of x and the layer's operand blocks below
 * 2 GiB each; CRN_EINVAL otherwise, before anything is written and without consuming the arming of crn_splitk_defer
 * (callers keep such layers on crn_conv_fwd).
 * Split-K partial sums use the per-stream scratch shared with crn_conv_fwd (crn_splitk_reserve).                */
int crn_conv2d_bf3(const crnView* x, const crnInTransform* tr, const void* wop, int Npad, const float* bias,
                   int bias_sB, const crnView* y, int kh, int kw, int ph, int pw, int accumulate, crnStream stream);

/* Weight gradient of a 1x1 layer on the split-bf16 MFMA (csrc/conv_e2d.hip: both operands straight from HBM, K =
 * positions): dw[c*Npad + n] += sum_{b,p} T(x)[b,c,p] * dy[b,n,p], the contract of crn_conv_wgrad for a 1x1x1 window
 * (Conv2d 1x1 of resnet50.py:62-69; dw zeroed by the caller or zero_first).  Dense NC(D)HW views with the same
 * extent, positions per sample a multiple of 32; CRN_EINVAL otherwise.                                          */
int crn_conv_wgrad_1x1_bf3(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                           int zero_first, crnStream stream);
/* ... and of a 1x1 (pads 0) or 3x3 (pads 1, W a multiple of 8, 2-D images) layer: for 3x3 the three zw taps of an
 * input row come from one aligned 8-position load plus its two edge elements (dw row = c*9 + zh*3 + zw).        */
int crn_conv_wgrad_2d_bf3(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                          int kh, int kw, int ph, int pw, int zero_first, crnStream stream);

/* Which kernel a call of the encoder engine gets and how it is laid out, as crn_conv_fwd_bf3_plan says it for the decoder
 * engine: the selection the launches themselves run, host arithmetic only (no GPU needed), CRN_EINVAL where the launch
 * returns it.  A launch that wants to split is described as it runs when the split-K scratch can be had.          */
#define CRN_E2D_K1 1      /* conv_e2d_kernel<1, 4, 16>: 1x1, chunks of 128 channels */
#define CRN_E2D_K3W16 2   /* conv_e2d_kernel<9, 1, 16>: 3x3, tiles of 4 x 16 positions */
#define CRN_E2D_K3W8 3    /* conv_e2d_kernel<9, 1, 8>: 3x3, tiles of 8 x 8 positions */
#define CRN_E2D_WG1 4     /* wgrad1x1_bf3_kernel */
#define CRN_E2D_WG3 5     /* wgrad3x3_bf3_kernel */
typedef struct {
  int32_t kernel;              /* CRN_E2D_* */
  int32_t tiles;               /* forward: position tiles of 64 per sample */
  int32_t nblk;                /* forward: 32-channel blocks of x */
  int32_t nchunks;             /* forward: chunks (3x3: one block, 1x1: four) */
  int32_t per_split, splits;   /* forward: chunks per split, splits = ceil(nchunks / per_split); weight gradient: splits of K */
  int32_t mode;                /* forward: 0 store, 1 accumulate, 3 partial sums to the scratch */
  int32_t tab;                 /* forward: entries of the scale / shift tables in LDS (0 without a transform) */
  int32_t lds_bytes;           /* forward: dynamic LDS */
  int32_t grid_x, grid_y, grid_z;
  int32_t row_tiles, col_tiles;   /* weight gradient: tiles of 64 channels (3x3: 32 (c, zh) pairs) x 32 columns */
  int32_t ksteps, per_block;   /* weight gradient: K steps of 32 positions, per workgroup along z */
  int64_t zero_bytes;          /* weight gradient: what zero_first clears (0: the caller cleared dw) */
} crnE2dPlan;
int crn_conv2d_bf3_plan(const crnView* x, const crnInTransform* tr, const void* wop, int Npad, const float* bias,
                        int bias_sB, const crnView* y, int kh, int kw, int ph, int pw, int accumulate, crnE2dPlan* out);
int crn_conv_wgrad_2d_bf3_plan(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                               int kh, int kw, int ph, int pw, int zero_first, crnE2dPlan* out);

/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0        (weight packing)            */
/* Tiled index copy between a reference-layout buffer and a packed buffer (weight pack / gradient un-pack).
 * Tile t covers packed positions desc[t][0] + r*desc[t][1] + c (r, c in 0..7); bit (r*8+c) of mask[t] says
 * whether the element exists; its reference-layout index is desc[t][2] + r*desc[t][3] + c*desc[t][4], or
 * explicit_idx[desc[t][5] + r*8 + c] when desc[t][5] >= 0.
 * reverse == 0: dst[packed position] = src[index];  reverse != 0: dst[index] = src[packed position].       */
int crn_copy_tiles_f32(const float* src, float* dst, const int32_t* desc /* [ntiles][6] */,
                       const uint64_t* mask /* [ntiles] */, const int32_t* explicit_idx, int64_t ntiles,
                       int reverse, crnStream s);
/* The same copy for index maps that are (batches of) 2-D transposes -- every plain convolution's forward and
 * data-gradient layout -- staged through LDS so that both sides move in runs of 64+ floats.  Block t holds
 * G x A x B elements (g, a, b) with  reference index = fbase + g*fg + a*fa + b,  packed position = pbase + g*pg + a*pa
 * + b*pb  (pa == 1 or pb == 1);  desc[t] = {A, B, G, fbase, fa, fg, pbase, pa, pb, pg, ceil(2^32/(A*B)), ceil(2^32/B),
 * ceil(2^32/A), 0, 0, 0} (the reciprocals as uint32; unused where the divisor is 1),  G*A*(B|1) <= 8448.
 * conv_geometry.mat_index derives the blocks from the same index arrays as the tiles and proves them equal.      */
int crn_copy_mats_f32(const float* src, float* dst, const int32_t* desc /* [nblocks][16] */, int64_t nblocks,
                      int reverse, crnStream s);
int crn_gather_f32(const float* src, const int32_t* idx, float* dst, int64_t n, crnStream s);
/* dst[idx[i]] (+)= src[i] for idx[i] >= 0      (gradient un-packing)        */
int crn_scatter_f32(const float* src, const int32_t* idx, float* dst, int64_t n,
                    int accumulate, crnStream s);
/* bias gradient: db[c] = sum_{b,s} dy[b,c,s]  (dy: [B][C][S], batch stride sB) */
int crn_bias_grad(const float* dy, int B, int C, int64_t S, int64_t sB, float* db,
                  int accumulate, double* workspace /* crn_batch_renorm_workspace_bytes(C) */,
                  size_t workspace_bytes, crnStream s);

/* ---------------- BatchRenorm (batch_renorm.py:33-62) ----------------------
 * x: [B][C][S] with batch stride sB (spatial contiguous).  pre_relu: statistics
 * of max(x,0) (decoder blocks are ReLU->BN->conv).
 * train: batch mean / biased var -> r,d clamps from num_batches_tracked,
 * running-stat update (Q3,Q4); writes per-channel
 *   scale = gamma*r/sigma_b, shift = beta + gamma*(d - mu*r/sigma_b)
 * and saves mu, 1/sigma_b, r, d for the backward.  eval: running stats (saved, running statistics and the workspace are
 * not touched).  B <= 64.  Every argument is checked before anything is launched or written: CRN_EINVAL for B > 64 or a
 * NULL tensor (num_batches_tracked and saved may be NULL in eval mode only), CRN_ENOMEM for a workspace smaller than
 * crn_batch_renorm_workspace_bytes(C) needs for this shape -- the same holds for crn_batch_renorm_bwd below.          */
int crn_batch_renorm_stats(const float* x, int B, int C, int64_t S, int64_t sB, int pre_relu,
                           const float* gamma, const float* beta,
                           float* running_mean, float* running_var,
                           const int64_t* num_batches_tracked /* read only; see crn_add_i64 */,
                           float eps, float momentum, int training,
                           float* scale, float* shift, float* saved /* [4][C] */,
                           double* workspace, size_t workspace_bytes, crnStream s);
size_t crn_batch_renorm_workspace_bytes(int C);
/* crn_batch_renorm_stats (pre_relu = 0) followed by crn_affine_add_relu(x, scale, shift, r, rscale, rshift, ...) -- the tail
 * of a ResNet bottleneck (resnet50.py:71-78: bn of the last conv + shortcut + ReLU) -- as ONE call: where a workgroup owns
 * a channel with all of it in registers (training, B*S <= 16384: every bottleneck of the encoder) the tail is written by
 * the statistics launch itself, otherwise by a second launch.  Same results as the two calls, bit for bit.
 * y2 (may be NULL): additionally the stride-2 compaction of y, y2[b,c,i,j] = y[b,c,2i,2j] (what crn_stride2_gather(y, ...) gives:
 * the input of the down-sampling block that follows, resnet50.py:94-97), W = row width of a channel plane (S = H * W; y dense
 * [B][C][H][W]); written from the same registers when W is a multiple of 4, by a gather launch otherwise.               */
int crn_batch_renorm_stats_tail(const float* x, int B, int C, int64_t S, int64_t sB,
                                const float* gamma, const float* beta, float* running_mean, float* running_var,
                                const int64_t* num_batches_tracked, float eps, float momentum, int training,
                                float* scale, float* shift, float* saved, double* workspace, size_t workspace_bytes,
                                const float* r, const float* rscale, const float* rshift, int64_t sB_r,
                                float* y_pre, int64_t sB_pre, float* y, int64_t sB_y, int relu,
                                float* y2, int W, crnStream s);

/* Eval mode (batch_renorm.py:59: (x - running_mean) / sqrt(running_var + eps) * weight + bias) for all
 * BatchRenorm instances of a model at once: n channels, table [n][5] = offsets of (weight, bias) in `params`,
 * of (running_mean, running_var) in `buffers`, and of the channel in the `scale` / `shift` output slabs.  */
int crn_batch_renorm_eval_affine(const float* params, const float* buffers, const int32_t* table,
                                 int n, float eps, float* scale, float* shift, crnStream s);

/* Backward.  With x' = pre_relu ? max(x,0) : x, xn = (x'-mu)*rstd,
 * out = x'*scale+shift, g = dy * (post_relu ? out>0 : 1):
 *   dbeta = sum g ; dgamma = sum g*(r*xn+d)
 *   dx = gamma*r*rstd*(g - mean(g) - xn*mean(g*xn)) * (pre_relu ? x>0 : 1)
 * saved = [4][C]: mu, rstd, r, d written by crn_batch_renorm_stats(training).
 * dgamma/dbeta are accumulated when accumulate != 0.
 * dsum (optional, may be NULL): dsum[c] = sum_{b,s} dx[b,c,s] for c < ndsum -- the bias
 * gradient of the convolution whose output x is (autograd's sum over the conv output
 * gradient, conv bias + norm in resnet50.py:40-61 / reconstruction_decoder.py:33-71),
 * fused here so that dx is not read again by crn_bias_grad.                        */
int crn_batch_renorm_bwd(const float* x, int64_t sB_x, const float* dy, int64_t sB_dy,
                         int B, int C, int64_t S, int pre_relu, int post_relu,
                         const float* gamma, const float* scale, const float* shift,
                         const float* saved, float* dx, int64_t sB_dx,
                         float* dgamma, float* dbeta, int accumulate,
                         float* dsum, int ndsum,
                         double* workspace, size_t workspace_bytes, crnStream s);

/* The second pass of crn_batch_renorm_bwd alone: `workspace` already holds the per-channel partial sums
 * [C][nparts][2] (sum g, sum g*xn) written by crn_conv_fwd_bf3_slabs_bnbwd (fuse->nparts > 0) on the same stream.
 * post_relu must be 0 (the fused sums do not mask).  Same dx / dgamma / dbeta / dsum as crn_batch_renorm_bwd up to the
 * summation order of the two sums.  In deterministic mode (crn_set_deterministic) with dsum the workspace is used a second
 * time, for ndsum * (slices * B) doubles of the ordered sum over dx: CRN_ENOMEM if it is too small for either use, before
 * anything is launched.                                                                                            */
int crn_batch_renorm_bwd_apply(const float* x, int64_t sB_x, const float* dy, int64_t sB_dy,
                               int B, int C, int64_t S, int pre_relu,
                               const float* gamma, const float* scale, const float* shift,
                               const float* saved, float* dx, int64_t sB_dx,
                               float* dgamma, float* dbeta, int accumulate,
                               float* dsum, int ndsum,
                               double* workspace, size_t workspace_bytes, int nparts, crnStream s);

/* crn_relu_bwd_add(g, act, g2 -> dy) followed by crn_batch_renorm_bwd(x, dy, pre_relu = post_relu = 0, ...) -- the backward
 * of a bottleneck's tail and of its last norm -- as ONE call: dy = (act > 0 ? g : 0) + g2 (g2 may be NULL) is formed and
 * stored by the norm's backward launch where a workgroup owns a channel in registers (B*S <= 16384), by a launch of its
 * own otherwise.  Same results as the two calls, bit for bit.
 * g_compact (may be NULL): g is the data gradient of the stride-2 1x1 convolutions of the down-sampling block behind this one
 * (resnet50.py:94-97), given in its compact form [B][C][ceil(H/2)][ceil(W/2)] (g = crn_stride2_scatter(g_compact), rows of width W,
 * S = H * W): the register form reads it from there and never touches `g`; otherwise the call expands it into `g` (which must
 * then be a dense [B][C][S] buffer) first.                                                                            */
int crn_batch_renorm_bwd_head(const float* x, int64_t sB_x, float* dy, int64_t sB_dy,
                              const float* g, int64_t sB_g, const float* act, int64_t sB_act,
                              const float* g2 /* may be NULL */, int64_t sB_g2,
                              int B, int C, int64_t S, const float* gamma, const float* scale, const float* shift,
                              const float* saved, float* dx, int64_t sB_dx, float* dgamma, float* dbeta,
                              int accumulate, float* dsum, int ndsum,
                              double* workspace, size_t workspace_bytes, const float* g_compact, int W, crnStream s);

/* y = act( x*scale[c]+shift[c] [+ r*rscale[c]+rshift[c]] ) ; optional second
 * output y_pre (before the final ReLU).  Encoder block tails
 * (resnet50.py:72-82,109-115).                                               */
int crn_affine_add_relu(const float* x, const float* scale, const float* shift,
                        const float* r, const float* rscale, const float* rshift,
                        int B, int C, int64_t S, int64_t sB_x, int64_t sB_r,
                        float* y_pre, int64_t sB_pre, float* y, int64_t sB_y,
                        int relu, crnStream s);

/* dx = dy * (y_pre > 0) [+ dy2]  : backward of the block-tail ReLU, merging the
 * gradient arriving through the skip connection (dy2 may be NULL).           */
int crn_relu_bwd_add(const float* dy, const float* y_pre, const float* dy2,
                     int B, int C, int64_t S, int64_t sB_dy, int64_t sB_pre, int64_t sB_dy2,
                     float* dx, int64_t sB_dx, crnStream s);

/* ---------------- the encoder's stem on its own kernels ----------------------
 * ZeroPad2d(3) + Conv2d(3 -> 64, 7x7, stride 2) of resnet50.py:122-124 on the preprocessed image img [B,3,H,W]
 * (H even, W % 8 == 0; CRN_EINVAL otherwise: the caller keeps crn_conv_fwd / crn_conv_wgrad on the 2x2 space-to-depth
 * view), y / dy [B,64,H/2,W/2] dense.  w_packed / dw_packed: the layer's packed weights / weight gradient as
 * crn_conv_fwd / crn_conv_wgrad see them ([12][16][64], conv_geometry.stem_fwd), bias [64] or NULL.
 * stats_ws != NULL: the forward also leaves sum(y), sum(y^2) per channel and workgroup in
 * stats_ws[(n * parts + i) * 2 + {0,1}], parts = crn_stem_conv_parts(B, H, W) (0: shape not covered), for
 * crn_batch_renorm_finalize -- the BatchRenorm of resnet50.py:125 without a statistics pass over y.
 * crn_stem_conv_wgrad ADDS to dw_packed (atomics); CRN_EINVAL in deterministic mode.                              */
size_t crn_stem_conv_parts(int B, int H, int W);
int crn_stem_conv_fwd(const float* img, int B, int H, int W, const float* w_packed, const float* bias,
                      float* y, double* stats_ws /* may be NULL */, size_t ws_bytes, crnStream s);
int crn_stem_conv_wgrad(const float* img, int B, int H, int W, const float* dy, float* dw_packed, crnStream s);
/* scale / shift / saved / running statistics of a BatchRenorm (batch_renorm.py:41-57, training mode) from partial sums
 * ws[(c * nparts + i) * 2 + {0,1}] = sum(x), sum(x^2) of part i; count = elements per channel.                   */
int crn_batch_renorm_finalize(const double* ws, int nparts, int C, double count,
                              const float* gamma, const float* beta, float* running_mean, float* running_var,
                              const int64_t* nbt, float eps, float momentum,
                              float* scale, float* shift, float* saved, crnStream s);

/* ---------------- encoder odds and ends -------------------------------------
 * preprocess_image_caffe (resnet50.py:189-204): u8 RGB -> f32 BGR + means.    */
int crn_preprocess_caffe(const uint8_t* img, int B, int H, int W, float* out, crnStream s);
/* ZeroPad2d(1)+MaxPool2d(3,2) on relu(x*scale+shift)  (resnet50.py:126-131).
 * argmax (int32 flat input index, -1 when the max is the zero pad) is saved. */
int crn_bn_relu_maxpool_fwd(const float* x, const float* scale, const float* shift,
                            int B, int C, int H, int W, float* y, int32_t* argmax, crnStream s);
int crn_bn_relu_maxpool_bwd(const float* dy, const int32_t* argmax, int B, int C, int H, int W,
                            float* dx_bn /* grad wrt bn output, relu applied */, crnStream s);
/* avg[b,c] = mean_s relu(x_pre[b,c,s]) (resnet50.py:183) and its backward,
 * added into dx.                                                              */
int crn_relu_mean_fwd(const float* x_pre, int B, int C, int64_t S, int64_t sB, float* avg, crnStream s);
/* y[b,n] = bias[n] + sum_k x[b,k] w[n,k]  (nn.Linear, reconstruction_decoder.py:49) */
int crn_linear_fwd(const float* x, const float* w, const float* bias, int B, int K, int N,
                   float* y, int ldy, crnStream s);
/* dx[b,k] = sum_n dy[b,n] w[n,k],  dw[n,k] = sum_b dy[b,n] x[b,k],  db[n] = sum_b dy[b,n].  Each of dx, dw, db may be
 * NULL and is then not computed; every non-NULL one is written, whichever of the others are given.                */
int crn_linear_bwd(const float* x, const float* w, const float* dy, int lddy, int B, int K, int N,
                   float* dx, float* dw, float* db, crnStream s);
/* dx[b,c,s] (+)= (x_pre>0) * davg[b,c] / S                                    */
int crn_relu_mean_bwd(const float* x_pre, const float* davg, int B, int C, int64_t S, int64_t sB,
                      float* dx, int64_t sB_dx, int accumulate, crnStream s);
/* Stride-2 sub-sampling of a contiguous [B][C][hin][win] tensor, y[b,c,i,j] = x[b,c,2i,2j] with h = ceil(hin/2),
 * w = ceil(win/2), and its adjoint (dx[b,c,2i,2j] = dy[b,c,i,j], zeros elsewhere; every element of dx is written): the
 * stride-2 1x1 convolutions of the ResNet downscale blocks (resnet50.py:94-97) run on the compacted tensor.           */
int crn_stride2_gather(const float* x, float* y, int B, int C, int h, int w, int hin, int win, crnStream s);
int crn_stride2_scatter(const float* dy, float* dx, int B, int C, int h, int w, int hin, int win, crnStream s);
/* fill channels [c0,c0+3) of a [B][Ctot][S] tensor with offset[b][j]
 * (reconstruction_decoder.py:108-110)                              */
int crn_fill_offset_channels(float* x, int B, int64_t sB, int64_t S, int c0,
                             const float* offset, crnStream s);

/* The decoder's per-call inputs in one launch: layer_mats[s][b] = v2s[b] . scale(f_s, f_s, f_s) for the nscales <= 4 skip grids
 * (reconstruction_decoder.py:111-116: layer_matrix = v2s . scale(resolution / grid); columns 0-2 of the row-major 4x4 times f_s,
 * exact) and offset_out = offset.  v2s [B][16], offset [B][3] device; scales: HOST array of nscales floats.                   */
int crn_decoder_inputs(const float* v2s, const float* offset, int B, int nscales, const float* scales,
                       float* layer_mats, float* offset_out, crnStream s);

/* ---------------- ray-traced skip connection --------------------------------
 * Gather part of SampleGrid2d.forward (ray_traced_skip_connection.py:91-144):
 * per voxel centre (x,y,z)+off: p = M*(.,1); u=(px/pw)/2+.5; ix=(int)(u*W);
 * iy likewise (C truncation); +1 and clamp into the 1-px zero pad;
 * zero when p.z < 0 (Q7).  map: element (b, c, iy, ix) at b*map_sB + c*map_sC +
 * (iy*w+ix)*map_sP: (h*w, 1) is [B][C][h][w]; (1, C) is the channel-last [B][h][w][C]
 * that the compress conv can write and that is gathered four channels per load.
 * out: channels [0,C) of a view with batch stride out_sB, spatial D*H*W.
 * matrix: [B][16] row-major layer matrix, offset: [B][3].                     */
int crn_ray_sample_fwd(const float* map, int64_t map_sB, int64_t map_sC, int64_t map_sP,
                       int B, int C, int h, int w, const float* matrix, const float* offset,
                       float* out, int64_t out_sB, int D, int H, int W, crnStream s);
/* Backward (reference: autograd index_put_(accumulate=True)): dmap must be
 * zeroed by the caller unless zero_first.  dmap is channel-major [B][C][h][w] with batch stride dmap_sB.
 * Without a saved index tensor the library projects into its own scratch first (crn_ray_project).          */
int crn_ray_sample_bwd(const float* dout, int64_t dout_sB, int B, int C, int D, int H, int W,
                       const float* matrix, const float* offset,
                       float* dmap, int64_t dmap_sB, int h, int w, int zero_first, crnStream s);
/* The saved index tensor.  The reference's forward builds the index tensors of its advanced indexing
 * (ray_traced_skip_connection.py:118-135) and autograd keeps them for the index_put_ of the backward pass; here the
 * forward leaves ONE uint16 per voxel, idx[b][z][y][x] = iy*w+ix of the pixel the voxel reads, 0xFFFF = the outside
 * value (behind the camera or off the image), and the backward scatters from it without projecting again (no
 * floating-point arithmetic but the sums themselves).  Needs h*w < 65535 (CRN_EINVAL otherwise: use the plain entry
 * points above).  crn_ray_project writes the index tensor alone.                                            */
int crn_ray_sample_fwd_idx(const float* map, int64_t map_sB, int64_t map_sC, int64_t map_sP,
                           int B, int C, int h, int w, const float* matrix, const float* offset,
                           float* out, int64_t out_sB, int D, int H, int W, uint16_t* idx, crnStream s);
int crn_ray_project(const float* matrix, const float* offset, int B, int D, int H, int W, int h, int w,
                    uint16_t* idx, crnStream s);
int crn_ray_sample_bwd_idx(const float* dout, int64_t dout_sB, int B, int C, int D, int H, int W,
                           const uint16_t* idx, float* dmap, int64_t dmap_sB, int h, int w, int zero_first,
                           crnStream s);

/* ---------------- losses (losses.py) ---------------------------------------
 * kind: 0 iou_fgbg (:64-114), 1 xent_times_iou_agnostic (:144-160),
 *       2 iou_agnostic (:19-61), 3 xent (:117-141), 4 xent_times_iou_fgbg.
 * logits [B][C][S] fp32, gt [B][S] int32 labels, weights [B][S] fp32 per-voxel
 * loss weights or NULL (losses.py:47-49,99-102,134-136).  Writes loss[0] and,
 * when dlogits != NULL, d loss / d logits * grad_scale.
 * workspace: crn_loss_workspace_bytes(B,C).  A label outside [0,C) (the
 * reference raises inside F.one_hot / cross_entropy) is computed as class 0 and
 * sets the int at crn_loss_status_ptr(workspace, B) (device memory) to 1; a call
 * without such a label sets it back to 0.  B <= 64, 2 <= C <= 32; a call outside
 * these returns CRN_EINVAL and launches nothing (loss, dlogits, workspace untouched).
 * The workspace begins with the first pass's partial sums, double [B][nblk][6] with
 * nblk = min(ceil(S / 2048), 512): block j sums, in a fixed order, the voxels v with
 * (v / 256) % nblk == j -- I_fg, U_fg, I_ag, U_ag, w * (logZ - logit[gt]), and the
 * number of labels outside [0,C).                                                      */
int crn_loss_fwd_bwd(int kind, const float* logits, const int32_t* gt, const float* weights,
                     int B, int C, int64_t S, float* loss, float* dlogits, float grad_scale,
                     void* workspace, size_t workspace_bytes, crnStream s);
size_t crn_loss_workspace_bytes(int B, int C);
const int* crn_loss_status_ptr(void* workspace, int B);

/* ---------------- eval epilogue ---------------------------------------------
 * argmax over classes + confusion matrix (evaluation_results.py:40-51,
 * voxel_metrics.py:33-58): cm[gt*K+pred] += 1 (int64).  labels may be NULL.   */
int crn_argmax_confusion(const float* logits, const int32_t* gt, int B, int C, int64_t S,
                         int32_t* labels, int64_t* cm, crnStream s);

/* Multi-offset inference epilogue (super_resolution.py:92-125): logits [m^3][B][C][D][H][W], one
 * native-resolution forward per sampling offset n = (iz*m+iy)*m+ix (offset = (ix,iy,iz)/m);
 * out [B][C][mD][mH][mW] = softmax over C, interleaved: out[b][c][z*m+iz][y*m+iy][x*m+ix].
 * m == 1: plain channel softmax (pipeline inference_fn, super_resolution.py:121-126).          */
int crn_softmax_superres(const float* logits, int m, int B, int C, int D, int H, int W, float* out,
                         crnStream s);

/* Streaming evaluation epilogue (evaluation_results.py:42-54,249-253 + super_resolution.py:92-112 without the pmf;
 * csrc/eval_labels.hip, host twin csrc/eval_labels_cpu.cpp).  scores [B][C][D][H][W] are the logits
 * (or any per-class scores) of ONE native pass of an x m inference, pass n = (iz*m + iy)*m + ix in the offset order of
 * crn_softmax_superres: coarse voxel (b, z, y, x) is fine voxel (b, z*m+iz, y*m+iy, x*m+ix) of the [B][mD][mH][mW] grids.
 *   pred    index of the first maximum over c (only a strictly larger score replaces the running best: a NaN never
 *           does, a NaN at class 0 stays), times scene_class[b] when scene_class is given (fg_bg: the scene's label)
 *   labels  (may be NULL) receives pred (as int32) at the fine voxel; the other m^3 - 1 sub-lattices are not touched
 *   gt      (may be NULL) the fine-grid label, times scene_class[b] when given: both it and pred in [0, K) ->
 *           cm[g*K + pred] += 1, otherwise bad[0] += 1 and nothing is counted.  cm int64 [K][K] and bad int32 [1] are
 *           ACCUMULATED (required with gt); integer sums: the same inputs give the same bits on every run
 * m = 1, n = 0, K = C, scene_class NULL computes what crn_argmax_confusion computes.  1 <= C <= 32, 1 <= K <= 64, m >= 1,
 * 0 <= n < m^3, B, D, H, W >= 1 (the GPU call: B <= 65535), the byte sizes of scores and of the fine grid
 * (4 * B * D * H * W * m^3) within int64, scores and one of gt / labels given: anything else returns
 * CRN_EINVAL, launches nothing and writes nothing.  The GPU call does not wait for the GPU; the twin takes HOST memory. */
#define CRN_EVAL_MAX_CLASSES 32
#define CRN_EVAL_MAX_BINS 64
int crn_eval_labels(const float* scores, const int32_t* gt, const int32_t* scene_class, int B, int C, int K, int D, int H,
                    int W, int m, int n, int32_t* labels, int64_t* cm, int32_t* bad, crnStream s);
int crn_eval_labels_cpu(const float* scores, const int32_t* gt, const int32_t* scene_class, int B, int C, int K, int D, int H,
                        int W, int m, int n, int32_t* labels, int64_t* cm, int32_t* bad, int num_threads);

/* Score-level evaluation epilogue (corenet_amd.score_metrics; csrc/eval_scores.hip, host twin csrc/eval_scores_cpu.cpp,
 * shared arithmetic csrc/eval_scores_common.h): ONE native pass of an x m inference, as in
 * crn_eval_labels (same pairing of coarse voxel (b, z, y, x) with fine voxel (b, z*m+iz, y*m+iy, x*m+ix), pass
 * n = (iz*m + iy)*m + ix), binned by score into a small per-class table from which reliability diagrams, calibration
 * errors, the Brier score, threshold sweeps and average precision follow exactly.
 *   scores  f32 [B][C][D][H][W]: a pmf, or with from_logits != 0 logits that go through the shared softmax first
 *           (es_softmax: first maximum over c, e_c = es_exp(x_c - max), sum in channel order, one IEEE division per
 *           channel, a quotient below FLT_MIN is 0, a NaN is the canonical quiet NaN; es_exp is built from +, *,
 *           comparisons and integer bit operations only and both builds compile with -ffp-contract=off, so kernel
 *           and twin agree to the bit)
 *   gt      int32 [B][mD][mH][mW]; s = scene_class ? scene_class[b] : 1, g = gt * s (crn_eval_labels' scaling)
 *   A voxel is BAD -- bad[0] += 1, counted nowhere else -- when s < 1, g is outside [0, K), (C-1)*s >= K, or any p_c
 *   is NaN or outside [0, 1].  Otherwise every channel c makes one entry: row r = c*s, y = (g == r),
 *   q = (int)rintf(p_c * 2^24) (exact), bin = min(nbins-1, (q*nbins) >> 24) in 64-bit integers; and one more entry goes
 *   to row K, the class-agnostic foreground: q = 2^24 - q(p_0), y = (g != 0).  An entry adds 1 and q to
 *   table[r][bin][y][0..1] and (e16*e16 + 128) >> 8 to sq[r][y], e = y ? 2^24 - q : q, e16 = (e + 128) >> 8 (the squared
 *   error in units of 2^-24; e is rounded to 16 bits first, so a voxel's term is within e * 2^-16 + 2^-25 of exact, to
 *   either side).
 *   table int64 [K+1][nbins][2][2], sq int64 [K+1][2] and bad int64 [1] are ACCUMULATED.  Every sum is an integer sum:
 *   the same inputs give the same bits on every run, on the GPU and on the twin, whatever crn_set_deterministic says.
 *   A row holds 2^39 voxels before a sum of q can wrap; the calls do not check that.
 * 1 <= C <= CRN_EVAL_MAX_CLASSES, 1 <= K <= CRN_EVAL_MAX_BINS, 1 <= nbins <= CRN_SCORE_MAX_NBINS,
 * (K+1)*nbins <= CRN_SCORE_MAX_ENTRIES, crn_eval_labels' rules for B, D, H, W, m, n and the byte sizes (the GPU call:
 * B <= 65535 and D*H*W below 2^24 chunks of CRN_SCORE_CHUNK voxels), every pointer but scene_class given: anything else
 * returns CRN_EINVAL, launches nothing and writes nothing.  The GPU call does not wait for the GPU; the twin takes HOST
 * memory.  crn_score_softmax(_cpu) writes es_softmax of logits [B][C][S] to out of the same shape (1 <= C <=
 * CRN_EVAL_MAX_CLASSES, B, S >= 1, sizes within int64).  crn_eval_scores_tiles writes (CRN_SCORE_CHUNK,
 * CRN_SCORE_MAX_ENTRIES, CRN_SCORE_MAX_NBINS).                                                                        */
#define CRN_SCORE_MAX_ENTRIES 2048
#define CRN_SCORE_MAX_NBINS 256
#define CRN_SCORE_CHUNK 8192
int crn_eval_scores_tiles(int32_t* out3);
int crn_eval_scores(const float* scores, int from_logits, const int32_t* gt, const int32_t* scene_class, int B, int C, int K,
                    int D, int H, int W, int m, int n, int nbins, int64_t* table, int64_t* sq, int64_t* bad, crnStream s);
int crn_eval_scores_cpu(const float* scores, int from_logits, const int32_t* gt, const int32_t* scene_class, int B, int C,
                        int K, int D, int H, int W, int m, int n, int nbins, int64_t* table, int64_t* sq, int64_t* bad,
                        int num_threads);
int crn_score_softmax(const float* logits, int B, int C, int64_t S, float* out, crnStream s);
int crn_score_softmax_cpu(const float* logits, int B, int C, int64_t S, float* out, int num_threads);

/* ---------------- optimizer --------------------------------------------------
 * torch.optim.Adam step (state.py:65; train hot loop pipeline.py:230) on a flat
 * fp32 parameter slab.  grad_scale multiplies the gradient first (1/world).   */
int crn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t n, float lr, float beta1, float beta2, float eps,
                  float grad_scale, int step, crnStream s);
/* The same step with its scalars read from device memory, for HIP-graph capture of the training step
 * (the replayed launch carries no per-step host value): hyper = 7 floats written by crn_adam_set_hyper
 * (lr, beta1, beta2, eps, grad_scale, 1 - beta1^step, sqrt(1 - beta2^step)) with an ordinary launch
 * ordered before the graph replay.                                                                     */
int crn_adam_set_hyper(float* hyper, float lr, float beta1, float beta2, float eps, float grad_scale,
                       int step, crnStream s);
int crn_adam_step_hyper(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        int64_t n, const float* hyper, crnStream s);

/* Decoder stage_6.t1 -- ConvTranspose3d(16 -> Cout <= 16, k 7, stride 2, padding 3, output_padding 1), the layer that writes the
 * logits (model/reconstruction_decoder.py:89-95) -- on its own parity-walk kernels of the split-bf16 MFMA engine
 * (csrc/convt_par.hip): the input patch of a 4 x 8 x 16 tile stays in LDS while the workgroup walks the 8 output parities over
 * exactly the window rows that hold weights.  Same arithmetic as crn_conv_fwd_bf3 on the layer's window-correlation form.
 * wimg: the weights as a step-ordered image of bf16 hi / lo entries, built by crn_bf3_gather_image from any fp32 array that
 * holds the reference weight [16][Cout][7][7][7] (e.g. the flat parameter slab) through a device table of int32 [n][10] rows
 * (8 source indices, -1 = zero; destination entry of the hi part; of the lo part: corenet_amd/model/conv_geometry.py
 * convt_par_fwd_table / convt_par_dgrad_table).
 * fwd:   x [B][16][D][H][W] (dense inside a sample, batch stride x_sB) with the input transform tr -> y [B][..][2D][2H][2W]
 *        channels [0, Cout) (+ bias[n]), strides y_sB / y_sC.  D % 4 == H % 8 == W % 16 == 0.
 * dgrad: dy [B][..][2D][2H][2W] channels [0, Cout) -> dx [B][16][D][H][W] (accumulate: dx +=).                              */
int crn_bf3_gather_image(const float* src, const int32_t* table, int n_entries, void* dst, crnStream s);
int crn_convt_s2k7_fwd_bf3(const float* x, int64_t x_sB, int B, int D, int H, int W, const crnInTransform* tr,
                           const void* wimg, const float* bias, float* y, int64_t y_sB, int64_t y_sC, int Cout, crnStream s);
int crn_convt_s2k7_dgrad_bf3(const float* dy, int64_t dy_sB, int64_t dy_sC, int Cout, int B, int D, int H, int W,
                             const void* wimg, float* dx, int64_t dx_sB, int accumulate, crnStream s);
/* The same two operations for exactly 2 classes (h7), where 8 parities x 2 classes are one 16-column block and the layer's
 * weights (64 KB as bf16 hi / lo) stay resident in LDS: one persistent workgroup per CU walks its tiles (convt_res_kernel).
 * Images: conv_geometry.convt_res_fwd_table / convt_res_dgrad_table.                                                     */
int crn_convt_s2k7_c2_fwd_bf3(const float* x, int64_t x_sB, int B, int D, int H, int W, const crnInTransform* tr,
                              const void* wimg, const float* bias, float* y, int64_t y_sB, int64_t y_sC, int Cout, crnStream s);
int crn_convt_s2k7_c2_dgrad_bf3(const float* dy, int64_t dy_sB, int64_t dy_sC, int Cout, int B, int D, int H, int W,
                                const void* wimg, float* dx, int64_t dx_sB, int accumulate, crnStream s);
/* wgrad of the same layer (autograd of reconstruction_decoder.py:89-95): dw += sum over (b, q) of T(x)[b, c, q + z - 1] *
 * dy[b, n, 2 q + r] into the layer's PACKED gradient [16][64 window taps][Npad] (parity-major columns: the layout crn_conv_wgrad
 * writes for the window-correlation form, conv_geometry.convt_fwd), partial sums over position slices added with atomics;
 * zero_first clears dw.  D % 2 == H % 8 == W % 16 == 0.  Returns CRN_EINVAL in deterministic mode (crn_set_deterministic):
 * the caller then takes crn_conv_wgrad_bf3_boxes, whose unsplit form has a fixed order.
 * ximg (may be NULL): the operand image of T(x) left by crn_convt_s2k7_ximage for the same x and tr -- the workgroups then copy
 * their patches from it instead of transforming and splitting x themselves (same operands bit for bit, same result).     */
int crn_convt_s2k7_wgrad_bf3(const float* x, int64_t x_sB, int B, int D, int H, int W, const crnInTransform* tr,
                             const float* dy, int64_t dy_sB, int64_t dy_sC, int Cout, float* dw, int Npad, int zero_first,
                             const void* ximg, crnStream s);
/* Operand image of that layer's input for the weight gradient: img[b][chunk * 2 + (hi, lo)][D * H * W] entries of 8 bf16 = the
 * split-bf16 halves of T(x)[b, chunk * 8 .. + 7, position] (T = the BatchRenorm + ReLU in front of the layer,
 * reconstruction_decoder.py:56-60, 89-95).  One pass: x read once, crn_convt_s2k7_ximage_bytes(B, D, H, W) written.     */
size_t crn_convt_s2k7_ximage_bytes(int B, int D, int H, int W);
int crn_convt_s2k7_ximage(const float* x, int64_t x_sB, int B, int D, int H, int W, const crnInTransform* tr,
                          void* img, size_t img_bytes, crnStream s);

/* ---------------- ground-truth side -------------------------------------------
 * fill_inside_voxels_gpu (cc/fill_voxels_gpu.cu:136-171, module.cc:18-29):
 * grid [N][D][H][W] of dtype (0 f32, 1 u8, 2 i32, 3 f64, 4 i64, 5 i16, 6 i8),
 * contiguous.  out may alias grid (inplace=True).  Output strictly {0,1}
 * (SURVEY Q10).  Bit-exact with the reference semantics for every input.     */
int crn_fill_voxels(const void* grid, void* out, int dtype, int N, int D, int H, int W,
                    void* workspace, size_t workspace_bytes, crnStream s);
size_t crn_fill_voxels_workspace_bytes(int N, int D, int H, int W);
/* The same operator on strided views: the reference reads `grid` and writes `result` through packed accessors
 * (cc/fill_voxels_gpu.cu:146-163), so non-contiguous tensors -- and in-place calls on them -- need no copy.
 * grid_strides / out_strides: 4 host int64 element strides (N, D, H, W), all >= 0; same workspace, same single
 * asynchronous launch, voxels move one per lane.                                                              */
int crn_fill_voxels_strided(const void* grid, const int64_t* grid_strides, void* out, const int64_t* out_strides,
                            int dtype, int N, int D, int H, int W, void* workspace, size_t workspace_bytes, crnStream s);
/* crn_fill_voxels never waits for the GPU (the reference op is asynchronous too,
 * fill_voxels_gpu.cu:158-165): ONE kernel launch per call (per 256-CU load of
 * grids); a workgroup that gives up raises a device-side flag and the last
 * workgroup to leave the launch redoes its grids.  The launch's control words
 * live in a buffer owned by the library, keyed by `workspace`: the first call
 * with a new workspace allocates it (not capturable), later calls are.        */

/* fill_inside_voxels_cpu (cc/module.cc:24-29, cc/fill_voxels_cpu.cc:158-183):
 * HOST memory in and out (out may alias grid), same dtype codes.  Reference CPU
 * semantics (fill_voxels_cpu.cc:150-154): voxels outside the empty
 * region connected to the x==0 / y==0 / z==0 faces become 1, every other voxel
 * keeps its input value (the GPU op writes strict {0,1}).  Grids are processed
 * by num_threads host threads (<= 0: all hardware threads).                    */
int crn_fill_voxels_cpu(const void* grid, void* out, int dtype, int N, int D, int H, int W,
                        int num_threads);

/* ---------------- marching cubes (corenet_amd.visualization) -----------------
 * Surface of level `level` (> 0) of N independent float32 objects grid[n][d][h][w] (element strides[0..2] arbitrary,
 * strides[3] must be 1), each padded by one zero voxel; indexed mesh in the padded index space, (x, y, z) = (w, h, d),
 * sample grid[n, d, h, w] at (w + 1, h + 1, d + 1).  Contract (corner classification f > level, vertex formula,
 * normals, table, output order): corenet_amd/visualization/marching_cubes.py and DESIGN section 13.
 * Outputs: vertices / normals [V][3] f32, faces [F][3] int32 (vertex ids local to the object), objects in order.
 * At most CRN_MC_MAX_OBJECT_CELLS cells ((D + 1)(H + 1)(W + 1)) per object: object-local vertex ids stay in int32.
 *
 * GPU, two calls on stream s: crn_marching_cubes_count writes counts[n] = (num_vertices, num_faces) (DEVICE int64
 * [N][2]) and keeps the scanned offsets in `workspace` (crn_marching_cubes_workspace_bytes(N, D, H, W)); after the
 * caller has sized the outputs from counts, crn_marching_cubes_emit with the same grid and workspace writes them.
 * Neither waits for the GPU.  matrices: NULL or DEVICE f32 [N][4][4] applied in emit (positions as points with the
 * homogeneous divide, normals as vectors, not renormalised).                                                      */
#define CRN_MC_MAX_OBJECT_CELLS ((int64_t)1 << 29)
size_t crn_marching_cubes_workspace_bytes(int N, int D, int H, int W);
int crn_marching_cubes_count(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                             void* workspace, size_t workspace_bytes, int64_t* counts, crnStream s);
int crn_marching_cubes_emit(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                            const float* matrices, void* workspace, size_t workspace_bytes, float* vertices,
                            float* normals, int32_t* faces, crnStream s);
/* k^3 box mean with zero padding [(k-1)/2, k-1-(k-1)/2] per axis (MarchingCubesArtifact's filter_kernel): in with
 * element strides[4] (N, D, H, W), out contiguous [N][D][H][W] (must not alias in); separable, w then h then d, each
 * tap sum in ascending order, the last pass times 1/k^3.  workspace: N*D*H*W floats.                              */
int crn_box_filter(const float* in, const int64_t* strides, float* out, int N, int D, int H, int W, int k,
                   void* workspace, size_t workspace_bytes, crnStream s);
/* Host twins (HOST memory, same contract and bit-identical results).  crn_marching_cubes_cpu with vertices == NULL
 * writes counts[N][2]; with vertices != NULL it reads those counts and writes the mesh.  num_threads <= 0: all. */
int crn_marching_cubes_cpu(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                           const float* matrices, int64_t* counts, float* vertices, float* normals, int32_t* faces,
                           int num_threads);
int crn_box_filter_cpu(const float* in, const int64_t* strides, float* out, int N, int D, int H, int W, int k,
                       int num_threads);

/* ---------------- rendering (corenet_amd.visualization.render) -----------------
 * Batched software renderer of triangle soups: I images of H x W, uint8 RGB out[I][H][W][3], row 0 = NDC y = -1.
 * Image i draws triangles [t0, t1) of the shared buffers triangles [T][3][3] (world space), normals [T][3][3]
 * (normal_mode 1: per vertex; 2: flat, normals[t][0]; 0: unused, the geometric normal) and material_ids [T] into
 * materials [M][10] (ambient 3, diffuse 3, specular 3, shininess; an id outside [0, M) shades black).  Coverage, depth
 * and shading rules: corenet_amd/visualization/render.py and DESIGN section 14.  The winner of a pixel is decided by
 * (depth, triangle index) alone, so the result does not depend on execution order; GPU and host twin give identical
 * images when no material has a nonzero specular term (powf may differ by one level otherwise).
 * inst0: the image's first setup record; images' records are consecutive, inst0 = sum of the earlier (t1 - t0).     */
#define CRN_RENDER_TILE 16
typedef struct {
  float vp[16];              /* view-projection, row major, clip = vp . (p, 1) */
  float light[3], cam[3], light_color[3], ambient_light[3], clear[3];
  int32_t cull, normal_mode, t0, t1, inst0, pad[4];
} crnRenderImage;
/* GPU, two calls on stream s.  crn_render_bin: setup records [num_inst][16] f32, per-(image, tile) triangle counts
 * bin_counts int32 [I * tiles] and their exclusive scan bin_offsets int64 [I * tiles + 1] (tiles = ceil(H / 16) *
 * ceil(W / 16)); the caller reads bin_offsets[I * tiles] and sizes bin_list int32 with it.  crn_render_raster with the
 * same images, records and bins fills the lists (consuming bin_counts) and writes out.  images: DEVICE
 * crnRenderImage[I]; max_len = max (t1 - t0).  Neither waits for the GPU.                                        */
int crn_render_bin(const float* triangles, const crnRenderImage* images, int I, int H, int W, int max_len,
                   int64_t num_inst, float* records, int32_t* bin_counts, int64_t* bin_offsets, crnStream s);
int crn_render_raster(const float* triangles, const float* normals, const int32_t* material_ids, const float* materials,
                      int M, const crnRenderImage* images, int I, int H, int W, int max_len, const float* records,
                      int32_t* bin_counts, const int64_t* bin_offsets, int32_t* bin_list, uint8_t* out, crnStream s);
/* Host twin (HOST memory): same contract, one image per task. */
int crn_render_cpu(const float* triangles, const float* normals, const int32_t* material_ids, const float* materials,
                   int M, const crnRenderImage* images, int I, int H, int W, uint8_t* out, int num_threads);
/* Diffuse textures: crn_render_raster / crn_render_cpu plus texcoords f32 [T][3][2] (NULL: all zero), texture_ids int32
 * [M] (NULL: no material is textured) and textures uint8 [L][Ht][Wt][4] (RGBA8, 4-byte aligned, alpha ignored, row 0 is
 * t = 0; NULL: none).  Material m is textured iff 0 <= texture_ids[m] < L; its diffuse colour is then multiplied by the
 * bilinear, repeat-wrapped fetch at the perspective-correct (s, t) of the pixel (the rule: csrc/render_common.h, DESIGN
 * section 14); only the winning fragment of a pixel samples.  With textures given, L, Ht, Wt must be in [1, 2^14]
 * (CRN_EINVAL otherwise); without textures or texture_ids the calls are crn_render_raster / crn_render_cpu.          */
int crn_render_raster_tex(const float* triangles, const float* normals, const int32_t* material_ids,
                          const float* materials, int M, const crnRenderImage* images, int I, int H, int W, int max_len,
                          const float* records, int32_t* bin_counts, const int64_t* bin_offsets, int32_t* bin_list,
                          uint8_t* out, const float* texcoords, const int32_t* texture_ids, const uint8_t* textures,
                          int L, int Ht, int Wt, crnStream s);
int crn_render_cpu_tex(const float* triangles, const float* normals, const int32_t* material_ids, const float* materials,
                       int M, const crnRenderImage* images, int I, int H, int W, uint8_t* out,
                       const float* texcoords, const int32_t* texture_ids, const uint8_t* textures, int L, int Ht, int Wt,
                       int num_threads);
/* Geometry buffers: what the raster stage decides per pixel, instead of a colour.  crn_render_raster_geometry follows
 * crn_render_bin exactly as crn_render_raster does (same images, records and bins; it consumes bin_counts and does not
 * wait for the GPU).  Four outputs, each NULL or contiguous [I][H][W] (barycentrics [I][H][W][3]); at least one must be
 * given (CRN_EINVAL otherwise):
 *   triangle_index  the index t into `triangles` of the pixel's winner, t0 + (record id - inst0) -- not the record id;
 *                   -1 where no fragment survives.  The winner is the colour renderer's: coverage with the top-left
 *                   rule, z_ndc in [-1, 1], the smallest z, the later triangle on equal z, culling per image.
 *   barycentrics    b_i = E_i / ((E0 + E1) + E2), the perspective-correct weights the shader interpolates position and
 *                   texture coordinates with; 0 on background.
 *   z_ndc           the very float that decided the winner; +inf on background.
 *   depth           the clip-space w of the fragment, ((E0 w0 + E1 w1) + E2 w2) / ((E0 + E1) + E2) with w_k the fourth
 *                   component of vp . (p_k, 1); +inf on background.  For a projection whose last row is (0, 0, 1, 0)
 *                   after the view transform (transformations.perspective_lh, the dataset's camera_transform) this is
 *                   the distance along the view axis.
 * Of crnRenderImage only vp, cull, t0, t1 and inst0 are read; lights, clear colour and normal_mode are ignored.  One
 * copy of the arithmetic (csrc/render_common.h, rd_geometry), compiled without contraction: the GPU and the host twin
 * agree bit for bit on all four outputs.  DESIGN section 21.                                                        */
int crn_render_raster_geometry(const float* triangles, const crnRenderImage* images, int I, int H, int W, int max_len,
                               const float* records, int32_t* bin_counts, const int64_t* bin_offsets, int32_t* bin_list,
                               int32_t* triangle_index, float* barycentrics, float* depth, float* z_ndc, crnStream s);
int crn_render_cpu_geometry(const float* triangles, const crnRenderImage* images, int I, int H, int W,
                            int32_t* triangle_index, float* barycentrics, float* depth, float* z_ndc, int num_threads);
/* Exposed faces of N label grids labels[n][d][h][w] (int32, contiguous) as the voxel renderer draws them: voxel
 * (x, y, z) = (w, h, d) is a unit cube iff palette[label] (f32 [P][3]) exists and has no negative channel; of its faces
 * +x, -x, +y, -y, +z, -z only those whose neighbour is not drawn (or outside) are emitted, each as two triangles.
 * Order: grid, voxel raster order, face order.  count: counts[n] (DEVICE int64 [N]) = triangles of grid n; with
 * box_matrices (f32 [N][16]) box_out[n] (f32 [N][6], min xyz then max xyz) = bounds of the transformed centres of the
 * voxels with label != 0 (zeros when there are none).  emit: triangles [T][3][3] through matrices[n] (f32 [N][16],
 * voxel -> view, no divide), normals [T][3][3] (the flat normal three times), material_ids [T] = material_base + label.
 * workspace: crn_voxel_faces_workspace_bytes(N, D, H, W), kept between count and emit.                            */
size_t crn_voxel_faces_workspace_bytes(int N, int D, int H, int W);
int crn_voxel_faces_count(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                          const float* box_matrices, float* box_out, void* workspace, size_t workspace_bytes,
                          int64_t* counts, crnStream s);
int crn_voxel_faces_emit(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                         const float* matrices, int material_base, void* workspace, size_t workspace_bytes,
                         float* triangles, float* normals, int32_t* material_ids, crnStream s);
/* Host twin: triangles == NULL -> counts (and box_out); else reads counts and writes the faces. */
int crn_voxel_faces_cpu(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                        const float* box_matrices, float* box_out, const float* matrices, int material_base,
                        int64_t* counts, float* triangles, float* normals, int32_t* material_ids, int num_threads);

/* ---------------- surface points and nearest neighbours (corenet_amd.mesh_metrics) -----------------
 * Objects are ragged and described by int64 offsets [N + 1] (CSR, non-decreasing, offsets[0] >= 0); an object may be
 * empty.  Arithmetic: csrc/point_metrics_common.h; rules: corenet_amd/mesh_metrics.py and DESIGN section 15.
 *
 * crn_sample_surface: S area-stratified samples of every object of the triangle soup triangles [T][3][3]; object n owns
 * triangles [tri_offsets[n], tri_offsets[n + 1]).  points f32 [N][S][3], tri_index int32 [N][S] (local to the object),
 * valid uint8 [N]: 0 when the object has no triangle of positive finite area (its points are 0, its indices -1).  A
 * triangle's weight is round(area / largest area of the object * 2^24), an integer; sample i takes the triangle whose
 * interval of the running integer sum contains floor((i + u_i) / S * total), then a point by the square-root warp of two
 * more uniforms; the uniforms are a hash of (seed, i, 0 / 1 / 2).  A row depends only on (the object's triangles, S, seed).
 * workspace: crn_sample_surface_workspace_bytes(T, N).  tri_offsets: DEVICE memory for the GPU call.
 *
 * crn_nearest: for query q of object n (a [Na][3], a_offsets) the candidate of object n (b [Nb][3], b_offsets) with the
 * smallest (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction; a candidate whose d2 is NaN is
 * never chosen; no eligible candidate: +inf and -1.  dist2 f32 [Na], index int32 [Na] (local to the object).
 * max_na / max_nb: the largest number of queries / candidates of one object (they size the launch; the offsets stay on
 * the device).  workspace: crn_nearest_workspace_bytes(Na) (64-bit keys for launches that split the candidates of an
 * object over several workgroups and merge with atomicMin on (bits(d2) << 32) | index: commutative, so deterministic).
 * Neither call waits for the GPU.  The host twins take HOST memory and run one object per task.                    */
#define CRN_PM_MAX_SAMPLES 2147483647LL
#define CRN_PM_MAX_CANDIDATES 2147483647LL
size_t crn_sample_surface_workspace_bytes(int64_t T, int N);
int crn_sample_surface(const float* triangles, const int64_t* tri_offsets, int N, int64_t T, int64_t S, uint32_t seed,
                       void* workspace, size_t workspace_bytes, float* points, int32_t* tri_index, uint8_t* valid,
                       crnStream s);
int crn_sample_surface_cpu(const float* triangles, const int64_t* tri_offsets, int N, int64_t S, uint32_t seed,
                           float* points, int32_t* tri_index, uint8_t* valid, int num_threads);
size_t crn_nearest_workspace_bytes(int64_t Na);
int crn_nearest(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int N, int64_t Na,
                int64_t max_na, int64_t max_nb, void* workspace, size_t workspace_bytes, float* dist2, int32_t* index,
                crnStream s);
int crn_nearest_cpu(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int N,
                    float* dist2, int32_t* index, int num_threads);

/* crn_point_triangle: for query q of object n (p [Np][3], p_offsets) the triangle of object n
 * (triangles [T][3][3], t_offsets) with the smallest (d2, index), d2 the squared Euclidean distance from the query to the
 * closed triangle in float32.  dist2 f32 [Np], index int32 [Np] (local to the object).
 *   eligible   a triangle is a candidate when pm_area_ok(pm_area(triangle)) holds (the sampler's rule: positive finite
 *              area); zero-area, collinear, NaN and infinite triangles are never chosen.
 *   no winner  a candidate is chosen only when its d2 is below +inf: a NaN d2 is never chosen, nor one that overflows
 *              float32.  A query without such a candidate (an empty object, no eligible triangle, a NaN query) gets +inf
 *              and -1.
 *   ties       to the lowest index (ascending candidates, strict <).
 *   arithmetic pm_tri_record / pm_tri_d2 of csrc/point_metrics_common.h, once, for the kernel and the host twin, without
 *              contraction: both return the same dist2 and index bit for bit.  A triangle becomes a record of 20 floats
 *              (an orthonormal frame at A, the edges' unit directions and lengths in it; a pre-pass on the GPU); the
 *              pair routine is z^2 plus the squared in-plane distance (0 inside, else the smallest of three clamped edge
 *              distances), selects only.
 * max_np / max_nt: the largest number of queries / triangles of one object (max_nt <= CRN_PM_MAX_CANDIDATES); they size
 * the launch, the offsets stay on the device.  workspace: crn_point_triangle_workspace_bytes(Np, T) (the records, and
 * 64-bit keys for launches that split the triangles of an object over crn_point_triangle_splits(N, max_np, max_nt) > 1
 * workgroups and merge with atomicMin, as crn_nearest).  A workgroup holds CRN_PT_QUERY_TILE queries and walks tiles of
 * CRN_PT_TRIANGLE_TILE records; shares are whole tiles.  crn_point_triangle_tile(0 / 1) returns the query / triangle
 * tile the library was built with (anything else: 0).  The call does not wait for the GPU.                           */
#define CRN_PT_QUERY_TILE 1024
#define CRN_PT_TRIANGLE_TILE 256
size_t crn_point_triangle_tile(int which);
size_t crn_point_triangle_workspace_bytes(int64_t Np, int64_t T);
size_t crn_point_triangle_splits(int N, int64_t max_np, int64_t max_nt);
int crn_point_triangle(const float* p, const int64_t* p_offsets, const float* triangles, const int64_t* t_offsets,
                       int N, int64_t Np, int64_t T, int64_t max_np, int64_t max_nt,
                       void* workspace, size_t workspace_bytes, float* dist2, int32_t* index, crnStream s);
int crn_point_triangle_cpu(const float* p, const int64_t* p_offsets, const float* triangles, const int64_t* t_offsets,
                           int N, float* dist2, int32_t* index, int num_threads);

/* ---------------- voxel components (corenet_amd.voxel_components) -----------------
 * Connected-component labelling of N independent grids grid[n][d][h][w] (element strides[0..2] arbitrary and >= 0,
 * strides[3] must be 1; dtype 1 = uint8, 2 = int32, the codes of crn_fill_voxels).  Contract: DESIGN section 17.
 *   foreground    value > 0.
 *   connectivity  6 (faces), 18 (+ edges) or 26 (+ corners); by_value != 0: two neighbouring foreground voxels belong
 *                 together only if their values are equal, by_value == 0: always.
 *   labels        int32 [N][D][H][W] contiguous: 0 on background, the components of grid n numbered 1 .. K_n in ascending
 *                 order of their lowest linear index d*H*W + h*W + w (for binary input scipy.ndimage.label's numbering).
 *                 D*H*W <= 2^31 - 1 (labels and parents are 32-bit per grid).  num_components: int64 [N].
 * The result is a function of the partition alone: identical from run to run and between the kernels and the host twin.
 *
 * GPU: crn_voxel_components queues six launches on stream s and does not wait for the GPU; no workgroup waits for
 * another one (bricks of CRN_VC_BRICK_D x _H x _W voxels labelled in LDS, seams united with atomicMin on a global parent
 * array, raster-order numbering by a chunked prefix sum).  workspace: crn_voxel_components_workspace_bytes(N, D, H, W)
 * (the parents and the chunk counts).  N <= 65535.  crn_voxel_components_bricks writes the three brick extents.
 *
 * crn_component_stats: for component c = offsets[n] + label - 1 of grid n (offsets int64 [N + 1], the exclusive prefix
 * sum of num_components; DEVICE memory for the GPU call; K = offsets[N]): size int64 [K] voxels, bbox int32 [K][6]
 * (d0, h0, w0, d1, h1, w1) with exclusive upper bounds, first int64 [K] the lowest linear index, and, when grid is not
 * NULL, value int32 [K] the grid's value at `first` (grid NULL: strides, dtype and value are not looked at).  Integer
 * atomics: order-independent.  Labels outside 1 .. K_n are ignored.
 *
 * Host twins (HOST memory, same contract, identical results): a two-pass union-find over the whole grid, one grid per
 * thread; num_threads <= 0: all.                                                                                    */
#define CRN_VC_BRICK_D 8
#define CRN_VC_BRICK_H 16
#define CRN_VC_BRICK_W 64
int crn_voxel_components_bricks(int32_t* out3);
size_t crn_voxel_components_workspace_bytes(int N, int D, int H, int W);
int crn_voxel_components(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int connectivity,
                         int by_value, void* workspace, size_t workspace_bytes, int32_t* labels, int64_t* num_components,
                         crnStream s);
int crn_component_stats(const int32_t* labels, const void* grid, const int64_t* strides, int dtype, int N, int D, int H,
                        int W, const int64_t* offsets, int64_t K, int64_t* size, int32_t* bbox, int64_t* first,
                        int32_t* value, crnStream s);
int crn_voxel_components_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                             int connectivity, int by_value, int32_t* labels, int64_t* num_components, int num_threads);
int crn_component_stats_cpu(const int32_t* labels, const void* grid, const int64_t* strides, int dtype, int N, int D,
                            int H, int W, const int64_t* offsets, int64_t K, int64_t* size, int32_t* bbox,
                            int64_t* first, int32_t* value, int num_threads);

/* ---------------- voxel distances (corenet_amd.voxel_distance) -----------------
 * Exact squared Euclidean distance transform of N independent grids grid[n][d][h][w] (strides and dtype as for
 * crn_voxel_components).  Contract: DESIGN section 18.
 *   mode    the target set T of a grid: CRN_VD_FOREGROUND the voxels with value > 0, CRN_VD_BACKGROUND all others,
 *           CRN_VD_SURFACE the foreground voxels with one of their 6 neighbours not foreground or outside the grid.
 *   d2      int32 [N][D][H][W] contiguous: min over u in T of |v - u|^2 in voxel units, an exact integer.
 *   index   NULL, or int32 [N][D][H][W] contiguous: the per-grid linear index d*H*W + h*W + w of the u that attains it,
 *           DEFINED by the separable recurrence: (1) the nearest target of the same row, ties to the lower w;
 *           (2) argmin_j g1[j] + (i - j)^2 over the column along h, ties to the lower j, the winner keeps row j's w;
 *           (3) the same along d.  The value is the true 3-D minimum; the index does not depend on scheduling.
 *   A grid with empty T: d2 = CRN_VD_NO_TARGET, index = -1 everywhere.
 * CRN_EINVAL: an empty extent (N == 0 is valid and does nothing), D*H*W > 2^31 - 1, or
 * (D-1)^2 + (H-1)^2 + (W-1)^2 >= 2^31 - 1.  Nothing depends on crn_set_deterministic.
 *
 * GPU: crn_voxel_distance queues a row pass and one line pass per axis h, d longer than 1 on stream s and does not wait
 * for the GPU; no workgroup waits for another one.  A line pass stages whole lines of up to CRN_VD_LINE_CAP elements x
 * 64 columns in LDS and keeps CRN_VD_LINE_R outputs per lane in registers; with the index it packs (value << bits) | j
 * into one word where (bound + 1) << bits <= 2^CRN_VD_PACK_BITS (bound: the largest value the pass can produce, the sum
 * of the squared extents - 1 up to its axis; bits = ceil(log2(line length))), else it compares and selects; longer lines
 * are read from a copy in global memory.  crn_voxel_distance_tiles writes those three constants.  workspace:
 * crn_voxel_distance_workspace_bytes(N, D, H, W, want_index) -- the second index buffer, and the copy for lines beyond
 * the capacity; it may be 0, and workspace NULL then.
 *
 * Host twin (HOST memory, same contract, identical results): one grid per thread; num_threads <= 0: all.          */
#define CRN_VD_FOREGROUND 0
#define CRN_VD_BACKGROUND 1
#define CRN_VD_SURFACE 2
#define CRN_VD_NO_TARGET 2147483647
#define CRN_VD_LINE_R 16
#define CRN_VD_LINE_CAP 512
#define CRN_VD_PACK_BITS 31
int crn_voxel_distance_tiles(int32_t* out3);
size_t crn_voxel_distance_workspace_bytes(int N, int D, int H, int W, int want_index);
int crn_voxel_distance(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int mode,
                       void* workspace, size_t workspace_bytes, int32_t* d2, int32_t* index, crnStream s);
int crn_voxel_distance_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int mode,
                           int32_t* d2, int32_t* index, int num_threads);

/* ---------------- voxel visibility (corenet_amd.voxel_visibility) -----------------
 * Which voxels of N independent grids grid[n][d][h][w] (strides and dtype as for crn_voxel_components; occupied iff
 * value > 0) an eye can see.  Contract: DESIGN section 19.  Space is measured in 1 / CRN_VV_SUBDIVISIONS of a voxel:
 * voxel (x, y, z) = index [z][y][x] is the cube [256x, 256x + 256] x [256y, ..] x [256z, ..] with centre
 * (256x + 128, 256y + 128, 256z + 128).
 *   eye_q       int32 [N][3] in HOST memory (both entries): the eye (x, y, z) of every grid in those units.
 *   occluded    uint8 [N][D][H][W] contiguous: 1 iff an occupied voxel u != v has its open interior met by the open
 *               segment from the centre of v to the eye (the traversed voxels of v); v's own value does not matter.
 *   first       NULL, or int32 [N][D][H][W] contiguous: the per-grid linear index z*H*W + y*W + x of the occupied
 *               traversed voxel nearest the eye, -1 where there is none.
 * The traversed voxels are DEFINED by the integer walk of DESIGN section 19 (three 64-bit face-crossing terms; all
 * axes whose term equals the minimum step together), which both entries run, so results are identical bit for bit.
 * CRN_EINVAL: an empty extent (N == 0 is valid and does nothing), an extent above CRN_VV_MAX_EXTENT, an eye
 * coordinate beyond +-CRN_VV_MAX_EYE, a flag the entry does not know.  Then every term of the walk stays below 2^61.
 *   flags       CRN_VV_FLAT (GPU): read the fine occupancy bits only (below).  CRN_VV_COUNT_STEPS (host twin only, needs
 *               first): first receives the trip count of every voxel's walk to the grid boundary or the eye instead.
 *
 * GPU: crn_voxel_visibility queues a memset, a pack pass and one walk launch per 64 grids on stream s and does not
 * wait for the GPU (the eyes travel as kernel arguments); no workgroup waits for another one.  The pack pass writes one
 * occupancy bit per voxel (a 64-bit word per 64 voxels of a row) and ORs one bit per brick of CRN_VV_BRICK^3 voxels
 * into a coarse map; the walk pass stages a grid's coarse map in LDS and reads a fine word only inside an occupied
 * brick.  A coarse map beyond CRN_VV_COARSE_CAP_BYTES, or CRN_VV_FLAT, selects the flat form, which reads fine words
 * only.  crn_voxel_visibility_tiles writes (CRN_VV_BRICK, CRN_VV_COARSE_CAP_BYTES, CRN_VV_WG_WORDS: the 64-voxel
 * words a workgroup of the walk pass owns).  workspace: crn_voxel_visibility_workspace_bytes(N, D, H, W), never 0
 * for N >= 1.
 *
 * Host twin (HOST memory, same contract, identical results): the planes of all grids are spread over num_threads
 * (<= 0: all).                                                                                                    */
#define CRN_VV_SUBDIVISIONS 256
#define CRN_VV_MAX_EXTENT 2048
#define CRN_VV_MAX_EYE (1 << 19)
#define CRN_VV_FLAT 1
#define CRN_VV_COUNT_STEPS 2
#define CRN_VV_BRICK 4
#define CRN_VV_COARSE_CAP_BYTES 65536
#define CRN_VV_WG_WORDS 256
int crn_voxel_visibility_tiles(int32_t* out3);
size_t crn_voxel_visibility_workspace_bytes(int N, int D, int H, int W);
int crn_voxel_visibility(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                         const int32_t* eye_q, int flags, void* workspace, size_t workspace_bytes, uint8_t* occluded,
                         int32_t* first, crnStream s);
int crn_voxel_visibility_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                             const int32_t* eye_q, int flags, uint8_t* occluded, int32_t* first, int num_threads);

/* ---------------- label overlaps of two voxel grids (corenet_amd.voxel_overlap) -----------------
 * How many voxels carry label i in grid a[n][d][h][w] and label j in grid b[n][d][h][w], for N independent pairs of
 * grids.  Contract: DESIGN section 20.  a and b have their own dtype (1 = uint8, 2 = int32: the codes of
 * crn_voxel_components) and their own strides [4] in elements: W stride 1, N / D / H strides arbitrary (>= 0).
 * D*H*W <= 2^31 - 1.
 *   num_a, num_b   int64 [N]: the highest valid label of every grid (e.g. crn_voxel_components' num).
 *   table_offsets  int64 [N + 1] in HOST memory (both entries), ascending from 0: the table of grid n is the
 *                  (num_a[n] + 1) x (num_b[n] + 1) int64 counts, row-major (a the row), at table + table_offsets[n].
 *                  Background (label 0) is an ordinary row and column.  The call zeroes the whole buffer first.
 *   bad            int64 [N]: voxels with a < 0, a > num_a[n], b < 0 or b > num_b[n]; they are counted nowhere else
 *                  (crn_eval_labels' rule).  A grid whose num_a / num_b is negative, or whose (num_a + 1) * (num_b + 1)
 *                  is not the length table_offsets gives it, has all its voxels in bad and its table left at zero: the
 *                  kernels never write outside a grid's own table.
 * CRN_EINVAL: an empty extent (N == 0 is valid and does nothing), an unknown dtype, a W stride other than 1,
 * table_offsets that descend, a grid with more than 2^31 - 1 entries (keys are 32-bit), a GPU call whose tables
 * together exceed CRN_VO_MAX_TABLE_ENTRIES; CRN_ENOMEM: table_bytes below crn_voxel_overlap_workspace_bytes.
 * crn_voxel_overlap_workspace_bytes(N, table_offsets) is the size of the table buffer in bytes (never 0 for N >= 1; 0
 * for offsets the call would refuse): the call needs no other device memory.
 *
 * GPU: crn_voxel_overlap queues two memsets and one launch per 64 grids on stream s and does not wait for the GPU (the
 * offsets travel as kernel arguments); no workgroup waits for another one.  A workgroup owns CRN_VO_CHUNK consecutive
 * voxels of one grid, each of its waves an equal share of them.  Rows are read with 16-byte loads (4 int32 or 16 uint8
 * voxels per lane per load) between a scalar head, up to the first voxel at which both rows are 16-byte aligned, and a
 * scalar tail; rows of a and b whose alignments never agree are read with scalar loads throughout.  A lane merges equal
 * neighbouring pairs before it counts and keeps the (0, 0) and bad counts in registers, reduced once per wave.  A grid
 * with at most CRN_VO_LDS_ENTRIES entries is counted in LDS (u32 atomics) and the non-zero entries are added to the
 * table at the end (64-bit atomics); a larger table receives the merged runs directly.  Integer adds only: the result is
 * the same from run to run and equal to the host twin's; nothing depends on crn_set_deterministic.
 * crn_voxel_overlap_tiles writes (CRN_VO_CHUNK, CRN_VO_LDS_ENTRIES, CRN_VO_MAX_TABLE_ENTRIES).
 *
 * Host twin (HOST memory, same contract without the cap on the tables together, identical results): chunks of
 * CRN_VO_CHUNK voxels are spread over num_threads (<= 0: all), every thread counts into tables of its own, summed at
 * the end; tables above 2^20 entries are added to directly.                                                       */
#define CRN_VO_CHUNK 65536
#define CRN_VO_LDS_ENTRIES 16384
#define CRN_VO_MAX_TABLE_ENTRIES (1 << 26)
int crn_voxel_overlap_tiles(int32_t* out3);
size_t crn_voxel_overlap_workspace_bytes(int N, const int64_t* table_offsets);
int crn_voxel_overlap(const void* a, const int64_t* strides_a, int dtype_a, const void* b, const int64_t* strides_b,
                      int dtype_b, int N, int D, int H, int W, const int64_t* num_a, const int64_t* num_b,
                      const int64_t* table_offsets, int64_t* table, size_t table_bytes, int64_t* bad, crnStream s);
int crn_voxel_overlap_cpu(const void* a, const int64_t* strides_a, int dtype_a, const void* b, const int64_t* strides_b,
                          int dtype_b, int N, int D, int H, int W, const int64_t* num_a, const int64_t* num_b,
                          const int64_t* table_offsets, int64_t* table, int64_t* bad, int num_threads);

/* ---------------- configuration histogram of voxel grids (corenet_amd.voxel_topology) -----------------
 * How often each of the 256 possible 2x2x2 voxel configurations occurs in N independent grids grid[n][d][h][w].
 * Contract: DESIGN section 23.  Every voxel outside the grid is background.  Cell (d, h, w), 0 <= d <= D, 0 <= h <= H,
 * 0 <= w <= W, holds the voxels (d - 1 + i, h - 1 + j, w - 1 + k), i, j, k in {0, 1}; for a mask X its code is the sum
 * of X(voxel) << (4 * i + 2 * j + k): a grid has (D + 1)(H + 1)(W + 1) cells and every voxel lies in 8 of them.
 *   grid        dtype 1 = uint8, 2 = int32 (the codes of crn_voxel_components), strides [4] in elements: W stride 1,
 *               N / D / H strides arbitrary (>= 0).  D*H*W <= 2^31 - 1.
 *   num_labels  L, 0 <= L <= CRN_VT_MAX_LABELS.
 *   mask        0: a label grid -- row 0 counts the mask value != 0, row l in 1 .. L the mask value == l, and a voxel
 *               with value < 0 or value > L is counted once in bad[n] and is background everywhere else.
 *               non-zero: a mask grid -- L must be 0, row 0 counts value != 0 and bad stays 0.
 *   table       int64 [N][L + 1][256]; bin 0 of every row is the number of cells minus the row's other bins, so every
 *               row sums to (D + 1)(H + 1)(W + 1).
 *   bad         int64 [N].
 * CRN_EINVAL: an empty extent (N == 0 is valid and does nothing), an unknown dtype, a W stride other than 1, a negative
 * stride, num_labels outside its range, mask with num_labels != 0.
 *
 * GPU: crn_voxel_topology queues two memsets and, per CRN_VT_BATCH grids, one counting launch and one launch that
 * derives bin 0, on stream s, and does not wait for the GPU; no workgroup waits for another one.  A workgroup owns a brick
 * of CRN_VT_BRICK_D x bh x CRN_VT_BRICK_W cells (bh = CRN_VT_BRICK_H_I32 for int32, CRN_VT_BRICK_H_U8 for uint8 grids)
 * and reads the voxels of its cells plus one voxel in front of them on every axis: the halo is the only voxel read by two
 * workgroups.  A lane owns 16 bytes of a row (4 int32 or 16 uint8 voxels), read with one 16-byte load where the unit lies
 * inside the row and is 16-byte aligned and element by element otherwise, keeps the rows of the plane before in
 * registers while it walks along D, merges equal neighbouring (row, code) keys into runs and adds a run that ends to the
 * u32 rows in LDS; after one barrier the non-zero entries go to the table with 64-bit atomics.  Integer adds only: the
 * result is the same from run to run and equal to the host twin's; nothing depends on crn_set_deterministic.
 * crn_voxel_topology_tiles writes (CRN_VT_BRICK_D, CRN_VT_BRICK_H_I32, CRN_VT_BRICK_H_U8, CRN_VT_BRICK_W,
 * CRN_VT_MAX_LABELS, CRN_VT_BATCH).
 *
 * Host twin (HOST memory, same contract, identical results): the (grid, d) cell planes are spread over num_threads
 * (<= 0: all); every thread counts into a table of its own, summed at the end.                                    */
#define CRN_VT_BRICK_D 16
#define CRN_VT_BRICK_H_I32 32
#define CRN_VT_BRICK_H_U8 128
#define CRN_VT_BRICK_W 256
#define CRN_VT_MAX_LABELS 63
#define CRN_VT_BATCH 1024
int crn_voxel_topology_tiles(int32_t* out6);
int crn_voxel_topology(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int num_labels,
                       int mask, int64_t* table, int64_t* bad, crnStream s);
int crn_voxel_topology_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int num_labels,
                           int mask, int64_t* table, int64_t* bad, int num_threads);

/* ---------------- mesh clean-up: incidence tables, smoothing, normals, clustering (corenet_amd.mesh_ops) --------------
 * Contract: DESIGN section 24 and the docstring of corenet_amd/mesh_ops.py.  A batch of N indexed meshes: vertices f32
 * [V][3], faces int32 [F][3] with vertex ids LOCAL to their object, and the ascending offsets voff / foff int64 [N + 1]
 * (voff[0] = foff[0] = 0): object n owns the vertices voff[n] .. voff[n + 1] - 1 and the faces foff[n] .. foff[n + 1] - 1.
 * "Global" ids have voff[n] added.  V <= 2^31 - 1 and 3 F <= 2^31 - 1.  All float arithmetic is float32 with IEEE + - * /
 * sqrtf in the order written here, never contracted; the positions of the clustering are float64.  Every GPU entry
 * queues its launches on stream s and does not wait for the GPU; the prefix sums between the entries are the caller's.
 * Integer atomics, per-list sorts and sums in list order only: results are the same from run to run and equal to the host
 * twin's bit for bit; nothing depends on crn_set_deterministic.  All pointers are device memory for the GPU entries and
 * host memory for the *_cpu twins.
 *
 * A bad id is a face id < 0 or >= its object's vertex count (or a face outside foff[N], or a global id >= V).  A face
 * with a bad id is in no list, has a zero normal and is never kept; the count of bad ids is what the caller raises on.
 *
 * Incidence (mesh_topology):
 *   crn_mesh_corner_count   deg int32 [V] <- the number of face corners that name each vertex (a face that names a vertex
 *                           twice counts twice), bad int64 [1] <- the number of bad ids.  vf_offsets is the caller's
 *                           exclusive prefix sum of deg, int64 [V + 1].
 *   crn_mesh_corner_lists   vf_corners int32 [3 F] <- per vertex its corners 3 * global_face + corner, ascending;
 *                           cand int32 [6 F] <- per vertex the sorted list of 2 w + d over its corners: w the global id of
 *                           the next (d = 0, the edge v -> w) and of the previous (d = 1, the edge w -> v) vertex of the
 *                           corner's face; vvdeg int32 [V] <- the number of distinct w != v; irregular uint8 [V] <- 1 where
 *                           some w has not exactly one entry of either direction, or w == v occurs (a self edge is never
 *                           regular).  cursor int32 [V], vf_tmp int32 [3 F], cand_tmp int32 [6 F]: scratch.
 *   crn_mesh_neighbours     vv_neighbours <- per vertex the distinct w != v of cand, ascending, at vv_offsets (the caller's
 *                           exclusive prefix sum of vvdeg, int64 [V + 1]).
 * Sorting: a list of up to CRN_MESH_SORT_LANE keys is sorted by one lane; a longer one by its workgroup of
 * CRN_MESH_THREADS threads, rank by counting through LDS tiles of CRN_MESH_SORT_TILE keys (quadratic in the list).
 *
 * crn_mesh_smooth_step: vout <- one step with factor f.  A vertex with k >= 1 neighbours and fixed[v] == 0 (fixed: uint8
 * [V] or NULL) gets, per component, s = ((n0 + n1) + n2) + ... over its neighbours in list order, m = s / float(k),
 * v' = v + f * (m - v); every other vertex is copied.  vin != vout.
 *
 * crn_mesh_face_normals: out f32 [F][3] <- (b - a) x (c - a) of the corners 0, 1, 2; component x is
 * (u.y * w.z) - (u.z * w.y) with u = b - a, w = c - a, y and z cyclically.
 * crn_mesh_vertex_normals: out f32 [V][3] <- per vertex 0 + the cross products of the faces of its corner list, in list
 * order (once per corner), divided by sqrtf((x * x + y * y) + z * z); a zero length gives (0, 0, 0).
 *
 * Clustering (cluster_decimate) on a lattice of pitch cell (> 0): per axis x = v / cell, c = floorf(x),
 * u = (int64)((x - c) * 2^20); a vertex that is not finite or has a c outside [CRN_MESH_CELL_MIN, CRN_MESH_CELL_MAX] is
 * bad.  A cluster is (object, c_x, c_y, c_z); its leader is its lowest vertex id; new vertices are ordered by leader.
 *   crn_mesh_cluster_build  table_keys int64 [2^table_log2] / table_leader int32 [2^table_log2]: scratch, 2^table_log2 >=
 *                           max(2, 2 V); slot_of int32 [V]: scratch; vflag int32 [V] <- 1 for leaders; fkeep int32 [F] <- 1
 *                           for faces whose three vertices lie in three clusters; bad int64 [1] <- bad vertices + bad ids.
 *                           N <= CRN_MESH_MAX_OBJECTS, V <= CRN_MESH_CLUSTER_MAX_VERTICES.
 *   crn_mesh_cluster_emit   vcs / fcs int64 [V] / [F]: the caller's INCLUSIVE prefix sums of vflag / fkeep; new_voff int64
 *                           [N + 1]: the first new vertex of every object; vertex_map int32 [V] <- old -> new global id;
 *                           cluster_size int32 [new_V]; sums int64 [new_V][3]: scratch, the exact sums of u;
 *                           new_vertices f32 [new_V][3] <- per axis
 *                           float((double(c) + (double(sum u) / double(count)) * 2^-20) * double(cell));
 *                           new_faces int32 [new_F][3] <- the kept faces in order, ids local to their object.
 * No slot of the table shows in any output.
 *
 * CRN_EINVAL: a size outside the limits, a missing pointer, cell <= 0 or NaN, a table that is too small.
 * crn_mesh_tiles writes (CRN_MESH_THREADS, CRN_MESH_SORT_LANE, CRN_MESH_SORT_TILE, CRN_MESH_CELL_MIN, CRN_MESH_CELL_MAX,
 * CRN_MESH_MAX_OBJECTS, CRN_MESH_CLUSTER_MAX_VERTICES).
 *
 * Host twins (same contract, identical results; plain sequential loops):
 *   crn_mesh_topology_cpu   all tables of mesh_topology in one call; counts int64 [2] <- (E, bad).  With vv_neighbours
 *                           NULL only the counts, vf_* , vv_offsets and irregular are written (the sizing call).
 *   crn_mesh_cluster_cpu    counts int64 [2 N + 1] <- new vertex counts, new face counts, bad; vertex_map always; the
 *                           other outputs when new_vertices is not NULL (the second call, sized by the first).      */
#define CRN_MESH_THREADS 256
#define CRN_MESH_SORT_LANE 32
#define CRN_MESH_SORT_TILE 2048
#define CRN_MESH_CELL_MIN (-32768)
#define CRN_MESH_CELL_MAX 32767
#define CRN_MESH_MAX_OBJECTS 65534
#define CRN_MESH_CLUSTER_MAX_VERTICES (1 << 30)
int crn_mesh_tiles(int32_t* out7);
int crn_mesh_corner_count(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V, int32_t* deg,
                          int64_t* bad, crnStream s);
int crn_mesh_corner_lists(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V,
                          const int64_t* vf_offsets, int32_t* cursor, int32_t* vf_tmp, int32_t* vf_corners, int32_t* cand_tmp,
                          int32_t* cand, int32_t* vvdeg, uint8_t* irregular, crnStream s);
int crn_mesh_neighbours(const int32_t* cand, const int64_t* vf_offsets, const int64_t* vv_offsets, int64_t V, int32_t* vv_neighbours,
                        crnStream s);
int crn_mesh_smooth_step(const float* vin, float* vout, const int64_t* vv_offsets, const int32_t* vv_neighbours, const uint8_t* fixed,
                         float factor, int64_t V, crnStream s);
int crn_mesh_face_normals(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N,
                          int64_t V, float* out, crnStream s);
int crn_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, int N, int64_t V,
                            const int64_t* vf_offsets, const int32_t* vf_corners, float* out, crnStream s);
int crn_mesh_cluster_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff,
                           int N, float cell, int64_t* table_keys, int32_t* table_leader, int table_log2, int32_t* slot_of,
                           int32_t* vflag, int32_t* fkeep, int64_t* bad, crnStream s);
int crn_mesh_cluster_emit(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff,
                          int N, float cell, const int32_t* table_leader, const int32_t* slot_of, const int32_t* vflag,
                          const int64_t* vcs, const int32_t* fkeep, const int64_t* fcs, const int64_t* new_voff, int64_t new_V,
                          int64_t new_F, int32_t* vertex_map, int64_t* sums, int32_t* cluster_size, float* new_vertices,
                          int32_t* new_faces, crnStream s);
int crn_mesh_topology_cpu(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V,
                          int64_t* vf_offsets, int32_t* vf_corners, int64_t* vv_offsets, int32_t* vv_neighbours, uint8_t* irregular,
                          int64_t* counts);
int crn_mesh_smooth_step_cpu(const float* vin, float* vout, const int64_t* vv_offsets, const int32_t* vv_neighbours,
                             const uint8_t* fixed, float factor, int64_t V);
int crn_mesh_face_normals_cpu(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N,
                              int64_t V, float* out);
int crn_mesh_vertex_normals_cpu(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, int N, int64_t V,
                                const int64_t* vf_offsets, const int32_t* vf_corners, float* out);
int crn_mesh_cluster_cpu(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff,
                         int N, float cell, int32_t* vertex_map, int64_t* counts, float* new_vertices, int32_t* cluster_size,
                         int32_t* new_faces);

/* voxelize_mesh (geometry/voxelization.py:32-164 + shaders/voxelize.{geom,frag}):
 * triangles [T][3][3] (view space), tri_mesh [T] mesh index per triangle
 * (misc_util.dynamic_tile), view2voxel [M][16]; grid [M][D][H][W] (or the
 * (2D+1)(2H+1)(2W+1) sub-grid when sub_grid_side>0) is zeroed then marked.    */
int crn_voxelize_mesh(const float* triangles, const int32_t* tri_mesh, int T,
                      const float* view2voxel, int M, int D, int H, int W,
                      int sub_grid_side, float image_resolution_multiplier,
                      int conservative, int depth_multiplier, float* grid, crnStream s);
/* batch() geometry (data/batched_example.py:73-81 -> geometry/transformations.py:139-169 transform_mesh):
 * out[t][k] = (mesh_matrix[tri_mesh[t]] . (triangles[t][k], 1)).xyz / .w for the object-space triangles
 * [T][3][3] of all meshes of a batch, mesh_matrix [M][16] = view_transform . object_to_world per mesh.
 * out may alias triangles.                                                                       */
int crn_transform_meshes(const float* triangles, const int32_t* tri_mesh, int T,
                         const float* mesh_matrix, int M, float* out, crnStream s);
/* per-scene label merge (batched_example.py:186-196): out[b] = max_m label_m*grid_m
 * over the meshes [scene_mesh_start[b], scene_mesh_start[b+1]) of scene b, int32.
 * sub_grid!=0: meshes_grid is the (2D+1)(2H+1)(2W+1) grid and the sub-grid
 * centres are taken (voxelization.get_sub_grid_centers :167-182).            */
int crn_merge_labels(const float* meshes_grid, const int32_t* scene_mesh_start,
                     const int32_t* mesh_label, int B, int D, int H, int W, int sub_grid,
                     int32_t* out, crnStream s);

/* ---------------- data parallelism: RCCL from the library ------------------------
 * The reference exchanges gradients through torch's DistributedDataParallel over NCCL (pipeline.py:199-200,229) and
 * broadcasts the BatchRenorm buffers from rank 0 (DDP broadcast_buffers).  Here the exchange can be enqueued by the
 * library itself on the caller's stream (the engine's side stream, behind the un-pack of a gradient bucket):
 *   rank 0: crn_comm_unique_id(id)  ->  the host hands the 128 bytes to every rank (torch.distributed store, MPI, ...)
 *   every rank (its GPU current): crn_comm_init(id, rank, nranks, &comm)
 *   crn_allreduce_f32(comm, buf, n, stream): in-place sum over the ranks, asynchronous, stream-ordered.
 * librccl.so is opened on first use; without it these calls return CRN_EINVAL and the rest of the library works.
 * RCCL picks ring / tree / direct by message size and topology; NCCL_ALGO / NCCL_PROTO (read by RCCL at communicator
 * creation) override it -- tools/scale_probe.sh times the engine's bucket sizes under each.                        */
int crn_comm_unique_id(void* id128 /* 128 bytes, host */);
int crn_comm_init(const void* id128, int rank, int nranks, void** comm);
int crn_comm_destroy(void* comm);
int crn_comm_info(void* comm /* may be NULL */, int* rccl_version, int* rank, int* nranks);
int crn_allreduce_f32(void* comm, float* buf, int64_t n, crnStream s);
int crn_broadcast_f32(void* comm, float* buf, int64_t n, int root, crnStream s);

/* rocprofv3 markers: a roctx range around the calls that follow (one per layer and direction when the Python engine
 * runs with CRN_ROCTX=1); `rocprofv3 --kernel-trace --marker-trace` then attributes kernels to layers.  No-ops
 * (CRN_EINVAL) when no roctx library can be opened.                                                                 */
int crn_roctx_push(const char* label);
int crn_roctx_pop(void);

/* Deterministic mode (also env CRN_DETERMINISTIC=1): every floating-point sum of the library is taken in an order that
 * does not depend on how workgroups are scheduled, so two runs from the same state are bit-identical -- a debugging
 * aid (the reference gets the same from torch.use_deterministic_algorithms; its index_put_(accumulate=True) and cuDNN
 * weight gradients are atomic-order dependent too).  Default mode: weight gradients, the bias gradient fused into the
 * BatchRenorm backward and the ray-sample scatter add partial sums with fire-and-forget atomics.  Deterministic mode:
 * one workgroup per weight-gradient element (slow: 10-50x for those launches), an ordered two-level reduction for the
 * bias gradient, 64-bit fixed-point accumulation (scale from max |dout|) for the scatter.  Process-wide.           */
int crn_set_deterministic(int on);

/* misc */
int crn_zero_f32(float* p, int64_t n, crnStream s);
/* p[i] += v, i < n : steps every BatchRenorm's num_batches_tracked (batch_renorm.py:57) */
int crn_add_i64(int64_t* p, int n, int64_t v, crnStream s);
const char* crn_version(void);

#ifdef CRN_TOOLS
/* Tuning aids: NOT in libcorenet_hip.so.  corenet_amd.build.build_tools() compiles the library a second time with
 * -DCRN_TOOLS into tools/_build/libcorenet_hip_tools.so for the scripts under tools/ (shader-clock stamps of workgroup 0 of
 * the last launch of the split-bf16 decoder kernels, CRN_BF3_STAMPS=1, the encoder engine, CRN_E2D_DBG=16, and the pointwise
 * kernel, CRN_PW_STAMPS=1; copied to the host after a device synchronize; CRN_EINVAL when the switch was not set).  The MFMA
 * hardware probe of DESIGN section 3e is tools/mfma_probe.hip -> tools/_build/libcrn_probe.so.                          */
int crn_bf3_debug_stamps(long long* out192);
int crn_e2d_debug_stamps(long long* out32);
int crn_pw_debug_stamps(long long* out32);
#endif

#ifdef __cplusplus
}
#endif
#endif  /* CORENET_HIP_H_ */
