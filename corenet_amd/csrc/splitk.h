// Split-K service of the convolution engines (splitk.hip): scratch, deferral and finish.  Included by crn_common.h.
//
// A convolution whose output grid cannot fill the chip splits its reduction over K and writes one partial sum per split
// to a dense [split][B][C][S] scratch.  Every producer (fp32 pointwise and generic engine in conv_igemm.hip, split-bf16
// decoder engine in conv_bf3.hip, encoder engine in conv_e2d.hip) follows one protocol:
//   begin    crn_splitk_begin: consume the arming of crn_splitk_defer, flush what an earlier call left pending
//   scratch  crn_splitk_scratch: nullptr -> do not split (or fall back to atomics)
//   redirect crn_splitk_scratch_view: the kernel writes split s of y to scratch + s * B*C*S
//   launch
//   finish   crn_splitk_finish: leave the sum pending for the next BatchRenorm launch over y, or reduce now
// CRN_ENTRY rule: a pending sum means y does not hold its values yet and the scratch is in use, so EVERY entry point of
// the library flushes first (CRN_ENTRY(stream)) -- except the producers above (crn_splitk_begin does it) and the
// BatchRenorm calls that can take the sum over (take_or_flush_pending in batch_renorm.hip).
// One scratch per (device, stream): convolutions that split on DIFFERENT streams (the engine runs the ray-traced skip
// path beside the encoder / decoder chain) must not share partial-sum storage; calls on ONE stream are ordered, so the
// next split launch may overwrite the scratch once the reduction before it has been enqueued.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/corenet_hip.h"

// A split-K convolution whose partial sums are still in the scratch: the next BatchRenorm launch over `y` adds them up
// itself (crn_splitk_defer); anything else that needs the scratch or y first calls crn_splitk_flush.
struct CrnSplitPending {
  bool armed = false, active = false;
  crnView y{};                 // the conv's real output (crn_splitk_dense)
  const float* scratch = nullptr;
  int splits = 0;
  hipStream_t stream = nullptr;  // the stream (and its device) the convolution ran on: only a BatchRenorm call on the SAME
  int device = -1;               // stream may take the sum over; a flush always runs on this stream, behind the conv
};
CrnSplitPending& crn_splitk_pending();                 // per host thread
// Run the pending reduction now, on the stream of the convolution that left it (no-op if none).
int crn_splitk_flush(hipStream_t st);
#define CRN_ENTRY(stream_arg)                                                          \
  do {                                                                                 \
    const int crn_rcf_ = crn_splitk_flush((hipStream_t)(stream_arg));                  \
    if (crn_rcf_ != CRN_OK) return crn_rcf_;                                           \
  } while (0)

// every sample a contiguous [C][D][H][W] block at a 16-byte aligned address: float4 access with no index arithmetic
inline bool plain_view(const crnView& v) {
  return v.chan_off == nullptr && v.sW == 1 && v.sH == v.W && (v.D == 1 || v.sD == v.H * v.W) &&
         v.sC == (int64_t)v.D * v.H * v.W && (((uintptr_t)v.base) & 15) == 0 && (v.sB & 3) == 0;
}
// [B][C][S] with nothing in between: the layout the BatchRenorm launch that takes a pending sum over stores to (no
// alignment terms: the consumer's own vec_ok decides alignment)
inline bool crn_splitk_dense(const crnView& y) {
  const int64_t S = (int64_t)y.D * y.H * y.W;
  return y.chan_off == nullptr && y.sW == 1 && y.sH == y.W && (y.D == 1 || y.sD == (int64_t)y.H * y.W) && y.sC == S &&
         y.sB == (int64_t)y.C * S;
}
// the dense [B][C][S] view of one split's slab: what the kernel writes instead of y
inline crnView crn_splitk_scratch_view(const crnView& y, float* scratch) {
  crnView v = y;
  const int64_t S = (int64_t)y.D * y.H * y.W;
  v.base = scratch; v.chan_off = nullptr;
  v.sW = 1; v.sH = y.W; v.sD = y.H * y.W; v.sC = S; v.sB = (int64_t)y.C * S;
  return v;
}

// consumes the arming of crn_splitk_defer (the return value) and flushes; *rc != CRN_OK: the flush failed
bool crn_splitk_begin(hipStream_t st, int* rc);
float* crn_splitk_scratch(size_t floats, hipStream_t st);      // per (device, stream), grown on demand; nullptr: none to be had
// y = (accumulate ? y : 0) + sum of the splits; split 0 first
int crn_splitk_reduce(const crnView& y, const float* scratch, int splits, int accumulate, hipStream_t st);
// the end of every split launch: the sum stays pending when the caller armed it and y is dense, otherwise it is reduced now
int crn_splitk_finish(const crnView& y, const float* scratch, int splits, int accumulate, bool armed, hipStream_t st);
