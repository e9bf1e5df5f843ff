// BatchRenorm statistics / backward and the fused per-channel elementwise
// kernels of the encoder/decoder blocks.  All HBM-bound: one coalesced float4
// pass per tensor, fp64 accumulation of the per-channel sums.
// Reference: model/batch_renorm.py:33-62, model/resnet50.py:72-82,109-115.
#include "crn_common.h"
#include <cstdlib>
#include <algorithm>
#include <type_traits>

namespace {

constexpr int kThreads = 256;

struct Slice { int64_t s0, s1; };
__device__ __forceinline__ Slice block_slice(int64_t S) {
  int64_t chunk = (S + gridDim.x - 1) / gridDim.x;
  chunk = (chunk + 3) & ~(int64_t)3;
  Slice r;
  r.s0 = (int64_t)blockIdx.x * chunk;
  r.s1 = min(S, r.s0 + chunk);
  return r;
}

// Applies f(s, vec4) over a contiguous slice; VEC needs 16-B aligned rows.
template <bool VEC, typename F4, typename F1>
__device__ __forceinline__ void for_slice(Slice sl, F4 f4, F1 f1) {
  if (VEC) {
#pragma unroll 4
    for (int64_t s = sl.s0 + (int64_t)threadIdx.x * 4; s + 3 < sl.s1; s += (int64_t)kThreads * 4) f4(s);
    const int64_t nfull = (sl.s1 > sl.s0) ? ((sl.s1 - sl.s0) & ~(int64_t)3) : 0;
    for (int64_t s = sl.s0 + nfull + threadIdx.x; s < sl.s1; s += kThreads) f1(s);
  } else {
    for (int64_t s = sl.s0 + threadIdx.x; s < sl.s1; s += kThreads) f1(s);
  }
}

// Sum over the `splits` partial results of a split-K convolution at one element (T = float) or float4 (T = f32x4): p = the
// element in split 0, `slab` = Ts per split ([split][b][c][pos], dense).  Split 0 first, the order of the reduction kernel.
// The loads of up to four splits are issued together, as in splitk_reduce_plain_kernel: walked one load latency after the other
// (a loop over a run-time `splits`) the first pass of the two-pass backward took 113 us per step where it now takes 97.
template <typename T>
__device__ __forceinline__ T bn_splitk_sum_at(const T* p, int splits, int64_t slab) {
  T sum = T{};
  int sp = 0;
  for (; sp + 4 <= splits; sp += 4) {       // the loads of four splits in flight, added in order (as the reduction kernel does)
    const T a = p[sp * slab], b = p[(sp + 1) * slab], c = p[(sp + 2) * slab], d = p[(sp + 3) * slab];
    sum += a; sum += b; sum += c; sum += d;
  }
  const int rest = splits - sp;             // 0..3 (uniform): loaded together as well
  if (rest > 0) {
    const T a = p[sp * slab], b = rest > 1 ? p[(sp + 1) * slab] : T{}, c = rest > 2 ? p[(sp + 2) * slab] : T{};
    sum += a;
    if (rest > 1) sum += b;
    if (rest > 2) sum += c;
  }
  return sum;
}

// The first pass of a two-pass launch over a pending split-K sum (part != nullptr; t = the dense [B][C][S] tensor whose
// values are still `splits` partial sums in the scratch): the workgroup that owns a slice adds it up, stores the sum to t for
// the second pass and every later reader, and accumulates from it.  at() = the value of t at offset o of the channel row.
// PEND is a template parameter of the kernels: the launches with nothing pending keep the plain loads' code.
template <bool PEND>
struct BnPendingRow {
  const float* part; float* t; int64_t slab; int splits;     // part, t: the (b, c) row; slab = B * C * S
  __device__ __forceinline__ f32x4 at4(int64_t o) const {
    if (!PEND) return *reinterpret_cast<const f32x4*>(t + o);
    const f32x4 v = bn_splitk_sum_at(reinterpret_cast<const f32x4*>(part + o), splits, slab / 4);
    *reinterpret_cast<f32x4*>(t + o) = v;
    return v;
  }
  __device__ __forceinline__ float at1(int64_t o) const {
    if (!PEND) return t[o];
    const float v = bn_splitk_sum_at(part + o, splits, slab);
    t[o] = v;
    return v;
  }
};
template <bool PEND>
__device__ __forceinline__ BnPendingRow<PEND> bn_pending_row(const float* t, int64_t sB, const float* part, int splits, int B,
                                                             int C, int64_t S, int b, int c) {
  BnPendingRow<PEND> r;
  r.t = const_cast<float*>(t) + (int64_t)b * sB + (int64_t)c * S;
  r.part = PEND ? part + ((int64_t)b * C + c) * S : nullptr;
  r.slab = (int64_t)B * C * S; r.splits = splits;
  return r;
}

// ---- statistics -------------------------------------------------------------
// One element into the fp64 sums of a channel: sum(x'), sum(x'^2) with x' = relu(x) under pre_relu.
__device__ __forceinline__ void bn_acc(float v, int pre_relu, double& s1, double& s2) {
  if (pre_relu) v = fmaxf(v, 0.f);
  s1 += (double)v;
  s2 += (double)v * (double)v;
}

template <bool VEC, bool PEND>
__global__ __launch_bounds__(kThreads) void bn_partial_kernel(const float* x, int64_t S, int64_t sB,
                                                               int pre_relu, double* ws, const float* part, int splits) {
  __shared__ double red[kThreads / 64];
  const int c = blockIdx.y, b = blockIdx.z;
  const BnPendingRow<PEND> p = bn_pending_row<PEND>(x, sB, part, splits, gridDim.z, gridDim.y, S, b, c);
  double s1 = 0.0, s2 = 0.0;
  auto one = [&](float v) { bn_acc(v, pre_relu, s1, s2); };
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) { const f32x4 v = p.at4(s);
                                  one(v.x); one(v.y); one(v.z); one(v.w); },
                 [&](int64_t s) { one(p.at1(s)); });
  const double t1 = crn_block_sum(s1, red);
  const double t2 = crn_block_sum(s2, red);
  if (threadIdx.x == 0) {
    const int nparts = gridDim.x * gridDim.z;
    double* o = ws + ((int64_t)c * nparts + (int64_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = t1; o[1] = t2;
  }
}

// One channel's statistics -> scale/shift, saved values, running statistics (batch_renorm.py:33-62).
// The five per-channel inputs of bn_finalize_channel, loaded at the START of an owner kernel (they do not depend on the
// statistics): their round trip to memory then overlaps the one of x instead of following the reduction.
struct BnChannelIn { float g, bt, rmean, rvar, nt; };
__device__ __forceinline__ BnChannelIn bn_channel_in(int c, const float* gamma, const float* beta,
                                                     const float* running_mean, const float* running_var,
                                                     const int64_t* nbt) {
  return BnChannelIn{gamma[c], beta[c], running_mean[c], running_var[c], (float)nbt[0]};
}
__device__ __forceinline__ void bn_finalize_channel(int c, int C, double s1, double s2, double count,
                                                    const BnChannelIn& in, float* running_mean, float* running_var,
                                                    float eps, float momentum, float* scale, float* shift, float* saved) {
  const float g = in.g, bt = in.bt;
  const double mean_d = s1 / count;
  double var_d = s2 / count - mean_d * mean_d;
  if (var_d < 0.0) var_d = 0.0;
  const float b_mean = (float)mean_d, b_var = (float)var_d;
  const float b_std = sqrtf(b_var + eps);
  const float run_std = sqrtf(in.rvar + eps);
  // batch_renorm.py:41-42: schedules from num_batches_tracked (before the increment)
  const float nt = in.nt;
  const float d_max = fminf(fmaxf(5.0f * (nt - 5000.f) / (25000.f - 5000.f), 0.f), 5.f);
  const float r_max = 1.0f + fminf(fmaxf(2.0f * (nt - 5000.f) / (40000.f - 5000.f), 0.f), 2.f);
  float r = b_std / run_std;
  r = fminf(fmaxf(r, 1.0f / r_max), r_max);
  float d = (b_mean - in.rmean) / run_std;
  d = fminf(fmaxf(d, -d_max), d_max);
  const float rstd = 1.0f / b_std;
  scale[c] = g * r * rstd;
  shift[c] = bt + g * (d - b_mean * r * rstd);
  saved[c] = b_mean; saved[C + c] = rstd; saved[2 * C + c] = r; saved[3 * C + c] = d;
  // batch_renorm.py:54-56 (the "unbiased" factor uses C = channel count)
  const float unbiased = b_var * (float)C / (float)(C - 1);
  running_var[c] = in.rvar + momentum * (unbiased - in.rvar);
  running_mean[c] = in.rmean + momentum * (b_mean - in.rmean);
}

__global__ void bn_finalize_kernel(const double* ws, int nparts, int C, double count,
                                   const float* gamma, const float* beta, float* running_mean,
                                   float* running_var, const int64_t* nbt, float eps, float momentum,
                                   int training, float* scale, float* shift, float* saved) {
  // one wave per channel: its lanes add the channel's partial sums up together (one thread per channel walked up to
  // 4096 of them one memory latency after the other: 9 us for a 100-channel launch)
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  if (!training) {          // batch_renorm.py:59: (x - running_mean) / running_std
    if (lane) return;
    const float g = gamma[c], bt = beta[c];
    const float rstd = 1.0f / sqrtf(running_var[c] + eps);
    scale[c] = g * rstd;
    shift[c] = bt - g * running_mean[c] * rstd;
    return;
  }
  const BnChannelIn cin = bn_channel_in(c, gamma, beta, running_mean, running_var, nbt);
  double s1 = 0.0, s2 = 0.0;
  for (int i = lane; i < nparts; i += 64) { s1 += ws[((int64_t)c * nparts + i) * 2]; s2 += ws[((int64_t)c * nparts + i) * 2 + 1]; }
  s1 = crn_wave_sum(s1); s2 = crn_wave_sum(s2);
  if (lane == 0)
    bn_finalize_channel(c, C, s1, s2, count, cin, running_mean, running_var, eps, momentum, scale, shift, saved);
}

// The same for MANY parts per channel (the partial sums a convolution's workgroups leave: 2048 for decoder stage_6.c1): one
// workgroup per channel, every thread has its share of the loads in flight at once (a wave's 64 lanes walked 32 of them one
// after the other: 12.7 us for 16 channels)
__global__ __launch_bounds__(kThreads) void bn_finalize_wide_kernel(const double* ws, int nparts, int C, double count,
                                                                    const float* gamma, const float* beta, float* running_mean,
                                                                    float* running_var, const int64_t* nbt, float eps, float momentum,
                                                                    float* scale, float* shift, float* saved) {
  __shared__ double red[2 * (kThreads / 64)];
  const int c = blockIdx.x;
  const BnChannelIn cin = bn_channel_in(c, gamma, beta, running_mean, running_var, nbt);
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  const f64x2* p = reinterpret_cast<const f64x2*>(ws) + (int64_t)c * nparts;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int i = threadIdx.x; i < nparts; i += kThreads) { const f64x2 v = p[i]; s1 += v.x; s2 += v.y; }
  double t1, t2;
  crn_block_sum2(s1, s2, red, t1, t2);
  if (threadIdx.x == 0)
    bn_finalize_channel(c, C, t1, t2, count, cin, running_mean, running_var, eps, momentum, scale, shift, saved);
}

// Eval mode: scale/shift of EVERY BatchRenorm of the model from the running statistics in one launch
// (batch_renorm.py:59); table rows = (gamma, beta offsets in the parameter slab; running_mean, running_var
// offsets in the buffer slab; output offset in the scale/shift slabs).  Same arithmetic as the eval branch of
// bn_finalize_kernel.
__global__ void bn_eval_affine_kernel(const float* params, const float* buffers, const int32_t* table, int n,
                                      float eps, float* scale, float* shift) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t* r = table + (int64_t)j * 5;
  const float g = params[r[0]], bt = params[r[1]];
  const float rstd = 1.0f / sqrtf(buffers[r[3]] + eps);
  scale[r[4]] = g * rstd;
  shift[r[4]] = bt - g * buffers[r[2]] * rstd;
}

// Channel-owner form for many small channels (the encoder from stage 3 on, the coarse decoder stages): one
// workgroup reduces all of (B, S) of its channel and finalizes it -- one launch instead of two, no workspace.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_owner_stats_kernel(
    const float* x, int B, int C, int64_t S, int64_t sB, int pre_relu, const float* gamma, const float* beta,
    float* running_mean, float* running_var, const int64_t* nbt, float eps, float momentum, float* scale,
    float* shift, float* saved) {
  __shared__ double red[kThreads / 64];
  const int c = blockIdx.x;
  const BnChannelIn cin = bn_channel_in(c, gamma, beta, running_mean, running_var, nbt);
  double s1 = 0.0, s2 = 0.0;
  auto one = [&](float v) { bn_acc(v, pre_relu, s1, s2); };
  Slice all; all.s0 = 0; all.s1 = S;
  for (int b = 0; b < B; ++b) {
    const float* p = x + (int64_t)b * sB + (int64_t)c * S;
    for_slice<VEC>(all,
                   [&](int64_t s) { const f32x4 v = *reinterpret_cast<const f32x4*>(p + s);
                                    one(v.x); one(v.y); one(v.z); one(v.w); },
                   [&](int64_t s) { one(p[s]); });
  }
  const double t1 = crn_block_sum(s1, red);
  const double t2 = crn_block_sum(s2, red);
  if (threadIdx.x == 0)
    bn_finalize_channel(c, C, t1, t2, (double)B * (double)S, cin, running_mean, running_var, eps, momentum, scale, shift,
                        saved);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Sum of the `splits` partial results ([split][b][c][pos], dense) a split-K convolution left in the scratch, for float4 s4 of
// (b, c): split 0 first, the order of the reduction kernel.
__device__ __forceinline__ f32x4 bn_splitk_sum(const float* part, int splits, int B, int C, int S4, int b, int c, int s4) {
  return bn_splitk_sum_at(reinterpret_cast<const f32x4*>(part) + ((int64_t)b * C + c) * S4 + s4, splits, (int64_t)B * C * S4);
}

// Where float4 s4 of channel c's full plane (rows of width W, a multiple of 4) lands in the stride-2 compaction [c][H2][W2] of
// the tensor: `off` = the offset of the float2 that holds its elements 0 and 2 (even columns); false on an odd row (nothing of it is
// kept).
__device__ __forceinline__ bool bn_stride2_offset(int c, int s4, int W, int W2, int H2, int64_t& off) {
  const int s = s4 * 4, row = s / W, col = s - row * W;
  off = ((int64_t)c * H2 + (row >> 1)) * W2 + (col >> 1);
  return !(row & 1);
}

// Register-resident owner kernels: when all of (B, S) of a channel fits in NV float4 per thread (B*S <= 1024*NV), every
// thread issues its NV loads at once (the loops above walk them one latency after the other: these launches are
// latency bound) and the backward kernel makes its second pass over registers instead of re-reading x and dy.
// part != nullptr: x is the output of a split-K convolution whose `splits` partial sums are still in the scratch
// ([split][b][c][pos], dense): they are added up here (split 0 first, the order of the reduction kernel) and the
// sum is stored to x on the way -- one launch instead of reduction + statistics (crn_splitk_defer).
// TAIL: the block tail of a ResNet bottleneck in the same launch -- the channel is in registers and its scale / shift are
// known to this workgroup the moment the statistics are finalized, so y = relu(x*scale + shift + residual) (the
// arithmetic of affine_add_relu_kernel, expression for expression) is written from here: 16 launches fewer per forward
// and one read of x instead of two.
// y2: the stride-2 compaction of y (y2[b,c,i,j] = y[b,c,2i,2j], crn_stride2_gather) for the down-sampling block that reads this
// block's output next (resnet50.py:94-97): written from the same registers, one launch less on the forward chain.  W = row width of
// the channel plane (a multiple of 4: a float4 never straddles rows), W2 = ceil(W / 2), H2 = ceil(H / 2).
struct BnTail {
  const float* r; const float* rscale; const float* rshift; int64_t sBr;
  float* y_pre; int64_t sBpre; float* y; int64_t sBy; int relu;
  float* y2; int64_t sBy2; int W, W2, H2;
};
template <int NV, bool TAIL = false>
__global__ __launch_bounds__(kThreads) void bn_owner_stats_reg_kernel(
    float* x, int B, int C, int S4, int64_t sB, int pre_relu, const float* gamma, const float* beta,
    float* running_mean, float* running_var, const int64_t* nbt, float eps, float momentum, float* scale,
    float* shift, float* saved, const float* part, int splits, BnTail tail = BnTail{}) {
  __shared__ double red[2 * (kThreads / 64)];
  __shared__ float tail_affine[2];
  crn_kernargs_now(x, B, C, S4, sB, pre_relu, gamma, beta, running_mean, running_var, nbt, eps, momentum, scale, shift,
                   saved, part, splits);
  if (TAIL) crn_kernargs_now(tail.r, tail.rscale, tail.rshift, tail.sBr, tail.y_pre, tail.sBpre, tail.y, tail.sBy, tail.relu);
  const int c = blockIdx.x, total4 = B * S4;
  const BnChannelIn cin = bn_channel_in(c, gamma, beta, running_mean, running_var, nbt);
  f32x4 v[NV];
  f32x4 rv[TAIL ? NV : 1];
  float rsc = 1.f, rsh = 0.f;
  if (TAIL && tail.r) { rsc = tail.rscale ? tail.rscale[c] : 1.f; rsh = tail.rshift ? tail.rshift[c] : 0.f; }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int e = threadIdx.x + k * kThreads;
    const int b = e / S4, s4 = e - b * S4;
    f32x4* xp = reinterpret_cast<f32x4*>(x + (int64_t)b * sB + ((int64_t)c * S4 + s4) * 4);
    if (TAIL)      // the residual rides on the same round trip
      rv[k] = (tail.r && e < total4) ? *reinterpret_cast<const f32x4*>(tail.r + (int64_t)b * tail.sBr + ((int64_t)c * S4 + s4) * 4)
                                     : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (part == nullptr) {
      v[k] = e < total4 ? *xp : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else {
      v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (e < total4) *xp = v[k] = bn_splitk_sum(part, splits, B, C, S4, b, c, s4);
    }
  }
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) bn_acc(v[k][i], pre_relu, s1, s2);
  double t1, t2;
  crn_block_sum2(s1, s2, red, t1, t2);
  if (threadIdx.x == 0) {
    bn_finalize_channel(c, C, t1, t2, (double)B * (double)S4 * 4.0, cin, running_mean, running_var, eps, momentum,
                        scale, shift, saved);
    if (TAIL) { tail_affine[0] = scale[c]; tail_affine[1] = shift[c]; }     // (the fp32 values the un-fused tail would load)
  }
  if (TAIL) {
    __syncthreads();
    const float sc = tail_affine[0], sh = tail_affine[1];
    const bool has_r = tail.r != nullptr;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int e = threadIdx.x + k * kThreads;
      if (e < total4) {
        const int b = e / S4, s4 = e - b * S4;
        const int64_t o = ((int64_t)c * S4 + s4) * 4;
        f32x4 q;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = v[k][i] * sc + sh + (has_r ? rv[k][i] * rsc + rsh : 0.f);
        if (tail.y_pre) *reinterpret_cast<f32x4*>(tail.y_pre + (int64_t)b * tail.sBpre + o) = q;
        if (tail.y) {
          if (tail.relu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = fmaxf(q[i], 0.f);
          }
          *reinterpret_cast<f32x4*>(tail.y + (int64_t)b * tail.sBy + o) = q;
          int64_t o2;
          if (tail.y2 && bn_stride2_offset(c, s4, tail.W, tail.W2, tail.H2, o2))
            *reinterpret_cast<f32x2*>(tail.y2 + (int64_t)b * tail.sBy2 + o2) = (f32x2){q[0], q[2]};
        }
      }
    }
  }
}

// ---- backward: the arithmetic every backward kernel shares ------------------------
// Per-channel values of the forward pass that the per-element terms need.
struct BnBwdChannel { float sc, sh, mu, rstd; };
__device__ __forceinline__ BnBwdChannel bn_bwd_channel(int c, int C, const float* scale, const float* shift, const float* saved) {
  return BnBwdChannel{scale[c], shift[c], saved[c], saved[C + c]};
}

// Reduction term of one element: g masked where the post-ReLU output is not positive, into sum(g) and sum(g * xhat).
__device__ __forceinline__ void bn_bwd_acc(float x, float g, int pre_relu, int post_relu, BnBwdChannel ch, double& s1, double& s2) {
  if (pre_relu) x = fmaxf(x, 0.f);
  if (post_relu && !(x * ch.sc + ch.sh > 0.f)) g = 0.f;
  s1 += (double)g;
  s2 += (double)g * (double)((x - ch.mu) * ch.rstd);
}

// dx of one element: k = gamma * r * rstd, mg / mgx = the channel's mean(g) / mean(g * xhat); zero where the pre-ReLU input is <= 0.
__device__ __forceinline__ float bn_bwd_dx(float xr, float g, int pre_relu, int post_relu, BnBwdChannel ch, float k, float mg, float mgx) {
  const float x = pre_relu ? fmaxf(xr, 0.f) : xr;
  if (post_relu && !(x * ch.sc + ch.sh > 0.f)) g = 0.f;
  float o = k * (g - mg - (x - ch.mu) * ch.rstd * mgx);
  if (pre_relu && !(xr > 0.f)) o = 0.f;
  return o;
}

// Closing of a channel's reduction (one thread): the two means go to sm[0], sm[1] for the apply pass of the workgroup, and
// the gradients of gamma and beta come back (r, d = the saved renorm factors).
struct BnAffineGrad { float dg, db; };
__device__ __forceinline__ BnAffineGrad bn_bwd_close(double s1, double s2, double count, float r, float d, float* sm) {
  sm[0] = (float)(s1 / count); sm[1] = (float)(s2 / count);
  return BnAffineGrad{(float)(r * s2 + d * s1), (float)s1};
}
__device__ __forceinline__ void bn_bwd_store_grad(BnAffineGrad g, int c, float* dgamma, float* dbeta, int accumulate) {
  if (accumulate) { dgamma[c] += g.dg; dbeta[c] += g.db; } else { dgamma[c] = g.dg; dbeta[c] = g.db; }
}

// fp32 sum of one value per thread over the workgroup, the waves in order (valid in thread 0): a channel's share of sum(dx),
// which the caller stores or adds atomically to dsum.  redf: kThreads / 64 floats.
__device__ __forceinline__ float bn_block_sum_f32(float v, float* redf) {
  const float w = crn_wave_sum(v);
  if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = w;
  __syncthreads();
  float tsum = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < kThreads / 64; ++i) tsum += redf[i];
  return tsum;
}

// part != nullptr: dy is the output of a split-K convolution (a data gradient) still in `splits` partial sums in the
// scratch: added up while they are loaded; dy itself is NOT written (its only reader is this kernel).
// HEAD: the backward of a bottleneck's tail in the same launch -- dy is not read but formed,
//   dy = (act > 0 ? g : 0) + g2      (the arithmetic of relu_bwd_add_kernel; g2 may be absent),
// and stored to `dy` on the way (the shortcut's norm and the block's input gradient read it later): 15 launches fewer
// per backward.
// gc != nullptr: g is given in its compact form -- it is the data gradient of a stride-2 1x1 convolution, non-zero only at even
// (row, column) (crn_stride2_scatter(gc) would expand it: g[2i][2j] = gc[i][j], zeros elsewhere): read from there, the expanded
// tensor is never written.  W = row width of the full plane (a multiple of 4), W2 = ceil(W / 2), H2 = ceil(H / 2).
struct BnHead { const float* g; int64_t sBg; const float* act; int64_t sBact; const float* g2; int64_t sBg2;
                const float* gc; int64_t sBgc; int W, W2, H2; };
template <int NV, bool HEAD = false>
__global__ __launch_bounds__(kThreads) void bn_owner_bwd_reg_kernel(
    const float* x, int64_t sBx, const float* dy, int64_t sBdy, int B, int S4, int C, int pre_relu,
    int post_relu, const float* gamma, const float* scale, const float* shift, const float* saved, float* dx,
    int64_t sBdx, float* dgamma, float* dbeta, int accumulate, float* dsum, int ndsum, const float* part, int splits,
    BnHead head = BnHead{}) {
  __shared__ double red[2 * (kThreads / 64)];
  __shared__ float sm[2];
  __shared__ float redf[kThreads / 64];
  crn_kernargs_now(x, sBx, dy, sBdy, B, S4, C, pre_relu, post_relu, gamma, scale, shift, saved, dx, sBdx, dgamma, dbeta,
                   accumulate, dsum, ndsum, part, splits);
  if (HEAD) crn_kernargs_now(head.g, head.sBg, head.act, head.sBact, head.g2, head.sBg2, head.gc, head.sBgc, head.W, head.W2, head.H2);
  const int c = blockIdx.x, total4 = B * S4;
  // every per-channel scalar of the kernel is loaded here, next to x and dy: one round trip to memory, not three
  const BnBwdChannel ch = bn_bwd_channel(c, C, scale, shift, saved);
  const float rr = saved[2 * C + c], dd = saved[3 * C + c], gam = gamma[c];
  float dg0 = 0.f, db0 = 0.f;
  if (accumulate && threadIdx.x == 0) { dg0 = dgamma[c]; db0 = dbeta[c]; }
  f32x4 xv[NV], gv[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int e = threadIdx.x + k * kThreads;
    const int b = e / S4, s4 = e - b * S4;
    const int64_t o = ((int64_t)c * S4 + s4) * 4;
    const bool ok = e < total4;
    xv[k] = ok ? *reinterpret_cast<const f32x4*>(x + (int64_t)b * sBx + o) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (HEAD) {
      const f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
      f32x4 g = z;
      if (ok && head.gc) {
        int64_t o2;
        if (bn_stride2_offset(c, s4, head.W, head.W2, head.H2, o2)) {
          const f32x2 v = *reinterpret_cast<const f32x2*>(head.gc + (int64_t)b * head.sBgc + o2);
          g[0] = v[0]; g[2] = v[1];
        }
      } else if (ok) {
        g = *reinterpret_cast<const f32x4*>(head.g + (int64_t)b * head.sBg + o);
      }
      const f32x4 a = ok ? *reinterpret_cast<const f32x4*>(head.act + (int64_t)b * head.sBact + o) : z;
      const f32x4 g2 = (ok && head.g2) ? *reinterpret_cast<const f32x4*>(head.g2 + (int64_t)b * head.sBg2 + o) : z;
      f32x4 d;
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = (a[i] > 0.f ? g[i] : 0.f) + g2[i];
      if (ok) *reinterpret_cast<f32x4*>(const_cast<float*>(dy) + (int64_t)b * sBdy + o) = d;
      gv[k] = d;
    } else if (part == nullptr) {
      gv[k] = ok ? *reinterpret_cast<const f32x4*>(dy + (int64_t)b * sBdy + o) : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else {
      gv[k] = ok ? bn_splitk_sum(part, splits, B, C, S4, b, c, s4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) bn_bwd_acc(xv[k][i], gv[k][i], pre_relu, post_relu, ch, s1, s2);
  double t1, t2;
  crn_block_sum2(s1, s2, red, t1, t2);
  if (threadIdx.x == 0) {
    const BnAffineGrad ag = bn_bwd_close(t1, t2, (double)B * (double)S4 * 4.0, rr, dd, sm);
    dgamma[c] = dg0 + ag.dg; dbeta[c] = db0 + ag.db;       // (dg0, db0 were loaded with everything else: not bn_bwd_store_grad)
  }
  __syncthreads();
  const float mg = sm[0], mgx = sm[1];
  const float kf = gam * rr * ch.rstd;
  float lsum = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int e = threadIdx.x + k * kThreads;
    if (e < total4) {
      const int b = e / S4, s4 = e - b * S4;
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = bn_bwd_dx(xv[k][i], gv[k][i], pre_relu, post_relu, ch, kf, mg, mgx);
        lsum += o[i];
      }
      *reinterpret_cast<f32x4*>(dx + (int64_t)b * sBdx + ((int64_t)c * S4 + s4) * 4) = o;
    }
  }
  if (dsum && c < ndsum) {       // bias gradient of the convolution that produced x: sum of dx
    const float tsum = bn_block_sum_f32(lsum, redf);
    if (threadIdx.x == 0) dsum[c] = tsum;
  }
}

// ---- backward ----------------------------------------------------------------
template <bool VEC, bool PEND>
__global__ __launch_bounds__(kThreads) void bn_bwd_partial_kernel(
    const float* x, int64_t sBx, const float* dy, int64_t sBdy, int64_t S, int C, int pre_relu,
    int post_relu, const float* scale, const float* shift, const float* saved, double* ws, float* dsum,
    int ndsum, const float* part, int splits) {
  __shared__ double red[kThreads / 64];
  const int c = blockIdx.y, b = blockIdx.z;
  // the apply kernel (next launch on this stream) accumulates sum(dx) here with atomics
  if (dsum && c < ndsum && blockIdx.x == 0 && b == 0 && threadIdx.x == 0) dsum[c] = 0.f;
  const float* px = x + (int64_t)b * sBx + (int64_t)c * S;
  // (part != nullptr: dy is a pending split-K sum -- added up and stored here, the apply kernel reads it from dy)
  const BnPendingRow<PEND> pg = bn_pending_row<PEND>(dy, sBdy, part, splits, gridDim.z, C, S, b, c);
  const BnBwdChannel ch = bn_bwd_channel(c, C, scale, shift, saved);
  double s1 = 0.0, s2 = 0.0;
  auto one = [&](float xv, float gv) { bn_bwd_acc(xv, gv, pre_relu, post_relu, ch, s1, s2); };
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) { const f32x4 a = *reinterpret_cast<const f32x4*>(px + s);
                                  const f32x4 g = pg.at4(s);
                                  one(a.x, g.x); one(a.y, g.y); one(a.z, g.z); one(a.w, g.w); },
                 [&](int64_t s) { one(px[s], pg.at1(s)); });
  const double t1 = crn_block_sum(s1, red);
  const double t2 = crn_block_sum(s2, red);
  if (threadIdx.x == 0) {
    const int nparts = gridDim.x * gridDim.z;
    double* o = ws + ((int64_t)c * nparts + (int64_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = t1; o[1] = t2;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(
    const float* x, int64_t sBx, const float* dy, int64_t sBdy, int64_t S, int C, int pre_relu,
    int post_relu, const float* gamma, const float* scale, const float* shift, const float* saved,
    const double* ws, int nparts, double count, float* dx, int64_t sBdx, float* dgamma,
    float* dbeta, int accumulate, float* dsum, int ndsum) {
  __shared__ float sm[2];
  __shared__ float red[kThreads / 64];
  __shared__ double redd[2 * (kThreads / 64)];
  const int c = blockIdx.y, b = blockIdx.z;
  // the partial sums of the channel are added up by the whole workgroup (one thread walking up to 4096 of them kept
  // the other 255 waiting at the barrier for several memory latencies), and the per-channel scalars used after the
  // barrier are loaded before it
  const BnBwdChannel ch = bn_bwd_channel(c, C, scale, shift, saved);
  const float k = gamma[c] * saved[2 * C + c] * ch.rstd;
  double p1 = 0.0, p2 = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) { p1 += ws[((int64_t)c * nparts + i) * 2]; p2 += ws[((int64_t)c * nparts + i) * 2 + 1]; }
  double s1, s2;
  crn_block_sum2(p1, p2, redd, s1, s2);
  if (threadIdx.x == 0) {
    const BnAffineGrad ag = bn_bwd_close(s1, s2, count, saved[2 * C + c], saved[3 * C + c], sm);
    if (blockIdx.x == 0 && b == 0) bn_bwd_store_grad(ag, c, dgamma, dbeta, accumulate);
  }
  __syncthreads();
  const float mg = sm[0], mgx = sm[1];
  const float* px = x + (int64_t)b * sBx + (int64_t)c * S;
  const float* pg = dy + (int64_t)b * sBdy + (int64_t)c * S;
  float* po = dx + (int64_t)b * sBdx + (int64_t)c * S;
  float lsum = 0.f;
  auto one = [&](float xr, float gv) -> float {
    const float o = bn_bwd_dx(xr, gv, pre_relu, post_relu, ch, k, mg, mgx);
    lsum += o;
    return o;
  };
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) { const f32x4 a = *reinterpret_cast<const f32x4*>(px + s);
                                  const f32x4 g = *reinterpret_cast<const f32x4*>(pg + s);
                                  f32x4 o; o.x = one(a.x, g.x); o.y = one(a.y, g.y);
                                  o.z = one(a.z, g.z); o.w = one(a.w, g.w);
                                  *reinterpret_cast<f32x4*>(po + s) = o; },
                 [&](int64_t s) { po[s] = one(px[s], pg[s]); });
  if (dsum && c < ndsum) {       // bias gradient of the convolution that produced x: sum of dx
    const float tsum = bn_block_sum_f32(lsum, red);
    if (threadIdx.x == 0) atomicAdd(dsum + c, tsum);
  }
}

// Channel-owner backward: reduce, then apply, in one workgroup per channel (second pass re-reads from L2).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void bn_owner_bwd_kernel(
    const float* x, int64_t sBx, const float* dy, int64_t sBdy, int B, int64_t S, int C, int pre_relu,
    int post_relu, const float* gamma, const float* scale, const float* shift, const float* saved, float* dx,
    int64_t sBdx, float* dgamma, float* dbeta, int accumulate, float* dsum, int ndsum) {
  __shared__ double red[kThreads / 64];
  __shared__ float sm[2];
  __shared__ float redf[kThreads / 64];
  const int c = blockIdx.x;
  const BnBwdChannel ch = bn_bwd_channel(c, C, scale, shift, saved);
  Slice all; all.s0 = 0; all.s1 = S;
  double s1 = 0.0, s2 = 0.0;
  auto acc = [&](float xv, float gv) { bn_bwd_acc(xv, gv, pre_relu, post_relu, ch, s1, s2); };
  for (int b = 0; b < B; ++b) {
    const float* px = x + (int64_t)b * sBx + (int64_t)c * S;
    const float* pg = dy + (int64_t)b * sBdy + (int64_t)c * S;
    for_slice<VEC>(all,
                   [&](int64_t s) { const f32x4 a = *reinterpret_cast<const f32x4*>(px + s);
                                    const f32x4 g = *reinterpret_cast<const f32x4*>(pg + s);
                                    acc(a.x, g.x); acc(a.y, g.y); acc(a.z, g.z); acc(a.w, g.w); },
                   [&](int64_t s) { acc(px[s], pg[s]); });
  }
  const double t1 = crn_block_sum(s1, red);
  const double t2 = crn_block_sum(s2, red);
  if (threadIdx.x == 0)
    bn_bwd_store_grad(bn_bwd_close(t1, t2, (double)B * (double)S, saved[2 * C + c], saved[3 * C + c], sm), c, dgamma, dbeta,
                      accumulate);
  __syncthreads();
  const float mg = sm[0], mgx = sm[1];
  const float k = gamma[c] * saved[2 * C + c] * ch.rstd;
  float lsum = 0.f;
  auto one = [&](float xr, float gv) -> float {
    const float o = bn_bwd_dx(xr, gv, pre_relu, post_relu, ch, k, mg, mgx);
    lsum += o;
    return o;
  };
  for (int b = 0; b < B; ++b) {
    const float* px = x + (int64_t)b * sBx + (int64_t)c * S;
    const float* pg = dy + (int64_t)b * sBdy + (int64_t)c * S;
    float* po = dx + (int64_t)b * sBdx + (int64_t)c * S;
    for_slice<VEC>(all,
                   [&](int64_t s) { const f32x4 a = *reinterpret_cast<const f32x4*>(px + s);
                                    const f32x4 g = *reinterpret_cast<const f32x4*>(pg + s);
                                    f32x4 o; o.x = one(a.x, g.x); o.y = one(a.y, g.y);
                                    o.z = one(a.z, g.z); o.w = one(a.w, g.w);
                                    *reinterpret_cast<f32x4*>(po + s) = o; },
                   [&](int64_t s) { po[s] = one(px[s], pg[s]); });
  }
  if (dsum && c < ndsum) {       // bias gradient of the convolution that produced x: sum of dx
    const float tsum = bn_block_sum_f32(lsum, redf);
    if (threadIdx.x == 0) dsum[c] = tsum;
  }
}

// many channels, little data per channel: the channel-owner kernels (bench.py: 17.15 -> 16.95 ms per step)
// one workgroup per channel pays when there are enough channels to fill the chip or the channel fits the register
// kernels; a 64-channel map of 65536 values per channel (the stem) keeps 64 CUs busy with 1 MB each (75 us for the
// backward pass against 2 x ~15 us for the partial + apply pair on all CUs)
inline bool owner_form(int64_t S, int C, int B) {
  return C >= 64 && (int64_t)B * S <= 65536 && ((int64_t)B * S <= 16384 || C >= 256);
}

// ---- block tails ---------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void affine_add_relu_kernel(
    const float* x, const float* scale, const float* shift, const float* r, const float* rscale,
    const float* rshift, int64_t S, int64_t sBx, int64_t sBr, float* y_pre, int64_t sBpre,
    float* y, int64_t sBy, int relu) {
  crn_kernargs_now(x, scale, shift, r, rscale, rshift, S, sBx, sBr, y_pre, sBpre, y, sBy, relu);
  const int c = blockIdx.y, b = blockIdx.z;
  const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  const float rsc = rscale ? rscale[c] : 1.f, rsh = rshift ? rshift[c] : 0.f;
  const float* px = x + (int64_t)b * sBx + (int64_t)c * S;
  const float* pr = r ? r + (int64_t)b * sBr + (int64_t)c * S : nullptr;
  float* pp = y_pre ? y_pre + (int64_t)b * sBpre + (int64_t)c * S : nullptr;
  float* py = y ? y + (int64_t)b * sBy + (int64_t)c * S : nullptr;
  auto one = [&](float xv, float rv) -> float { return xv * sc + sh + (pr ? rv * rsc + rsh : 0.f); };
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) {
                   const f32x4 a = *reinterpret_cast<const f32x4*>(px + s);
                   f32x4 q = (f32x4){0.f, 0.f, 0.f, 0.f};
                   if (pr) q = *reinterpret_cast<const f32x4*>(pr + s);
                   f32x4 o; o.x = one(a.x, q.x); o.y = one(a.y, q.y); o.z = one(a.z, q.z); o.w = one(a.w, q.w);
                   if (pp) *reinterpret_cast<f32x4*>(pp + s) = o;
                   if (py) {
                     if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                     *reinterpret_cast<f32x4*>(py + s) = o;
                   }
                 },
                 [&](int64_t s) {
                   const float o = one(px[s], pr ? pr[s] : 0.f);
                   if (pp) pp[s] = o;
                   if (py) py[s] = relu ? fmaxf(o, 0.f) : o;
                 });
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void relu_bwd_add_kernel(
    const float* dy, const float* y_pre, const float* dy2, int64_t S, int64_t sBdy, int64_t sBpre,
    int64_t sBdy2, float* dx, int64_t sBdx) {
  crn_kernargs_now(dy, y_pre, dy2, S, sBdy, sBpre, sBdy2, dx, sBdx);
  const int c = blockIdx.y, b = blockIdx.z;
  const float* pg = dy ? dy + (int64_t)b * sBdy + (int64_t)c * S : nullptr;
  const float* pp = y_pre + (int64_t)b * sBpre + (int64_t)c * S;
  const float* p2 = dy2 ? dy2 + (int64_t)b * sBdy2 + (int64_t)c * S : nullptr;
  float* po = dx + (int64_t)b * sBdx + (int64_t)c * S;
  auto one = [&](float g, float p, float g2) -> float { return (p > 0.f ? g : 0.f) + g2; };
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) {
                   f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f}, g2 = g;
                   if (pg) g = *reinterpret_cast<const f32x4*>(pg + s);
                   const f32x4 p = *reinterpret_cast<const f32x4*>(pp + s);
                   if (p2) g2 = *reinterpret_cast<const f32x4*>(p2 + s);
                   f32x4 o; o.x = one(g.x, p.x, g2.x); o.y = one(g.y, p.y, g2.y);
                   o.z = one(g.z, p.z, g2.z); o.w = one(g.w, p.w, g2.w);
                   *reinterpret_cast<f32x4*>(po + s) = o;
                 },
                 [&](int64_t s) { po[s] = one(pg ? pg[s] : 0.f, pp[s], p2 ? p2[s] : 0.f); });
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void bias_grad_partial_kernel(const float* dy, int64_t S,
                                                                      int64_t sB, double* ws) {
  __shared__ double red[kThreads / 64];
  const int c = blockIdx.y, b = blockIdx.z;
  const float* p = dy + (int64_t)b * sB + (int64_t)c * S;
  double s1 = 0.0;
  for_slice<VEC>(block_slice(S),
                 [&](int64_t s) { const f32x4 v = *reinterpret_cast<const f32x4*>(p + s);
                                  s1 += (double)v.x + (double)v.y + (double)v.z + (double)v.w; },
                 [&](int64_t s) { s1 += (double)p[s]; });
  const double t1 = crn_block_sum(s1, red);
  if (threadIdx.x == 0) {
    const int nparts = gridDim.x * gridDim.z;
    ws[(int64_t)c * nparts + (int64_t)b * gridDim.x + blockIdx.x] = t1;
  }
}

// small tensors (the skip-compress convs: <= 64 k elements per channel): one workgroup owns a channel and reduces it
// over batch and positions -- one launch instead of partial + final
__global__ __launch_bounds__(kThreads) void bias_grad_owner_kernel(const float* dy, int B, int64_t S, int64_t sB,
                                                                    float* db, int accumulate) {
  __shared__ double red[kThreads / 64];
  crn_kernargs_now(dy, B, S, sB, db, accumulate);
  const int c = blockIdx.x;
  double s1 = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* p = dy + (int64_t)b * sB + (int64_t)c * S;
    for (int64_t i = threadIdx.x; i < S; i += kThreads) s1 += (double)p[i];
  }
  const double t1 = crn_block_sum(s1, red);
  if (threadIdx.x == 0) db[c] = accumulate ? db[c] + (float)t1 : (float)t1;
}

__global__ void bias_grad_final_kernel(const double* ws, int nparts, int C, float* db, int accumulate) {
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // a wave per channel
  if (c >= C) return;
  double s = 0.0;
  for (int i = lane; i < nparts; i += 64) s += ws[(int64_t)c * nparts + i];
  s = crn_wave_sum(s);
  if (lane) return;
  if (accumulate) db[c] += (float)s; else db[c] = (float)s;
}

inline bool vec_ok(int64_t S, std::initializer_list<int64_t> strides, std::initializer_list<const void*> ptrs) {
  if (S & 3) return false;
  for (int64_t s : strides) if (s & 3) return false;
  for (const void* p : ptrs) if (p && ((uintptr_t)p & 15)) return false;
  return true;
}

inline int nsplit_for(int64_t S, int C, int B) {
  // enough blocks to fill 256 CUs x 8, >= 4096 elements per block
  constexpr int kWant = 2048;
  int64_t want = std::max<int64_t>(1, kWant / std::max(1, C * B));
  int64_t maxs = std::max<int64_t>(1, S / 4096);
  return (int)std::min<int64_t>(std::min(want, maxs), 64);
}

constexpr int kMaxParts = 64 * 64;   // nsplit(<=64) * B(<=64)

// The launch dispatchers: f gets the compile-time value as a std::integral_constant / std::bool_constant argument.
// NV of the register kernels: the smallest of 1, 2, 4, 8, 16 float4 per thread that hold the B * S values of a channel.
template <typename F>
inline void with_nv(int64_t BS, F f) {
  const int per = (int)crn_cdiv(BS / 4, kThreads);
  if (per <= 1) f(std::integral_constant<int, 1>{}); else if (per <= 2) f(std::integral_constant<int, 2>{});
  else if (per <= 4) f(std::integral_constant<int, 4>{}); else if (per <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}
template <typename F>
inline void with_bool(bool on, F f) {
  if (on) f(std::true_type{}); else f(std::false_type{});
}

// A split-K convolution may have left the partial sums of its output pending (crn_splitk_defer).  If that output is `base`
// and the launch about to be made, on the same stream, is one that can add them up itself (`can_take`: a register kernel, or
// the first pass of a two-pass launch, which stores the sum for the second), it does: *part / *splits say where they are.
// The kernel stores the sum as [B][C][S] with nothing in between: only base, the extents and sB are compared here, the rest
// is the producer's guarantee (a sum is left pending only for a crn_splitk_dense view, splitk.h).  A pending sum meant for
// anything else is flushed first.
int take_or_flush_pending(const float* base, int64_t sB, int B, int C, int64_t S, hipStream_t st, bool can_take,
                          const float** part, int* splits) {
  *part = nullptr; *splits = 0;
  CrnSplitPending& pend = crn_splitk_pending();
  if (!pend.active) return CRN_OK;
  const crnView& py = pend.y;
  if (can_take && pend.stream == st && py.base == base && py.B == B && py.C == C && (int64_t)py.D * py.H * py.W == S && sB == (int64_t)C * S) {
    *part = pend.scratch; *splits = pend.splits; pend.active = false;
    return CRN_OK;
  }
  return crn_splitk_flush(st);
}

// out[c] (+)= sum of src[:, c, :] for c < n in an order that does not depend on how workgroups are scheduled: ns * B fp64
// partial sums per channel into ws, then one wave per channel adds them up.
int bias_grad_ordered(const float* src, int B, int n, int64_t S, int64_t sB, int ns, float* out, int accumulate, double* ws,
                      size_t ws_bytes, hipStream_t st) {
  const int nparts = ns * B;
  if (ws_bytes < (size_t)n * nparts * sizeof(double)) return CRN_ENOMEM;
  with_bool(vec_ok(S, {sB}, {src}), [&](auto vec) {
    hipLaunchKernelGGL(bias_grad_partial_kernel<decltype(vec)::value>, dim3(ns, n, B), dim3(kThreads), 0, st, src, S, sB, ws);
  });
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(bias_grad_final_kernel, dim3(crn_cdiv(n, 4)), dim3(256), 0, st, ws, nparts, n, out, accumulate);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

}  // namespace

extern "C" size_t crn_batch_renorm_workspace_bytes(int C) {
  return (size_t)C * kMaxParts * 2 * sizeof(double);
}

// tail != nullptr: the block tail (crn_affine_add_relu's arguments) is wanted in the same launch; *tail_done says whether
// the launch taken could do it (the register form of the owner kernel), otherwise the caller runs it separately
static int bn_stats_impl(const float* x, int B, int C, int64_t S, int64_t sB, int pre_relu,
                         const float* gamma, const float* beta, float* running_mean,
                         float* running_var, const int64_t* nbt, float eps, float momentum,
                         int training, float* scale, float* shift, float* saved,
                         double* ws, size_t ws_bytes, crnStream stream, const BnTail* tail, bool* tail_done) {
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || B > 64) return CRN_EINVAL;
  if (!x || !gamma || !beta || !running_mean || !running_var || !scale || !shift) return CRN_EINVAL;
  if (training && (!nbt || !saved)) return CRN_EINVAL;
  int nparts = 1;
  const bool reg_form = training && owner_form(S, C, B) && vec_ok(S, {sB}, {x}) && (int64_t)B * S <= 16384;
  // a split-K convolution left the partial sums of x pending (crn_splitk_defer): the register kernel adds them up, or the
  // first pass of the two-pass form (the owner kernel in between reads x twice: it gets the sum flushed)
  // (a launch that is about to fail for want of workspace must not swallow the sum)
  const bool two_pass = training && !owner_form(S, C, B) && ws_bytes >= (size_t)C * nsplit_for(S, C, B) * B * 2 * sizeof(double);
  const float* part;
  int psplits;
  const int rcp = take_or_flush_pending(x, sB, B, C, S, st, reg_form || two_pass, &part, &psplits);
  if (rcp != CRN_OK) return rcp;
  if (reg_form) {
    const bool with_tail = tail && vec_ok(S, {tail->r ? tail->sBr : 0, tail->y_pre ? tail->sBpre : 0, tail->y ? tail->sBy : 0},
                                          {tail->r, tail->y_pre, tail->y});
    with_nv((int64_t)B * S, [&](auto nv) {
      with_bool(with_tail, [&](auto fused) {
        hipLaunchKernelGGL((bn_owner_stats_reg_kernel<decltype(nv)::value, decltype(fused)::value>), dim3(C), dim3(kThreads), 0, st,
                           const_cast<float*>(x), B, C, (int)(S / 4), sB, pre_relu, gamma, beta, running_mean, running_var, nbt,
                           eps, momentum, scale, shift, saved, part, psplits, with_tail ? *tail : BnTail{});
      });
    });
    if (with_tail) *tail_done = true;
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  if (training && owner_form(S, C, B)) {
    with_bool(vec_ok(S, {sB}, {x}), [&](auto vec) {
      hipLaunchKernelGGL(bn_owner_stats_kernel<decltype(vec)::value>, dim3(C), dim3(kThreads), 0, st, x, B, C, S, sB, pre_relu,
                         gamma, beta, running_mean, running_var, nbt, eps, momentum, scale, shift, saved);
    });
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  if (training) {
    const int ns = nsplit_for(S, C, B);
    nparts = ns * B;
    if (ws_bytes < (size_t)C * nparts * 2 * sizeof(double)) return CRN_ENOMEM;
    dim3 grid(ns, C, B);
    with_bool(vec_ok(S, {sB}, {x}), [&](auto vec) {
      with_bool(part != nullptr, [&](auto pend) {
        hipLaunchKernelGGL((bn_partial_kernel<decltype(vec)::value, decltype(pend)::value>), grid, dim3(kThreads), 0, st, x, S, sB,
                           pre_relu, ws, part, psplits);
      });
    });
    CRN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(crn_cdiv(C, 4)), dim3(256), 0, st, ws, nparts, C,
                     (double)B * (double)S, gamma, beta, running_mean, running_var, nbt, eps, momentum,
                     training, scale, shift, saved);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

extern "C" int crn_batch_renorm_stats(const float* x, int B, int C, int64_t S, int64_t sB, int pre_relu,
                                      const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, const int64_t* nbt, float eps, float momentum,
                                      int training, float* scale, float* shift, float* saved,
                                      double* ws, size_t ws_bytes, crnStream stream) {
  return bn_stats_impl(x, B, C, S, sB, pre_relu, gamma, beta, running_mean, running_var, nbt, eps, momentum, training,
                       scale, shift, saved, ws, ws_bytes, stream, nullptr, nullptr);
}

// The second half of crn_batch_renorm_stats alone: the partial sums ws[(c * nparts + i) * 2 + {0, 1}] = sum(x), sum(x^2)
// of part i came out of the launch that produced x (crn_stem_conv_fwd); count = elements per channel.
extern "C" int crn_batch_renorm_finalize(const double* ws, int nparts, int C, double count,
                                         const float* gamma, const float* beta, float* running_mean,
                                         float* running_var, const int64_t* nbt, float eps, float momentum,
                                         float* scale, float* shift, float* saved, crnStream stream) {
  CRN_ENTRY(stream);
  if (!ws || nparts < 1 || nparts > kMaxParts || C < 1 || !(count >= 1.0)) return CRN_EINVAL;
  constexpr int kWide = 512;      // parts per channel from which on
  if (nparts >= kWide && (((uintptr_t)ws) & 15) == 0)
    hipLaunchKernelGGL(bn_finalize_wide_kernel, dim3(C), dim3(kThreads), 0, (hipStream_t)stream, ws, nparts, C, count,
                       gamma, beta, running_mean, running_var, nbt, eps, momentum, scale, shift, saved);
  else
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(crn_cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, ws, nparts, C, count,
                     gamma, beta, running_mean, running_var, nbt, eps, momentum, 1, scale, shift, saved);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

int crn_affine_add_relu_impl(const float* x, const float* scale, const float* shift, const float* r, const float* rscale,
                             const float* rshift, int B, int C, int64_t S, int64_t sB_x, int64_t sB_r, float* y_pre,
                             int64_t sB_pre, float* y, int64_t sB_y, int relu, crnStream stream);

extern "C" int crn_batch_renorm_stats_tail(const float* x, int B, int C, int64_t S, int64_t sB,
                                           const float* gamma, const float* beta, float* running_mean,
                                           float* running_var, const int64_t* nbt, float eps, float momentum,
                                           int training, float* scale, float* shift, float* saved,
                                           double* ws, size_t ws_bytes,
                                           const float* r, const float* rscale, const float* rshift, int64_t sB_r,
                                           float* y_pre, int64_t sB_pre, float* y, int64_t sB_y, int relu,
                                           float* y2, int W, crnStream stream) {
  if (!y && !y_pre) return CRN_EINVAL;      // (no CRN_ENTRY: a pending split-K sum of x is taken over below)
  if (y2 && (!y || W < 1 || S % W || sB_y != (int64_t)C * S)) return CRN_EINVAL;
  const int H = y2 ? (int)(S / W) : 0, H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  const bool y2_fused = y2 && W % 4 == 0 && (((uintptr_t)y2) & 7) == 0;      // (a float4 inside one row, 8-byte stores)
  const BnTail tail{r, rscale, rshift, sB_r, y_pre, sB_pre, y, sB_y, relu, y2_fused ? y2 : nullptr, (int64_t)C * H2 * W2, W, W2, H2};
  bool done = false;
  const int rc = bn_stats_impl(x, B, C, S, sB, 0, gamma, beta, running_mean, running_var, nbt, eps, momentum, training,
                               scale, shift, saved, ws, ws_bytes, stream, &tail, &done);
  if (rc != CRN_OK) return rc;
  if (!done) {
    const int rc2 = crn_affine_add_relu_impl(x, scale, shift, r, rscale, rshift, B, C, S, sB, sB_r, y_pre, sB_pre, y, sB_y, relu, stream);
    if (rc2 != CRN_OK) return rc2;
  }
  if (y2 && !(done && y2_fused)) return crn_stride2_gather(y, y2, B, C, H2, W2, H, W, stream);
  return CRN_OK;
}

extern "C" int crn_batch_renorm_eval_affine(const float* params, const float* buffers, const int32_t* table,
                                            int n, float eps, float* scale, float* shift, crnStream stream) {
  CRN_ENTRY(stream);
  if (n < 0 || (n > 0 && (!params || !buffers || !table || !scale || !shift))) return CRN_EINVAL;
  if (n == 0) return CRN_OK;
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(crn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, params,
                     buffers, table, n, eps, scale, shift);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

int crn_relu_bwd_add_impl(const float* dy, const float* y_pre, const float* dy2, int B, int C, int64_t S, int64_t sB_dy,
                          int64_t sB_pre, int64_t sB_dy2, float* dx, int64_t sB_dx, crnStream stream);

// head != nullptr: dy is to be formed first from (g, act, g2) -- in the same launch where a workgroup owns a channel in
// registers, by crn_relu_bwd_add's kernel otherwise
static int bn_bwd_impl(const float* x, int64_t sB_x, const float* dy, int64_t sB_dy,
                       int B, int C, int64_t S, int pre_relu, int post_relu,
                       const float* gamma, const float* scale, const float* shift,
                       const float* saved, float* dx, int64_t sB_dx, float* dgamma,
                       float* dbeta, int accumulate, float* dsum, int ndsum, double* ws,
                       size_t ws_bytes, crnStream stream, const BnHead* head) {
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || B > 64) return CRN_EINVAL;
  if (!x || !dy || !gamma || !scale || !shift || !saved || !dx || !dgamma || !dbeta) return CRN_EINVAL;
  const bool v = vec_ok(S, {sB_x, sB_dy, sB_dx}, {x, dy, dx});
  // The register-resident owner kernel keeps 16 float4 of x and of dy per thread when a channel has up to 16384 elements: 359
  // registers, i.e. a workgroup that only fits on a CU with NO wave of a weight-gradient kernel (206-250 registers x 2 waves per
  // SIMD) on it.  In the decoder's backward those run beside the data-gradient chain all the time: stage 4's two norms (64 / 112
  // channels = workgroups) took 125-150 us each inside the step against ~35 us alone.  The two-pass form (50 / 46 registers, many
  // workgroups) slots in beside them: step 7.30 -> 7.19 ms.  Applies to the pre-ReLU norms (the decoder's; the encoder's run
  // beside small weight gradients), from 8192 elements per channel on.
  const bool big_dec = pre_relu && !head && (int64_t)B * S > 8192;
  const bool owner_ok = owner_form(S, C, B) && !big_dec;
  const bool reg_form = owner_ok && v && (int64_t)B * S <= 16384;
  if (head) {
    const int rcf = crn_splitk_flush(st);          // (dy is formed here: nothing pending can be meant for this call)
    if (rcf != CRN_OK) return rcf;
    const bool hv = vec_ok(S, {head->sBg, head->sBact, head->g2 ? head->sBg2 : 0}, {head->g, head->act, head->g2});
    BnHead expanded = *head;
    if (head->gc && !(reg_form && hv && head->W % 4 == 0 && (((uintptr_t)head->gc) & 7) == 0)) {
      // the launch below reads the expanded gradient: expand it into the caller's buffer first
      const int H = (int)(S / head->W);
      const int rcs = crn_stride2_scatter(head->gc, const_cast<float*>(head->g), B, C, head->H2, head->W2, H, head->W, stream);
      if (rcs != CRN_OK) return rcs;
      expanded.gc = nullptr;
      head = &expanded;
    }
    if (reg_form && hv) {
      with_nv((int64_t)B * S, [&](auto nv) {
        hipLaunchKernelGGL((bn_owner_bwd_reg_kernel<decltype(nv)::value, true>), dim3(C), dim3(kThreads), 0, st, x, sB_x, dy, sB_dy,
                           B, (int)(S / 4), C, pre_relu, post_relu, gamma, scale, shift, saved, dx, sB_dx, dgamma, dbeta,
                           accumulate, dsum, ndsum, (const float*)nullptr, 0, *head);
      });
      CRN_CHECK_LAUNCH();
      return CRN_OK;
    }
    const int rch = crn_relu_bwd_add_impl(head->g, head->act, head->g2, B, C, S, head->sBg, head->sBact, head->sBg2,
                                          const_cast<float*>(dy), sB_dy, stream);
    if (rch != CRN_OK) return rch;
  }
  // a split-K convolution (a data gradient) left the partial sums of dy pending: the register kernel adds them up, or the
  // first pass of the two-pass form, which also stores the sum to dy for the apply pass
  const float* part;
  int psplits;
  // (a launch that is about to fail for want of workspace must not swallow the sum)
  const bool two_pass = !owner_ok && ws_bytes >= (size_t)C * nsplit_for(S, C, B) * B * 2 * sizeof(double);
  const int rcp = take_or_flush_pending(dy, sB_dy, B, C, S, st, reg_form || two_pass, &part, &psplits);
  if (rcp != CRN_OK) return rcp;
  if (reg_form) {
    with_nv((int64_t)B * S, [&](auto nv) {        // float4 per thread of x and of dy
      hipLaunchKernelGGL(bn_owner_bwd_reg_kernel<decltype(nv)::value>, dim3(C), dim3(kThreads), 0, st, x, sB_x, dy, sB_dy, B,
                         (int)(S / 4), C, pre_relu, post_relu, gamma, scale, shift, saved, dx, sB_dx, dgamma, dbeta, accumulate,
                         dsum, ndsum, part, psplits);
    });
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  if (owner_ok) {
    with_bool(v, [&](auto vec) {
      hipLaunchKernelGGL(bn_owner_bwd_kernel<decltype(vec)::value>, dim3(C), dim3(kThreads), 0, st, x, sB_x, dy, sB_dy, B, S, C,
                         pre_relu, post_relu, gamma, scale, shift, saved, dx, sB_dx, dgamma, dbeta, accumulate, dsum, ndsum);
    });
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  const int ns = nsplit_for(S, C, B);
  const int nparts = ns * B;
  if (ws_bytes < (size_t)C * nparts * 2 * sizeof(double)) return CRN_ENOMEM;
  dim3 grid(ns, C, B);
  // deterministic mode: the ns * B workgroups of a channel add their share of sum(dx) atomically below; instead the
  // sum is taken afterwards by the ordered two-level reduction of crn_bias_grad over dx
  float* const dsum_det = (dsum && ndsum > 0 && crn_deterministic()) ? dsum : nullptr;
  if (dsum_det) dsum = nullptr;
  with_bool(v, [&](auto vec) {
    with_bool(part != nullptr, [&](auto pend) {
      hipLaunchKernelGGL((bn_bwd_partial_kernel<decltype(vec)::value, decltype(pend)::value>), grid, dim3(kThreads), 0, st, x, sB_x,
                         dy, sB_dy, S, C, pre_relu, post_relu, scale, shift, saved, ws, dsum, ndsum, part, psplits);
    });
  });
  CRN_CHECK_LAUNCH();
  with_bool(v, [&](auto vec) {
    hipLaunchKernelGGL(bn_bwd_apply_kernel<decltype(vec)::value>, grid, dim3(kThreads), 0, st, x, sB_x, dy, sB_dy, S, C,
                       pre_relu, post_relu, gamma, scale, shift, saved, ws, nparts,
                       (double)B * (double)S, dx, sB_dx, dgamma, dbeta, accumulate, dsum, ndsum);
  });
  CRN_CHECK_LAUNCH();
  // (ws held 2 * C * nparts doubles above: the ndsum * nparts of this second use fit for ndsum <= 2 * C)
  if (dsum_det) return bias_grad_ordered(dx, B, ndsum, S, sB_dx, ns, dsum_det, 0, ws, ws_bytes, st);
  return CRN_OK;
}

extern "C" int crn_batch_renorm_bwd(const float* x, int64_t sB_x, const float* dy, int64_t sB_dy,
                                    int B, int C, int64_t S, int pre_relu, int post_relu,
                                    const float* gamma, const float* scale, const float* shift,
                                    const float* saved, float* dx, int64_t sB_dx, float* dgamma,
                                    float* dbeta, int accumulate, float* dsum, int ndsum, double* ws,
                                    size_t ws_bytes, crnStream stream) {
  return bn_bwd_impl(x, sB_x, dy, sB_dy, B, C, S, pre_relu, post_relu, gamma, scale, shift, saved, dx, sB_dx, dgamma, dbeta,
                     accumulate, dsum, ndsum, ws, ws_bytes, stream, nullptr);
}

extern "C" int crn_batch_renorm_bwd_apply(const float* x, int64_t sB_x, const float* dy, int64_t sB_dy,
                                          int B, int C, int64_t S, int pre_relu,
                                          const float* gamma, const float* scale, const float* shift,
                                          const float* saved, float* dx, int64_t sB_dx, float* dgamma,
                                          float* dbeta, int accumulate, float* dsum, int ndsum, double* ws,
                                          size_t ws_bytes, int nparts, crnStream stream) {
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || B > 64 || nparts < 1 || !ws) return CRN_EINVAL;
  if (!x || !dy || !gamma || !scale || !shift || !saved || !dx || !dgamma || !dbeta) return CRN_EINVAL;
  if (ws_bytes < (size_t)C * nparts * 2 * sizeof(double)) return CRN_ENOMEM;
  const int ns = nsplit_for(S, C, B);
  // deterministic mode: sum(dx) by the ordered two-level reduction over dx afterwards (as in crn_batch_renorm_bwd); it re-uses
  // `ws` once the apply kernel has read the partial sums -- with few parts given and many slices of its own that second use
  // is the larger one, and it is checked here, before anything is launched
  float* const dsum_det = (dsum && ndsum > 0 && crn_deterministic()) ? dsum : nullptr;
  if (dsum_det && ws_bytes < (size_t)ndsum * ns * B * sizeof(double)) return CRN_ENOMEM;
  { const int rcf = crn_splitk_flush(st); if (rcf != CRN_OK) return rcf; }
  dim3 grid(ns, C, B);
  if (dsum_det) dsum = nullptr;
  with_bool(vec_ok(S, {sB_x, sB_dy, sB_dx}, {x, dy, dx}), [&](auto vec) {
    hipLaunchKernelGGL(bn_bwd_apply_kernel<decltype(vec)::value>, grid, dim3(kThreads), 0, st, x, sB_x, dy, sB_dy, S, C,
                       pre_relu, 0, gamma, scale, shift, saved, ws, nparts,
                       (double)B * (double)S, dx, sB_dx, dgamma, dbeta, accumulate, dsum, ndsum);
  });
  CRN_CHECK_LAUNCH();
  if (dsum_det) return bias_grad_ordered(dx, B, ndsum, S, sB_dx, ns, dsum_det, 0, ws, ws_bytes, st);
  return CRN_OK;
}

extern "C" int crn_batch_renorm_bwd_head(const float* x, int64_t sB_x, float* dy, int64_t sB_dy,
                                         const float* g, int64_t sB_g, const float* act, int64_t sB_act,
                                         const float* g2, int64_t sB_g2,
                                         int B, int C, int64_t S, const float* gamma, const float* scale,
                                         const float* shift, const float* saved, float* dx, int64_t sB_dx,
                                         float* dgamma, float* dbeta, int accumulate, float* dsum, int ndsum,
                                         double* ws, size_t ws_bytes, const float* g_compact, int W, crnStream stream) {
  if (!g || !act || !dy) return CRN_EINVAL;
  if (g_compact && (W < 1 || S % W || sB_g != (int64_t)C * S)) return CRN_EINVAL;
  const int H = g_compact ? (int)(S / W) : 0, H2 = (H + 1) / 2, W2 = (W + 1) / 2;
  const BnHead head{g, sB_g, act, sB_act, g2, sB_g2, g_compact, (int64_t)C * H2 * W2, W, W2, H2};
  return bn_bwd_impl(x, sB_x, dy, sB_dy, B, C, S, 0, 0, gamma, scale, shift, saved, dx, sB_dx, dgamma, dbeta,
                     accumulate, dsum, ndsum, ws, ws_bytes, stream, &head);
}

extern "C" int crn_affine_add_relu(const float* x, const float* scale, const float* shift,
                                   const float* r, const float* rscale, const float* rshift,
                                   int B, int C, int64_t S, int64_t sB_x, int64_t sB_r,
                                   float* y_pre, int64_t sB_pre, float* y, int64_t sB_y, int relu,
                                   crnStream stream) {
  CRN_ENTRY(stream);
  return crn_affine_add_relu_impl(x, scale, shift, r, rscale, rshift, B, C, S, sB_x, sB_r, y_pre, sB_pre, y, sB_y, relu, stream);
}
int crn_affine_add_relu_impl(const float* x, const float* scale, const float* shift, const float* r, const float* rscale,
                             const float* rshift, int B, int C, int64_t S, int64_t sB_x, int64_t sB_r, float* y_pre,
                             int64_t sB_pre, float* y, int64_t sB_y, int relu, crnStream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || (!y && !y_pre)) return CRN_EINVAL;
  dim3 grid(nsplit_for(S, C, B), C, B);
  with_bool(vec_ok(S, {sB_x, r ? sB_r : 0, y_pre ? sB_pre : 0, y ? sB_y : 0}, {x, r, y_pre, y}), [&](auto vec) {
    hipLaunchKernelGGL(affine_add_relu_kernel<decltype(vec)::value>, grid, dim3(kThreads), 0, st, x, scale, shift, r, rscale,
                       rshift, S, sB_x, sB_r, y_pre, sB_pre, y, sB_y, relu);
  });
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

extern "C" int crn_relu_bwd_add(const float* dy, const float* y_pre, const float* dy2, int B, int C,
                                int64_t S, int64_t sB_dy, int64_t sB_pre, int64_t sB_dy2, float* dx,
                                int64_t sB_dx, crnStream stream) {
  CRN_ENTRY(stream);
  return crn_relu_bwd_add_impl(dy, y_pre, dy2, B, C, S, sB_dy, sB_pre, sB_dy2, dx, sB_dx, stream);
}
int crn_relu_bwd_add_impl(const float* dy, const float* y_pre, const float* dy2, int B, int C, int64_t S, int64_t sB_dy,
                          int64_t sB_pre, int64_t sB_dy2, float* dx, int64_t sB_dx, crnStream stream) {
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || !y_pre || !dx) return CRN_EINVAL;
  dim3 grid(nsplit_for(S, C, B), C, B);
  with_bool(vec_ok(S, {dy ? sB_dy : 0, sB_pre, dy2 ? sB_dy2 : 0, sB_dx}, {dy, y_pre, dy2, dx}), [&](auto vec) {
    hipLaunchKernelGGL(relu_bwd_add_kernel<decltype(vec)::value>, grid, dim3(kThreads), 0, st, dy, y_pre, dy2, S, sB_dy,
                       sB_pre, sB_dy2, dx, sB_dx);
  });
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

extern "C" int crn_bias_grad(const float* dy, int B, int C, int64_t S, int64_t sB, float* db,
                             int accumulate, double* ws, size_t ws_bytes, crnStream stream) {
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  if (B < 1 || C < 1 || S < 1 || B > 64) return CRN_EINVAL;
  if ((int64_t)B * S <= 65536) {
    hipLaunchKernelGGL(bias_grad_owner_kernel, dim3(C), dim3(kThreads), 0, st, dy, B, S, sB, db, accumulate);
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  return bias_grad_ordered(dy, B, C, S, sB, nsplit_for(S, C, B), db, accumulate, ws, ws_bytes, st);
}
