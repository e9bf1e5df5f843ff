// fp32 MFMA implicit-GEMM convolution engine for gfx950 (CDNA4).
//
// One stride-1 window correlation over a logical NCDHW view; Conv2d / Conv3d /
// ConvTranspose3d forward + data-gradient + weight-gradient of the reference
// (resnet50.py:62-69,95-107,124; reconstruction_decoder.py:49-95;
// ray_traced_skip_connection.py:38) all map onto it through views and packed
// weights built by corenet_amd/model/conv_geometry.py.
//
// Design (MI355X-first, not a cuDNN/im2col translation):
//  * A workgroup (4 waves) owns a TDxTHxTW tile of output positions and an
//    N-tile of NSUB*16 output channels.  For each chunk of CC input channels it
//    stages the raw input PATCH (tile + window halo) and the weight chunk in
//    LDS once, then walks the window taps: every tap is an LDS *offset*, not a
//    new gather, so each HBM/L2 byte of the patch feeds kd*kh*kw*N MACs.
//  * v_mfma_f32_16x16x4_f32: rows = 16 output positions (an mh x mw sub-tile),
//    cols = 16 output channels, k = 4 input channels at one tap.  Exact fp32
//    (the reference is fp32 end to end), 157 TF/s peak.
//  * Register-staged software pipeline: the global loads of chunk c+1 are
//    issued into VGPRs before the MFMA loop of chunk c and written to LDS after
//    it, so HBM/L2 latency hides under the matrix pipe (cdna guide T14).
//  * LDS strides are padded to 16 (mod 32) banks so the two 32-lane halves of a
//    ds_read_b32 (k = 0,1 / 2,3) never collide.
//  * BatchRenorm-apply + ReLU of the producer are fused into the patch staging
//    (crnInTransform), so normalised activations are never written to HBM.
#include "conv_kernels.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>

namespace {
using namespace crnk;

// --------------------------- pointwise (1x1x1) convolutions ---------------------------------
// Y[b][n][m] = bias[n] + sum_c W[c][n] * T(X[b][c][m]) for plain views with contiguous positions:
// a GEMM whose A operand is already K-major in memory (NCHW), so global loads are float4 rows
// and no index arithmetic is needed.  Block = 64 positions x 32 channels, K chunks of 32 staged
// through LDS with register prefetch; wave w owns positions [16w, 16w+16) x 32 channels.
// Used for ResNet 1x1 convs and their data gradients (resnet50.py:62-69,95-107) and the skip
// compress convs (ray_traced_skip_connection.py:38).
struct PwGeom {
  const float* x; float* y; const float* w; const float* bias;
  crnInTransform tr;
  int B, C, N, Npad, S;            // S = positions per sample
  int64_t xsB, ysB;                // batch strides; x channel stride = S
  int64_t ysC, ysP;                // y channel / position strides: (S, 1) plain, (1, row pitch) channel-last
  int bias_sB, mode;
  int splits, cps;                 // split-K: blockIdx.z = split*B + b, cps input channels per split (multiple
                                   // of 32); partial sums go to the dense scratch y (mode 0), split*B + b as batch
  long long* stamps;               // tuning aid (CRN_PW_STAMPS=1): shader-clock stamps of workgroup 0
  // PAIR launches (crn_conv1x1_fwd_pair): a second K source.  Channels [0, C1) of the reduction are rows of x / w, channels
  // [C1, C) rows C - C1.. of x2 / w2 (same S and Npad); C1 % 64 == 0 and cps % 64 == 0, so a chunk never straddles the two
  const float* x2; const float* w2;
  int64_t x2sB;
  int C1;
};

constexpr int kPwBM = 64;           // positions of one workgroup
constexpr int kPwBN = 32;           // output columns of one workgroup (64 x 32 tiles)
constexpr int kPwKC = 64;           // input channels of one chunk (KC 64: half the barriers of KC 32)
constexpr int kPwPad = 16;          // LDS row pad of both operands: 16 (mod 32) banks
constexpr int kPwTab = 2048;        // channels of one workgroup (its split's range) whose scale / shift are staged in LDS
constexpr int kPwLds = kPwKC * (kPwBM + kPwPad + kPwBN + kPwPad) * 4;   // static LDS of the kernel: both operand chunks
// NS = 16-column blocks per workgroup (kPwBN / 16); PAIR: two K sources onto one output (PwGeom), no input transform
template <int NS, bool PAIR = false>
__global__ __launch_bounds__(256) void pointwise_fwd_kernel(PwGeom g) {
  constexpr int BM = kPwBM, BN = NS * 16, KC = kPwKC, SA = BM + kPwPad, SB = BN + kPwPad;
  constexpr int NRA = KC / 16;
  __shared__ __attribute__((aligned(16))) float ldsA[KC * SA];
  __shared__ __attribute__((aligned(16))) float ldsB[KC * SB];
  static_assert(NS * 16 != kPwBN || sizeof(ldsA) + sizeof(ldsB) == kPwLds, "");
  crn_kernargs_now(g.x, g.y, g.w, g.bias, g.tr.scale, g.tr.shift, g.tr.pre_relu, g.tr.post_relu, g.B, g.C, g.N, g.Npad,
                   g.S, g.xsB, g.ysB, g.ysC, g.ysP, g.bias_sB, g.mode, g.splits, g.cps);
  if (PAIR) crn_kernargs_now(g.x2, g.w2, g.x2sB, g.C1);
  const long long t_entry = (long long)__builtin_amdgcn_s_memtime();
  const long long r_entry = (long long)__builtin_amdgcn_s_memrealtime();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kk = lane >> 4;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const bool stamp = g.stamps && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0;
  int nmark = 0;
  auto mark = [&]() { if (stamp && nmark < 30) g.stamps[nmark] = (long long)__builtin_amdgcn_s_memtime() - t_entry; ++nmark; };
  mark();
  const int split = blockIdx.z / g.B, b = blockIdx.z - split * g.B;
  const int cbeg = split * g.cps, cend = min(g.C, cbeg + g.cps);
  const float* xb = g.x + (int64_t)b * g.xsB;
  // staging roles: A: KC/16 float4 per thread (rows ka, ka+16, ...), B: NRB float4 per thread
  const int ka = tid >> 4, ca = (tid & 15) * 4;       // A row / column
  constexpr int BQ = BN / 4, BROWS = 256 / BQ, NRB = KC / BROWS;   // B: float4 per row, rows per pass, passes (1 or 2)
  const int kb = tid / BQ, cb = (tid % BQ) * 4;       // B row / column
  const bool a_ok = (m0 + ca) < g.S;                  // S % 4 == 0 (checked on the host)
  const bool b_ok = (n0 + cb) < g.Npad;
  // Two chunks of loads are in flight (a chunk's MFMAs take 0.45 us, a load 1-2 us: with one chunk in flight every
  // iteration waited out most of a memory latency), hand-tracked like in conv_e2d.hip: asm buffer loads, s_waitcnt
  // vmcnt(N) with the N the issue order implies, out-of-range offsets (zeros, no traffic) past the end.  The
  // BatchRenorm scale / shift of the workgroup's channels are staged into LDS once, next to the first loads (read from
  // global inside the loop they cost another exposed latency per chunk).
  // (dynamic LDS, 2 * cps floats: static tables for 2048 channels took a third of the kernel's LDS and with it the
  // fourth and fifth resident workgroup -- and residency is what these latency chains are short of, see the host side)
  extern __shared__ float pw_tables[];
  const bool has_tr = g.tr.scale != nullptr;
  float* tsc = pw_tables; float* tsh = pw_tables + g.cps;
  constexpr unsigned kOOBo = 0x80000000u;
  constexpr int NL = NRA + NRB;                      // loads per thread and chunk
  const crn_rsrc xrs = crnk::make_rsrc(xb);
  const crn_rsrc wrs = crnk::make_rsrc(g.w);
  // PAIR: the descriptors of the second source, built once; which pair a chunk reads is uniform (c0 and C1 are scalars)
  const crn_rsrc x2rs = crnk::make_rsrc(PAIR ? g.x2 + (int64_t)b * g.x2sB : xb);
  const crn_rsrc w2rs = crnk::make_rsrc(PAIR ? g.w2 : g.w);
  f32x4 ra[2][NRA], rb[2][NRB];
  auto issue = [&](int c0, f32x4 (&pa_)[NRA], f32x4 (&pb_)[NRB]) {
    const bool second = PAIR && c0 >= g.C1;
    const crn_rsrc ars = second ? x2rs : xrs;
    const crn_rsrc brs = second ? w2rs : wrs;
    const int cs = second ? g.C1 : 0;                  // first row of the chunk's source in the concatenated K
#pragma unroll
    for (int q = 0; q < NRA; ++q) {
      const int c_a = c0 + ka + q * 16;
      const unsigned off = (a_ok && c_a < cend) ? (unsigned)((c_a - cs) * g.S + m0 + ca) * 4u : kOOBo;
      crnk::crn_bload4(pa_[q], ars, off);
    }
#pragma unroll
    for (int q = 0; q < NRB; ++q) {
      const int c_b = c0 + kb + q * BROWS;
      const unsigned off = (b_ok && c_b < cend) ? (unsigned)((c_b - cs) * g.Npad + n0 + cb) * 4u : kOOBo;
      crnk::crn_bload4(pb_[q], brs, off);
    }
  };
  auto wait_slot = [&](f32x4 (&pa_)[NRA], f32x4 (&pb_)[NRB]) {   // the other slot's NL loads were issued later
#pragma unroll
    for (int q = 0; q < NRA; ++q) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pa_[q]) : "n"(NL));
#pragma unroll
    for (int q = 0; q < NRB; ++q) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pb_[q]) : "n"(NL));
  };
  auto xform = [&](f32x4 v, int c) -> f32x4 {
    if (has_tr && a_ok && c < cend) {
      const float sc = tsc[c - cbeg], sh = tsh[c - cbeg];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = in_transform(v[i], g.tr.pre_relu, sc, sh, g.tr.post_relu);
    }
    return v;
  };
  f32x4 acc[NS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns) acc[ns] = (f32x4){0.f, 0.f, 0.f, 0.f};
  issue(cbeg, ra[0], rb[0]);
  issue(cbeg + KC, ra[1], rb[1]);
  mark();
  if (has_tr)
    for (int c = tid; c < cend - cbeg; c += 256) { tsc[c] = g.tr.scale[cbeg + c]; tsh[c] = g.tr.shift[cbeg + c]; }
  auto step = [&](int c0, f32x4 (&pa_)[NRA], f32x4 (&pb_)[NRB]) {
    wait_slot(pa_, pb_);
    mark();
    __syncthreads();                                   // (first step: the tables; later: the previous chunk's MFMA reads)
#pragma unroll
    for (int q = 0; q < NRA; ++q) *reinterpret_cast<f32x4*>(ldsA + (ka + q * 16) * SA + ca) = xform(pa_[q], c0 + ka + q * 16);
#pragma unroll
    for (int q = 0; q < NRB; ++q) *reinterpret_cast<f32x4*>(ldsB + (kb + q * BROWS) * SB + cb) = pb_[q];
    __syncthreads();
    mark();
    issue(c0 + 2 * KC, pa_, pb_);                      // this slot's registers are free: the chunk after the next
    const float* pa = ldsA + kk * SA + wave * 16 + i16;
    const float* pb = ldsB + kk * SB + i16;
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const float a = pa[ks * 4 * SA];
      float bv[NS];
#pragma unroll
      for (int ns = 0; ns < NS; ++ns) bv[ns] = pb[ks * 4 * SB + ns * 16];
#pragma unroll
      for (int ns = 0; ns < NS; ++ns) acc[ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[ns], acc[ns], 0, 0, 0);
    }
    mark();
  };
  for (int c0 = cbeg; c0 < cend; c0 += 2 * KC) {
    step(c0, ra[0], rb[0]);
    if (c0 + KC < cend) step(c0 + KC, ra[1], rb[1]);
  }
  // the loads issued past the end (zeros) still target the staging registers: keep them allocated until they landed
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
#pragma unroll
    for (int q = 0; q < NRA; ++q) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[sl][q]));
#pragma unroll
    for (int q = 0; q < NRB; ++q) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rb[sl][q]));
  }
  // D: rows kk*4..kk*4+3 = 4 consecutive positions, col i16 = channel -> one float4 per lane
  const int m = m0 + wave * 16 + kk * 4;
  if (m < g.S) {
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
      const int n = n0 + ns * 16 + i16;
      if (n < g.N) {
        const float bsv = (g.bias && split == 0) ? g.bias[(int64_t)b * g.bias_sB + n] : 0.f;
        float* dst = g.y + (int64_t)(split * g.B + b) * g.ysB + (int64_t)n * g.ysC + (int64_t)m * g.ysP;
        f32x4 v = acc[ns] + bsv;
        if (g.ysP == 1) {
          if (g.mode == 1) v += *reinterpret_cast<const f32x4*>(dst);
          *reinterpret_cast<f32x4*>(dst) = v;
        } else {          // channel-last output: the 16 lanes of a row group write 16 consecutive channels
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[i * g.ysP] = g.mode == 1 ? dst[i * g.ysP] + v[i] : v[i];
        }
      }
    }
  }
  if (stamp) {
    g.stamps[31] = (long long)__builtin_amdgcn_s_memtime() - t_entry;
    g.stamps[30] = (long long)__builtin_amdgcn_s_memrealtime() - r_entry;      // 100 MHz: cycles / this = shader clock
  }
}

// --------------------------- dense layers on 1^3 grids ------------------------------------------------------
// decoder stage_1 (reconstruction_decoder.py:52-54): ConvTranspose3d(k=4) from a 1^3 grid = a dense layer from
// 67 channels onto 16384 logical channels, i.e. ONE position per sample.  The tile engine needs 16 positions per
// MFMA row block and spent 67 / 76 / 47 us (forward / data gradient / weight gradient) on 1.1 M multiply-adds per
// sample; these three loops are bandwidth bound on the 4.4 MB of weights instead.
constexpr int kDenseB = 8;      // samples per launch
constexpr int kDenseColsLds = 3 * kDenseB * 64 * 4;   // static LDS of dense_cols_kernel: the partial sums of waves 1..3
// many output columns, few input channels: a workgroup owns 64 columns, its four waves split the input channels (one
// thread per column and 256 columns per workgroup left 192 CUs idle and walked the 67 rows in three batches of loads:
// 25 us for 4.4 MB of weights); the weight rows of a thread are in flight before the inputs are staged
__global__ __launch_bounds__(256) void dense_cols_kernel(const float* x, int64_t xsB, int64_t xsC, crnInTransform tr,
                                                         const float* w, int Npad, int N, int C, int B,
                                                         const float* bias, int bias_sB, float* y, int64_t ysB,
                                                         int64_t ysC, int accumulate) {
  extern __shared__ float xs[];                        // [B][C] transformed inputs
  __shared__ float red[3][kDenseB][64];
  static_assert(sizeof(red) == kDenseColsLds, "");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + lane;
  const int cq = (C + 3) >> 2, cbeg = wave * cq, cend = min(C, cbeg + cq);
  const bool col = n < N;
  float wv[32];
#pragma unroll
  for (int u = 0; u < 32; ++u) wv[u] = (col && cbeg + u < cend) ? w[(int64_t)(cbeg + u) * Npad + n] : 0.f;
  for (int i = threadIdx.x; i < B * C; i += blockDim.x) {
    const int b = i / C, c = i - b * C;
    float v = x[b * xsB + c * xsC];
    if (tr.scale) v = in_transform(v, tr.pre_relu, tr.scale[c], tr.shift[c], tr.post_relu);
    xs[i] = v;
  }
  __syncthreads();
  float acc[kDenseB];
#pragma unroll
  for (int b = 0; b < kDenseB; ++b) acc[b] = 0.f;
  for (int c = cbeg; c < cend; c += 32) {
    if (c > cbeg) {
#pragma unroll
      for (int u = 0; u < 32; ++u) wv[u] = (col && c + u < cend) ? w[(int64_t)(c + u) * Npad + n] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 32; ++u)
#pragma unroll
      for (int b = 0; b < kDenseB; ++b)
        if (b < B && c + u < cend) acc[b] += xs[b * C + c + u] * wv[u];
  }
  if (wave) {
#pragma unroll
    for (int b = 0; b < kDenseB; ++b) red[wave - 1][b][lane] = acc[b];
  }
  __syncthreads();
  if (wave || !col) return;
#pragma unroll
  for (int b = 0; b < kDenseB; ++b)
    if (b < B) {
      float* d = y + b * ysB + n * ysC;
      const float v = ((acc[b] + red[0][b][lane]) + (red[1][b][lane] + red[2][b][lane])) +
                      (bias ? bias[(int64_t)b * bias_sB + n] : 0.f);
      *d = accumulate ? *d + v : v;
    }
}
// few output columns, many input channels: a workgroup owns (sample b, 8 columns), its 256 threads stride over the
// channels (two float4 of weights per channel), and the 256 partial sums of every column are added in the workgroup
__global__ __launch_bounds__(256) void dense_rows_kernel(const float* x, int64_t xsB, int64_t xsC, const float* w,
                                                         int Npad, int N, int C, const float* bias, int bias_sB,
                                                         float* y, int64_t ysB, int64_t ysC, int accumulate,
                                                         int cps) {
  // blockIdx.z = slice of cps input channels (gridDim.z > 1: y was zeroed / holds the accumulation base and every
  // slice adds its part atomically -- 36 workgroups walking 32768 rows each took 47 us)
  __shared__ float red[4][8];
  const int b = blockIdx.y, n0 = blockIdx.x * 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const float* xb = x + b * xsB;
  const int cbeg = blockIdx.z * cps, cend = min(C, cbeg + cps);
#pragma unroll 4
  for (int c = cbeg + threadIdx.x; c < cend; c += 256) {
    const float xv = xb[c * xsC];
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + (int64_t)c * Npad + n0);
    const f32x4 w1 = *reinterpret_cast<const f32x4*>(w + (int64_t)c * Npad + n0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc[j] += xv * w0[j]; acc[4 + j] += xv * w1[j]; }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = crn_wave_sum(acc[j]);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8 && n0 + (int)threadIdx.x < N) {
    const int n = n0 + threadIdx.x;
    float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (bias && blockIdx.z == 0) v += bias[(int64_t)b * bias_sB + n];
    float* d = y + b * ysB + n * ysC;
    if (gridDim.z > 1) atomicAdd(d, v);
    else *d = accumulate ? *d + v : v;
  }
}
// weight gradient: dw[c][n] += sum_b T(x)[b][c] * dy[b][n]
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const float* x, int64_t xsB, int64_t xsC, crnInTransform tr,
                                                          const float* dy, int64_t dsB, int64_t dsC, float* dw,
                                                          int Npad, int N, int C, int B) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (n >= N) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    float v = x[b * xsB + c * xsC];
    if (tr.scale) v = in_transform(v, tr.pre_relu, tr.scale[c], tr.shift[c], tr.post_relu);
    acc += v * dy[b * dsB + n * dsC];
  }
  dw[(int64_t)c * Npad + n] += acc;
}

bool one_position(const crnView& v) { return v.D == 1 && v.H == 1 && v.W == 1 && v.chan_off == nullptr; }

// 16-byte staging: unit W stride and every offset a multiple of 4 floats
bool vec_view(const crnView& v) {
  return v.chan_off == nullptr && v.sW == 1 && (v.W & 3) == 0 && (v.sH & 3) == 0 && (v.sD & 3) == 0 &&
         (v.sC & 3) == 0 && (v.sB & 3) == 0 && (((uintptr_t)v.base) & 15) == 0;
}
int vec_lead(int pw) { return ((-pw) % 4 + 4) % 4; }   // (w0 - pw - lead) % 4 == 0 for 4-aligned tile origins

// y of a pointwise conv: positions flatten to one index with a single stride (plain: 1; channel-last
// [B][pos][C]: the pixel pitch), channels have their own stride
bool flat_out_view(const crnView& v) {
  if (plain_view(v)) return true;
  return v.chan_off == nullptr && v.sH == (int64_t)v.W * v.sW && (v.D == 1 || v.sD == (int64_t)v.H * v.W * v.sW) &&
         v.sC >= 1 && v.sW >= 1;
}

__global__ void zero_view_kernel(crnView v) {
  const int64_t per_b = (int64_t)v.C * v.D * v.H * v.W;
  const int64_t total = per_b * v.B;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = e;
    const int w = r % v.W; r /= v.W;
    const int h = r % v.H; r /= v.H;
    const int d = r % v.D; r /= v.D;
    const int c = r % v.C; r /= v.C;
    const int64_t co = v.chan_off ? (int64_t)v.chan_off[c] : (int64_t)c * v.sC;
    v.base[r * v.sB + co + (int64_t)d * v.sD + (int64_t)h * v.sH + (int64_t)w * v.sW] = 0.f;
  }
}

int ilog2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
unsigned magic20(int d) { return (unsigned)(((1u << 20) + d - 1) / d); }
// staging slots (planes padded to a power of two) needed for nplanes planes of `plane` elements
int stage_passes(int nplanes, int plane) {
  if (plane > 512) return 1 << 30;      // staging handles planes padded to at most 512 slots
  return crn_cdiv((int64_t)nplanes << ilog2_ceil(plane), 256);
}

int pad16mod32(int v) {  // smallest v' >= v with v' % 32 == 16
  int r = v % 32;
  return r <= 16 ? v + (16 - r) : v + (48 - r);
}

constexpr size_t kLdsBudget = 72 * 1024;   // 2 workgroups per CU (160 KiB LDS)

// ---------------- forward configuration search -------------------------------
struct FwdCfg {
  int MSUB, NSUB, CC, mw, mh, tsd, tsh, tsw;
  int PSP;                   // LDS channel stride of the patch
  int64_t blocks;
  size_t lds;
};

// Sub-tile = 1 x mh x mw output positions (16 MFMA rows); tile = tsd x tsh x tsw sub-tiles.
// lead >= 0: vector staging with `lead` extra patch columns on the left (units of `unit` = 4 positions for
// unit-stride views, 2 for stride-2 space-to-depth views); lead < 0: scalar staging
int patch_width(int TW, int kw, int lead, int unit) {
  return lead < 0 ? TW + kw - 1 : (lead + TW + kw - 1 + unit - 1) / unit * unit;
}

crnInTransform tr_or_none(const crnInTransform* tr) { return tr ? *tr : crnInTransform{nullptr, nullptr, 0, 0}; }

// The one patch geometry of a launch: the patch of a TD x TH x TW tile under a kd x kh x kw window, staged in 16-byte
// units of `unit` positions with `lead` extra columns (lead >= 0) or as scalars (lead < 0), CC channels at a time,
// PSP floats apart in LDS.
void fill_patch(PatchDesc& p, const crnView& x, const crnInTransform* tr, int pd, int ph, int pw, int TD, int TH, int TW,
                int kd, int kh, int kw, int lead, int unit, int CC, int PSP) {
  p.x = x; p.tr = tr_or_none(tr);
  p.lead = lead >= 0 ? lead : 0;
  p.pd = pd; p.ph = ph; p.pw = pw + p.lead;
  p.PD = TD + kd - 1; p.PH = TH + kh - 1; p.PW = patch_width(TW, kw, lead, unit);
  p.plane = p.PH * p.PW; p.PSP = PSP;
  p.lg2 = ilog2_ceil(p.plane); p.npass = lead >= 0 ? 0 : stage_passes(CC * p.PD, p.plane);
  p.magic_PW = magic20(p.PW); p.magic_PD = magic20(p.PD);
  if (lead >= 0) {
    p.plu = p.plane / unit; p.pw4 = p.PW / unit; p.nunits = CC * p.PD * p.plu;
    p.magic_PLU = magic20(p.plu); p.magic_PW4 = magic20(p.pw4);
  }
}

bool fwd_cfg(int MSUB, int NSUB, int B, int Cin, int Npad, int D, int H, int W, int kd, int kh, int kw, int lead,
             int unit, FwdCfg* out) {
  FwdCfg c;
  c.MSUB = MSUB; c.NSUB = NSUB;
  c.mw = W >= 16 ? 16 : (W >= 8 ? 8 : (W >= 4 ? 4 : (W >= 2 ? 2 : 1)));
  c.mh = 16 / c.mw;
  const int want = 4 * MSUB;
  const int T = kd * kh * kw;
  double best = 1e300;
  c.tsd = 1; c.tsh = 1; c.tsw = want;
  for (int a = 1; a <= want; a *= 2)
    for (int bq = 1; a * bq <= want; bq *= 2) {
      const int cw = want / (a * bq);
      const int TD = a, TH = bq * c.mh, TW = cw * c.mw;
      const double tiles = (double)crn_cdiv(D, TD) * crn_cdiv(H, TH) * crn_cdiv(W, TW);
      const double patch = (double)(TD + kd - 1) * (TH + kh - 1) * patch_width(TW, kw, lead, unit);
      const double cost = tiles * (patch + 0.25 * TD * TH * TW);   // loads + wasted MFMA rows
      if (cost < best) { best = cost; c.tsd = a; c.tsh = bq; c.tsw = cw; }
    }
  const int TD = c.tsd, TH = c.tsh * c.mh, TW = c.tsw * c.mw;
  if (lead >= 0 && (TW % unit)) return false;
  const int PDp = TD + kd - 1, plane = (TH + kh - 1) * patch_width(TW, kw, lead, unit);
  const int PS = PDp * plane;
  const int PSP = pad16mod32(PS), WSP = pad16mod32(T * NSUB * 16);
  auto fits = [&](int cc) {
    const bool staged = lead >= 0 ? (int64_t)cc * PS / unit <= 256 * NVX : stage_passes(cc * PDp, plane) <= PREG;
    return (size_t)cc * (PSP + WSP) * 4 + 2 * kChTab * 4 <= kLdsBudget && staged &&
           (int64_t)cc * T * NSUB * 16 <= 256 * WREG * 4;
  };
  if (!fits(4)) return false;
  int CC = 4;
  const int cin4 = (Cin + 3) & ~3;
  while (CC * 2 <= cin4 && CC * 2 <= 64 && fits(CC * 2)) CC *= 2;
  c.CC = CC; c.PSP = PSP;
  c.lds = (size_t)CC * (PSP + WSP) * 4 + 2 * kChTab * 4;
  c.blocks = (int64_t)B * crn_cdiv(D, TD) * crn_cdiv(H, TH) * crn_cdiv(W, TW) * crn_cdiv(Npad, NSUB * 16);
  *out = c;
  return true;
}

// ---------------- forward plan: which kernel a call gets ---------------------
// Host arithmetic on the views' extents, strides and alignment only: crn_conv_fwd launches what fwd_select says, and
// crn_conv_fwd_plan reports it, so there is one copy of the selection.
int fwd_check_args(const crnView* x, const float* w, int Npad, const crnView* y, int kd, int kh, int kw,
                   const crnTapBoxes* boxes) {
  if (boxes && (boxes->n_groups < 0 || boxes->n_groups > 8 || boxes->c_groups < 0 || boxes->c_groups > 8)) return CRN_EINVAL;
  if (!x || !y || !w || Npad <= 0 || (Npad & 15) || x->B != y->B || kd < 1 || kh < 1 || kw < 1)
    return CRN_EINVAL;
  if (y->C > Npad) return CRN_EINVAL;
  return CRN_OK;
}

struct FwdSel {
  int path;                  // CRN_PLAN_*
  int zs;                    // dense_rows: slices of the input channels
  int pw_splits, pw_cps;     // pointwise: K splits to ask the scratch for (1: none) and their channels
  int pw_cps_whole;          // ... channels of the only split when the launch does not split
  FwdCfg cfg;                // generic: tile configuration,
  int xvec, lead, unit;      // staging of x (0 scalar, 1 float4 units, 2 position pairs), its left lead (-1: scalar) and the
                             // positions per 16-byte unit (4 or 2),
  bool forced;               // scalar staging because no 16-byte configuration fits,
  int splits, nchunks;       // splits of the nchunks channel chunks the launch asks for
};

// epilogue of the generic kernels: float4 stores (y = the tensor actually written, the scratch view when splitting)
bool fwd_vec_store(const crnView& y, int mw, int mode) {
  return y.sW == 1 && mw >= 4 && (y.W & 3) == 0 && (y.sH & 3) == 0 && (y.sD & 3) == 0 && (y.sB & 3) == 0 &&
         (y.sC & 3) == 0 && (((uintptr_t)y.base) & 15) == 0 && y.chan_off == nullptr && mode != 2;
}

// K splits a pointwise launch over C channels asks for when its output grid has `blocks` workgroups (1: none): long
// reductions over few positions split their channels to fill the chip.  One copy for crn_conv_fwd's 1x1 path and
// crn_conv1x1_fwd_pair; each rounds the channels per split to its own chunk.
int pw_auto_splits(int C, int64_t blocks) {
  constexpr int pw_blocks = 256, pw_fill = 512, pw_minc = 128;
  if (blocks >= pw_blocks || C < 2 * pw_minc) return 1;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(C / pw_minc, 16), crn_cdiv(pw_fill, blocks)));
}

// Launch tail of both pointwise entry points: pw_split, then pw_launch.  p describes the unsplit launch onto y (S positions
// per sample); with splits > 1, and the scratch to be had, the partial sums over cps channels each go to the dense scratch
// instead (p.y) and crn_splitk_finish adds them up (or hands them to the BatchRenorm launch the caller armed).
void pw_split(PwGeom& p, const crnView& y, int64_t S, int splits, int cps, hipStream_t st) {
  float* scratch = splits > 1 ? crn_splitk_scratch((size_t)splits * y.B * y.C * S, st) : nullptr;
  if (scratch) {
    p.splits = splits; p.cps = cps;
    p.y = scratch; p.ysB = (int64_t)y.C * S; p.ysC = S; p.ysP = 1; p.mode = 0;
  }
}
template <bool PAIR>
int pw_launch(const PwGeom& p, const crnView& y, int64_t S, int accumulate, bool armed, hipStream_t st) {
  float* scratch = p.splits > 1 ? p.y : nullptr;
  dim3 grid((unsigned)crn_cdiv(S, kPwBM), (unsigned)crn_cdiv(y.C, kPwBN), (unsigned)(y.B * p.splits));
  const size_t tab_bytes = p.tr.scale ? (size_t)2 * p.cps * sizeof(float) : 0;
  hipLaunchKernelGGL((pointwise_fwd_kernel<kPwBN / 16, PAIR>), grid, dim3(256), tab_bytes, st, p);
  CRN_CHECK_LAUNCH();
  return p.splits > 1 ? crn_splitk_finish(y, scratch, p.splits, accumulate, armed, st) : CRN_OK;
}

int fwd_select(const crnView* x, const crnInTransform* tr, const float* w, int Npad, const crnView* y,
               int kd, int kh, int kw, int pd, int ph, int pw, int splits, FwdSel* s) {
  *s = FwdSel{};
  const int64_t Sx = (int64_t)x->D * x->H * x->W;
  const bool has_scale = tr && tr->scale;
  if (kd * kh * kw == 1 && pd == 0 && ph == 0 && pw == 0 && splits <= 1 && one_position(*x) && one_position(*y) &&
      x->B <= kDenseB) {
    if (y->C >= 1024 && x->C <= 2048) { s->path = CRN_PLAN_DENSE_COLS; return CRN_OK; }   // wide output: a thread per column
    if (y->C <= 256 && !has_scale && x->C >= 1024) {   // long reduction onto few columns
      s->path = CRN_PLAN_DENSE_ROWS;
      s->zs = (y->sC == 1 && y->sB >= y->C && !crn_deterministic()) ? std::max(1, std::min(16, x->C / 2048)) : 1;   // slices of >= 2048 rows
      return CRN_OK;
    }
  }
  if (kd * kh * kw == 1 && pd == 0 && ph == 0 && pw == 0 && splits <= 1 && plain_view(*x) && flat_out_view(*y) &&
      Sx == (int64_t)y->D * y->H * y->W && (Sx & 3) == 0 && (((uintptr_t)w) & 15) == 0 &&
      (int64_t)x->C * Sx * 4 < ((int64_t)1 << 31) && (int64_t)x->C * Npad * 4 < ((int64_t)1 << 31) &&
      (!has_scale || x->C <= kPwTab)) {           // (buffer offsets of the hand-tracked loads; the LDS tables)
    s->path = CRN_PLAN_POINTWISE;
    s->pw_splits = 1; s->pw_cps = s->pw_cps_whole = (x->C + 63) & ~63;
    // long reductions over few positions (stage4/5 of the encoder: K = 1024..2048, 64..256 positions per sample):
    // split the channels over blocks, partial sums to the split-K scratch, one reduction launch
    // (64-column tiles were measured equal to 32-column ones on the whole step, 10.07 vs 10.04 ms: these launches are
    // latency bound, not operand-traffic bound)
    const int64_t blocks = crn_cdiv(Sx, kPwBM) * crn_cdiv(y->C, kPwBN) * (int64_t)x->B;
    if (splits < 1) {
      int sp = pw_auto_splits(x->C, blocks);
      if (sp > 1) {
        const int cps = (crn_cdiv(x->C, sp) + 31) & ~31;
        sp = crn_cdiv(x->C, cps);
        if (sp > 1) { s->pw_splits = sp; s->pw_cps = cps; }
        s->pw_cps_whole = (x->C + 31) & ~31;
      }
    }
    return CRN_OK;
  }
  s->path = CRN_PLAN_GENERIC;
  // Score every (MSUB, NSUB) tile: useful MFMA rows x operand reuse of the tile x how well
  // the grid (with split-K as a fallback) fills 256 CUs.
  static const int kM[4] = {8, 4, 2, 1};
  static const int kN[3] = {4, 2, 1};
  // staging of x: float4 units (unit-stride views), position pairs (stride-2 space-to-depth views), scalars
  const int xmode = vec_view(*x) ? 1 : ((x->sW == 2 && (x->W & 1) == 0) ? 2 : 0);   // s2d views and stride-2 views
  const int unit = xmode == 2 ? 2 : 4;
  const int lead = xmode == 1 ? vec_lead(pw) : (xmode == 2 ? ((pw % 2) + 2) % 2 : -1);
  // Estimated cycles per CU (calibrated on tools/sweep_fwd.sh): work that adds up on the SIMDs
  // (MFMA issue at ~77% + staging instructions, which do not hide under MFMAs) plus one exposed
  // load->commit->barrier latency per chunk and pair of resident workgroups; split-K pays a
  // zero-fill launch and an atomic epilogue.
  // split-K now costs one small reduction launch (tuned on bench.py: 20000 / 512 beat 40000 / 256 by 0.3 ms)
  constexpr double kSplitPenalty = 20000.0;
  constexpr int kSplitFill = 512;
  FwdCfg best{}; bool have = false; double best_cost = 1e300; int best_splits = 1;
  for (int mi = 0; mi < 4; ++mi)
    for (int ni = 0; ni < 3; ++ni) {
      if (kN[ni] > 1 && kN[ni] * 16 > Npad) continue;
      if (kM[mi] * kN[ni] > 8) continue;              // instantiated tiles (conv_kernels.h)
      FwdCfg c;
      if (!fwd_cfg(kM[mi], kN[ni], y->B, x->C, Npad, y->D, y->H, y->W, kd, kh, kw, lead, unit, &c)) continue;
      const int T = kd * kh * kw, nchunks = crn_cdiv(x->C, c.CC), NB = kN[ni] * 16;
      const int TD = c.tsd, TH = c.tsh * c.mh, TW = c.tsw * c.mw;
      const double patch = (double)c.CC * (TD + kd - 1) * (TH + kh - 1) * patch_width(TW, kw, lead, unit);
      const double slots = (lead >= 0 ? patch / unit / 256 * (unit == 4 ? 450.0 : 400.0) : patch / 256 * 350.0) +
                           (double)c.CC * T * NB / 4 / 256 * 300.0;
      const double chunk_work = (double)kM[mi] * kN[ni] * (c.CC / 4) * T * 32.0 * 1.3 + slots;
      for (int sp = 1; sp <= (splits < 1 ? std::min(nchunks, 64) : 1); sp *= 2) {
        if (sp > 1 && c.blocks * (sp / 2) >= kSplitFill) break;   // split only to fill the chip
        const int cps = crn_cdiv(nchunks, sp);
        const double bpc = std::max(1.0, std::ceil((double)c.blocks * sp / 256.0));
        double cost = bpc * cps * chunk_work + cps * std::ceil(bpc / 2.0) * 9000.0 + (sp > 1 ? kSplitPenalty : 0.0);
        if (cost < best_cost) { best_cost = cost; best = c; have = true; best_splits = sp; }
      }
    }
  bool forced = false;
  int xvec = lead >= 0 ? xmode : 0;
  if (!have && xvec) {       // no 16-byte configuration fits (tiny W): scalar staging
    xvec = 0;
    for (int mi = 0; mi < 4 && !have; ++mi) {
      FwdCfg c;
      if (fwd_cfg(kM[mi], 1, y->B, x->C, Npad, y->D, y->H, y->W, kd, kh, kw, -1, unit, &c)) { best = c; have = true; forced = true; }
    }
  }
  if (!have) return CRN_EINVAL;
  s->cfg = best; s->xvec = xvec; s->lead = xvec ? lead : -1; s->unit = unit; s->forced = forced;
  s->nchunks = crn_cdiv(x->C, best.CC);
  if (splits < 1) {   // auto split-K (atomic accumulate) only when the output grid cannot fill the chip
    splits = forced ? (best.blocks >= 192 ? 1 : (int)std::min<int64_t>(std::min(s->nchunks, 16), crn_cdiv(256, best.blocks)))
                    : best_splits;
  }
  if (splits > s->nchunks) splits = s->nchunks;
  s->splits = crn_cdiv(s->nchunks, crn_cdiv(s->nchunks, splits));
  return CRN_OK;
}

}  // namespace

static long long* g_pw_stamps = nullptr;
#ifdef CRN_TOOLS      // tools/_build/libcorenet_hip_tools.so only (corenet_amd.build.build_tools)
extern "C" int crn_pw_debug_stamps(long long* out32) {       // tuning aid (CRN_PW_STAMPS=1)
  if (!g_pw_stamps) return CRN_EINVAL;
  CRN_HIP(hipDeviceSynchronize());
  CRN_HIP(hipMemcpy(out32, g_pw_stamps, 32 * sizeof(long long), hipMemcpyDeviceToHost));
  return CRN_OK;
}
#endif
extern "C" int crn_conv_fwd(const crnView* x, const crnInTransform* tr, const float* w, int Npad,
                            const float* bias, int bias_sB, const crnView* y,
                            int kd, int kh, int kw, int pd, int ph, int pw,
                            int splits, int accumulate, const crnTapBoxes* boxes, crnStream stream) {
  const int rca = fwd_check_args(x, w, Npad, y, kd, kh, kw, boxes);
  if (rca != CRN_OK) return rca;
  hipStream_t st = (hipStream_t)stream;
  int rcf;
  const bool armed = crn_splitk_begin(st, &rcf);
  if (rcf != CRN_OK) return rcf;
  FwdSel sel;
  const int rcs = fwd_select(x, tr, w, Npad, y, kd, kh, kw, pd, ph, pw, splits, &sel);
  if (rcs != CRN_OK) return rcs;
  const int64_t Sx = (int64_t)x->D * x->H * x->W;
  if (sel.path == CRN_PLAN_DENSE_COLS) {
    hipLaunchKernelGGL(dense_cols_kernel, dim3((unsigned)crn_cdiv(y->C, 64)), dim3(256), (size_t)x->B * x->C * 4, st,
                       x->base, x->sB, x->sC, tr_or_none(tr), w, Npad, y->C, x->C, x->B, bias, bias_sB, y->base, y->sB, y->sC,
                       accumulate);
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  if (sel.path == CRN_PLAN_DENSE_ROWS) {
    const int zs = sel.zs;
    if (zs > 1 && !accumulate)
      CRN_HIP(hipMemset2DAsync(y->base, (size_t)y->sB * 4, 0, (size_t)y->C * 4, (size_t)x->B, st));
    hipLaunchKernelGGL(dense_rows_kernel, dim3((unsigned)crn_cdiv(y->C, 8), (unsigned)x->B, (unsigned)zs), dim3(256), 0, st,
                       x->base, x->sB, x->sC, w, Npad, y->C, x->C, bias, bias_sB, y->base, y->sB, y->sC, accumulate,
                       crn_cdiv(x->C, zs));
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  if (sel.path == CRN_PLAN_POINTWISE) {
    PwGeom p{};
    p.x = x->base; p.y = y->base; p.w = w; p.bias = bias;
    p.tr = tr_or_none(tr);
    p.B = x->B; p.C = x->C; p.N = y->C; p.Npad = Npad; p.S = (int)Sx;
    p.xsB = x->sB; p.ysB = y->sB; p.bias_sB = bias_sB; p.mode = accumulate ? 1 : 0;
    p.ysC = y->sC; p.ysP = y->sW;
    p.splits = 1; p.cps = sel.pw_cps_whole;
    pw_split(p, *y, Sx, sel.pw_splits, sel.pw_cps, st);
#ifdef CRN_TOOLS
    static const bool want_stamps = getenv("CRN_PW_STAMPS") != nullptr;
#else
    constexpr bool want_stamps = false;
#endif
    static long long* pw_stamps = nullptr;
    if (want_stamps) {
      if (!pw_stamps) CRN_HIP(hipMalloc(&pw_stamps, 32 * sizeof(long long)));
      CRN_HIP(hipMemsetAsync(pw_stamps, 0, 32 * sizeof(long long), st));
      p.stamps = pw_stamps;
      g_pw_stamps = pw_stamps;
    }
    return pw_launch<false>(p, *y, Sx, accumulate, armed, st);
  }
  const FwdCfg& best = sel.cfg;
  const int xvec = sel.xvec;
  splits = sel.splits;
  ConvGeom g{};
  g.y = *y;
  g.w = w; g.bias = bias; g.Npad = Npad; g.bias_sB = bias_sB;
  g.kd = kd; g.kh = kh; g.kw = kw; g.T = kd * kh * kw;
  g.mw = best.mw; g.mh = best.mh; g.nsh = best.tsh; g.nsw = best.tsw;
  g.TD = best.tsd; g.TH = best.tsh * best.mh; g.TW = best.tsw * best.mw;
  const int NSUB = best.NSUB, CC = best.CC;
  fill_patch(g, *x, tr, pd, ph, pw, g.TD, g.TH, g.TW, kd, kh, kw, sel.lead, sel.unit, CC, best.PSP);
  g.tilesD = crn_cdiv(y->D, g.TD); g.tilesH = crn_cdiv(y->H, g.TH); g.tilesW = crn_cdiv(y->W, g.TW);
  g.CC = CC; g.WSP = pad16mod32(g.T * NSUB * 16);
  g.nchunks = sel.nchunks;
  g.chunks_per_split = crn_cdiv(g.nchunks, splits);
  g.mode = splits > 1 ? 2 : (accumulate ? 1 : 0);
  g.magic_T = magic20(g.T);
  // split-K: partial sums into a dense scratch tensor + one reduction launch (mode 3); atomics (mode 2)
  // only when the scratch cannot be had
  const crnView yreal = *y;
  const int64_t ytot = (int64_t)y->B * y->C * y->D * y->H * y->W;
  float* scratch = g.mode == 2 ? crn_splitk_scratch((size_t)splits * ytot, st) : nullptr;
  if (scratch) {
    g.mode = 3;
    g.y = crn_splitk_scratch_view(yreal, scratch);
  }
  y = &g.y;                                // epilogue alignment below refers to the tensor actually written
  if (g.mode == 2 && !accumulate) {
    hipLaunchKernelGGL(zero_view_kernel, dim3((unsigned)std::min<int64_t>(crn_cdiv(ytot, 256), 4096)),
                       dim3(256), 0, st, yreal);
    CRN_CHECK_LAUNCH();
  }
  dim3 grid((unsigned)(g.tilesD * g.tilesH * g.tilesW * y->B), (unsigned)crn_cdiv(Npad, NSUB * 16),
            (unsigned)splits);
  const size_t lds_bytes = best.lds;
  g.vec_store = fwd_vec_store(*y, g.mw, g.mode) ? 1 : 0;
  if (boxes) {
    // groups must divide the channel counts, otherwise the information is ignored
    if (boxes->n_groups > 0 && y->C % boxes->n_groups == 0) { g.n_groups = boxes->n_groups; memcpy(g.n_box, boxes->n_box, sizeof(g.n_box)); }
    if (boxes->c_groups > 0 && x->C % boxes->c_groups == 0) { g.c_groups = boxes->c_groups; memcpy(g.c_box, boxes->c_box, sizeof(g.c_box)); }
  }
  int rc = CRN_EINVAL;
#define CRN_FWD_CASE(M, N) if (best.MSUB == M && NSUB == N) rc = crn_launch_fwd_##M##_##N(g, xvec, grid, lds_bytes, st);
  CRN_FWD_CONFIGS(CRN_FWD_CASE)
#undef CRN_FWD_CASE
  // the next BatchRenorm launch over y adds the partial sums up itself when the caller armed it (crn_splitk_defer) -- like the
  // pointwise and the split-bf16 paths: the encoder's fp32 3x3 layers and decoder stage 2 lose their reduction launch
  if (rc == CRN_OK && g.mode == 3) rc = crn_splitk_finish(yreal, scratch, splits, accumulate, armed, st);
  return rc;
}

// Two pointwise convolutions onto one output in one launch: y (+)= w1^T x1 + w2^T x2, the reduction running over the
// channels of x1 followed by those of x2 (pointwise_fwd_kernel<., true>).  The data gradients of a down-sampling bottleneck
// (op_a and the shortcut, resnet50.py:94-107) are such a pair.
extern "C" int crn_conv1x1_fwd_pair(const crnView* x1, const float* w1, const crnView* x2, const float* w2, int Npad,
                                    const crnView* y, int splits, int accumulate, crnStream stream) {
  if (!x1 || !x2 || !w1 || !w2 || !y || Npad <= 0 || (Npad & 15) || y->C > Npad || y->C < 1) return CRN_EINVAL;
  if (!plain_view(*x1) || !plain_view(*x2) || !plain_view(*y)) return CRN_EINVAL;
  const int64_t S = (int64_t)x1->D * x1->H * x1->W;
  if ((int64_t)x2->D * x2->H * x2->W != S || (int64_t)y->D * y->H * y->W != S || (S & 3)) return CRN_EINVAL;
  if (x1->B < 1 || x2->B != x1->B || y->B != x1->B || x1->C < 1 || (x1->C & 63) || x2->C < 1) return CRN_EINVAL;
  if ((((uintptr_t)w1) & 15) || (((uintptr_t)w2) & 15)) return CRN_EINVAL;
  constexpr int64_t kRange = (int64_t)1 << 31;                   // buffer offsets of the hand-tracked loads
  const int C1 = x1->C, C = C1 + x2->C;
  if ((int64_t)std::max(C1, x2->C) * std::max<int64_t>(S, Npad) * 4 >= kRange || splits < 0) return CRN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int rcf;
  const bool armed = crn_splitk_begin(st, &rcf);
  if (rcf != CRN_OK) return rcf;
  // the split rule of the single launch (fwd_select) on the concatenated K; splits > 1: as asked.  cps a multiple of 64
  int sp = splits;
  if (sp == 0) sp = pw_auto_splits(C, crn_cdiv(S, kPwBM) * crn_cdiv(y->C, kPwBN) * (int64_t)y->B);
  sp = std::max(1, std::min(sp, C / 64));
  int cps = (crn_cdiv(C, sp) + 63) & ~63;
  sp = crn_cdiv(C, cps);
  PwGeom p{};
  p.x = x1->base; p.w = w1; p.x2 = x2->base; p.w2 = w2; p.y = y->base;
  p.B = y->B; p.C = C; p.C1 = C1; p.N = y->C; p.Npad = Npad; p.S = (int)S;
  p.xsB = x1->sB; p.x2sB = x2->sB; p.ysB = y->sB; p.ysC = y->sC; p.ysP = 1; p.mode = accumulate ? 1 : 0;
  p.splits = 1; p.cps = (C + 63) & ~63;
  pw_split(p, *y, S, sp, cps, st);
  return pw_launch<true>(p, *y, S, accumulate, armed, st);
}

namespace {
struct WgCand { int TD, TH, TW, RSUB, NSUB, CC, PSP, POSP; double cost; size_t lds; };

// One weight-grad configuration: position tile TDxTHxTW, RSUB x NSUB MFMA tiles per wave.
// xlead >= 0: x staged in 16-byte units of `unit` positions; dvec: dy staging mode (0 scalar, 1 float4 units, 2 position pairs).
constexpr int kWgUnit = 4;                       // x patches of the weight gradient: float4 units only
bool wg_cand(int TD, int TH, int TW, int RSUB, int NSUB, int Cin, int Npad, int kd, int kh, int kw, int xlead, int unit,
             int dvec, size_t lds_budget, WgCand* out) {
  const int T = kd * kh * kw, NB = NSUB * 16, npos = TD * TH * TW;
  if (npos > 512 || RSUB * NSUB > 8 || (NSUB > 1 && NB > Npad)) return false;
  if ((xlead >= 0 || dvec) && (TW & 3)) return false;
  if (dvec == 1 ? (int64_t)NB * npos / 4 > 256 * NV
                : dvec == 2 ? (int64_t)NB * npos / 2 > 256 * NVX : stage_passes(NB, npos) > DREG) return false;
  const int PDp = TD + kd - 1, PH = TH + kh - 1, PW = patch_width(TW, kw, xlead, unit), plane = PH * PW;
  int CC = std::min(std::min(std::max(1, (64 * RSUB) / T), Cin), 64);
  auto staged = [&](int cc) {
    return xlead >= 0 ? (int64_t)cc * PDp * plane / 4 <= 256 * NVX : stage_passes(cc * PDp, plane) <= PREG;
  };
  while (CC > 1 && !staged(CC)) --CC;
  if (!staged(CC)) return false;
  const int PSP = xlead >= 0 ? pad16mod32(PDp * plane) : PDp * plane + 1;
  const int POSP = npos + 4;
  const size_t lds = ((size_t)CC * PSP + (size_t)NB * POSP + 2 * kChTab) * 4;
  if (lds > lds_budget) return false;
  const int rows = CC * T;
  if (rows > 64 * RSUB) return false;
  // cycles per wave and tile: MFMA issue plus staging instructions (they do not overlap: every
  // VALU/SALU instruction costs MFMA issue time), per useful multiply-add
  const double mfma = (double)RSUB * NSUB * (npos / 4.0) * 32.0;
  const double xslots = xlead >= 0 ? (double)CC * PDp * plane / 4 / 256 * 450.0 : (double)CC * PDp * plane / 256 * 350.0;
  const double dslots = dvec == 1 ? (double)NB * npos / 4 / 256 * 300.0
                                  : dvec == 2 ? (double)NB * npos / 2 / 256 * 300.0 : (double)NB * npos / 256 * 300.0;
  const double useful = (double)rows * std::min(NB, Npad) * npos;
  *out = WgCand{TD, TH, TW, RSUB, NSUB, CC, PSP, POSP, (mfma + xslots + dslots + 800.0) / useful, lds};
  return true;
}
}  // namespace

namespace {
// ---------------- weight-gradient plan ---------------------------------------
// As fwd_select: host arithmetic only, shared by the launch and crn_conv_wgrad_plan.
int wgrad_check_args(const crnView* x, const crnView* dy, const float* dw, int Npad, int kd, int kh, int kw) {
  if (!x || !dy || !dw || Npad <= 0 || (Npad & 15) || x->B != dy->B) return CRN_EINVAL;
  if (kd * kh * kw > 512) return CRN_EINVAL;
  return CRN_OK;
}
// dense layer on a 1^3 grid (stage_1)
bool wgrad_dense(const crnView* x, const crnView* dy, int T) {
  return T == 1 && one_position(*x) && one_position(*dy) && dy->C >= 1024;
}

struct WgSel {
  WgCand best;
  int xlead, dvec;                 // staging of x (>= 0: float4 units with that lead) and of dy (0 scalar, 1 float4, 2 pairs)
  int ntiles, cblocks, nblocks;
  int splits, tiles_per_split;     // position-tile splits the launch asks for
  bool balanced;                   // per-group splits from the tap boxes
};

int wg_select(const crnView* x, const crnView* dy, int Npad, int kd, int kh, int kw, int pw, const crnTapBoxes* boxes,
              WgSel* s) {
  const int T = kd * kh * kw;
  const int Dy = dy->D, Hy = dy->H, Wy = dy->W;
  const int TWc = Wy >= 16 ? 16 : ((Wy + 3) & ~3);
  int xlead = vec_view(*x) ? vec_lead(pw) : -1;
  // dy staging: float4 units for unit-stride views, position pairs for the stride-2 space-to-depth views of
  // the transposed convolutions (one float4 holds two positions of this parity), scalars otherwise
  int dvec = vec_view(*dy) ? 1 : ((dy->sW == 2 && dy->chan_off != nullptr && (dy->W & 1) == 0) ? 2 : 0);
  WgCand best{}; bool have = false;
  auto consider = [&](int TD, int TH, int RSUB, int NSUB, size_t budget) {
    WgCand c;
    if (!wg_cand(std::min(TD, Dy), std::min(TH, Hy), TWc, RSUB, NSUB, x->C, Npad, kd, kh, kw, xlead, kWgUnit, dvec, budget, &c))
      return false;
    if (RSUB > 1 && c.CC * T <= 32 * RSUB) return false;   // a smaller RSUB covers it
    if (!have || c.cost < best.cost) { best = c; have = true; }
    return true;
  };
  auto search = [&]() {
    static const int kTD[4] = {4, 3, 2, 1};
    static const int kTH[6] = {16, 8, 6, 4, 2, 1};
    for (int tdi = 0; tdi < 4; ++tdi)
      for (int thi = 0; thi < 6; ++thi)
        for (int NSUB = 4; NSUB >= 1; NSUB >>= 1)
          for (int RSUB = 8; RSUB >= 1; RSUB >>= 1) consider(kTD[tdi], kTH[thi], RSUB, NSUB, kLdsBudget);
  };
  search();
  if (!have && (xlead >= 0 || dvec)) { xlead = -1; dvec = 0; search(); }   // tiny maps: scalar staging
  if (!have) return CRN_EINVAL;
  if (xlead < 0) dvec = 0;                           // instantiated variants: scalar, x, x+dy, x+dy pairs
  if (xlead < 0 || !dvec) {
    // the candidate was costed with dvec; re-derive it with the variant that will run
    WgCand c;
    if (!wg_cand(best.TD, best.TH, best.TW, best.RSUB, best.NSUB, x->C, Npad, kd, kh, kw, xlead, kWgUnit, dvec, 150 * 1024, &c)) {
      have = false; search();
      if (!have) return CRN_EINVAL;
    } else {
      best = c;
    }
  }
  s->best = best; s->xlead = xlead; s->dvec = dvec;
  const int NB = best.NSUB * 16;
  s->ntiles = crn_cdiv(Dy, best.TD) * crn_cdiv(Hy, best.TH) * crn_cdiv(Wy, best.TW) * dy->B;
  s->cblocks = crn_cdiv(x->C, best.CC); s->nblocks = crn_cdiv(Npad, NB);
  // one resident round: at most 512 (= 2 per CU) workgroups, or the stragglers double the time
  constexpr int budget = 512;
  int splits = std::max(1, std::min(s->ntiles, budget / (s->cblocks * s->nblocks)));
  if (crn_deterministic()) splits = 1;                       // (the per-group splits of the launch follow: min(ntiles, ~splits))
  s->tiles_per_split = crn_cdiv(s->ntiles, splits);
  s->splits = crn_cdiv(s->ntiles, s->tiles_per_split);
  s->balanced = boxes && boxes->n_groups > 0 && boxes->n_groups <= 8 && dy->C % boxes->n_groups == 0 &&
                (dy->C / boxes->n_groups) % NB == 0;           // every block's columns belong to one group
  return CRN_OK;
}

// One weight-gradient launch: window kd x kh x kw, dw [Cin][T][Npad].
int wgrad_launch(const crnView* x, const crnInTransform* tr, const crnView* dy, float* dw, int Npad,
                 int kd, int kh, int kw, int pd, int ph, int pw, const crnTapBoxes* boxes, hipStream_t st) {
  const int T = kd * kh * kw;
  WgSel sel;
  const int rcs = wg_select(x, dy, Npad, kd, kh, kw, pw, boxes, &sel);
  if (rcs != CRN_OK) return rcs;
  const WgCand& best = sel.best;
  const int xlead = sel.xlead, dvec = sel.dvec;
  const int Dy = dy->D, Hy = dy->H, Wy = dy->W;
  WgradGeom g{};
  g.dy = *dy;
  g.dw = dw; g.Npad = Npad;
  g.kd = kd; g.kh = kh; g.kw = kw; g.T = T;
  g.TD = best.TD; g.TH = best.TH; g.TW = best.TW;
  g.POSP = best.POSP;
  const int NSUB = best.NSUB, RSUB = best.RSUB, NB = NSUB * 16, CC = best.CC;
  const int npos = g.TD * g.TH * g.TW;
  fill_patch(g, *x, tr, pd, ph, pw, g.TD, g.TH, g.TW, kd, kh, kw, xlead, kWgUnit, CC, best.PSP);
  g.CC = CC;
  g.tilesD = crn_cdiv(Dy, g.TD); g.tilesH = crn_cdiv(Hy, g.TH); g.tilesW = crn_cdiv(Wy, g.TW);
  g.ntiles = sel.ntiles;
  const int cblocks = sel.cblocks, nblocks = sel.nblocks, splits = sel.splits;
  g.tiles_per_split = sel.tiles_per_split;
  if (sel.balanced) {
    g.n_groups = boxes->n_groups; memcpy(g.n_box, boxes->n_box, sizeof(g.n_box));
    // blocks of a group with fewer real taps do less MFMA work per tile: give them proportionally more
    // tiles (fewer splits), the heavy groups more splits; the total stays within the resident budget
    double w[8], wsum = 0.0;
    for (int gi = 0; gi < g.n_groups; ++gi) {
      const signed char* b = boxes->n_box[gi];
      w[gi] = 0.35 * T + std::max(0, b[1] - b[0]) * std::max(0, b[3] - b[2]) * std::max(0, b[5] - b[4]);  // + staging share
      wsum += w[gi];
    }
    g.balanced = 1; g.nbpg = (dy->C / boxes->n_groups) / NB;
    g.zoff[0] = 0;
    for (int gi = 0; gi < g.n_groups; ++gi) {
      const int sgi = crn_deterministic() ? 1 : std::max(1, std::min(g.ntiles, (int)(splits * w[gi] * g.n_groups / wsum + 0.5)));
      g.tps[gi] = crn_cdiv(g.ntiles, sgi);
      g.sg[gi] = crn_cdiv(g.ntiles, g.tps[gi]);
      g.zoff[gi + 1] = g.zoff[gi] + g.nbpg * g.sg[gi];
    }
  }
  g.dlg2 = ilog2_ceil(npos); g.dnpass = dvec ? 0 : stage_passes(NB, npos);
  g.magic_TW = magic20(g.TW); g.magic_TH = magic20(g.TH);
  if (dvec) { g.np4 = npos / (dvec == 2 ? 2 : 4); g.dnunits = NB * g.np4; g.magic_NP4 = magic20(g.np4); }
  dim3 grid((unsigned)cblocks, (unsigned)(g.balanced ? 1 : nblocks), (unsigned)(g.balanced ? g.zoff[g.n_groups] : splits));
  const size_t lds_bytes = best.lds;
#define CRN_WG_CASE(R, N) \
  if (RSUB == R && NSUB == N) return crn_launch_wgrad_##R##_##N(g, xlead >= 0, dvec, grid, lds_bytes, st);
  CRN_WG_CONFIGS(CRN_WG_CASE)
#undef CRN_WG_CASE
  return CRN_EINVAL;
}
}  // namespace

extern "C" int crn_conv_wgrad(const crnView* x, const crnInTransform* tr, const crnView* dy,
                              float* dw, int Npad, int kd, int kh, int kw, int pd, int ph, int pw,
                              int zero_first, const crnTapBoxes* boxes, crnStream stream) {
  CRN_ENTRY(stream);
  const int rca = wgrad_check_args(x, dy, dw, Npad, kd, kh, kw);
  if (rca != CRN_OK) return rca;
  hipStream_t st = (hipStream_t)stream;
  const int T = kd * kh * kw;
  if (zero_first) CRN_HIP(hipMemsetAsync(dw, 0, (size_t)x->C * T * Npad * 4, st));
  if (wgrad_dense(x, dy, T)) {
    hipLaunchKernelGGL(dense_wgrad_kernel, dim3((unsigned)crn_cdiv(dy->C, 256), (unsigned)x->C), dim3(256), 0, st, x->base,
                       x->sB, x->sC, tr_or_none(tr), dy->base, dy->sB, dy->sC, dw, Npad, dy->C, x->C, x->B);
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  // Tap boxes: inside the single launch every block enumerates only the (channel, tap) rows of its output
  // group's box (conv_wgrad_kernel).  The alternative -- one launch per output parity with a smaller
  // window -- LOSES on MI355X (eight prologues and atomic epilogues: s5t1 1.02 ms vs 0.94 ms).
  return wgrad_launch(x, tr, dy, dw, Npad, kd, kh, kw, pd, ph, pw, boxes, st);
}

// ---------------- plan queries: no HIP call, nothing dereferenced but the view structs ----------------
extern "C" int crn_conv_fwd_plan(const crnView* x, const crnInTransform* tr, const float* w, int Npad,
                                 const float* bias, int bias_sB, const crnView* y,
                                 int kd, int kh, int kw, int pd, int ph, int pw,
                                 int splits, int accumulate, const crnTapBoxes* boxes, crnConvPlan* out) {
  (void)bias; (void)bias_sB; (void)accumulate;
  if (!out) return CRN_EINVAL;
  const int rca = fwd_check_args(x, w, Npad, y, kd, kh, kw, boxes);
  if (rca != CRN_OK) return rca;
  FwdSel sel;
  const int rcs = fwd_select(x, tr, w, Npad, y, kd, kh, kw, pd, ph, pw, splits, &sel);
  if (rcs != CRN_OK) return rcs;
  crnConvPlan p{};
  p.path = sel.path; p.splits = 1; p.chunks = 1; p.lds_budget = (int)kLdsBudget;
  if (sel.path == CRN_PLAN_DENSE_COLS) {
    p.lds_bytes = x->B * x->C * 4 + kDenseColsLds;
  } else if (sel.path == CRN_PLAN_DENSE_ROWS) {
    p.splits = sel.zs; p.chunks = crn_cdiv(x->C, 256); p.lds_bytes = 4 * 8 * 4;
  } else if (sel.path == CRN_PLAN_POINTWISE) {
    // 64 positions x 32 columns per workgroup, K chunks of 64 (pointwise_fwd_kernel)
    p.msub = 4; p.nsub = kPwBN / 16; p.xstage = 1; p.cc = kPwKC; p.td = 1; p.th = 1; p.tw = kPwBM; p.mw = 16;
    p.splits = sel.pw_splits; p.chunks = crn_cdiv(x->C, 32);
    p.vec_store = (sel.pw_splits > 1 || y->sW == 1) ? 1 : 0;
    p.lds_bytes = kPwLds + ((tr && tr->scale) ? 2 * sel.pw_cps * 4 : 0);
  } else {
    const FwdCfg& c = sel.cfg;
    p.msub = c.MSUB; p.nsub = c.NSUB; p.xstage = sel.xvec; p.forced = sel.forced ? 1 : 0; p.cc = c.CC;
    p.td = c.tsd; p.th = c.tsh * c.mh; p.tw = c.tsw * c.mw; p.mw = c.mw;
    p.splits = sel.splits; p.chunks = sel.nchunks; p.lds_bytes = (int)c.lds;
    // the scratch view a split launch writes is dense; whether the scratch can be had is only known at the launch
    p.vec_store = sel.splits > 1 ? fwd_vec_store(crn_splitk_scratch_view(*y, nullptr), c.mw, 3) : fwd_vec_store(*y, c.mw, 0);
  }
  *out = p;
  return CRN_OK;
}

extern "C" int crn_conv_wgrad_plan(const crnView* x, const crnInTransform* tr, const crnView* dy,
                                   float* dw, int Npad, int kd, int kh, int kw, int pd, int ph, int pw,
                                   int zero_first, const crnTapBoxes* boxes, crnConvPlan* out) {
  (void)tr; (void)pd; (void)ph; (void)zero_first;
  if (!out) return CRN_EINVAL;
  const int rca = wgrad_check_args(x, dy, dw, Npad, kd, kh, kw);
  if (rca != CRN_OK) return rca;
  crnConvPlan p{};
  p.splits = 1; p.chunks = 1; p.lds_budget = (int)kLdsBudget;
  if (wgrad_dense(x, dy, kd * kh * kw)) {
    p.path = CRN_PLAN_DENSE_WGRAD;
    *out = p;
    return CRN_OK;
  }
  WgSel sel;
  const int rcs = wg_select(x, dy, Npad, kd, kh, kw, pw, boxes, &sel);
  if (rcs != CRN_OK) return rcs;
  p.path = CRN_PLAN_GENERIC;
  p.msub = sel.best.RSUB; p.nsub = sel.best.NSUB; p.xstage = sel.xlead >= 0 ? 1 : 0; p.dystage = sel.dvec;
  p.cc = sel.best.CC; p.td = sel.best.TD; p.th = sel.best.TH; p.tw = sel.best.TW;
  p.splits = sel.splits; p.chunks = sel.ntiles; p.balanced = sel.balanced ? 1 : 0; p.lds_bytes = (int)sel.best.lds;
  *out = p;
  return CRN_OK;
}
