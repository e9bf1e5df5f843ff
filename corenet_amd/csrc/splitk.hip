// Split-K scratch, deferral and finish of the convolution engines: the protocol is in splitk.h.
#include "crn_common.h"
#include <algorithm>
#include <mutex>
#include <vector>

namespace {

// y[b,c,pos] (view) = (accumulate ? y : 0) + sum_s scratch[s][b][c][pos] (dense)
__global__ void splitk_reduce_kernel(crnView v, const float* scratch, int splits, int accumulate) {
  const int64_t S = (int64_t)v.D * v.H * v.W, per_b = (int64_t)v.C * S;
  const int64_t total = per_b * v.B;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = e;
    const int w = r % v.W; r /= v.W;
    const int h = r % v.H; r /= v.H;
    const int d = r % v.D; r /= v.D;
    const int c = r % v.C; r /= v.C;
    float sum = 0.f;
    for (int s = 0; s < splits; ++s) sum += scratch[(int64_t)s * total + e];
    const int64_t co = v.chan_off ? (int64_t)v.chan_off[c] : (int64_t)c * v.sC;
    float* dst = v.base + r * v.sB + co + (int64_t)d * v.sD + (int64_t)h * v.sH + (int64_t)w * v.sW;
    *dst = accumulate ? *dst + sum : sum;
  }
}

// the same reduction for plain outputs (every sample a contiguous [C][D][H][W] block): float4 elements, no index
// arithmetic, and the loads of four splits in flight at a time (the generic kernel walks its splits one load latency
// after the other and spends five integer divisions per element; 60 of these launches sit on the step's critical path)
__global__ __launch_bounds__(256) void splitk_reduce_plain_kernel(float* y, int64_t ysB, const float* scratch,
                                                                  int64_t per_b4, int64_t total4, int splits,
                                                                  int accumulate) {
  crn_kernargs_now(y, ysB, scratch, per_b4, total4, splits, accumulate);
  const f32x4* sc4 = reinterpret_cast<const f32x4*>(scratch);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total4; e += (int64_t)gridDim.x * blockDim.x) {
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 4 <= splits; s += 4) {
      const f32x4 a = sc4[(int64_t)s * total4 + e], b = sc4[(int64_t)(s + 1) * total4 + e];
      const f32x4 c = sc4[(int64_t)(s + 2) * total4 + e], d = sc4[(int64_t)(s + 3) * total4 + e];
      sum += a; sum += b; sum += c; sum += d;               // same order as the generic kernel: split 0 first
    }
    for (; s < splits; ++s) sum += sc4[(int64_t)s * total4 + e];
    const int64_t b = e / per_b4, r = e - b * per_b4;
    f32x4* dst = reinterpret_cast<f32x4*>(y + b * ysB) + r;
    *dst = accumulate ? *dst + sum : sum;
  }
}

// The scratch table: one buffer per (device, stream), grown on demand; hipFree synchronises the device, so a buffer is
// never released under a kernel that still uses it.
constexpr int kSkSlots = 64;
// pinned: the slot belongs to a stream whose launches are CAPTURED into HIP graphs (crn_splitk_reserve): a graph holds the
// buffer's address, so a pinned slot that has to grow keeps its outgrown buffers (`retired`) until crn_splitk_release.
struct SkSlot { int dev; hipStream_t st; float* buf; size_t cap; bool used; bool pinned; std::vector<float*>* retired; };
SkSlot g_sk_slots[kSkSlots] = {};
std::mutex g_sk_mu;                      // the table is shared by every host thread that launches (autograd worker, main)

// the slot of (dev, st), made if there is none yet; nullptr: the table is full.  Call with g_sk_mu held.
SkSlot* find_or_make_slot(int dev, hipStream_t st) {
  for (int i = 0; i < kSkSlots; ++i)
    if (g_sk_slots[i].used && g_sk_slots[i].dev == dev && g_sk_slots[i].st == st) return &g_sk_slots[i];
  for (int i = 0; i < kSkSlots; ++i)
    if (!g_sk_slots[i].used) { g_sk_slots[i] = SkSlot{dev, st, nullptr, 0, true, false, nullptr}; return &g_sk_slots[i]; }
  return nullptr;
}

void crn_splitk_set_pending(const crnView& y, const float* scratch, int splits, hipStream_t st) {
  CrnSplitPending& p = crn_splitk_pending();
  p.active = true; p.y = y; p.scratch = scratch; p.splits = splits; p.stream = st;
  if (hipGetDevice(&p.device) != hipSuccess) p.device = 0;
}

}  // namespace

float* crn_splitk_scratch(size_t floats, hipStream_t st) {
  std::lock_guard<std::mutex> lock(g_sk_mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  SkSlot* sl = find_or_make_slot(dev, st);
  if (!sl) return nullptr;
  if (floats > sl->cap) {
    if (floats > ((size_t)256 << 20) / 4) return nullptr;       // larger outputs keep the atomic path
    // a stream that is being captured cannot allocate (hipMalloc would fail the capture): the launch keeps the atomic path
    // (crn_splitk_reserve sizes the scratch BEFORE a capture, so this only catches a launch that needs more
    // than any eager run before it did)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    if (sl->buf) {
      if (sl->pinned) {
        if (!sl->retired) sl->retired = new std::vector<float*>();
        sl->retired->push_back(sl->buf);                       // a captured graph may still read / write it
      } else {
        (void)hipFree(sl->buf);
      }
    }
    sl->cap = sl->pinned ? floats : std::max(floats, ((size_t)16 << 20) / 4);     // (a capture stream gets what was asked for)
    if (hipMalloc(&sl->buf, sl->cap * 4) != hipSuccess) { sl->buf = nullptr; sl->cap = 0; }
  }
  return sl->buf;
}

CrnSplitPending& crn_splitk_pending() {
  static thread_local CrnSplitPending p;
  return p;
}
int crn_splitk_flush(hipStream_t st) {
  CrnSplitPending& p = crn_splitk_pending();
  if (!p.active) return CRN_OK;
  p.active = false;
  (void)st;                       // the sum is ordered behind the convolution: it runs on the conv's own stream / device
  int cur = -1;
  CRN_HIP(hipGetDevice(&cur));
  if (cur != p.device) CRN_HIP(hipSetDevice(p.device));
  const int rc = crn_splitk_reduce(p.y, p.scratch, p.splits, 0, p.stream);
  if (cur != p.device) CRN_HIP(hipSetDevice(cur));
  return rc;
}
bool crn_splitk_begin(hipStream_t st, int* rc) {
  CrnSplitPending& p = crn_splitk_pending();
  const bool armed = p.armed;
  p.armed = false;                                     // the arming of crn_splitk_defer holds for ONE convolution call
  *rc = crn_splitk_flush(st);
  return armed;
}
extern "C" int crn_splitk_defer(int on) {
  crn_splitk_pending().armed = on != 0;
  return CRN_OK;
}
// A stream that is about to be CAPTURED into a HIP graph cannot allocate: give it, ahead of the capture, a scratch as
// large as the largest one any stream of this device has needed so far (floats == 0) or `floats`.
extern "C" int crn_splitk_reserve(int64_t floats, crnStream stream) {
  int dev = 0;
  CRN_HIP(hipGetDevice(&dev));
  size_t want = floats > 0 ? (size_t)floats : 0;
  {
    std::lock_guard<std::mutex> lock(g_sk_mu);
    if (!want)
      for (int i = 0; i < kSkSlots; ++i)
        if (g_sk_slots[i].used && g_sk_slots[i].dev == dev) want = std::max(want, g_sk_slots[i].cap);
    SkSlot* sl = find_or_make_slot(dev, (hipStream_t)stream);     // mark (or create) the stream's slot as pinned first
    if (!sl) return CRN_ENOMEM;
    sl->pinned = true;
  }
  if (!want) return CRN_OK;
  return crn_splitk_scratch(want, (hipStream_t)stream) ? CRN_OK : CRN_ENOMEM;
}
// Gives back the scratch of a stream that is about to be destroyed (a capture stream whose graphs are gone); hipFree waits for
// the device, so nothing that still reads the buffer can be running.  Unknown streams are not an error.
extern "C" int crn_splitk_release(crnStream stream) {
  int dev = 0;
  CRN_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_sk_mu);
  for (int i = 0; i < kSkSlots; ++i) {
    SkSlot& sl = g_sk_slots[i];
    if (sl.used && sl.dev == dev && sl.st == (hipStream_t)stream) {
      if (sl.buf) CRN_HIP(hipFree(sl.buf));
      if (sl.retired) {
        for (float* b : *sl.retired) (void)hipFree(b);
        delete sl.retired;
      }
      sl = SkSlot{};
    }
  }
  return CRN_OK;
}
int crn_splitk_reduce(const crnView& y, const float* scratch, int splits, int accumulate, hipStream_t st) {
  const int64_t ytot = (int64_t)y.B * y.C * y.D * y.H * y.W;
  const int64_t per_b = (int64_t)y.C * y.D * y.H * y.W;
  if (plain_view(y) && (per_b & 3) == 0 && (((uintptr_t)scratch) & 15) == 0) {
    const int64_t total4 = ytot / 4;
    hipLaunchKernelGGL(splitk_reduce_plain_kernel, dim3((unsigned)std::min<int64_t>(crn_cdiv(total4, 256), 4096)), dim3(256),
                       0, st, y.base, y.sB, scratch, per_b / 4, total4, splits, accumulate);
    CRN_CHECK_LAUNCH();
    return CRN_OK;
  }
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)std::min<int64_t>(crn_cdiv(ytot, 256), 4096)), dim3(256), 0, st,
                     y, scratch, splits, accumulate);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}
int crn_splitk_finish(const crnView& y, const float* scratch, int splits, int accumulate, bool armed, hipStream_t st) {
  if (armed && !accumulate && crn_splitk_dense(y)) {
    crn_splitk_set_pending(y, scratch, splits, st);
    return CRN_OK;
  }
  return crn_splitk_reduce(y, scratch, splits, accumulate, st);
}
