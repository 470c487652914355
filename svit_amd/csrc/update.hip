// What the solver did to every tensor, measured inside the step (svit_update_snapshot, svit_update_stats) -- gfx950.
//
// Two launch groups bracket the solver's launch of a guarded optimizer.  In front of it ONE launch copies the weights of
// the trainable segments into a shadow buffer; behind it two launches compare the weights with the shadow, tensor by
// tensor, and leave in a row of a ring in device memory (include/svit_hip.h: svit_update_stats) the fp64 sums of
// squares of the step Delta = p_new - p_old, of the new weights, of the gradient and of the first moment, the sum of the
// second moment, the signed dot product of Delta and g, the largest |Delta| and two counts taken on the weights' bits:
// the elements that did not change and those that moved to an adjacent float.  No update rule is restated here: the
// numbers are those of whatever solver ran in between.  The yardstick is svit_amd/updmon.py update_host.
//
// A step is due when the guard applied it and its index s = applied + skipped - 1 is a multiple of `every`; both entry
// points read that off the guard's record, which no solver kernel writes (csrc/misc.hip: only the guard's last workgroup
// does; csrc/solver.hip takes the record as const), so they agree.  When the step is not due every workgroup of all three
// launches returns before its first load.
//
// The walks are csrc/monitor.hip's and csrc/solver.hip's.  Snapshot: workgroups stride over windows of 1024 floats, a
// workgroup-uniform cursor into the segment table (kernel arguments) only moves forward, 16-byte accesses.  Stage 1 of
// the statistics: workgroup w takes the window [w * 4096, (w + 1) * 4096), issues its loads first (the quads inside a
// segment), finds the first tensor that ends past the window's begin by bisection and walks on; every (window, tensor)
// piece is reduced lane -> wave -> workgroup in a fixed order and stored as ONE 64-byte partial at slot window + tensor.
// Stage 2: one wave per tensor folds its partials in ascending window order, then a fixed butterfly, and writes the
// entry; the wave of tensor 0 writes the header.  No atomics, no ticket, no counter a kernel advances: a row is the same
// bit for bit from run to run and from the eager step to a replay.
//
// The library is built with -ffast-math: the two counts compare integer images and never floats, the maximum is taken on
// the integer image of (float) |Delta| (integer order is float order for non-negative floats).  Delta is one fp64
// subtraction; the squares of floats are exact in fp64; a product may be fused into the addition that follows it.
#include <cstring>

#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int kWindow = 4096;              // floats per window of the statistics: svit_tensor_stats_window()
constexpr int kThreads = 256;
constexpr int kPasses = kWindow / (kThreads * 4);
constexpr int64_t kMaxTensors = 4096;

struct alignas(16) Entry {                 // one (window, tensor) piece, and the ring's entry of one tensor
  double sumsq_d, sumsq_p, dot_dg, sumsq_g, sumsq_m, sum_v;
  uint32_t absmax_bits;                    // the image of a non-negative float
  int32_t n_still, n_one_ulp, reserved;
};
static_assert(sizeof(Entry) == 64, "a partial and a ring entry are 64 bytes");

struct SegTable {
  int64_t v[SVIT_MAX_SEGS][2];
  int32_t S;
};

// the step this launch belongs to and whether it is due: applied, and every `every`-th
__device__ __forceinline__ bool due_step(const svit_step_dev* d, int64_t every, int64_t& s) {
  s = d->applied + d->skipped - 1;
  return d->apply == 1 && s >= 0 && s % every == 0;
}

// is the position inside a segment?  S == 0: every position is.  (A tensor is trainable when its begin is.)
__device__ __forceinline__ bool trainable(const SegTable& T, int64_t i) {
  if (T.S == 0) return true;
  bool in = false;
  for (int j = 0; j < T.S; ++j) in |= (i >= T.v[j][0]) & (i < T.v[j][1]);
  return in;
}

// is the quad at float index i of the window [lo, hi) inside a segment?  k: first segment that ends past lo
__device__ __forceinline__ bool seg_holds(const SegTable& T, int& k, int64_t lo, int64_t hi, int64_t i) {
  if (T.S == 0) return true;
  while (k < T.S && T.v[k][1] <= lo) ++k;
  bool in = false;
  for (int j = k; j < T.S && T.v[j][0] < hi; ++j) in |= (i >= T.v[j][0]) & (i < T.v[j][1]);
  return in;
}

// 8 B per parameter on a due step: p read, shadow written
__global__ __launch_bounds__(kThreads) void update_snapshot_kernel(const float* __restrict__ p, float* __restrict__ shadow,
                                                                   int64_t n, const svit_step_dev* __restrict__ d,
                                                                   int64_t every, const SegTable T) {
  int64_t s;
  if (!due_step(d, every, s)) return;
  const int64_t window = (int64_t)kThreads * 4, stride = (int64_t)gridDim.x * window;
  int k = 0;
  for (int64_t lo = (int64_t)blockIdx.x * window; lo < n; lo += stride) {
    const int64_t i = lo + (int64_t)threadIdx.x * 4;
    if (i >= n || !seg_holds(T, k, lo, lo + window, i)) continue;
    if (i + 4 <= n) {
      *(float4*)(shadow + i) = *(const float4*)(p + i);
    } else {                               // the last quad of a whole buffer with n % 4 != 0: element by element, below n
      for (int e = 0; e < 4; ++e)
        if (i + e < n) shadow[i + e] = p[i + e];
    }
  }
}

struct Acc {
  double sd, sp, dg, sg, sm, sv;
  uint32_t amax;
  int32_t still, one;
};

__device__ __forceinline__ int64_t ulp_key(uint32_t bits) {
  const int32_t i = (int32_t)bits;
  return (int64_t)(i ^ ((i >> 31) & 0x7fffffff));
}

// the value as the walk's loop sees it: a new one in every turn.  Without it the compiler hoists the 80 conversions to fp64
// and the products of a lane's 16 elements out of the loop over the tensors of a window -- 300 registers, one wave per
// SIMD; with it a piece costs its own arithmetic (nearly every window lies inside one tensor) at 152 registers, three waves
// per SIMD.
__device__ __forceinline__ float this_turn(float x) {
  __asm__ volatile("" : "+v"(x));
  return x;
}

template <bool HAS_M, bool HAS_V>
__device__ __forceinline__ void acc_element(Acc& a, float pn, float po, float g, float m, float v) {
  const uint32_t bn = __float_as_uint(pn), bo = __float_as_uint(po);
  const double pd = (double)pn, gd = (double)g;
  const double dl = pd - (double)po;
  a.sd += dl * dl;
  a.sp += pd * pd;
  a.dg += dl * gd;
  a.sg += gd * gd;
  if (HAS_M) a.sm += (double)m * (double)m;
  if (HAS_V) a.sv += (double)v;
  const uint32_t mag = __float_as_uint((float)dl) & 0x7fffffffu;
  a.amax = mag > a.amax ? mag : a.amax;
  a.still += bn == bo ? 1 : 0;
  const int64_t kd = ulp_key(bn) - ulp_key(bo);
  a.one += (kd == 1 || kd == -1) ? 1 : 0;
}

__device__ __forceinline__ void acc_add(Acc& a, const Entry& q) {
  a.sd += q.sumsq_d; a.sp += q.sumsq_p; a.dg += q.dot_dg; a.sg += q.sumsq_g; a.sm += q.sumsq_m; a.sv += q.sum_v;
  a.amax = q.absmax_bits > a.amax ? q.absmax_bits : a.amax;
  a.still += q.n_still;
  a.one += q.n_one_ulp;
}

__device__ __forceinline__ Entry acc_entry(const Acc& a) {
  Entry q;
  q.sumsq_d = a.sd; q.sumsq_p = a.sp; q.dot_dg = a.dg; q.sumsq_g = a.sg; q.sumsq_m = a.sm; q.sum_v = a.sv;
  q.absmax_bits = a.amax; q.n_still = a.still; q.n_one_ulp = a.one; q.reserved = 0;
  return q;
}

// all 64 lanes leave with the wave's values; the order of the additions is fixed
__device__ __forceinline__ void wave_fold(Acc& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.sd += __shfl_xor(a.sd, o, 64);
    a.sp += __shfl_xor(a.sp, o, 64);
    a.dg += __shfl_xor(a.dg, o, 64);
    a.sg += __shfl_xor(a.sg, o, 64);
    a.sm += __shfl_xor(a.sm, o, 64);
    a.sv += __shfl_xor(a.sv, o, 64);
    const uint32_t m = (uint32_t)__shfl_xor((int)a.amax, o, 64);
    a.amax = m > a.amax ? m : a.amax;
    a.still += __shfl_xor(a.still, o, 64);
    a.one += __shfl_xor(a.one, o, 64);
  }
}

__device__ __forceinline__ void load_quad(float (&dst)[4], const float* __restrict__ src, int64_t i, int64_t n) {
  if (i + 4 <= n) {
    const float4 X = *(const float4*)(src + i);
    dst[0] = X.x; dst[1] = X.y; dst[2] = X.z; dst[3] = X.w;
  } else {                                 // the last quad of a buffer with n % 4 != 0: element by element, below n
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < n) dst[e] = src[i + e];
  }
}

// 20 B per parameter on a due step with both moments: p, shadow, g, m, v read
template <bool HAS_M, bool HAS_V>
__global__ __launch_bounds__(kThreads) void update_stats_pieces(const float* __restrict__ p, const float* __restrict__ shadow,
                                                                const float* __restrict__ g, const float* __restrict__ m,
                                                                const float* __restrict__ v, int64_t n,
                                                                const int64_t* __restrict__ table, int Tn,
                                                                const svit_step_dev* __restrict__ d, int64_t every,
                                                                Entry* __restrict__ part, const SegTable T) {
  int64_t s;
  if (!due_step(d, every, s)) return;
  __shared__ Entry red[2][kThreads / 64];
  const int64_t w = blockIdx.x, lo = w * kWindow, hi = (lo + kWindow < n) ? lo + kWindow : n;
  // the lane's quads first, so that the loads are in flight while the table is searched: a quad is loaded when it lies
  // inside a segment (segments hold whole tensors); what a lane did not load it never counts
  float pn[kPasses][4], po[kPasses][4], gv[kPasses][4], mv[kPasses][4], vv[kPasses][4];
#pragma unroll
  for (int j = 0; j < kPasses; ++j) {
    const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[j][e] = po[j][e] = gv[j][e] = mv[j][e] = vv[j][e] = 0.f;
    if (i >= hi || !trainable(T, i)) continue;
    load_quad(pn[j], p, i, n);
    load_quad(po[j], shadow, i, n);
    load_quad(gv[j], g, i, n);
    if (HAS_M) load_quad(mv[j], m, i, n);
    if (HAS_V) load_quad(vv[j], v, i, n);
  }
  int a = 0, b = Tn;                       // first tensor that ends past lo
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (table[2 * mid + 1] <= lo) a = mid + 1; else b = mid;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int par = 0;
  for (int t = a; t < Tn; ++t) {
    const int64_t tb = table[2 * t], te = table[2 * t + 1];
    if (tb >= hi) break;
    if (!trainable(T, tb)) continue;
    Acc acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0, 0};
    bool any = false;
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
      if (i < tb || i >= te || i >= hi) continue;
      any = true;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < te)
          acc_element<HAS_M, HAS_V>(acc, this_turn(pn[j][e]), this_turn(po[j][e]), this_turn(gv[j][e]),
                                    HAS_M ? this_turn(mv[j][e]) : 0.f, HAS_V ? this_turn(vv[j][e]) : 0.f);
    }
    if (__any(any)) wave_fold(acc);
    if (lane == 0) red[par][wave] = acc_entry(acc);
    __syncthreads();
    if (threadIdx.x == 0) {
      Acc sum = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0, 0};
#pragma unroll
      for (int k = 0; k < kThreads / 64; ++k) acc_add(sum, red[par][k]);
      part[w + t] = acc_entry(sum);
    }
    par ^= 1;      // the other buffer next: a wave writes it only behind the barrier thread 0 reaches after this read
  }
}

__global__ __launch_bounds__(64) void update_stats_fold(const int64_t* __restrict__ table, int Tn,
                                                        const svit_step_dev* __restrict__ d, int64_t every, int flags,
                                                        const Entry* __restrict__ part, unsigned char* __restrict__ ring,
                                                        int64_t R, const SegTable T) {
  int64_t s;
  if (!due_step(d, every, s)) return;
  const int t = blockIdx.x, lane = threadIdx.x;
  unsigned char* row = ring + (s % R) * (int64_t)(16 + 64 * (int64_t)Tn);
  if (t == 0 && lane == 0) {
    *(int64_t*)row = s;
    ((int32_t*)row)[2] = flags;
    ((int32_t*)row)[3] = 0;
  }
  const int64_t tb = table[2 * t], te = table[2 * t + 1];
  if (!trainable(T, tb)) return;
  const int64_t w0 = tb / kWindow, w1 = (te - 1) / kWindow;
  Acc acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0, 0};
  for (int64_t w = w0 + lane; w <= w1; w += 64) acc_add(acc, part[w + t]);
  wave_fold(acc);
  if (lane == 0) *(Entry*)(row + 16 + 64 * (int64_t)t) = acc_entry(acc);
}

// the `_seg` rules with their error codes; S == 0: no table, the whole buffer
int segs_take(const int64_t* segs, int64_t S, int64_t n, SegTable* out) {
  memset(out, 0, sizeof *out);
  if (S == 0) return SVIT_OK;
  if (!segs || S < 0 || S > SVIT_MAX_SEGS) return SVIT_ERR_ARG;
  int64_t prev = 0;
  for (int64_t i = 0; i < S; ++i) {
    const int64_t b = segs[2 * i], e = segs[2 * i + 1];
    if (b < prev || e <= b || e > n) return SVIT_ERR_ARG;
    if ((b | e) & 3) return SVIT_ERR_ALIGN;
    out->v[i][0] = b;
    out->v[i][1] = e;
    prev = e;
  }
  out->S = (int32_t)S;
  return SVIT_OK;
}

template <bool HAS_M, bool HAS_V>
void launch_pieces(unsigned windows, hipStream_t stream, const float* p, const float* shadow, const float* g,
                   const float* m, const float* v, int64_t n, const int64_t* table, int Tn, const svit_step_dev* d,
                   int64_t every, Entry* part, const SegTable& T) {
  hipLaunchKernelGGL((update_stats_pieces<HAS_M, HAS_V>), dim3(windows), dim3(kThreads), 0, stream, p, shadow, g, m, v, n,
                     table, Tn, d, every, part, T);
}
}  // namespace

extern "C" int svit_update_snapshot(const float* p, float* shadow, int64_t n, const int64_t* segs, int64_t S,
                                    const svit_step_dev* dev_rec, int64_t every, void* stream) {
  if (!p || !shadow || !dev_rec || n <= 0 || every < 1) return SVIT_ERR_ARG;
  SegTable T;
  if (int rc = segs_take(segs, S, n, &T)) return rc;
  if (((uintptr_t)p | (uintptr_t)shadow) & 15) return SVIT_ERR_ALIGN;
  if ((uintptr_t)dev_rec & 7) return SVIT_ERR_ALIGN;
  const int64_t span = S == 0 ? n : T.v[S - 1][1];
  int64_t blocks = (span + kThreads * 4 - 1) / (kThreads * 4);
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(update_snapshot_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p, shadow,
                     span, dev_rec, every, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int64_t svit_update_stats_workspace(int64_t n, int64_t Tn) {
  if (n <= 0 || Tn < 1 || Tn > kMaxTensors) return SVIT_ERR_ARG;
  return ((n + kWindow - 1) / kWindow + Tn) * (int64_t)sizeof(Entry);
}

extern "C" int svit_update_stats(const float* p, const float* shadow, const float* g, const float* m, const float* v,
                                 int64_t n, const int64_t* table_dev, const int64_t* table_host, int64_t Tn,
                                 const int64_t* segs, int64_t S, const svit_step_dev* dev_rec, void* ring, int64_t R,
                                 int64_t every, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!p || !shadow || !g || !table_dev || !dev_rec || !ring || !workspace || R < 1 || every < 1) return SVIT_ERR_ARG;
  if (int rc = svit_tensor_table_check(table_host, Tn, n)) return rc;
  SegTable T;
  if (int rc = segs_take(segs, S, n, &T)) return rc;
  if (workspace_bytes < svit_update_stats_workspace(n, Tn)) return SVIT_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)shadow | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ring |
       (uintptr_t)workspace) & 15)
    return SVIT_ERR_ALIGN;
  if (((uintptr_t)table_dev | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  const int64_t windows = (n + kWindow - 1) / kWindow;
  if (windows > 0x7fffffff) return SVIT_ERR_ARG;
  const int flags = (m ? 1 : 0) | (v ? 2 : 0);
  const hipStream_t st = (hipStream_t)stream;
  Entry* part = (Entry*)workspace;
  switch (flags) {
    case 3: launch_pieces<true, true>((unsigned)windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    case 1: launch_pieces<true, false>((unsigned)windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    case 2: launch_pieces<false, true>((unsigned)windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    default: launch_pieces<false, false>((unsigned)windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
  }
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(update_stats_fold, dim3((unsigned)Tn), dim3(64), 0, st, table_dev, (int)Tn, dev_rec, every, flags,
                     (const Entry*)workspace, (unsigned char*)ring, R, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
