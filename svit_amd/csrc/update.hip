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
// launches returns before its first load.  The header's third word says which moments were there.
//
// Snapshot: workgroups stride over windows of 1024 floats as csrc/solver.hip's do, a workgroup-uniform cursor into the
// segment table (kernel arguments) only moves forward, 16-byte accesses.  The two stages of the statistics are
// csrc/tensor_walk.h's walk, a partial and a ring entry being one 64-byte struct.
//
// The library is built with -ffast-math: the two counts compare integer images and never floats, the maximum is taken on
// the integer image of (float) |Delta| (integer order is float order for non-negative floats).  Delta is one fp64
// subtraction; the squares of floats are exact in fp64; a product may be fused into the addition that follows it.
#include "tensor_walk.h"

namespace {
struct alignas(16) Entry {                 // one (window, tensor) piece, and the ring's entry of one tensor
  double sumsq_d, sumsq_p, dot_dg, sumsq_g, sumsq_m, sum_v;
  uint32_t absmax_bits;                    // the image of a non-negative float
  int32_t n_still, n_one_ulp, reserved;
};
static_assert(sizeof(Entry) == 64, "a partial and a ring entry are 64 bytes");

// the step this launch belongs to and whether it is due: applied, and every `every`-th
__device__ __forceinline__ bool due_step(const svit_step_dev* d, int64_t every, int64_t& s) {
  s = d->applied + d->skipped - 1;
  return d->apply == 1 && s >= 0 && s % every == 0;
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
    if (i >= n || !seg_inside<true>(T, k, lo, lo + window, i)) continue;             // no table: the whole buffer
    if (i + 4 <= n) {
      *(float4*)(shadow + i) = *(const float4*)(p + i);
    } else {                               // the last quad of a whole buffer with n % 4 != 0: element by element, below n
      for (int e = 0; e < 4; ++e)
        if (i + e < n) shadow[i + e] = p[i + e];
    }
  }
}

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
struct UpdateStat {
  struct Acc {
    double sd, sp, dg, sg, sm, sv;
    uint32_t amax;
    int32_t still, one;
  };
  using Partial = ::Entry;                 // the one above, which the kernels' signatures name
  using Entry = ::Entry;
  static constexpr int kStreams = 5;       // p, shadow, g, m, v
  __device__ static constexpr bool live(int s) { return s < 3 || (s == 3 ? HAS_M : HAS_V); }
  __device__ static __forceinline__ Acc zero() { return {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0, 0}; }

  // called inside the walk's loop over a window's tensors, which is where this_turn has to act
  __device__ static __forceinline__ void element(Acc& a, const float (&x)[kStreams], int32_t) {
    const float pn = this_turn(x[0]), po = this_turn(x[1]), g = this_turn(x[2]);
    const float m = HAS_M ? this_turn(x[3]) : 0.f, v = HAS_V ? this_turn(x[4]) : 0.f;
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

  __device__ static __forceinline__ void add(Acc& a, const Entry& q) {
    a.sd += q.sumsq_d; a.sp += q.sumsq_p; a.dg += q.dot_dg; a.sg += q.sumsq_g; a.sm += q.sumsq_m; a.sv += q.sum_v;
    a.amax = q.absmax_bits > a.amax ? q.absmax_bits : a.amax;
    a.still += q.n_still;
    a.one += q.n_one_ulp;
  }

  // the order of the additions is fixed
  __device__ static __forceinline__ void wave_fold(Acc& a) {
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

  __device__ static __forceinline__ Entry partial(const Acc& a) {
    return {a.sd, a.sp, a.dg, a.sg, a.sm, a.sv, a.amax, a.still, a.one, 0};
  }
  __device__ static __forceinline__ Entry entry(const Acc& a) { return partial(a); }
};

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
  const float* const src[5] = {p, shadow, g, m, v};
  walk_pieces<UpdateStat<HAS_M, HAS_V>>(src, n, table, Tn, part, T);
}

__global__ __launch_bounds__(64) void update_stats_fold(const int64_t* __restrict__ table, int Tn,
                                                        const svit_step_dev* __restrict__ d, int64_t every, int flags,
                                                        const Entry* __restrict__ part, unsigned char* __restrict__ ring,
                                                        int64_t R, const SegTable T) {
  int64_t s;
  if (!due_step(d, every, s)) return;
  walk_fold<UpdateStat<true, true>>(table, Tn, s, flags, part, ring, R, T);      // the fold reads no stream
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

extern "C" int64_t svit_update_stats_workspace(int64_t n, int64_t Tn) { return walk_workspace(n, Tn, sizeof(Entry)); }

extern "C" int svit_update_stats(const float* p, const float* shadow, const float* g, const float* m, const float* v,
                                 int64_t n, const int64_t* table_dev, const int64_t* table_host, int64_t Tn,
                                 const int64_t* segs, int64_t S, const svit_step_dev* dev_rec, void* ring, int64_t R,
                                 int64_t every, void* workspace, int64_t workspace_bytes, void* stream) {
  SegTable T;
  unsigned windows;
  if (int rc = walk_args({p, shadow, g, ring, workspace}, {m, v}, table_dev, table_host, Tn, n, segs, S, dev_rec, R,
                         every, workspace_bytes, sizeof(Entry), &T, &windows))
    return rc;
  const int flags = (m ? 1 : 0) | (v ? 2 : 0);
  const hipStream_t st = (hipStream_t)stream;
  Entry* part = (Entry*)workspace;
  switch (flags) {
    case 3: launch_pieces<true, true>(windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    case 1: launch_pieces<true, false>(windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    case 2: launch_pieces<false, true>(windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
    default: launch_pieces<false, false>(windows, st, p, shadow, g, m, v, n, table_dev, (int)Tn, dev_rec, every, part, T); break;
  }
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(update_stats_fold, dim3((unsigned)Tn), dim3(64), 0, st, table_dev, (int)Tn, dev_rec, every, flags,
                     (const Entry*)workspace, (unsigned char*)ring, R, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
