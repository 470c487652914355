// Per-tensor gradient and weight statistics inside the captured step (svit_tensor_stats) -- gfx950.
//
// Two launches between the guard and the solver leave, per tensor of the flat gradient and weight buffers, the fp64 sums
// of squares of g and p, the largest finite |g|, the number of non-finite elements of g and the offset of the first one,
// in a row of a ring in device memory (include/svit_hip.h: svit_tensor_stats).  The yardstick is svit_amd/monitor.py
// stats_host.  The two stages are csrc/tensor_walk.h's walk; here is what it accumulates and when.
//
// A step is recorded when its index s = applied + skipped - 1 is a multiple of `every`, and whenever the guard dropped
// it; the header's third word is the guard's decision.
//
// The library is built with -ffast-math: an element is classified by its exponent bits, the maximum is taken on the
// integer image of |g| (integer order is float order for finite non-negative floats), and a non-finite element enters
// the sum as the integer image of 0.0f.  (double) x * (double) x is exact for every float, so only the fp64 additions
// round.
#include "tensor_walk.h"

namespace {
// the step this launch belongs to and whether it is recorded: every `every`-th step, and every dropped one
__device__ __forceinline__ bool recorded_step(const svit_step_dev* d, int64_t every, int64_t& s) {
  s = d->applied + d->skipped - 1;
  return s >= 0 && (d->apply == 0 || s % every == 0);
}

struct alignas(16) Partial {               // one (window, tensor) piece
  double sumsq_g, sumsq_p;
  uint32_t absmax_bits;
  int32_t n_bad, first_bad, reserved;      // first_bad: in-tensor offset, kNone when none
};
struct alignas(16) Entry {                 // the ring's entry of one tensor (include/svit_hip.h)
  double sumsq_g, sumsq_p;
  float absmax_g;
  int32_t n_bad, first_bad, reserved;      // first_bad: -1 when none
};
static_assert(sizeof(Partial) == 32 && sizeof(Entry) == 32, "a partial and a ring entry are 32 bytes");

struct TensorStat {
  struct Acc {
    double sg, sp;
    uint32_t amax;
    int32_t nbad, first;
  };
  using Partial = ::Partial;               // the two above, which the kernels' signatures name
  using Entry = ::Entry;
  static constexpr int kStreams = 2;       // g, p
  __device__ static constexpr bool live(int) { return true; }
  __device__ static __forceinline__ Acc zero() { return {0.0, 0.0, 0u, 0, kNone}; }

  __device__ static __forceinline__ void element(Acc& a, const float (&x)[kStreams], int32_t offset) {
    const uint32_t bits = __float_as_uint(x[0]);
    const bool finite = (bits & 0x7f800000u) != 0x7f800000u;
    const uint32_t mag = bits & 0x7fffffffu;
    const double gd = (double)__uint_as_float(finite ? bits : 0u), pd = (double)x[1];
    a.sg += gd * gd;
    a.sp += pd * pd;
    a.amax = (finite && mag > a.amax) ? mag : a.amax;
    a.nbad += finite ? 0 : 1;
    a.first = (!finite && offset < a.first) ? offset : a.first;
  }

  __device__ static __forceinline__ void add(Acc& a, const Partial& q) {
    a.sg += q.sumsq_g;
    a.sp += q.sumsq_p;
    a.amax = q.absmax_bits > a.amax ? q.absmax_bits : a.amax;
    a.nbad += q.n_bad;
    a.first = q.first_bad < a.first ? q.first_bad : a.first;
  }

  // the order of the additions is fixed
  __device__ static __forceinline__ void wave_fold(Acc& a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a.sg += __shfl_xor(a.sg, o, 64);
      a.sp += __shfl_xor(a.sp, o, 64);
      const uint32_t m = (uint32_t)__shfl_xor((int)a.amax, o, 64);
      a.amax = m > a.amax ? m : a.amax;
      a.nbad += __shfl_xor(a.nbad, o, 64);
      const int32_t f = __shfl_xor(a.first, o, 64);
      a.first = f < a.first ? f : a.first;
    }
  }

  __device__ static __forceinline__ Partial partial(const Acc& a) { return {a.sg, a.sp, a.amax, a.nbad, a.first, 0}; }
  __device__ static __forceinline__ Entry entry(const Acc& a) {
    return {a.sg, a.sp, __uint_as_float(a.amax), a.nbad, a.first == kNone ? -1 : a.first, 0};
  }
};

__global__ __launch_bounds__(kThreads) void tensor_stats_pieces(const float* __restrict__ g, const float* __restrict__ p,
                                                                int64_t n, const int64_t* __restrict__ table, int Tn,
                                                                const svit_step_dev* __restrict__ d, int64_t every,
                                                                Partial* __restrict__ part, const SegTable T) {
  int64_t s;
  if (!recorded_step(d, every, s)) return;
  const float* const src[2] = {g, p};
  walk_pieces<TensorStat>(src, n, table, Tn, part, T);
}

__global__ __launch_bounds__(64) void tensor_stats_fold(const int64_t* __restrict__ table, int Tn,
                                                        const svit_step_dev* __restrict__ d, int64_t every,
                                                        const Partial* __restrict__ part, unsigned char* __restrict__ ring,
                                                        int64_t R, const SegTable T) {
  int64_t s;
  if (!recorded_step(d, every, s)) return;
  walk_fold<TensorStat>(table, Tn, s, d->apply, part, ring, R, T);
}
}  // namespace

extern "C" int svit_tensor_stats_window(void) { return kWindow; }

extern "C" int svit_tensor_table_check(const int64_t* table, int64_t Tn, int64_t n) { return table_check(table, Tn, n); }

extern "C" int64_t svit_tensor_stats_workspace(int64_t n, int64_t Tn) { return walk_workspace(n, Tn, sizeof(Partial)); }

extern "C" int svit_tensor_stats(const float* g, const float* p, int64_t n, const int64_t* table_dev,
                                 const int64_t* table_host, int64_t Tn, const int64_t* segs, int64_t S,
                                 const svit_step_dev* dev_rec, void* ring, int64_t R, int64_t every, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  SegTable T;
  unsigned windows;
  if (int rc = walk_args({g, p, ring, workspace}, {}, table_dev, table_host, Tn, n, segs, S, dev_rec, R, every,
                         workspace_bytes, sizeof(Partial), &T, &windows))
    return rc;
  hipLaunchKernelGGL(tensor_stats_pieces, dim3(windows), dim3(kThreads), 0, (hipStream_t)stream, g, p, n, table_dev,
                     (int)Tn, dev_rec, every, (Partial*)workspace, T);
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(tensor_stats_fold, dim3((unsigned)Tn), dim3(64), 0, (hipStream_t)stream, table_dev, (int)Tn,
                     dev_rec, every, (const Partial*)workspace, (unsigned char*)ring, R, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
