// Per-tensor gradient and weight statistics inside the captured step (svit_tensor_stats) -- gfx950.
//
// The flat gradient and weight buffers hold every parameter behind one tensor table (begin, end per tensor, in device
// memory).  Two launches between the guard and the solver leave, per tensor, the fp64 sums of squares of g and p, the
// largest finite |g|, the number of non-finite elements of g and the offset of the first one, in a row of a ring in
// device memory (include/svit_hip.h: svit_tensor_stats).  The yardstick is svit_amd/monitor.py stats_host.
//
// Stage 1, tensor_stats_pieces: workgroup w takes the window [w * 4096, (w + 1) * 4096) of the buffers, finds the first
// tensor that ends past the window's begin by bisection and walks on from there with a cursor that only moves forward;
// the loop over the tensors a window meets is workgroup-uniform (the table is read at uniform addresses).  Begins are
// multiples of 4, so a quad of floats lies in one tensor or in none: a lane loads each of its four quads once, 16 bytes
// at a time, BEFORE the search (the loads fly while the table is read) and only inside a trainable segment.  Each
// (window, tensor) piece is reduced lane -> wave -> workgroup in a fixed order and stored as ONE partial at slot
// window + tensor: along the walk every new piece increases one of the two indices, so no two pieces share a slot and
// n_windows + Tn slots suffice.
// Stage 2, tensor_stats_fold: one wave per tensor folds its partials (lane l takes the tensor's windows l, l + 64, ... in
// ascending order, then the lanes combine in a fixed butterfly) and writes the tensor's entry of the ring row; the wave
// of tensor 0 also writes the row's header.
//
// No atomics, no ticket, no counter a kernel advances: the step index is derived from the guard's record, which the
// guard in front has already written.  Every result is therefore the same bit for bit from run to run and from the
// eager step to a replay.
//
// The library is built with -ffast-math: an element is classified by its exponent bits, the maximum is taken on the
// integer image of |g| (integer order is float order for finite non-negative floats), and a non-finite element enters
// the sum as the integer image of 0.0f.  (double) x * (double) x is exact for every float, so only the fp64 additions
// round.
#include <cstring>

#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int kWindow = 4096;              // floats per window
constexpr int kThreads = 256;
constexpr int kPasses = kWindow / (kThreads * 4);
constexpr int64_t kMaxTensors = 4096;

struct alignas(16) Partial {               // one (window, tensor) piece
  double sumsq_g, sumsq_p;
  uint32_t absmax_bits;
  int32_t n_bad, first_bad, reserved;      // first_bad: in-tensor offset, INT32_MAX when none
};
static_assert(sizeof(Partial) == 32, "a partial is 32 bytes");

struct alignas(16) Entry {                 // the ring's entry of one tensor (include/svit_hip.h)
  double sumsq_g, sumsq_p;
  float absmax_g;
  int32_t n_bad, first_bad, reserved;
};
static_assert(sizeof(Entry) == 32, "a ring entry is 32 bytes");

constexpr int32_t kNone = 0x7fffffff;

struct SegTable {
  int64_t v[SVIT_MAX_SEGS][2];
  int32_t S;
};

// the step this launch belongs to and whether it is recorded: every `every`-th step, and every dropped one
__device__ __forceinline__ bool recorded_step(const svit_step_dev* d, int64_t every, int64_t& s) {
  s = d->applied + d->skipped - 1;
  return s >= 0 && (d->apply == 0 || s % every == 0);
}

// a tensor is trainable when its begin lies inside a segment (segments are unions of whole slots, so every position of
// the tensor then does); S == 0: all are
__device__ __forceinline__ bool trainable(const SegTable& T, int64_t begin) {
  if (T.S == 0) return true;
  bool in = false;
  for (int j = 0; j < T.S; ++j) in |= (begin >= T.v[j][0]) & (begin < T.v[j][1]);
  return in;
}

struct Acc {
  double sg, sp;
  uint32_t amax;
  int32_t nbad, first;
};

__device__ __forceinline__ void acc_element(Acc& a, float g, float p, int32_t offset) {
  const uint32_t bits = __float_as_uint(g);
  const bool finite = (bits & 0x7f800000u) != 0x7f800000u;
  const uint32_t mag = bits & 0x7fffffffu;
  const double gd = (double)__uint_as_float(finite ? bits : 0u), pd = (double)p;
  a.sg += gd * gd;
  a.sp += pd * pd;
  a.amax = (finite && mag > a.amax) ? mag : a.amax;
  a.nbad += finite ? 0 : 1;
  a.first = (!finite && offset < a.first) ? offset : a.first;
}

// all 64 lanes leave with the wave's values; the order of the additions is fixed
__device__ __forceinline__ void wave_fold(Acc& a) {
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

__global__ __launch_bounds__(kThreads) void tensor_stats_pieces(const float* __restrict__ g, const float* __restrict__ p,
                                                                int64_t n, const int64_t* __restrict__ table, int Tn,
                                                                const svit_step_dev* __restrict__ d, int64_t every,
                                                                Partial* __restrict__ part, const SegTable T) {
  int64_t s;
  if (!recorded_step(d, every, s)) return;
  __shared__ Partial red[2][kThreads / 64];
  const int64_t w = blockIdx.x, lo = w * kWindow, hi = (lo + kWindow < n) ? lo + kWindow : n;
  // the lane's quads first, so that the loads are in flight while the table is searched: a quad is loaded when it lies
  // inside a segment (the segments ride in the kernel arguments and hold whole tensors, so this is "inside a trainable
  // tensor or its padding"); what a lane did not load it never counts
  float gv[kPasses][4], pv[kPasses][4];
#pragma unroll
  for (int j = 0; j < kPasses; ++j) {
    const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[j][e] = pv[j][e] = 0.f;
    if (i >= hi || !trainable(T, i)) continue;
    if (i + 4 <= n) {
      const float4 G = *(const float4*)(g + i), P = *(const float4*)(p + i);
      gv[j][0] = G.x; gv[j][1] = G.y; gv[j][2] = G.z; gv[j][3] = G.w;
      pv[j][0] = P.x; pv[j][1] = P.y; pv[j][2] = P.z; pv[j][3] = P.w;
    } else {                               // the last quad of a buffer with n % 4 != 0: element by element, below n
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) {
          gv[j][e] = g[i + e];
          pv[j][e] = p[i + e];
        }
    }
  }
  int a = 0, b = Tn;                       // first tensor that ends past lo
  while (a < b) {
    const int m = (a + b) >> 1;
    if (table[2 * m + 1] <= lo) a = m + 1; else b = m;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int par = 0;
  for (int t = a; t < Tn; ++t) {
    const int64_t tb = table[2 * t], te = table[2 * t + 1];
    if (tb >= hi) break;
    if (!trainable(T, tb)) continue;
    Acc acc = {0.0, 0.0, 0u, 0, kNone};
    bool any = false;
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
      if (i < tb || i >= te || i >= hi) continue;
      any = true;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < te) acc_element(acc, gv[j][e], pv[j][e], (int32_t)(i + e - tb));
    }
    if (__any(any)) wave_fold(acc);
    if (lane == 0) {
      Partial q;
      q.sumsq_g = acc.sg; q.sumsq_p = acc.sp; q.absmax_bits = acc.amax;
      q.n_bad = acc.nbad; q.first_bad = acc.first; q.reserved = 0;
      red[par][wave] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      Partial q = red[par][0];
#pragma unroll
      for (int v = 1; v < kThreads / 64; ++v) {
        const Partial r = red[par][v];
        q.sumsq_g += r.sumsq_g;
        q.sumsq_p += r.sumsq_p;
        q.absmax_bits = r.absmax_bits > q.absmax_bits ? r.absmax_bits : q.absmax_bits;
        q.n_bad += r.n_bad;
        q.first_bad = r.first_bad < q.first_bad ? r.first_bad : q.first_bad;
      }
      part[w + t] = q;
    }
    par ^= 1;      // the other buffer next: a wave writes it only behind the barrier thread 0 reaches after this read
  }
}

__global__ __launch_bounds__(64) void tensor_stats_fold(const int64_t* __restrict__ table, int Tn,
                                                        const svit_step_dev* __restrict__ d, int64_t every,
                                                        const Partial* __restrict__ part, unsigned char* __restrict__ ring,
                                                        int64_t R, const SegTable T) {
  int64_t s;
  if (!recorded_step(d, every, s)) return;
  const int t = blockIdx.x, lane = threadIdx.x;
  unsigned char* row = ring + (s % R) * (int64_t)(16 + 32 * (int64_t)Tn);
  if (t == 0 && lane == 0) {
    *(int64_t*)row = s;
    ((int32_t*)row)[2] = d->apply;
    ((int32_t*)row)[3] = 0;
  }
  const int64_t tb = table[2 * t], te = table[2 * t + 1];
  if (!trainable(T, tb)) return;
  const int64_t w0 = tb / kWindow, w1 = (te - 1) / kWindow;
  Acc acc = {0.0, 0.0, 0u, 0, kNone};
  for (int64_t w = w0 + lane; w <= w1; w += 64) {
    const Partial q = part[w + t];
    acc.sg += q.sumsq_g;
    acc.sp += q.sumsq_p;
    acc.amax = q.absmax_bits > acc.amax ? q.absmax_bits : acc.amax;
    acc.nbad += q.n_bad;
    acc.first = q.first_bad < acc.first ? q.first_bad : acc.first;
  }
  wave_fold(acc);
  if (lane == 0) {
    Entry e;
    e.sumsq_g = acc.sg; e.sumsq_p = acc.sp; e.absmax_g = __uint_as_float(acc.amax);
    e.n_bad = acc.nbad; e.first_bad = acc.first == kNone ? -1 : acc.first; e.reserved = 0;
    *(Entry*)(row + 16 + 32 * (int64_t)t) = e;
  }
}

int table_check(const int64_t* table, int64_t Tn, int64_t n) {
  if (!table || Tn < 1 || Tn > kMaxTensors || n <= 0) return SVIT_ERR_ARG;
  int64_t prev = 0;
  for (int64_t t = 0; t < Tn; ++t) {
    const int64_t b = table[2 * t], e = table[2 * t + 1];
    if (b < prev || e <= b || e > n || e - b >= (int64_t)kNone) return SVIT_ERR_ARG;
    if (b & 3) return SVIT_ERR_ALIGN;
    prev = e;
  }
  return SVIT_OK;
}

// the `_seg` rules with their error codes; S == 0: no table, the whole buffer
int segs_take(const int64_t* segs, int64_t S, int64_t n, SegTable* out) {
  out->S = 0;
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
}  // namespace

extern "C" int svit_tensor_stats_window(void) { return kWindow; }

extern "C" int svit_tensor_table_check(const int64_t* table, int64_t Tn, int64_t n) { return table_check(table, Tn, n); }

extern "C" int64_t svit_tensor_stats_workspace(int64_t n, int64_t Tn) {
  if (n <= 0 || Tn < 1 || Tn > kMaxTensors) return SVIT_ERR_ARG;
  return ((n + kWindow - 1) / kWindow + Tn) * (int64_t)sizeof(Partial);
}

extern "C" int svit_tensor_stats(const float* g, const float* p, int64_t n, const int64_t* table_dev,
                                 const int64_t* table_host, int64_t Tn, const int64_t* segs, int64_t S,
                                 const svit_step_dev* dev_rec, void* ring, int64_t R, int64_t every, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  if (!g || !p || !table_dev || !dev_rec || !ring || !workspace || R < 1 || every < 1) return SVIT_ERR_ARG;
  if (int rc = table_check(table_host, Tn, n)) return rc;
  SegTable T;
  if (int rc = segs_take(segs, S, n, &T)) return rc;
  if (workspace_bytes < svit_tensor_stats_workspace(n, Tn)) return SVIT_ERR_ARG;
  if (((uintptr_t)g | (uintptr_t)p | (uintptr_t)ring | (uintptr_t)workspace) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)table_dev | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  const int64_t windows = (n + kWindow - 1) / kWindow;
  if (windows > 0x7fffffff) return SVIT_ERR_ARG;
  hipLaunchKernelGGL(tensor_stats_pieces, dim3((unsigned)windows), dim3(kThreads), 0, (hipStream_t)stream, g, p, n,
                     table_dev, (int)Tn, dev_rec, every, (Partial*)workspace, T);
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(tensor_stats_fold, dim3((unsigned)Tn), dim3(64), 0, (hipStream_t)stream, table_dev, (int)Tn,
                     dev_rec, every, (const Partial*)workspace, (unsigned char*)ring, R, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
