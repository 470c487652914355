// The walk of the flat parameter buffer behind a tensor table, once: csrc/monitor.hip and csrc/update.hip put their
// statistics on it -- gfx950.  The segment table and its tests are csrc/seg_table.h's.
//
// The buffers hold every parameter behind one tensor table (begin, end per tensor, in device memory); the trainable
// segments (unions of whole tensors; S == 0: the whole buffer) ride in the kernel arguments as a SegTable.
//
// Stage 1, walk_pieces: workgroup w takes the window [w * 4096, (w + 1) * 4096) of the buffers, finds the first tensor
// that ends past the window's begin by bisection and walks on from there with a cursor that only moves forward; the loop
// over the tensors a window meets is workgroup-uniform (the table is read at uniform addresses).  Begins are multiples of
// 4, so a quad of floats lies in one tensor or in none: a lane loads each of its four quads once per stream, 16 bytes at
// a time, BEFORE the search (the loads fly while the table is read) and only inside a trainable segment.  Each (window,
// tensor) piece is reduced lane -> wave -> workgroup in a fixed order and stored as ONE partial at slot window + tensor:
// along the walk every new piece increases one of the two indices, so no two pieces share a slot and n_windows + Tn slots
// suffice.
// Stage 2, walk_fold: one wave per tensor folds its partials (lane l takes the tensor's windows l, l + 64, ... in
// ascending order, then the lanes combine in the statistic's fixed butterfly) and writes the tensor's entry of the ring
// row; the wave of tensor 0 also writes the row's 16-byte header.
//
// No atomics, no ticket, no counter a kernel advances: the step index comes from the guard's record, which the guard in
// front has already written, so a row is the same bit for bit from run to run and from the eager step to a replay.  The
// library is built with -ffast-math; that promise rests on the fp64 additions of a statistic staying in the order its
// element / add / wave_fold write them.
//
// A statistic `Stat` supplies: the types Acc (a lane's running values), Partial (a workspace slot) and Entry (a tensor's
// part of the ring row, after the header); kStreams and live(s), the float buffers it reads and which of them this
// instantiation reads at all; zero(); element(acc, x, offset) with x[s] the element's value in stream s (0 where the
// stream is not live) and offset its position in the tensor; add(acc, partial); wave_fold(acc), after which all 64 lanes
// hold the wave's values; partial(acc) and entry(acc).  The __global__ kernels stay with the statistic: each decides by
// its own rule whether the step is due and says what the header's third word is.
//
// The streams reach walk_pieces as an array of pointers, so the kernels' __restrict__ on them ends at the call: they are
// only read, before the first store, and the timings of tools/bench_monitor.py and tools/bench_updmon.py hold with it.
// Everything sits in an unnamed namespace, as the kernels that take a SegTable do: every source keeps its own copy.
#pragma once
#include <cstring>
#include <initializer_list>

#include "seg_table.h"

namespace {
constexpr int kWindow = 4096;              // floats per window: svit_tensor_stats_window()
constexpr int kThreads = 256;
constexpr int kPasses = kWindow / (kThreads * 4);
constexpr int64_t kMaxTensors = 4096;
constexpr int32_t kNone = 0x7fffffff;      // no offset; a tensor is shorter than this

// stage 1 of a due step: this workgroup's window, one partial per tensor it meets
template <class Stat>
__device__ __forceinline__ void walk_pieces(const float* const (&src)[Stat::kStreams], int64_t n,
                                            const int64_t* __restrict__ table, int Tn,
                                            typename Stat::Partial* __restrict__ part, const SegTable& T) {
  __shared__ typename Stat::Partial red[2][kThreads / 64];
  const int64_t w = blockIdx.x, lo = w * kWindow, hi = (lo + kWindow < n) ? lo + kWindow : n;
  // the lane's quads first, so that the loads are in flight while the table is searched: a quad is loaded when it lies
  // inside a segment (segments hold whole tensors, so this is "inside a trainable tensor or its padding"); what a lane did
  // not load it never counts.  The array of a stream that is not live is never written and never read.
  float x[Stat::kStreams][kPasses][4];
#pragma unroll
  for (int j = 0; j < kPasses; ++j) {
    const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
#pragma unroll
    for (int s = 0; s < Stat::kStreams; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) x[s][j][e] = 0.f;
    if (i >= hi || !trainable(T, i)) continue;
    if (i + 4 <= n) {
#pragma unroll
      for (int s = 0; s < Stat::kStreams; ++s)
        if (Stat::live(s)) {
          const float4 X = *(const float4*)(src[s] + i);
          x[s][j][0] = X.x; x[s][j][1] = X.y; x[s][j][2] = X.z; x[s][j][3] = X.w;
        }
    } else {                               // the last quad of a buffer with n % 4 != 0: element by element, below n
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) {
#pragma unroll
          for (int s = 0; s < Stat::kStreams; ++s)
            if (Stat::live(s)) x[s][j][e] = src[s][i + e];
        }
    }
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
    typename Stat::Acc acc = Stat::zero();
    bool any = false;
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
      const int64_t i = lo + (int64_t)j * (kThreads * 4) + (int64_t)threadIdx.x * 4;
      if (i < tb || i >= te || i >= hi) continue;
      any = true;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < te) {
          float xe[Stat::kStreams];
#pragma unroll
          for (int s = 0; s < Stat::kStreams; ++s) xe[s] = Stat::live(s) ? x[s][j][e] : 0.f;
          Stat::element(acc, xe, (int32_t)(i + e - tb));
        }
    }
    if (__any(any)) Stat::wave_fold(acc);
    if (lane == 0) red[par][wave] = Stat::partial(acc);
    __syncthreads();
    if (threadIdx.x == 0) {
      typename Stat::Acc sum = Stat::zero();
#pragma unroll
      for (int k = 0; k < kThreads / 64; ++k) Stat::add(sum, red[par][k]);
      part[w + t] = Stat::partial(sum);
    }
    par ^= 1;      // the other buffer next: a wave writes it only behind the barrier thread 0 reaches after this read
  }
}

// stage 2 of the due step s: this wave's tensor; `word` is the header's third
template <class Stat>
__device__ __forceinline__ void walk_fold(const int64_t* __restrict__ table, int Tn, int64_t s, int32_t word,
                                          const typename Stat::Partial* __restrict__ part,
                                          unsigned char* __restrict__ ring, int64_t R, const SegTable& T) {
  constexpr int64_t kEntry = sizeof(typename Stat::Entry);
  const int t = blockIdx.x, lane = threadIdx.x;
  unsigned char* row = ring + (s % R) * (int64_t)(16 + kEntry * (int64_t)Tn);
  if (t == 0 && lane == 0) {
    *(int64_t*)row = s;
    ((int32_t*)row)[2] = word;
    ((int32_t*)row)[3] = 0;
  }
  const int64_t tb = table[2 * t], te = table[2 * t + 1];
  if (!trainable(T, tb)) return;
  const int64_t w0 = tb / kWindow, w1 = (te - 1) / kWindow;
  typename Stat::Acc acc = Stat::zero();
  for (int64_t w = w0 + lane; w <= w1; w += 64) Stat::add(acc, part[w + t]);
  Stat::wave_fold(acc);
  if (lane == 0) *(typename Stat::Entry*)(row + 16 + kEntry * (int64_t)t) = Stat::entry(acc);
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline int table_check(const int64_t* table, int64_t Tn, int64_t n) {
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

// the `_seg` rules with their error codes; S == 0: no table, the whole buffer.  The table is a by-value kernel argument:
// all of it is written
inline int segs_take(const int64_t* segs, int64_t S, int64_t n, SegTable* out) {
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

inline int64_t walk_windows(int64_t n) { return (n + kWindow - 1) / kWindow; }

// n_windows + Tn slots (above)
inline int64_t walk_workspace(int64_t n, int64_t Tn, size_t partial_bytes) {
  if (n <= 0 || Tn < 1 || Tn > kMaxTensors) return SVIT_ERR_ARG;
  return (walk_windows(n) + Tn) * (int64_t)partial_bytes;
}

// what the two `*_stats` entry points check, in one order: `needed` and `optional` (may be null) are the pointers of
// 16-byte accesses -- streams, ring, workspace.  -> the segment table and the stage-1 grid
inline int walk_args(std::initializer_list<const void*> needed, std::initializer_list<const void*> optional,
                     const int64_t* table_dev, const int64_t* table_host, int64_t Tn, int64_t n, const int64_t* segs,
                     int64_t S, const svit_step_dev* dev_rec, int64_t R, int64_t every, int64_t workspace_bytes,
                     size_t partial_bytes, SegTable* T, unsigned* windows) {
  uintptr_t bits = 0;
  for (const void* q : needed) {
    if (!q) return SVIT_ERR_ARG;
    bits |= (uintptr_t)q;
  }
  for (const void* q : optional) bits |= (uintptr_t)q;
  if (!table_dev || !dev_rec || R < 1 || every < 1) return SVIT_ERR_ARG;
  if (int rc = table_check(table_host, Tn, n)) return rc;
  if (int rc = segs_take(segs, S, n, T)) return rc;
  if (workspace_bytes < walk_workspace(n, Tn, partial_bytes)) return SVIT_ERR_ARG;
  if (bits & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)table_dev | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  if (walk_windows(n) > 0x7fffffff) return SVIT_ERR_ARG;
  *windows = (unsigned)walk_windows(n);
  return SVIT_OK;
}
}  // namespace
