// Per-block forward statistics from the statistics the forward already keeps (svit_act_stats) -- gfx950.
//
// A training forward saves, for its backward, the per-row LayerNorm statistics in front of every block's attention
// branch (mean1 / rstd1), in front of its MLP (mean2 / rstd2) and in front of the final norm, and the attention's
// log-sum-exp per (sample, head, query).  ln_fwd_kernel forms `mean` as a plain sum and `rstd` from the two-pass
// variance with no clamp, so one non-finite element of a row is visible in that row's mean or rstd, and for a finite
// row  mean^2 + 1 / rstd^2 - eps  is the row's mean square.  Two launches read those small arrays -- never the
// activations -- and leave one 32-byte entry per site in a row of a ring in device memory (include/svit_hip.h:
// svit_act_stats).  The yardstick is svit_amd/actmon.py acts_host.
//
// The site table (at most 96 x 24 bytes) rides in the KERNEL ARGUMENTS: an eager pass has fresh arrays every time, a
// capture bakes its pool's static addresses, and neither needs a table in device memory that somebody has to update.
//
// Stage 1, act_stats_windows: workgroup w takes window w of the concatenated sites (4096 rows of ONE site), finds its
// site by bisection over first_window -- blockIdx-derived, hence workgroup-uniform reads of the arguments -- issues its
// 16 + 16 coalesced 4-byte loads, then reduces lane -> wave -> workgroup in a fixed order and stores ONE partial at
// slot w of the workspace, which no other workgroup shares.
// Stage 2, act_stats_fold: ONE workgroup.  Thread s folds the partials of site s in window order and writes the
// site's entry at its slot of ring row (pass % R); the slots no site names get the empty entry (n_bad = -1); thread 0
// writes the header and then advances the pass counter state[0], which it alone read at entry (the contract of
// svit_meter_push: a single workgroup reads the counter at entry and writes it at exit; stage 1 never reads it).
//
// No atomics, no ticket: a row is the same bit for bit from run to run and from the eager pass to a replay.
//
// The library is built with -ffast-math, so nothing here relies on a float comparison or on isfinite: rows are
// classified on the integer images (exponent bits, sign bit, zero), extrema are taken on integer keys that are monotone
// in the float order of finite values (-0.0 below +0.0), and the extremum and its row travel as ONE 64-bit key
// (key << 32 | row) whose minimum is the extremum with the smallest row among ties.
//
// The term of a good LayerNorm row is  (double) mean * mean + 1 / ((double) rstd * rstd).  Both products are exact in
// fp64 (24 x 24 bits), and fma(m, m, r) rounds the same exact value as m * m + r, so contraction changes nothing.  The
// reciprocal is NOT left to what -ffast-math makes of an fp64 division: d = rstd^2 lies in [2^-298, 2^256], well inside
// the normal range with its reciprocal; v_rcp_f64 gives x0 with |1 - d x0| <= 2^-23 at the very least (the ISA
// documents it far tighter); a Newton step e = fma(-d, x, 1), x' = fma(x, e, x) leaves |1 - d x'| <= e^2 + 2^-52, so
// two steps give 2^-46 -> below 2^-51, and the final addition rounds once more: relative error of a term <= 2^-40 with
// a wide margin.  Only the fp64 additions of the sum round beyond that.
#include <cstring>

#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int kWindow = 4096;              // rows per window
constexpr int kThreads = 256;
constexpr int kPer = kWindow / kThreads;   // rows per thread
constexpr int kMaxSites = SVIT_ACT_MAX_SITES;
constexpr int kMaxSlots = 1024;
constexpr int32_t kMaxRows = 1 << 24;
constexpr uint64_t kNoBest = ~0ull;
constexpr int32_t kNone = 0x7fffffff;

struct SiteTable {                          // the kernels' copy: first_window filled in by the host wrapper
  svit_act_site s[kMaxSites];
  int32_t slot[kMaxSites];
  int32_t n_sites, n_slots, total_windows, reserved;
};

struct alignas(16) Partial {               // one window of one site
  double sum;
  uint64_t best;                           // key << 32 | row, kNoBest when the window has no good row
  uint32_t ext2_bits;                      // largest |mean| as its integer image
  int32_t n_bad, first_bad, reserved;      // first_bad: in-site row, kNone when none
};
static_assert(sizeof(Partial) == 32, "a partial is 32 bytes");

struct alignas(8) Entry {                  // include/svit_hip.h: the ring's entry of one slot
  double sum;
  float ext, ext2;
  int32_t arg, n_bad, first_bad, rows;
};
static_assert(sizeof(Entry) == 32, "a ring entry is 32 bytes");

struct Header {
  int64_t pass, step;
  int32_t B, Tx, T0, H0, W0, n_sites, reserved[2];
};
static_assert(sizeof(Header) == SVIT_ACT_HEADER_BYTES, "the row header is 48 bytes");

struct Geom { int32_t v[5]; };

__device__ __forceinline__ bool exp_all_ones(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }

// monotone in the float order of finite values; -0.0 sorts below +0.0
__device__ __forceinline__ uint32_t order_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t order_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

__device__ __forceinline__ double recip_sq(float rstd) {
  const double d = (double)rstd * (double)rstd;
  double x = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, x, 1.0);
  x = __builtin_fma(x, e, x);
  e = __builtin_fma(-d, x, 1.0);
  return __builtin_fma(x, e, x);
}

struct Acc {
  double sum;
  uint64_t best;
  uint32_t ext2;
  int32_t nbad, first;
};

__device__ __forceinline__ void acc_merge(Acc& a, double sum, uint64_t best, uint32_t ext2, int32_t nbad, int32_t first) {
  a.sum += sum;
  a.best = best < a.best ? best : a.best;
  a.ext2 = ext2 > a.ext2 ? ext2 : a.ext2;
  a.nbad += nbad;
  a.first = first < a.first ? first : a.first;
}

// all 64 lanes leave with the wave's values; the order of the additions is fixed
__device__ __forceinline__ void wave_fold(Acc& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double s = __shfl_xor(a.sum, o, 64);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)a.best, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(a.best >> 32), o, 64);
    const uint32_t m = (uint32_t)__shfl_xor((int)a.ext2, o, 64);
    const int32_t nb = __shfl_xor(a.nbad, o, 64);
    const int32_t f = __shfl_xor(a.first, o, 64);
    acc_merge(a, s, ((uint64_t)hi << 32) | lo, m, nb, f);
  }
}

__global__ __launch_bounds__(kThreads) void act_stats_windows(const SiteTable T, Partial* __restrict__ part) {
  __shared__ Partial red[kThreads / 64];
  const int w = blockIdx.x;
  int lo = 0, hi = T.n_sites;              // the last site whose first_window <= w
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (T.s[m].first_window <= w) lo = m; else hi = m;
  }
  const float* __restrict__ pa = T.s[lo].a;
  const float* __restrict__ pb = T.s[lo].b;
  const int32_t rows = T.s[lo].rows;
  const int32_t base = (w - T.s[lo].first_window) * kWindow;
  const bool ln = pb != nullptr;
  // the loads first: rows past the site's end are never touched
  uint32_t av[kPer], bv[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int32_t r = base + j * kThreads + (int)threadIdx.x;
    av[j] = 0u;
    bv[j] = 0x3f800000u;
    if (r < rows) {
      av[j] = __float_as_uint(pa[r]);
      if (ln) bv[j] = __float_as_uint(pb[r]);
    }
  }
  Acc acc = {0.0, kNoBest, 0u, 0, kNone};
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int32_t r = base + j * kThreads + (int)threadIdx.x;
    if (r >= rows) continue;
    const uint32_t a = av[j], b = bv[j];
    bool bad;
    double term;
    uint32_t key, e2 = 0u;
    if (ln) {
      bad = exp_all_ones(a) || exp_all_ones(b) || (b & 0x80000000u) != 0u || b == 0u;
      // a bad row's operands are replaced by 0 and 1 so that no NaN is ever formed, then left out
      const float m = __uint_as_float(bad ? 0u : a), s = __uint_as_float(bad ? 0x3f800000u : b);
      term = __builtin_fma((double)m, (double)m, recip_sq(s));
      key = b;                               // rstd > 0: the integer order is the float order; the smallest wins
      e2 = a & 0x7fffffffu;
    } else {
      bad = exp_all_ones(a);
      term = (double)__uint_as_float(bad ? 0u : a);
      key = ~order_key(a);                   // the largest value wins
    }
    if (bad) {
      acc.nbad += 1;
      acc.first = r < acc.first ? r : acc.first;
    } else {
      acc_merge(acc, term, ((uint64_t)key << 32) | (uint32_t)r, e2, 0, kNone);
    }
  }
  wave_fold(acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    Partial q;
    q.sum = acc.sum; q.best = acc.best; q.ext2_bits = acc.ext2; q.n_bad = acc.nbad; q.first_bad = acc.first;
    q.reserved = 0;
    red[wave] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial q = red[0];
    Acc t = {q.sum, q.best, q.ext2_bits, q.n_bad, q.first_bad};
#pragma unroll
    for (int v = 1; v < kThreads / 64; ++v) {
      const Partial r = red[v];
      acc_merge(t, r.sum, r.best, r.ext2_bits, r.n_bad, r.first_bad);
    }
    q.sum = t.sum; q.best = t.best; q.ext2_bits = t.ext2; q.n_bad = t.nbad; q.first_bad = t.first; q.reserved = 0;
    part[w] = q;
  }
}

__global__ __launch_bounds__(kThreads) void act_stats_fold(const SiteTable T, const Geom G,
                                                           const svit_step_dev* __restrict__ d,
                                                           const Partial* __restrict__ part,
                                                           unsigned char* __restrict__ ring, int64_t R,
                                                           int64_t* __restrict__ state) {
  __shared__ int64_t pass_s;
  __shared__ int32_t named[kMaxSlots];
  const int t = threadIdx.x;
  if (t == 0) pass_s = state[0];
  for (int k = t; k < T.n_slots; k += kThreads) named[k] = 0;
  __syncthreads();
  if (t < T.n_sites) named[T.slot[t]] = 1;
  __syncthreads();
  const int64_t pass = pass_s;
  const int64_t rr = ((pass % R) + R) % R;
  unsigned char* row = ring + rr * (int64_t)(SVIT_ACT_HEADER_BYTES + 32 * (int64_t)T.n_slots);
  Entry* entries = (Entry*)(row + SVIT_ACT_HEADER_BYTES);
  for (int k = t; k < T.n_slots; k += kThreads)
    if (!named[k]) {
      Entry e;
      e.sum = 0.0; e.ext = 0.f; e.ext2 = 0.f; e.arg = -1; e.n_bad = -1; e.first_bad = -1; e.rows = 0;
      entries[k] = e;
    }
  if (t < T.n_sites) {
    const int w0 = T.s[t].first_window;
    const int w1 = w0 + (T.s[t].rows + kWindow - 1) / kWindow;
    const bool ln = T.s[t].b != nullptr;
    Acc acc = {0.0, kNoBest, 0u, 0, kNone};
    for (int w = w0; w < w1; ++w) {
      const Partial q = part[w];
      acc_merge(acc, q.sum, q.best, q.ext2_bits, q.n_bad, q.first_bad);
    }
    Entry e;
    e.sum = acc.sum;
    e.n_bad = acc.nbad;
    e.first_bad = acc.first == kNone ? -1 : acc.first;
    e.rows = T.s[t].rows;
    if (acc.best == kNoBest) {
      e.ext = 0.f; e.ext2 = 0.f; e.arg = -1;
    } else {
      const uint32_t key = (uint32_t)(acc.best >> 32);
      e.ext = __uint_as_float(ln ? key : order_bits(~key));
      e.ext2 = __uint_as_float(acc.ext2);
      e.arg = (int32_t)(uint32_t)acc.best;
    }
    entries[T.slot[t]] = e;
  }
  if (t == 0) {
    Header h;
    h.pass = pass;
    h.step = d ? d->applied + d->skipped : -1;
    h.B = G.v[0]; h.Tx = G.v[1]; h.T0 = G.v[2]; h.H0 = G.v[3]; h.W0 = G.v[4];
    h.n_sites = T.n_sites;
    h.reserved[0] = h.reserved[1] = 0;
    *(Header*)row = h;
  }
  __syncthreads();
  if (t == 0) state[0] = pass + 1;
}

// the table's rules with their error codes; fills the kernels' copy when `out` is given
int sites_take(const svit_act_site* sites, const int32_t* slots, int64_t n_sites, int64_t n_slots, SiteTable* out,
               int64_t* total_windows) {
  if (!sites || !slots || n_sites < 1 || n_sites > kMaxSites || n_slots < 1 || n_slots > kMaxSlots) return SVIT_ERR_ARG;
  bool used[kMaxSlots] = {false};
  int64_t windows = 0;
  for (int64_t i = 0; i < n_sites; ++i) {
    const svit_act_site& s = sites[i];
    if (!s.a || s.rows < 1 || s.rows > kMaxRows) return SVIT_ERR_ARG;
    if (slots[i] < 0 || slots[i] >= n_slots || used[slots[i]]) return SVIT_ERR_ARG;
    used[slots[i]] = true;
    if (out) {
      out->s[i] = s;
      out->s[i].first_window = (int32_t)windows;
      out->slot[i] = slots[i];
    }
    windows += (s.rows + kWindow - 1) / kWindow;
  }
  for (int64_t i = 0; i < n_sites; ++i)
    if (((uintptr_t)sites[i].a | (uintptr_t)sites[i].b) & 3) return SVIT_ERR_ALIGN;
  if (out) {
    out->n_sites = (int32_t)n_sites;
    out->n_slots = (int32_t)n_slots;
    out->total_windows = (int32_t)windows;
    out->reserved = 0;
  }
  if (total_windows) *total_windows = windows;
  return SVIT_OK;
}
}  // namespace

extern "C" int svit_act_stats_window(void) { return kWindow; }

extern "C" int64_t svit_act_stats_workspace(int64_t total_windows) {
  if (total_windows < 1 || total_windows > (int64_t)kMaxSites * (kMaxRows / kWindow)) return SVIT_ERR_ARG;
  return total_windows * (int64_t)sizeof(Partial);
}

extern "C" int svit_act_sites_check(const svit_act_site* sites, const int32_t* slots, int64_t n_sites, int64_t n_slots,
                                    int64_t* total_windows) {
  return sites_take(sites, slots, n_sites, n_slots, nullptr, total_windows);
}

extern "C" int svit_act_stats(const svit_act_site* sites, const int32_t* slots, int64_t n_sites, int64_t n_slots,
                              const int32_t* geom, const svit_step_dev* dev_rec, void* ring, int64_t R, int64_t* state,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  SiteTable T;
  memset(&T, 0, sizeof(T));
  int64_t windows = 0;
  if (int rc = sites_take(sites, slots, n_sites, n_slots, &T, &windows)) return rc;
  if (!geom || !ring || !state || !workspace || R < 1) return SVIT_ERR_ARG;
  if (workspace_bytes < svit_act_stats_workspace(windows)) return SVIT_ERR_ARG;
  if (((uintptr_t)ring | (uintptr_t)workspace) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)state | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  Geom G;
  for (int i = 0; i < 5; ++i) G.v[i] = geom[i];
  hipLaunchKernelGGL(act_stats_windows, dim3((unsigned)windows), dim3(kThreads), 0, (hipStream_t)stream, T,
                     (Partial*)workspace);
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(act_stats_fold, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, T, G, dev_rec,
                     (const Partial*)workspace, (unsigned char*)ring, R, state);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
