// Per-head attention statistics of chosen query rows from the operands the forward already keeps (svit_attn_stats) --
// gfx950.
//
// A saving forward keeps qa, ka and lse2 of every block for its backward, and by svit_attn_fwd's operand convention
// qa . ka^T over columns [0, 96 + J) IS the score in the log2 domain, bias included: p[q, k] = exp2(qa[q] . ka[k] -
// lse2[q]).  Two launches recompute that for a few probe rows per (sample, head) -- the cls row, the object rows, K
// evenly spaced patch rows -- and leave entropy, peak and key-mass sums per (block, head, group) in a row of a ring in
// device memory (include/svit_hip.h: svit_attn_stats).  The yardstick is svit_amd/attnmon.py attn_host.
//
// The site table (at most 32 x 80 bytes) rides in the KERNEL ARGUMENTS, as svit_act_stats's does.
//
// Stage 1, attn_stats_rows: workgroup w belongs to ONE (site, sample, head, group), found by bisection over first_wg --
// blockIdx-derived, hence workgroup-uniform reads of the arguments.  With a step record whose step is not due it
// returns before any load of an operand.  Its 4 waves take the group's rows in turn (wave v rows v, v + 4, ...), four
// rows of a wave per pass over the keys, and the lanes of a wave the keys (lane l keys l, l + 64, ...).  64 keys at a
// time are staged in LDS by coalesced 16-byte loads (ka comes from L2: at most 522 KB per (sample, head), read once per
// 16 rows) in rows padded to an odd number of 16-byte units, so that the lanes' ds_read_b128 of their own key rows meet
// no bank conflict, and the next tile's loads are in flight while this one is worked on; a wave's four query rows sit in
// its own corner of LDS and come back as broadcast reads.  The products bf16 x bf16 are exact in fp32 and are accumulated in column order by one fma chain per (row, key).  A lane sums its keys in fp64 in key order, an xor butterfly
// folds the wave (every lane leaves with the same bits), the wave folds its rows in row order, thread 0 folds the waves
// in wave order and stores ONE 64-byte partial at slot w of the workspace, which no other workgroup shares.
// Stage 2, attn_stats_fold: ONE workgroup.  Thread e folds the partials of entry e in sample order into ring row
// (rows written % R); the entries no site owns get the empty entry; thread 0 writes the header and then the counters
// it alone read at entry (svit_meter_push's contract; stage 1 never reads them).
//
// No atomics, no ticket: a row is the same bit for bit from run to run and from the eager pass to a replay.
//
// The library is built with -ffast-math, so nothing here relies on a float comparison or on isfinite: a row is
// classified on the integer images of lse2 and of every s_k, extrema are taken on integer keys, and the columns past
// 96 + J are masked as INTEGERS on both operands before they become floats (0 x 0 adds an exact zero), so a NaN there
// never reaches an fma.
#include <cstring>

#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 4;                   // rows a wave carries through one pass over the keys
constexpr int kQStride = 160 / 8;           // 16-byte units of a query row in LDS
constexpr int kStage = 64 * (160 / 8) / kThreads;   // 16-byte units of a key tile per thread: 5
constexpr int kTileStride = 160 / 8 + 1;   // 16-byte units of a key row in LDS at DA = 160, padded by one
constexpr int kMaxSites = SVIT_ATTN_MAX_SITES;
constexpr int kMaxEnt = 1024;
constexpr int kMaxSlots = 1024;
constexpr int64_t kMaxWgs = 1 << 20;
constexpr uint64_t kNoBest = ~0ull;
constexpr int32_t kNone = 0x7fffffff;

struct Table {                              // the kernels' copy: first_wg filled in by the host wrapper
  svit_attn_site s[kMaxSites];
  svit_attn_probe p;
  int32_t n_sites, n_slots, ent_slots, total_wgs;
};

struct alignas(16) Partial {                // one (site, sample, head, group); an Entry's fields in wider types
  double sum_H, sum_pmax, sum_cls, sum_obj, sum_p;
  uint64_t min_H;                           // order_key(H) << 32 | row code, kNoBest when there is no good row
  uint32_t dev_bits;                        // largest |sum_p - 1| as its integer image
  int32_t rows, n_bad, first_bad;           // first_bad: row code, kNone when none
};
static_assert(sizeof(Partial) == 64, "a partial is 64 bytes");

struct alignas(8) Entry {                   // include/svit_hip.h: the ring's entry of one (slot, head, group)
  double sum_H, sum_pmax, sum_cls, sum_obj, sum_p;
  float min_H;
  int32_t min_row;
  float sum_dev;
  int32_t rows, n_bad, first_bad;
};
static_assert(sizeof(Entry) == SVIT_ATTN_ENTRY_BYTES, "a ring entry is 64 bytes");

struct Header {
  int64_t pass, step;
  int32_t B, Tx, T0, H0, W0, n_sites, row, reserved;
};
static_assert(sizeof(Header) == SVIT_ATTN_HEADER_BYTES, "the row header is 48 bytes");

struct Geom { int32_t v[5]; };

__host__ __device__ __forceinline__ int group_rows(int kind, int Lq, int n_obj, int K) {
  return kind == SVIT_ATTN_CLS ? 1 : kind == SVIT_ATTN_OBJ ? n_obj : (Lq <= K ? Lq : K);
}
__device__ __forceinline__ int group_row(int kind, int r, int Lq, int K) {
  if (kind == SVIT_ATTN_CLS) return 0;
  if (kind == SVIT_ATTN_OBJ) return 1 + Lq + r;
  return Lq <= K ? 1 + r : 1 + ((2 * r + 1) * Lq) / (2 * K);
}

__device__ __forceinline__ bool exp_all_ones(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }
// monotone in the float order of finite values; -0.0 sorts below +0.0
__device__ __forceinline__ uint32_t order_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t order_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

__device__ __forceinline__ double wave_sum(double x) {       // every lane leaves with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

// eight columns of one key: the two operands as their packed bf16 pairs; `valid` of them count (8 unless Masked)
template <bool Masked>
__device__ __forceinline__ float dot8(float acc, const uint4 q, const uint4 k, int valid) {
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w}, kw[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t q0 = qw[i] << 16, q1 = qw[i] & 0xffff0000u, k0 = kw[i] << 16, k1 = kw[i] & 0xffff0000u;
    if (Masked) {
      if (2 * i >= valid) q0 = k0 = 0u;
      if (2 * i + 1 >= valid) q1 = k1 = 0u;
    }
    acc = __builtin_fmaf(__uint_as_float(q0), __uint_as_float(k0), acc);
    acc = __builtin_fmaf(__uint_as_float(q1), __uint_as_float(k1), acc);
  }
  return acc;
}

// the units of key tile k0 this thread stages: unit u = threadIdx.x + j * 256 of the tile's (rows * per), rows past Nk
// never touched
__device__ __forceinline__ void load_tile(uint4 (&stage)[kStage], const uint16_t* __restrict__ ka, int k0, int Nk,
                                          int per) {
  const int units = (Nk - k0 < 64 ? Nk - k0 : 64) * per;
  const uint4* __restrict__ src = (const uint4*)ka + (int64_t)k0 * per;
#pragma unroll
  for (int j = 0; j < kStage; ++j) {
    const int u = (int)threadIdx.x + j * kThreads;
    stage[j] = u < units ? src[u] : uint4{0u, 0u, 0u, 0u};
  }
}

struct Acc {                                // a wave's, then the workgroup's, running partial
  double sum_H, sum_pmax, sum_cls, sum_obj, sum_p;
  uint64_t min_H;
  uint32_t dev_bits;
  int32_t rows, n_bad, first_bad;
};

__device__ __forceinline__ void acc_merge(Acc& a, const Partial& b) {
  a.sum_H += b.sum_H; a.sum_pmax += b.sum_pmax; a.sum_cls += b.sum_cls; a.sum_obj += b.sum_obj; a.sum_p += b.sum_p;
  a.min_H = b.min_H < a.min_H ? b.min_H : a.min_H;
  a.dev_bits = b.dev_bits > a.dev_bits ? b.dev_bits : a.dev_bits;
  a.rows += b.rows; a.n_bad += b.n_bad;
  a.first_bad = b.first_bad < a.first_bad ? b.first_bad : a.first_bad;
}
__device__ __forceinline__ Partial acc_partial(const Acc& a) {
  Partial p;
  p.sum_H = a.sum_H; p.sum_pmax = a.sum_pmax; p.sum_cls = a.sum_cls; p.sum_obj = a.sum_obj; p.sum_p = a.sum_p;
  p.min_H = a.min_H; p.dev_bits = a.dev_bits; p.rows = a.rows; p.n_bad = a.n_bad; p.first_bad = a.first_bad;
  return p;
}

__global__ __launch_bounds__(kThreads, 4) void attn_stats_rows(const Table T, const svit_step_dev* __restrict__ d,
                                                            Partial* __restrict__ part) {
  __shared__ Partial red[kWaves];
  __shared__ uint4 tile[64 * kTileStride];  // 64 keys of the (sample, head), every wave's operand
  __shared__ uint4 qs[kWaves * kRows * kQStride];   // the query rows a wave carries, read back as broadcasts
  // not due: nothing is loaded but the step record (workgroup-uniform, so every thread leaves)
  if (d && (d->applied + d->skipped) % (int64_t)T.p.every != 0) return;
  const int w = blockIdx.x;
  int lo = 0, hi = T.n_sites;               // the last site whose first_wg <= w
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (T.s[m].first_wg <= w) lo = m; else hi = m;
  }
  const int G = T.p.n_groups, K = T.p.K;
  const int heads = T.s[lo].heads, Nq = T.s[lo].Nq, Nk = T.s[lo].Nk, DA = T.s[lo].DA;
  const int Lq = T.s[lo].Lq, Lk = T.s[lo].Lk, n_obj = T.s[lo].n_obj;
  const int J = T.s[lo].bias_cols ? T.s[lo].bias_cols : DA - 96;
  const int C = 96 + J;                     // columns that count; C <= DA
  const int local = w - T.s[lo].first_wg;   // (sample * heads + head) * G + group
  const int g = local % G, bh = local / G;
  const int b = bh / heads;
  int kind = 0, nrows = 0, prow0 = 0, n_probe = 0;
  for (int i = 0; i < G; ++i) {
    const int cnt = group_rows(T.p.kind[i], Lq, n_obj, K);
    if (i == g) { kind = T.p.kind[i]; nrows = cnt; prow0 = n_probe; }
    n_probe += cnt;
  }
  const uint16_t* __restrict__ qa = (const uint16_t*)T.s[lo].qa + (int64_t)bh * Nq * DA;
  const uint16_t* __restrict__ ka = (const uint16_t*)T.s[lo].ka + (int64_t)bh * Nk * DA;
  const float* __restrict__ lse2 = T.s[lo].lse2 + (int64_t)bh * Nq;
  float* __restrict__ map = nullptr;
  if (T.s[lo].maps && b < T.p.maps_samples) map = T.s[lo].maps + ((int64_t)bh * n_probe + prow0) * Nk;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int full = C >> 3, tail = C & 7;    // whole 8-column chunks, columns of the last partial one

  const int per = DA >> 3;                  // 16-byte units of an operand row
  const int stride = per + 1;               // a key row in the tile, in 16-byte units: 17 or 21 -- odd, hence conflict-free

  Acc acc = {0.0, 0.0, 0.0, 0.0, 0.0, kNoBest, 0u, 0, 0, kNone};
  // kWaves * kRows rows per batch (wave v rows v, v + 4, ... as ever: a wave folds its rows in ascending order); every
  // wave walks every batch and every key tile, so the barriers are workgroup-uniform whatever rows it owns
  for (int r0 = 0; r0 < nrows; r0 += kWaves * kRows) {
    float lse[kRows];
    bool bad[kRows];
    double sp[kRows], sh[kRows], so[kRows], sc[kRows];
    uint32_t pm[kRows];
    int nmine = 0;                          // rows of this batch the wave owns: the first nmine of kRows
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const int r = r0 + wave + kWaves * i;
      if (r < nrows) nmine = i + 1;
      const int q = group_row(kind, r < nrows ? r : r0, Lq, K);  // < Nq by the checker's 1 + Lq + n_obj == Nq
      // the wave's own corner of LDS: written here, read below behind the tile loop's first barrier
      if (lane < per) qs[(wave * kRows + i) * kQStride + lane] = ((const uint4*)(qa + (int64_t)q * DA))[lane];
      const uint32_t lbits = __float_as_uint(lse2[q]);
      lse[i] = __uint_as_float(lbits);
      bad[i] = exp_all_ones(lbits);
      sp[i] = sh[i] = so[i] = sc[i] = 0.0;
      pm[i] = 0u;
    }
    // a tile is 64 * per <= 1280 16-byte units: at most kStage per thread, consecutive threads consecutive units of ka;
    // the NEXT tile's units are loaded into registers before this tile is worked on, so L2's latency hides behind it
    uint4 stage[kStage];
    load_tile(stage, ka, 0, Nk, per);
    for (int k0 = 0; k0 < Nk; k0 += 64) {
      __syncthreads();                      // the tile's readers are done
      const int units = (Nk - k0 < 64 ? Nk - k0 : 64) * per;
#pragma unroll
      for (int j = 0; j < kStage; ++j) {
        const int u = (int)threadIdx.x + j * kThreads;
        if (u < units) {
          const int row = u / per, col = u - row * per;
          tile[row * stride + col] = stage[j];
        }
      }
      __syncthreads();
      if (k0 + 64 < Nk) load_tile(stage, ka, k0 + 64, Nk, per);
      const int k = k0 + lane;
      if (k < Nk && nmine > 0) {
        const uint4* krow = tile + lane * stride;
        const uint4* qrow = qs + wave * kRows * kQStride;
        float s[kRows];
#pragma unroll
        for (int i = 0; i < kRows; ++i) s[i] = 0.f;
#pragma unroll 2
        for (int c = 0; c < full; ++c) {
          const uint4 kv = krow[c];
#pragma unroll
          for (int i = 0; i < kRows; ++i) s[i] = dot8<false>(s[i], qrow[i * kQStride + c], kv, 8);
        }
        if (tail) {
          const uint4 kv = krow[full];
#pragma unroll
          for (int i = 0; i < kRows; ++i) s[i] = dot8<true>(s[i], qrow[i * kQStride + full], kv, tail);
        }
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
          if (i < nmine) {
            bad[i] = bad[i] || exp_all_ones(__float_as_uint(s[i]));
            const float dk = s[i] - lse[i];
            const float p = __builtin_amdgcn_exp2f(dk);
            if (map) map[(int64_t)(r0 + wave + kWaves * i) * Nk + k] = p;
            const double pd = (double)p;
            sp[i] += pd;
            sh[i] = __builtin_fma(-pd, (double)dk, sh[i]);    // the product is exact in fp64 (24 x 24 bits)
            if (k > Lk) so[i] += pd;
            if (k == 0) sc[i] = pd;
            const uint32_t pb = __float_as_uint(p);           // p >= 0: the integer order is the float order
            pm[i] = pb > pm[i] ? pb : pm[i];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (i >= nmine) continue;             // wave-uniform
      const int q = group_row(kind, r0 + wave + kWaves * i, Lq, K);
      const int32_t code = b * Nq + q;
      acc.rows += 1;
      if (__any(bad[i]) != 0) {
        acc.n_bad += 1;
        acc.first_bad = code < acc.first_bad ? code : acc.first_bad;
      } else {
        const double wp = wave_sum(sp[i]), wh = wave_sum(sh[i]), wo = wave_sum(so[i]), wc = wave_sum(sc[i]);
        const uint32_t wm = wave_max(pm[i]);
        acc.sum_H += wh; acc.sum_pmax += (double)__uint_as_float(wm); acc.sum_cls += wc; acc.sum_obj += wo;
        acc.sum_p += wp;
        const uint64_t hk = ((uint64_t)order_key(__float_as_uint((float)wh)) << 32) | (uint32_t)code;
        acc.min_H = hk < acc.min_H ? hk : acc.min_H;
        const double dev = wp - 1.0;
        const uint32_t db = __float_as_uint((float)dev) & 0x7fffffffu;
        acc.dev_bits = db > acc.dev_bits ? db : acc.dev_bits;
      }
    }
  }
  __syncthreads();
  if (lane == 0) red[wave] = acc_partial(acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc t = {0.0, 0.0, 0.0, 0.0, 0.0, kNoBest, 0u, 0, 0, kNone};
#pragma unroll
    for (int v = 0; v < kWaves; ++v) acc_merge(t, red[v]);
    part[w] = acc_partial(t);
  }
}

__global__ __launch_bounds__(kThreads) void attn_stats_fold(const Table T, const Geom G,
                                                            const svit_step_dev* __restrict__ d,
                                                            const Partial* __restrict__ part,
                                                            unsigned char* __restrict__ ring, int64_t R,
                                                            int64_t* __restrict__ state) {
  __shared__ int64_t pass_s, rows_s;
  __shared__ int32_t owner[kMaxEnt];
  const int t = threadIdx.x;
  if (t == 0) { pass_s = state[0]; rows_s = state[1]; }
  for (int e = t; e < T.ent_slots; e += kThreads) owner[e] = -1;
  __syncthreads();
  const int Gn = T.p.n_groups;
  bool any_map = false;
  for (int s = 0; s < T.n_sites; ++s) {     // the checker made the ranges disjoint and inside [0, ent_slots)
    const int n = T.s[s].heads * Gn;
    for (int e = t; e < n; e += kThreads) owner[T.s[s].ent_base + e] = s;
    any_map = any_map || (T.s[s].maps != nullptr && T.p.maps_samples > 0);
  }
  __syncthreads();
  const int64_t pass = pass_s, rows_written = rows_s;
  const int64_t step = d ? d->applied + d->skipped : -1;
  const bool due = (d ? step : pass) % (int64_t)T.p.every == 0;
  if (due) {
    const int64_t rr = ((rows_written % R) + R) % R;
    unsigned char* row = ring + rr * (int64_t)(SVIT_ATTN_HEADER_BYTES + SVIT_ATTN_ENTRY_BYTES * (int64_t)T.ent_slots);
    Entry* entries = (Entry*)(row + SVIT_ATTN_HEADER_BYTES);
    for (int e = t; e < T.ent_slots; e += kThreads) {
      Entry out;
      const int s = owner[e];
      if (s < 0) {
        out.sum_H = out.sum_pmax = out.sum_cls = out.sum_obj = out.sum_p = 0.0;
        out.min_H = 0.f; out.min_row = -1; out.sum_dev = 0.f; out.rows = 0; out.n_bad = -1; out.first_bad = -1;
      } else {
        const int le = e - T.s[s].ent_base;                   // head * groups + group
        const int stride = T.s[s].heads * Gn;
        Acc acc = {0.0, 0.0, 0.0, 0.0, 0.0, kNoBest, 0u, 0, 0, kNone};
        for (int b = 0; b < T.s[s].B; ++b) acc_merge(acc, part[T.s[s].first_wg + b * stride + le]);
        out.sum_H = acc.sum_H; out.sum_pmax = acc.sum_pmax; out.sum_cls = acc.sum_cls; out.sum_obj = acc.sum_obj;
        out.sum_p = acc.sum_p;
        if (acc.min_H == kNoBest) {
          out.min_H = 0.f; out.min_row = -1;
        } else {
          out.min_H = __uint_as_float(order_bits((uint32_t)(acc.min_H >> 32)));
          out.min_row = (int32_t)(uint32_t)acc.min_H;
        }
        out.sum_dev = __uint_as_float(acc.dev_bits);
        out.rows = acc.rows; out.n_bad = acc.n_bad;
        out.first_bad = acc.first_bad == kNone ? -1 : acc.first_bad;
      }
      entries[e] = out;
    }
    if (t == 0) {
      Header h;
      h.pass = pass; h.step = step;
      h.B = G.v[0]; h.Tx = G.v[1]; h.T0 = G.v[2]; h.H0 = G.v[3]; h.W0 = G.v[4];
      h.n_sites = T.n_sites; h.row = (int32_t)rows_written; h.reserved = 0;
      *(Header*)row = h;
    }
  }
  __syncthreads();
  if (t == 0) {
    if (any_map && (due || !d)) state[2] = pass;              // (stage 1 stored its maps on this pass)
    if (due) state[1] = rows_written + 1;
    state[0] = pass + 1;
  }
}

// the table's rules with their error codes; fills the kernels' copy when `out` is given
int sites_take(const svit_attn_site* sites, int64_t n_sites, int64_t n_slots, int64_t ent_slots,
               const svit_attn_probe* probe, Table* out, int64_t* total_wgs) {
  if (!sites || !probe || n_sites < 1 || n_sites > kMaxSites || n_slots < 1 || n_slots > kMaxSlots || ent_slots < 1 ||
      ent_slots > kMaxEnt)
    return SVIT_ERR_ARG;
  if (probe->n_groups < 1 || probe->n_groups > 3 || probe->every < 1 || probe->maps_samples < 0) return SVIT_ERR_ARG;
  bool seen[3] = {false, false, false};
  for (int i = 0; i < probe->n_groups; ++i) {
    const int k = probe->kind[i];
    if (k < 0 || k > 2 || seen[k]) return SVIT_ERR_ARG;
    seen[k] = true;
    if (k == SVIT_ATTN_PATCH && (probe->K < 1 || probe->K > 256)) return SVIT_ERR_ARG;
  }
  bool used[kMaxSlots] = {false};
  bool owned[kMaxEnt] = {false};
  int64_t wgs = 0;
  for (int64_t i = 0; i < n_sites; ++i) {
    const svit_attn_site& s = sites[i];
    if (!s.qa || !s.ka || !s.lse2) return SVIT_ERR_ARG;
    if (s.B < 1 || s.heads < 1 || s.Lq < 1 || s.Lk < 1 || s.n_obj < 0) return SVIT_ERR_ARG;
    if (s.DA != 128 && s.DA != 160) return SVIT_ERR_ARG;
    if (s.bias_cols < 0 || s.bias_cols > s.DA - 96) return SVIT_ERR_ARG;
    if ((int64_t)1 + s.Lq + s.n_obj != s.Nq || (int64_t)1 + s.Lk + s.n_obj != s.Nk) return SVIT_ERR_ARG;
    const int64_t n = s.Nq > s.Nk ? s.Nq : s.Nk;
    if ((int64_t)s.B * s.heads * n > 0x7fffffffll) return SVIT_ERR_ARG;
    if (s.slot < 0 || s.slot >= n_slots || used[s.slot]) return SVIT_ERR_ARG;
    used[s.slot] = true;
    const int64_t ne = (int64_t)s.heads * probe->n_groups;
    if (s.ent_base < 0 || s.ent_base + ne > ent_slots) return SVIT_ERR_ARG;
    for (int64_t e = s.ent_base; e < s.ent_base + ne; ++e) {
      if (owned[e]) return SVIT_ERR_ARG;
      owned[e] = true;
    }
    wgs += (int64_t)s.B * ne;
    if (wgs > kMaxWgs) return SVIT_ERR_ARG;
  }
  if (out) {
    // the kernels' copy in order of falling work per workgroup (keys x columns), ties in table order: the dispatcher
    // starts workgroups roughly in index order, and the long ones should not be the last to start
    int order[kMaxSites];
    for (int i = 0; i < (int)n_sites; ++i) {
      int j = i;
      const int64_t wi = (int64_t)sites[i].Nk * sites[i].DA;
      for (; j > 0 && (int64_t)sites[order[j - 1]].Nk * sites[order[j - 1]].DA < wi; --j) order[j] = order[j - 1];
      order[j] = i;
    }
    int64_t first = 0;
    for (int i = 0; i < (int)n_sites; ++i) {
      out->s[i] = sites[order[i]];
      out->s[i].first_wg = (int32_t)first;
      first += (int64_t)out->s[i].B * out->s[i].heads * probe->n_groups;
    }
  }
  for (int64_t i = 0; i < n_sites; ++i) {
    if (((uintptr_t)sites[i].qa | (uintptr_t)sites[i].ka) & 15) return SVIT_ERR_ALIGN;
    if (((uintptr_t)sites[i].lse2 | (uintptr_t)sites[i].maps) & 3) return SVIT_ERR_ALIGN;
  }
  if (out) {
    out->p = *probe;
    out->n_sites = (int32_t)n_sites;
    out->n_slots = (int32_t)n_slots;
    out->ent_slots = (int32_t)ent_slots;
    out->total_wgs = (int32_t)wgs;
  }
  if (total_wgs) *total_wgs = wgs;
  return SVIT_OK;
}
}  // namespace

extern "C" int64_t svit_attn_stats_workspace(int64_t total_wgs) {
  if (total_wgs < 1 || total_wgs > kMaxWgs) return SVIT_ERR_ARG;
  return total_wgs * (int64_t)sizeof(Partial);
}

extern "C" int svit_attn_sites_check(const svit_attn_site* sites, int64_t n_sites, int64_t n_slots, int64_t ent_slots,
                                     const svit_attn_probe* probe, int64_t* total_wgs) {
  return sites_take(sites, n_sites, n_slots, ent_slots, probe, nullptr, total_wgs);
}

extern "C" int svit_attn_stats(const svit_attn_site* sites, int64_t n_sites, int64_t n_slots, int64_t ent_slots,
                               const svit_attn_probe* probe, const int32_t* geom, const svit_step_dev* dev_rec,
                               void* ring, int64_t R, int64_t* state, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  Table T;
  memset(&T, 0, sizeof(T));
  int64_t wgs = 0;
  if (int rc = sites_take(sites, n_sites, n_slots, ent_slots, probe, &T, &wgs)) return rc;
  if (!geom || !ring || !state || !workspace || R < 1) return SVIT_ERR_ARG;
  if (workspace_bytes < svit_attn_stats_workspace(wgs)) return SVIT_ERR_ARG;
  if (((uintptr_t)ring | (uintptr_t)workspace) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)state | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  Geom G;
  for (int i = 0; i < 5; ++i) G.v[i] = geom[i];
  hipLaunchKernelGGL(attn_stats_rows, dim3((unsigned)wgs), dim3(kThreads), 0, (hipStream_t)stream, T, dev_rec,
                     (Partial*)workspace);
  SVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_stats_fold, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, T, G, dev_rec,
                     (const Partial*)workspace, (unsigned char*)ring, R, state);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
