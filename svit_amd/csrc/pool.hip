// Pooled q/k/v path of MultiScaleAttention (SURVEY.md K5/K6/K3, K9/K10 query side) -- gfx950.
//
// The reference reshapes to channels-first [B*h,96,T,H,W], runs a depthwise Conv3d and
// permutes back (two full copies, attention.py:35-43).  Here everything stays token-major /
// channels-last: 4 lanes own one output token (24 channels each, 16-byte bf16 vector loads),
// the 27-tap stencil reads the qkv GEMM output in place, the object-token branch is the closed
// form obj*g(w), and LayerNorm(96) is fused (4-lane shuffle reduce).
#include <algorithm>
#include <mutex>
#include <vector>
#include <cmath>
#include <cstddef>
#include <cstring>
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int HD = 96;

__device__ __forceinline__ int pooled(int n, int s) { return (n - 1) / s + 1; }

// n / d for n < 65536 by one multiply-high with m = ceil(2^32 / d) (exact while n * d < 2^32)
// (d = 1: ceil(2^32 / 1) does not fit 32 bits and wraps to 0 -- fdiv takes m = 0 as "divide by one".  Round 3's y-chunked
// slab planes divided by the rows of a chunk, which is 1 for a ragged last chunk: every output of that chunk landed in
// its first t-plane -- the "wrong rows at stride 2" of DESIGN.md section 5c)
__device__ __forceinline__ int fdiv(int n, unsigned m) { return m ? (int)__umulhi((unsigned)n, m) : n; }
__device__ __forceinline__ unsigned fdiv_magic_dev(int d) { return 0xFFFFFFFFu / (unsigned)d + 1u; }   // = ceil(2^32 / d); 0 for d = 1

// per-axis tap counts of the object branch: how many output positions of a zero-padded 3-cube
// see tap i in range, and the number of output positions (attention.py:45-53)
__device__ __forceinline__ void obj_counts(int s, float n[3], float* inv_p) {
  const int n_out = (3 - 1) / s + 1;
  n[0] = n[1] = n[2] = 0.f;
  for (int o = 0; o < n_out; ++o)
    for (int tap = 0; tap < 3; ++tap) {
      const int i = o * s - 1 + tap;
      if (i >= 0 && i < 3) n[tap] += 1.f;
    }
  *inv_p = 1.f / (float)n_out;
}

__device__ __forceinline__ void unpack8(const uint4 v, float f[8]) {
  f[0] = lo_bf16(v.x); f[1] = hi_bf16(v.x); f[2] = lo_bf16(v.y); f[3] = hi_bf16(v.y);
  f[4] = lo_bf16(v.z); f[5] = hi_bf16(v.z); f[6] = lo_bf16(v.w); f[7] = hi_bf16(v.w);
}
__device__ __forceinline__ uint4 pack8(const float f[8]) {
  uint4 o;
  o.x = pack_bf16x2(f[0], f[1]); o.y = pack_bf16x2(f[2], f[3]);
  o.z = pack_bf16x2(f[4], f[5]); o.w = pack_bf16x2(f[6], f[7]);
  return o;
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// LDS image of the conv weights, tap-major so one lane reads its 24 channels contiguously.
// Entries are "selector weights": bf16(w) sits in the half of a dword that matches the channel's
// position inside a packed bf16 pair (even channel: low half, odd: high half, other half zero),
// so  acc = v_dot2c_f32_bf16(packed_pair, entry, acc)  multiplies exactly that channel -- no
// bf16->f32 unpacking in the stencil loops (it cost twice as many VALU ops as the FMAs).  The
// weights are thereby rounded to bf16, as CUDA autocast does for the reference's Conv3d.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ float dot2_sel(uint32_t pair, uint32_t sel, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, pair),
                                         __builtin_bit_cast(bf16x2_t, sel), acc, false);
}
// acc[8u .. 8u+7] += v (8 packed bf16 channels) * the selector weights at w
__device__ __forceinline__ void fma8_sel(float (&acc)[24], int u, const uint4 v, const float* w) {
  const uint4 w0 = *(const uint4*)(w + u * 8), w1 = *(const uint4*)(w + u * 8 + 4);
  acc[u * 8 + 0] = dot2_sel(v.x, w0.x, acc[u * 8 + 0]);
  acc[u * 8 + 1] = dot2_sel(v.x, w0.y, acc[u * 8 + 1]);
  acc[u * 8 + 2] = dot2_sel(v.y, w0.z, acc[u * 8 + 2]);
  acc[u * 8 + 3] = dot2_sel(v.y, w0.w, acc[u * 8 + 3]);
  acc[u * 8 + 4] = dot2_sel(v.z, w1.x, acc[u * 8 + 4]);
  acc[u * 8 + 5] = dot2_sel(v.z, w1.y, acc[u * 8 + 5]);
  acc[u * 8 + 6] = dot2_sel(v.w, w1.z, acc[u * 8 + 6]);
  acc[u * 8 + 7] = dot2_sel(v.w, w1.w, acc[u * 8 + 7]);
}
__device__ __forceinline__ void load_weights(const float* __restrict__ conv_w, float* w_lds,
                                             float* g_lds, int stride_hw) {
  for (int i = threadIdx.x; i < 27 * HD; i += blockDim.x) {
    const int c = i / 27, tap = i % 27;
    w_lds[tap * HD + c] = __uint_as_float((uint32_t)f32_to_bf16(conv_w[i]) << (16 * (c & 1)));
  }
  if (g_lds) {
    float nt[3], nh[3], ipt, iph;
    obj_counts(1, nt, &ipt);
    obj_counts(stride_hw, nh, &iph);
    for (int c = threadIdx.x; c < HD; c += blockDim.x) {
      float g = 0.f;
      for (int kt = 0; kt < 3; ++kt)
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx)
            g += conv_w[c * 27 + (kt * 3 + ky) * 3 + kx] * nt[kt] * nh[ky] * nh[kx];
      g_lds[c] = g * ipt * iph * iph;
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------
// LayerNorm(96) over the 4 lanes of a token + stores: out (LN result, + one-hot key
// coordinates in mode 1), pre (bf16 pre-LN value, saved for backward), mean / rstd.  All 256
// threads of the workgroup call it (the quad shuffles need the whole quad).
__device__ __forceinline__ void pool_ln_finish(const svit_pool_args& a, float (&acc)[24], bool live,
                                               int tok, bool is_patch, int py, int px, int pt,
                                               int bh, int Nout, int Ho, int Wo, bf16_t* lds_row = nullptr) {
  const int sub = threadIdx.x & 3, c0 = sub * 24;
  // the saved pre-LN value is the bf16-rounded one: normalise exactly what backward will see
#pragma unroll
  for (int i = 0; i < 24; ++i) acc[i] = bf16_to_f32(f32_to_bf16(acc[i]));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 24; ++i) sum += acc[i];
  const float mean = quad_sum(sum) * (1.f / HD);
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 24; ++i) sq += (acc[i] - mean) * (acc[i] - mean);
  const float rstd = rsqrtf(quad_sum(sq) * (1.f / HD) + a.eps);
  if (!live) return;
  const size_t orow = (size_t)bh * Nout + tok;
  if (sub == 0 && a.mean) { a.mean[orow] = mean; a.rstd[orow] = rstd; }
  bf16_t* outp = (bf16_t*)a.out + orow * a.ld_out + c0;
  bf16_t* prep = a.pre ? (bf16_t*)a.pre + orow * HD + c0 : nullptr;   // NULL: nothing saved
  const float osc = a.out_scale != 0.f ? a.out_scale : 1.f;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = ((acc[v * 8 + e] - mean) * rstd * a.gamma[c0 + v * 8 + e] + a.beta[c0 + v * 8 + e]) * osc;
    const uint4 pk = pack8(o);
    *(uint4*)(outp + v * 8) = pk;
    if (lds_row) *(uint4*)(lds_row + c0 + v * 8) = pk;     // (the slab kernel's rel-pos product reads it back)
    if (prep) *(uint4*)(prep + v * 8) = pack8(&acc[v * 8]);
  }
  if (a.mode == 1) {  // one-hot key coordinates [y | kh+x | kh+kw+t], zeros elsewhere
    const int extra = a.ld_out - HD, per = extra / 4;
    bf16_t* ex = (bf16_t*)a.out + orow * a.ld_out + HD + sub * per;
    for (int v = 0; v < per; v += 8) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = sub * per + v + e;
        o[e] = (is_patch && (j == py || j == Ho + px || j == Ho + Wo + pt)) ? 1.f : 0.f;
      }
      *(uint4*)(ex + v) = pack8(o);
    }
  }
}


__device__ __forceinline__ void pool_ln_fwd_body(const svit_pool_args& a, const float* w_lds,
                                                 const float* g_lds, int tb) {
  const int s = a.stride_hw;
  const int Ho = pooled(a.H, s), Wo = pooled(a.W, s);
  const int L = a.T * a.H * a.W, Lo = a.T * Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int bh = blockIdx.y, b = bh / a.heads, head = bh % a.heads;
  const int tok = tb * 64 + (threadIdx.x >> 2);
  const int sub = threadIdx.x & 3, c0 = sub * 24;
  const bool live = tok < Nout;
  const bf16_t* qkv = (const bf16_t*)a.qkv;
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const bf16_t* base = qkv + (size_t)b * N * tok_stride + ((size_t)a.which * a.heads + head) * HD + c0;

  float acc[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) acc[i] = 0.f;
  int py = 0, px = 0, pt = 0;
  bool is_patch = false;
  if (live) {
    if (tok == 0 || tok > Lo) {
      const int src = (tok == 0) ? 0 : (1 + L + (tok - 1 - Lo));
      const bf16_t* p = base + (size_t)src * tok_stride;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        float f[8];
        unpack8(*(const uint4*)(p + v * 8), f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          acc[v * 8 + e] = (tok == 0) ? f[e] : f[e] * g_lds[c0 + v * 8 + e];
      }
    } else {
      is_patch = true;
      const int p = tok - 1;
      px = p % Wo; py = (p / Wo) % Ho; pt = p / (Wo * Ho);
    }
  }
  // 27-tap stencil, one t-plane (9 taps x 48 B per lane) per round: every load of a round is
  // issued before the first FMA consumes one (out-of-volume taps read token 0 and are skipped),
  // so a lane pays 3 memory round trips instead of 27.
  if (__any(is_patch)) {
#pragma unroll 1
    for (int kt = 0; kt < 3; ++kt) {
      const int t = pt - 1 + kt;
      const bool tv = is_patch && t >= 0 && t < a.T;
      if (!__any(tv)) continue;        // whole wave outside the volume (T' = 1; clip borders)
      uint4 v[9][3];
      bool ok[9];
#pragma unroll
      for (int k9 = 0; k9 < 9; ++k9) {
        const int y = py * s - 1 + k9 / 3, x = px * s - 1 + k9 % 3;
        ok[k9] = tv && y >= 0 && y < a.H && x >= 0 && x < a.W;
        const int ti = ok[k9] ? 1 + (t * a.H + y) * a.W + x : 0;
        const bf16_t* src = base + (size_t)ti * tok_stride;
#pragma unroll
        for (int u = 0; u < 3; ++u) v[k9][u] = *(const uint4*)(src + u * 8);
      }
#pragma unroll
      for (int k9 = 0; k9 < 9; ++k9) {
        if (!ok[k9]) continue;
        const float* w = w_lds + (kt * 9 + k9) * HD + c0;
#pragma unroll
        for (int u = 0; u < 3; ++u) fma8_sel(acc, u, v[k9][u], w);
      }
    }
  }
  pool_ln_finish(a, acc, live, tok, is_patch, py, px, pt, bh, Nout, Ho, Wo);
}


// ---------------------------------------------------------------------------------------
// Stride-1 depthwise 3x3x3 stencil, LDS-tiled (round 2).  The streaming kernels above fetch every
// tap from global memory: 81 sixteen-byte loads per lane and token, each input element 27 times
// through the texture path (rocprofv3 round 1: 3.2x the algorithmic read traffic, 0.21 of the HBM
// roofline).  Here a workgroup owns a TY x TX patch of output positions of one (batch, head,
// tensor) and walks t: the halo of three consecutive input planes lives in an LDS ring (one new
// plane per step, fetched ONCE with coalesced 16-byte loads while the previous plane is being
// computed), so global memory sees each element ~1.7 times and the 27 taps are LDS reads.
//   * Wave w owns the channels [24w, 24w+24) of every token of the patch, lane = token.  The
//     weights of a wave are therefore wave-uniform: the forward takes them as scalar operands
//     (SW = true: s_load from the "selector" tables of svit_pool_weight_sel, one (kt, ky) row of
//     72 dwords at a time, like the slab kernel further down); the dgrad reads them from an LDS
//     image it builds from conv_w (two thirds of its LDS reads; as scalars it measured no faster).
//   * Token rows are 208 bytes apart in LDS (13 sixteen-byte slots, odd): the 16 lanes of a
//     ds_read_b128 group are 16 consecutive tokens and hit 16 distinct slots of the bank row.
//   * LayerNorm(96) spans the four waves: two tiny exchanges (sum, then squared deviations)
//     through LDS per plane.
//   (forward only since round 5: the dgrad form of this body -- flipped kernel, dqkv rows instead of LayerNorm -- went
//    with the fused conv backward further down)
constexpr int TL_ROW = 208;       // LDS bytes per token row (192 + 16 pad)

struct PoolTilePlan {
  int tiled;          // 1: this tensor runs the tiled body
  int tiles_x, tiles_y, tch, tlen, n_wgs, n_special;
};

// ds_read_b128 serves a wave in four groups of 16 lanes that are NOT consecutive lanes
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32: MI355X guide, LDS table).  Position of a lane in
// that order: the lanes of one group then own 16 consecutive tokens of the patch, whose rows
// (13 slots apart) fall on 16 distinct 16-byte slots of the bank row -- conflict-free reads.
__device__ __forceinline__ int b128_group_order(int lane) {
  const int l = lane & 31;
  int g, k;
  if (l < 4) { g = 0; k = l; }
  else if (l < 12) { g = 1; k = l - 4; }
  else if (l < 16) { g = 0; k = l - 8; }
  else if (l < 20) { g = 1; k = l - 8; }
  else if (l < 28) { g = 0; k = l - 12; }
  else { g = 1; k = l - 16; }
  return (lane & 32) + g * 16 + k;
}

template <int TX, int TY, bool SW>
__device__ __forceinline__ void pool_tiled_body(
    const bf16_t* __restrict__ in_base, size_t in_tok_stride /* elements */, int in_first /* token index of patch 0 */,
    const float* __restrict__ w_lds /* [27][96] selector dwords in LDS (!SW) */,
    const uint32_t* __restrict__ sel /* the same table in global memory (SW: read as scalar operands) */,
    int T, int H, int W, int wg,
    const PoolTilePlan& pl, unsigned char* ring, float* xch /* [2][4][64] */,
    const svit_pool_args* fa, int bh) {
  constexpr int HX = TX + 2, HY = TY + 2, HTOK = HX * HY, PLANE_B = HTOK * TL_ROW;
  constexpr int CH = HTOK * 12, PER = (CH + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tc = wg % pl.tch, txi = (wg / pl.tch) % pl.tiles_x, tyi = wg / (pl.tch * pl.tiles_x);
  const int y0 = tyi * TY, x0 = txi * TX;
  const int t0 = tc * pl.tlen, t1 = min(T, t0 + pl.tlen);
  uint4 sreg[PER];
  auto fetch = [&](int tp) {        // global -> registers (zero outside the volume)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int q = tid + u * 256;
      const int tok = q / 12, cc = q % 12, hy = tok / HX, hx = tok % HX;
      const int y = y0 - 1 + hy, x = x0 - 1 + hx;
      sreg[u] = make_uint4(0, 0, 0, 0);
      if (q < CH && tp >= 0 && tp < T && y >= 0 && y < H && x >= 0 && x < W)
        sreg[u] = *(const uint4*)(in_base + (size_t)(in_first + (tp * H + y) * W + x) * in_tok_stride + cc * 8);
    }
  };
  auto store = [&](int tp) {        // registers -> ring slot (tp + 1) % 3
    unsigned char* dst = ring + ((tp + 1) % 3) * PLANE_B;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int q = tid + u * 256;
      if (q < CH) *(uint4*)(dst + (q / 12) * TL_ROW + (q % 12) * 16) = sreg[u];
    }
  };
  // lane -> output position of the patch (lanes past TX*TY idle on position 0)
  const int vl = b128_group_order(lane);
  const int lt = vl < TX * TY ? vl : 0;
  const int ty = lt / TX, tx = lt % TX;
  const bool live = vl < TX * TY && y0 + ty < H && x0 + tx < W;
  const unsigned ldsoff = (unsigned)((ty * HX + tx) * TL_ROW + wave * 48);
  const float* wsel = w_lds + wave * 24;            // this wave's 24 channels of every tap

  __syncthreads();                 // the ring is free (previous work item of this workgroup)
  fetch(t0 - 1); store(t0 - 1);
  fetch(t0);     store(t0);
  fetch(t0 + 1);
  for (int t = t0; t < t1; ++t) {
    store(t + 1);
    __syncthreads();
    if (t + 1 < t1) fetch(t + 2);  // travels while this plane is computed
    float acc[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0.f;
    // one t-plane (9 taps, 27 LDS reads in flight) at a time: fully unrolled the scheduler hoists
    // all 81 reads and spills
    if constexpr (SW) {
      // weights as scalar operands (uniform constant-address loads -> s_load): the LDS pipe then serves the
      // 81 data reads of a plane only, not 162 broadcast weight reads on top; one (kt, ky) row = 72 SGPRs at a time
      typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
      const cptr_t selw = (cptr_t)(sel + wave * 24);
#pragma unroll 1
      for (int kt = 0; kt < 3; ++kt) {
        const unsigned char* pl_base = ring + ((t + kt) % 3) * PLANE_B + ldsoff;
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
          const int tap0 = (kt * 3 + ky) * 3;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const cptr_t w = selw + (tap0 + kx) * HD;
            const unsigned char* p = pl_base + (ky * HX + kx) * TL_ROW;
            const uint4 v0 = *(const uint4*)(p), v1 = *(const uint4*)(p + 16), v2 = *(const uint4*)(p + 32);
            acc[0] = dot2_sel(v0.x, w[0], acc[0]);   acc[1] = dot2_sel(v0.x, w[1], acc[1]);
            acc[2] = dot2_sel(v0.y, w[2], acc[2]);   acc[3] = dot2_sel(v0.y, w[3], acc[3]);
            acc[4] = dot2_sel(v0.z, w[4], acc[4]);   acc[5] = dot2_sel(v0.z, w[5], acc[5]);
            acc[6] = dot2_sel(v0.w, w[6], acc[6]);   acc[7] = dot2_sel(v0.w, w[7], acc[7]);
            acc[8] = dot2_sel(v1.x, w[8], acc[8]);   acc[9] = dot2_sel(v1.x, w[9], acc[9]);
            acc[10] = dot2_sel(v1.y, w[10], acc[10]); acc[11] = dot2_sel(v1.y, w[11], acc[11]);
            acc[12] = dot2_sel(v1.z, w[12], acc[12]); acc[13] = dot2_sel(v1.z, w[13], acc[13]);
            acc[14] = dot2_sel(v1.w, w[14], acc[14]); acc[15] = dot2_sel(v1.w, w[15], acc[15]);
            acc[16] = dot2_sel(v2.x, w[16], acc[16]); acc[17] = dot2_sel(v2.x, w[17], acc[17]);
            acc[18] = dot2_sel(v2.y, w[18], acc[18]); acc[19] = dot2_sel(v2.y, w[19], acc[19]);
            acc[20] = dot2_sel(v2.z, w[20], acc[20]); acc[21] = dot2_sel(v2.z, w[21], acc[21]);
            acc[22] = dot2_sel(v2.w, w[22], acc[22]); acc[23] = dot2_sel(v2.w, w[23], acc[23]);
          }
        }
      }
    } else {
#pragma unroll 1
    for (int kt = 0; kt < 3; ++kt) {
      const unsigned char* pl_base = ring + ((t + kt) % 3) * PLANE_B + ldsoff;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int tap = (kt * 3 + ky) * 3 + kx;
          const float* wt = wsel + tap * HD;   // wave-uniform: broadcast LDS reads
          const unsigned char* p = pl_base + (ky * HX + kx) * TL_ROW;
#pragma unroll
          for (int u = 0; u < 3; ++u) fma8_sel(acc, u, *(const uint4*)(p + u * 16), wt);
        }
    }
    }
    const int y = y0 + ty, x = x0 + tx;
    {
      // LayerNorm over the 96 channels of the token = over the four waves
#pragma unroll
      for (int i = 0; i < 24; ++i) acc[i] = bf16_to_f32(f32_to_bf16(acc[i]));   // what backward sees
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 24; ++i) sum += acc[i];
      xch[wave * 64 + lane] = sum;          // (indexed by lane: every wave uses the same lane -> token map)
      __syncthreads();
      const float mean = ((xch[lane] + xch[64 + lane]) + (xch[128 + lane] + xch[192 + lane])) * (1.f / HD);
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < 24; ++i) sq += (acc[i] - mean) * (acc[i] - mean);
      xch[256 + wave * 64 + lane] = sq;
      __syncthreads();
      const float var = ((xch[256 + lane] + xch[320 + lane]) + (xch[384 + lane] + xch[448 + lane])) * (1.f / HD);
      const float rstd = rsqrtf(var + fa->eps);
      if (live) {
        const int Lo = T * H * W, Nout = 1 + Lo + fa->n_obj;
        const int tok = 1 + (t * H + y) * W + x, c0 = wave * 24;
        const size_t orow = (size_t)bh * Nout + tok;
        if (wave == 0 && fa->mean) { fa->mean[orow] = mean; fa->rstd[orow] = rstd; }
        bf16_t* outp = (bf16_t*)fa->out + orow * fa->ld_out + c0;
        bf16_t* prep = fa->pre ? (bf16_t*)fa->pre + orow * HD + c0 : nullptr;
        const float osc = fa->out_scale != 0.f ? fa->out_scale : 1.f;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          float o8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            o8[e] = ((acc[v * 8 + e] - mean) * rstd * fa->gamma[c0 + v * 8 + e] + fa->beta[c0 + v * 8 + e]) * osc;
          *(uint4*)(outp + v * 8) = pack8(o8);
          if (prep) *(uint4*)(prep + v * 8) = pack8(&acc[v * 8]);
        }
        if (fa->mode == 1) {   // one-hot key coordinates [y | kh+x | kh+kw+t], zeros elsewhere
          const int extra = fa->ld_out - HD, per = extra / 4;
          bf16_t* ex = (bf16_t*)fa->out + orow * fa->ld_out + HD + wave * per;
          for (int v = 0; v < per; v += 8) {
            float o8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int j = wave * per + v + e;
              o8[e] = (j == y || j == H + x || j == H + W + t) ? 1.f : 0.f;
            }
            *(uint4*)(ex + v) = pack8(o8);
          }
        }
      }
    }
    __syncthreads();               // ring slot of plane t-1 (and xch) are overwritten next step
  }
}

// cls and object tokens of a tiled forward tensor: out = LN(x) / LN(x * g(w)) (the closed form of
// the cube branch).  Token list = [0, Lo+1 .. Lo+n_obj], 64 per workgroup.
__device__ __forceinline__ void pool_ln_special_body(const svit_pool_args& a, const float* g_lds, int blk) {
  const int L = a.T * a.H * a.W, Lo = L;          // stride 1: Lo == L
  const int N = 1 + L + a.n_obj, Nout = N;
  const int bh = blockIdx.y, b = bh / a.heads, head = bh % a.heads;
  const int idx = blk * 64 + (threadIdx.x >> 2);
  const int sub = threadIdx.x & 3, c0 = sub * 24;
  const bool live = idx <= a.n_obj;
  const int tok = idx == 0 ? 0 : Lo + idx;
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const bf16_t* base = (const bf16_t*)a.qkv + (size_t)b * N * tok_stride + ((size_t)a.which * a.heads + head) * HD + c0;
  float acc[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) acc[i] = 0.f;
  if (live) {
    const bf16_t* p = base + (size_t)tok * tok_stride;       // tok == source index at stride 1
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      float f[8];
      unpack8(*(const uint4*)(p + v * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[v * 8 + e] = (tok == 0) ? f[e] : f[e] * g_lds[c0 + v * 8 + e];
    }
  }
  pool_ln_finish(a, acc, live, tok, false, 0, 0, 0, bh, Nout, a.H, a.W);
}

// Workgroups are persistent over token blocks (blockIdx.x strides by gridDim.x): the conv weights
// go to LDS once per workgroup instead of once per 64 tokens.
__global__ __launch_bounds__(256) void pool_ln_fwd_kernel(svit_pool_args a) {
  __shared__ __attribute__((aligned(16))) float w_lds[27 * HD];
  __shared__ __attribute__((aligned(16))) float g_lds[HD];
  load_weights(a.conv_w, w_lds, g_lds, a.stride_hw);
  const int Nout = 1 + a.T * pooled(a.H, a.stride_hw) * pooled(a.W, a.stride_hw) + a.n_obj;
  for (int tb = blockIdx.x; tb * 64 < Nout; tb += gridDim.x) pool_ln_fwd_body(a, w_lds, g_lds, tb);
}

// q, k and v of one block in one launch (blockIdx.z = which): the three stencils differ only in
// stride, and at the 14x14 / 7x7 stages each of them is a few-microsecond latency chain, so
// running them side by side costs the time of the longest one.
struct PoolFwd3 { svit_pool_args p[3]; PoolTilePlan plan[3]; const uint32_t* sel[3]; int skip[3]; };
__global__ __launch_bounds__(256) void pool_ln_fwd3_kernel(PoolFwd3 g) {
  __shared__ __attribute__((aligned(16))) float w_lds[27 * HD];   // streaming body: selector weights
  __shared__ __attribute__((aligned(16))) float g_lds[HD];
  extern __shared__ __attribute__((aligned(16))) unsigned char pool_dyn[];   // tiled body: ring + exchange
  if (g.skip[blockIdx.z]) return;               // this tensor went through the slab kernels
  const svit_pool_args& a = g.p[blockIdx.z];
  const PoolTilePlan& pl = g.plan[blockIdx.z];
  if (pl.tiled) {
    const int wg = blockIdx.x;
    if (wg >= pl.n_wgs + pl.n_special) return;
    if (wg >= pl.n_wgs) {                       // cls / object tokens
      load_weights(a.conv_w, w_lds, g_lds, a.stride_hw);
      pool_ln_special_body(a, g_lds, wg - pl.n_wgs);
      return;
    }
    const int bh = blockIdx.y, b = bh / a.heads, head = bh % a.heads;
    const int N = 1 + a.T * a.H * a.W + a.n_obj;
    const size_t ts = (size_t)3 * a.heads * HD;
    const bf16_t* base = (const bf16_t*)a.qkv + (size_t)b * N * ts + ((size_t)a.which * a.heads + head) * HD;
    float* xch = (float*)pool_dyn;
    unsigned char* ring = pool_dyn + 512 * sizeof(float);
    const uint32_t* sel = g.sel[blockIdx.z];      // scalar weights: nothing to stage in LDS
    if (a.W > 8)
      pool_tiled_body<16, 4, true>(base, ts, 1, w_lds, sel, a.T, a.H, a.W, wg, pl, ring, xch, &a, bh);
    else
      pool_tiled_body<8, 8, true>(base, ts, 1, w_lds, sel, a.T, a.H, a.W, wg, pl, ring, xch, &a, bh);
    return;
  }
  const int Nout = 1 + a.T * pooled(a.H, a.stride_hw) * pooled(a.W, a.stride_hw) + a.n_obj;
  if ((int)blockIdx.x * 64 >= Nout) return;
  load_weights(a.conv_w, w_lds, g_lds, a.stride_hw);
  for (int tb = blockIdx.x; tb * 64 < Nout; tb += gridDim.x) pool_ln_fwd_body(a, w_lds, g_lds, tb);
}

// selector table of a depthwise weight: dst[tap][c] = bf16(w[c][tap]) in the half of the dword that
// matches c's position in a packed bf16 pair (see dot2_sel) -- the scalar operand of the tiled
// stencils.  One launch converts a list of [96][27] fp32 weights (src_off: element offsets into
// src_base) -- the engine runs it once per step for all blocks next to the bf16 weight mirror.
__global__ void pool_weight_sel_kernel(const float* __restrict__ src_base, const int64_t* __restrict__ src_off,
                                       uint32_t* __restrict__ dst, int n) {
  const int t = blockIdx.y;
  if (t >= n) return;
  const float* w = src_base + src_off[t];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 27 * HD; i += gridDim.x * blockDim.x) {
    const int tap = i / HD, c = i % HD;
    dst[(size_t)t * 27 * HD + i] = (uint32_t)f32_to_bf16(w[c * 27 + tap]) << (16 * (c & 1));
  }
}

// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void pool_ln_bwd_body(const svit_pool_ln_bwd_args& a, float* prow) {
  __shared__ float red[2][HD];
  for (int i = threadIdx.x; i < 2 * HD; i += blockDim.x) (&red[0][0])[i] = 0.f;
  __syncthreads();
  // channel map of a thread's 24 values: SVIT_POOL_LNB_MAP 1 (round 4) = three groups of 8 at 32 v + 8 sub -- the four lanes of a token
  // read 64 contiguous bytes (bf16) / 128 (fp32) per instruction; 0 = one run of 24 at 24 sub (four 16-byte pieces 48 bytes apart)
#ifndef SVIT_POOL_LNB_MAP
#define SVIT_POOL_LNB_MAP 1
#endif
  const int sub = threadIdx.x & 3;
  constexpr int GS = SVIT_POOL_LNB_MAP ? 32 : 8;          // element stride between a thread's groups of 8
  const int c0 = SVIT_POOL_LNB_MAP ? sub * 8 : sub * 24;
  auto chan = [&](int i) { return c0 + (i >> 3) * GS + (i & 7); };
  const int64_t total = (int64_t)a.B * a.heads * a.Nout;
  float gam[24], dg[24], db[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) { gam[i] = a.gamma[chan(i)]; dg[i] = 0.f; db[i] = 0.f; }
  const int64_t iters = (total + (int64_t)gridDim.x * 64 - 1) / ((int64_t)gridDim.x * 64);
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t row = (it * gridDim.x + blockIdx.x) * 64 + (threadIdx.x >> 2);
    const bool live = row < total;
    float d[24], xh[24];
    float mean = 0.f, rstd = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) { d[i] = 0.f; xh[i] = 0.f; }
    if (live) {
      const int tok = (int)(row % a.Nout);
      const int bh = (int)(row / a.Nout), b = bh / a.heads, head = bh % a.heads;
      mean = a.mean[row]; rstd = a.rstd[row];
      if (a.d_main) {
        if (a.main_is_f32) {
          // main_parts planes (the attention backward's per-query-split partial dk / dv) are added here
          const float* p = (const float*)a.d_main + row * a.ld_main + c0;
          for (int part = 0; part < (a.main_parts > 1 ? a.main_parts : 1); ++part, p += a.main_part_stride) {
#pragma unroll
            for (int v = 0; v < 6; ++v) {
              const float4 f = *(const float4*)(p + (v >> 1) * GS + (v & 1) * 4);
              d[v * 4] += f.x; d[v * 4 + 1] += f.y; d[v * 4 + 2] += f.z; d[v * 4 + 3] += f.w;
            }
          }
        } else {
          const bf16_t* p = (const bf16_t*)a.d_main + row * a.ld_main + c0;
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            float f[8];
            unpack8(*(const uint4*)(p + v * GS), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) d[v * 8 + e] += f[e];
          }
        }
      }
      if (a.d_res && tok > 0) {
        const bf16_t* p = (const bf16_t*)a.d_res + ((size_t)b * a.Nout + tok) * a.heads * HD + head * HD + c0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          float f[8];
          unpack8(*(const uint4*)(p + v * GS), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) d[v * 8 + e] += f[e];
        }
      }
      if (a.d_extra && a.extra_is_bf16) {
        const bf16_t* p = (const bf16_t*)a.d_extra + row * HD + c0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          float f[8];
          unpack8(*(const uint4*)(p + v * GS), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) d[v * 8 + e] += f[e];
        }
      } else if (a.d_extra) {
        const float* p = (const float*)a.d_extra + row * HD + c0;
#pragma unroll
        for (int v = 0; v < 6; ++v) {
          const float4 f = *(const float4*)(p + (v >> 1) * GS + (v & 1) * 4);
          d[v * 4] += f.x; d[v * 4 + 1] += f.y; d[v * 4 + 2] += f.z; d[v * 4 + 3] += f.w;
        }
      }
      const bf16_t* pp = (const bf16_t*)a.pre + row * HD + c0;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        float f[8];
        unpack8(*(const uint4*)(pp + v * GS), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) xh[v * 8 + e] = (f[e] - mean) * rstd;
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      dg[i] += d[i] * xh[i];
      db[i] += d[i];
      d[i] *= gam[i];
      s1 += d[i];
      s2 += d[i] * xh[i];
    }
    s1 = quad_sum(s1) * (1.f / HD);
    s2 = quad_sum(s2) * (1.f / HD);
    if (live) {
      bf16_t* o = (bf16_t*)a.dpre + row * HD + c0;
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = rstd * (d[v * 8 + e] - s1 - xh[v * 8 + e] * s2);
        *(uint4*)(o + v * GS) = pack8(f);
      }
    }
  }
  // reduce the 16 tokens of each wave with shuffles (lanes l, l+4, ... share a channel group),
  // then the 4 waves through LDS
  __shared__ float wred[4][2][HD];
#pragma unroll
  for (int i = 0; i < 24; ++i) {
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
      dg[i] += __shfl_xor(dg[i], o, 64);
      db[i] += __shfl_xor(db[i], o, 64);
    }
  }
  if ((threadIdx.x & 63) < 4) {
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      wred[threadIdx.x >> 6][0][chan(i)] = dg[i];
      wred[threadIdx.x >> 6][1][chan(i)] = db[i];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * HD; c += blockDim.x)
    (&red[0][0])[c] = (&wred[0][0][0])[c] + (&wred[1][0][0])[c] + (&wred[2][0][0])[c] + (&wred[3][0][0])[c];
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * HD; c += blockDim.x) prow[c] = (&red[0][0])[c];
}
__global__ __launch_bounds__(256) void pool_ln_bwd_kernel(svit_pool_ln_bwd_args a) {
  pool_ln_bwd_body(a, a.workspace + (size_t)blockIdx.x * 2 * HD);
}
struct PoolLnBwd3 { svit_pool_ln_bwd_args p[3]; };
__global__ __launch_bounds__(256) void pool_ln_bwd3_kernel(PoolLnBwd3 g) {
  // partial rows [block][which][dgamma | dbeta] in the first entry's workspace
  pool_ln_bwd_body(g.p[blockIdx.y],
                   g.p[0].workspace + ((size_t)blockIdx.x * 3 + blockIdx.y) * 2 * HD);
}

// ---------------------------------------------------------------------------------------
// DIAGNOSTIC BUILD ONLY (-DSVIT_DIAG_POOL_STREAMING, tools/diag/build_variant.py; round 6): the streaming conv backward of
// rounds 1-4 -- pool_dgrad3 (gather form) + pool_wgrad3 (LDS-tiled) and their single-tensor forms.  Since round 5 the fused
// plane-walk kernel below takes EVERY block of every configuration the suite runs (tools/diag/pool_bwd_paths.py: 9 configs x 16
// blocks, no fallback), and it is pinned against autograd of the oracle (tests/test_kernels_gpu.py::
// test_pool_backward_vs_oracle_at_the_step_shapes, ::test_pool_conv_bwd_fused_small_planes), so these kernels are no longer a
// product path nor its comparator: the product library does not contain them, svit_pool_conv_bwd_qkv fails loudly
// (SVIT_ERR_SHAPE) where the fused plan does not fit, and the four streaming entry points exist only in this build.
#ifdef SVIT_DIAG_POOL_STREAMING
#define SVIT_POOL_STREAMING_PART 1
#include "../../tools/diag/variants/pool_streaming.inc"
#undef SVIT_POOL_STREAMING_PART
#endif
// ---------------------------------------------------------------------------------------
// Fused conv backward (round 5): conv dgrad AND conv wgrad of q, k, v in ONE launch, replacing
// pool_dgrad3 (27-tap gather of dpre through L2: 5x its bytes fetched) + pool_wgrad3 (x halo ring + dpre re-read).
//   * A workgroup owns (batch*head, tensor, 32-CHANNEL group, t-chunk, y-chunk): 32 channels = 64 bytes = exactly one
//     cache line of every token row it touches in dpre, qkv and dqkv -- no line is shared between workgroups, every byte
//     of x is read once and every byte of dqkv written once.
//   * dpre of the chunk's output planes and rows (+ the halo plane each side in t and, at stride 1, the halo row each
//     side in y) is staged ONCE in LDS by LDS-DMA, zero-padded: image row = output row - ybase, cell(row, xo) =
//     row * P + xo + 1 with pitch P = Wo + 1 (the right halo of a row is the left halo of the next); halo cells, rows
//     outside [0, Ho) and planes outside [0, T) come from past the end of the buffer descriptor = zeros.  Every tap of
//     every token is then an unconditional LDS read: no bounds tests, no clamped addresses.
//   * The workgroup walks its INPUT tokens once (gather form), in UNITS that share a neighbourhood of dpre cells:
//       stride 1: one token; its 27 taps read the 3 x 3 cells around (y, x) in planes t+1, t, t-1;
//       stride 2: the 2 x 2 tokens (2a .. 2a+1, 2b .. 2b+1).  Even coordinates are hit by tap 1 only (cell a), odd ones by
//         tap 0 (cell a + 1) and tap 2 (cell a): together the four tokens use every (ky, kx) exactly once per plane on
//         the 2 x 2 cells (a .. a+1, b .. b+1) -- 12 reads and 27 taps per unit, the same arithmetic per step as stride 1;
//       stride >= 3: the 3 x 3 tokens under ONE output cell (windows do not overlap): 3 reads and 27 taps per unit;
//         the tokens between the windows get their zeros from a 16-byte-store pass in front of the walk.
//     Thread = (channel pair, unit slot); per tap ONE ds_read_b32 (the pair's two bf16 dpre values) feeds
//     dx += w * dpre (dgrad) and dw += x * dpre (wgrad) as four v_dot2_f32_bf16 against "selector" operands (the other
//     half of the pair zero): no bf16 unpacking.  The 27 weights and 27 weight-gradient sums of both channels live in
//     registers.  The walk is bound by VALU issue (in-kernel stamps: 0.47 us per 16-unit step at two workgroups per CU).
//   * x (qkv) and dx (dqkv) go through buffer descriptors with per-lane byte offsets: an invalid token (past the last unit,
//     or hanging over the plane's edge) carries an offset past the end -- its x reads as zero, its dx store is dropped:
//     the loop has no per-token branches.  x of the unit D steps ahead is fetched into the ring slot just consumed.
//   * dw: unit slots meet through shuffles + LDS, one partial row [32 channels][27] per workgroup, summed by the
//     second-stage reduce (fixed order: bit-reproducible).  cls / object rows (dx = dpre, dx = dpre * g(w), the closed-form
//     object share of dw) ride on chunk 0.
// The host planner cuts T and the unit rows per tensor so that the items are about equally long and fill the chip.
constexpr int PF_NT = 256, PF_ROWB = 64, PF_SLOTS = PF_NT / 16;
#ifdef SVIT_POOL_STAMPS
__device__ unsigned long long g_pf_wg[8 * 2048];      // per workgroup of pool_bwd_fused_kernel: start, staged, walked, end, which, chunk, hw id
#define PFSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (threadIdx.x == 0 && blockIdx.x < 2048) g_pf_wg[8 * blockIdx.x + (i)] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PFSTAMP(i) do {} while (0)
#endif
struct PoolBwdFused {
  svit_pool_dgrad_args d[3];
  const void* qkv;
  float* partial;            // [B*heads * max_chunks][3][96][27]
  int n_per[3], t_chunks[3]; // input planes per chunk / chunks along t, per tensor
  int r_per[3], y_chunks[3]; // unit rows per chunk / chunks along y
  int order[3];              // tensors in launch order (longest items first)
  int first_item[4];         // item ranges of order[0..2]
  int max_chunks;            // max over the tensors of t_chunks * y_chunks
};
// stride class (1, 2, 3 = any stride >= 3) -> rows / columns of units of a plane, image rows of a chunk of R unit rows
__host__ __device__ inline int pf_class(int s) { return s >= 3 ? 3 : s; }
__host__ __device__ inline int pf_unit_rows(int sc, int H, int Ho) { return sc == 1 ? H : sc == 2 ? (H + 1) >> 1 : Ho; }
__host__ __device__ inline int pf_image_rows(int sc, int R) { return sc == 1 ? R + 2 : sc == 2 ? R + 1 : R; }
__host__ __device__ inline int pf_plane_bytes(int image_rows, int Wo) { return (image_rows * (Wo + 1) + 1) * PF_ROWB; }

// lb = LDS byte address of the unit's base cell in the slot of plane t.  ALL reads of the unit are issued before the first
// dot2 (a scheduling barrier keeps hipcc from sinking each read next to its use, which exposed one LDS round trip per tap
// with only two waves per SIMD to hide it).
template <int SC, int NT>
__device__ __forceinline__ void pf_unit(unsigned lb, int plane_b, int rowb, const uint32_t (&xs0)[NT], const uint32_t (&xs1)[NT],
                                        const uint32_t (&w0)[27], const uint32_t (&w1)[27], float (&dw0)[27],
                                        float (&dw1)[27], float (&a0)[NT], float (&a1)[NT]) {
  constexpr int NR = SC == 1 ? 3 : SC == 2 ? 2 : 1;              // cell rows / columns read per plane
  uint32_t v[3][NR * NR];
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int cidx = 0; cidx < NR; ++cidx) {
        const int dr = SC == 1 ? r - 1 : r, dc = SC == 1 ? cidx - 1 : cidx;     // stride 1: rows y-1 .. y+1; stride 2: rows a, a+1
        v[kt][r * NR + cidx] = *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)(
            lb + (1 - kt) * plane_b + dr * rowb + dc * PF_ROWB);
      }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int k = (kt * 3 + ky) * 3 + kx;
        // stride 1: output (y + 1 - ky, x + 1 - kx) = cell row 2 - ky of the 3 read.  stride 2: tap 0 -> odd token, cell + 1;
        // tap 1 -> even token, cell + 0; tap 2 -> odd token, cell + 0.  stride >= 3: token (ky, kx) of the window, its one cell
        const int r = SC == 1 ? 2 - ky : SC == 2 ? (ky == 0 ? 1 : 0) : 0, cidx = SC == 1 ? 2 - kx : SC == 2 ? (kx == 0 ? 1 : 0) : 0;
        const int tok = SC == 1 ? 0 : SC == 2 ? (ky == 1 ? 0 : 2) + (kx == 1 ? 0 : 1) : ky * 3 + kx;
        const uint32_t d = v[kt][r * NR + cidx];
        a0[tok] = dot2_sel(d, w0[k], a0[tok]);
        a1[tok] = dot2_sel(d, w1[k], a1[tok]);
        dw0[k] = dot2_sel(d, xs0[tok], dw0[k]);
        dw1[k] = dot2_sel(d, xs1[tok], dw1[k]);
      }
}

template <int SC>
__device__ __forceinline__ void pool_bwd_fused_body(const PoolBwdFused& g, int which, int bh, int group, int tchunk,
                                                    int ychunk, unsigned char* smem) {
  const svit_pool_dgrad_args& a = g.d[which];
  const int tid = threadIdx.x, cp = tid & 15, ts = tid >> 4, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = group * 32 + 2 * cp;
  const int s = a.stride_hw;
  const int T = a.T, H = a.H, W = a.W;
  const int Ho = pooled(H, s), Wo = pooled(W, s);
  const int L = T * H * W, Lo = T * Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int b = bh / a.heads, head = bh % a.heads;
  const int chunk = tchunk * g.y_chunks[which] + ychunk;
  const int n_per = g.n_per[which];
  const int t0 = tchunk * n_per, t1 = min(T, t0 + n_per), np = t1 - t0;
  // unit rows [ur0, ur1) of this chunk; image row 0 = output row ybase
  const int UR = pf_unit_rows(SC, H, Ho), UC = SC == 1 ? W : SC == 2 ? (W + 1) >> 1 : Wo;
  const int ur0 = ychunk * g.r_per[which], ur1 = min(UR, ur0 + g.r_per[which]), Rc = ur1 - ur0;
  const int ybase = SC == 1 ? ur0 - 1 : ur0, RR = pf_image_rows(SC, Rc);
  const int P = Wo + 1, rows = RR * P + 1, plane_b = rows * PF_ROWB, rowb = P * PF_ROWB;
  const bf16_t* dsrc = (const bf16_t*)a.dpre + (size_t)bh * Nout * HD + group * 32;
  PFSTAMP(0);
  // ---- stage dpre planes t0-1 .. t1 (slot sl holds output plane t0 - 1 + sl) by LDS-DMA: the whole image is cut into
  // 1-KiB pieces, a lane's 16 bytes come from its cell's row of dpre, or -- halo cells, rows / planes outside the volume, the
  // tail of the last piece -- from past the end of the buffer descriptor, which reads as zeros.  All pieces of a wave are
  // in flight at once: one memory round trip for the whole prologue.
  {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)dsrc, 0, (int)((size_t)Nout * HD * 2), 0x00020000);
    const unsigned mP = fdiv_magic_dev(P), mR = fdiv_magic_dev(rows);
    const int pieces = ((np + 2) * plane_b + 1023) >> 10;
    for (int q = wave; q < pieces; q += PF_NT / 64) {
      const int o = q * 1024 + lane * 16;
      const int cell = o >> 6, part = (o >> 4) & 3;
      const int sl = fdiv(cell, mR), cr = cell - sl * rows;
      const int rr = fdiv(cr, mP), xx = cr - rr * P;
      const int to = t0 - 1 + sl, yo = ybase + rr;
      const bool ok = sl < np + 2 && to >= 0 && to < T && rr < RR && yo >= 0 && yo < Ho && xx >= 1 && xx <= Wo;
      const unsigned voff = ok ? (unsigned)((1 + (to * Ho + yo) * Wo + xx - 1) * (HD * 2) + part * 16) : 0x7ffffff0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + q * 1024), 16, voff, 0, 0, 0);
    }
  }
  // ---- this thread's weights (bf16-rounded selectors, like every stencil of this file) and accumulators
  uint32_t w0[27], w1[27];
  float dw0[27], dw1[27];
  float nt[3], nh[3], ipt, iph;
  obj_counts(1, nt, &ipt);
  obj_counts(s, nh, &iph);
  const float onorm = ipt * iph * iph;
  float g0 = 0.f, g1 = 0.f;                   // object gains g(w) of the two channels, from the fp32 weights (as the forward)
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const float f0 = a.conv_w[(size_t)c * 27 + k], f1 = a.conv_w[(size_t)(c + 1) * 27 + k];
    const float coef = nt[k / 9] * nh[(k / 3) % 3] * nh[k % 3] * onorm;
    g0 += f0 * coef; g1 += f1 * coef;
    w0[k] = (uint32_t)f32_to_bf16(f0);
    w1[k] = (uint32_t)f32_to_bf16(f1) << 16;
    dw0[k] = 0.f; dw1[k] = 0.f;
  }
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const size_t col = ((size_t)which * a.heads + head) * HD + c;
  const bf16_t* xin = (const bf16_t*)g.qkv + (size_t)b * N * tok_stride + col;
  bf16_t* dxo = (bf16_t*)a.dqkv + (size_t)b * N * tok_stride + col;
  // ---- stride >= 3: the tokens between the 3 x 3 windows get zeros.  The chunk's input rows (the windows of its unit
  // rows and the gap below each; the last chunk runs to the plane's end) are contiguous tokens: 16-byte stores, 4 lanes
  // per token.  They are complete (s_waitcnt below) before any wave stores a window's dx over them.
  if (SC == 3) {
    const int ylo = max(0, s * ur0 - 1), yhi = ur1 == UR ? H : min(H, s * ur1 - 1);
    const int cnt4 = (yhi - ylo) * W * 4;
    char* zb = (char*)a.dqkv + ((size_t)b * N * tok_stride + ((size_t)which * a.heads + head) * HD + group * 32) * 2;
    for (int pl = 0; pl < np; ++pl) {
      const size_t tok0 = 1 + (size_t)((t0 + pl) * H + ylo) * W;
      for (int i = tid; i < cnt4; i += PF_NT)
        *(uint4*)(zb + (tok0 + (i >> 2)) * tok_stride * 2 + (i & 3) * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  // ---- the walk: unit f = slot + 16 i of thread slot ts
  {
    constexpr int NT = SC == 1 ? 1 : SC == 2 ? 4 : 9, D = SC == 3 ? 2 : 4;
    const int U = Rc * UC, total = np * U;
    const unsigned mU = fdiv_magic_dev(U), mC = fdiv_magic_dev(UC);
    const unsigned stride_b = (unsigned)(tok_stride * 2);
    const size_t span = (size_t)N * tok_stride * 2;                                 // bytes of one clip in qkv / dqkv
    const unsigned col_b = (unsigned)((((size_t)which * a.heads + head) * HD + c) * 2);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)g.qkv + (size_t)b * span), 0, (int)span, 0x00020000);
    const auto drs = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)a.dqkv + (size_t)b * span), 0, (int)span, 0x00020000);
    constexpr unsigned OOB = 0x7ffffff0u;
    const unsigned lds0 = (unsigned)(uintptr_t)smem;
    // unit f of this thread -> byte offsets of its tokens, LDS address of its base cell
    auto locate = [&](int f, unsigned (&off)[NT], unsigned* lb) {
      const bool live = f < total;
      const int fc = live ? f : 0;
      const int pl = fdiv(fc, mU), u = fc - pl * U;
      const int ur = fdiv(u, mC), uc = u - ur * UC;
      const int gr = ur0 + ur;                                                      // unit row in the plane
      const int y = SC == 1 ? gr : SC == 2 ? 2 * gr : s * gr - 1, x = SC == 1 ? uc : SC == 2 ? 2 * uc : s * uc - 1;
      const int tokidx = 1 + ((t0 + pl) * H + y) * W + x;                           // (y, x = -1: the window hangs over the edge)
      const unsigned o = (unsigned)tokidx * stride_b + col_b;
      *lb = lds0 + (unsigned)((pl + 1) * plane_b + ((SC == 1 ? ur + 1 : ur) * P + uc + 1) * PF_ROWB + cp * 4);
      if (SC == 1) {
        off[0] = live ? o : OOB;
      } else if (SC == 2) {
        const bool vx = live && x + 1 < W, vy = live && y + 1 < H;
        off[0] = live ? o : OOB;
        off[1] = vx ? o + stride_b : OOB;
        off[2] = vy ? o + (unsigned)W * stride_b : OOB;
        off[3] = vx && vy ? o + (unsigned)(W + 1) * stride_b : OOB;
      } else {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const bool v = live && y + ky >= 0 && y + ky < H && x + kx >= 0 && x + kx < W;
            off[ky * 3 + kx] = v ? o + (unsigned)(ky * W + kx) * stride_b : OOB;
          }
      }
    };
    // (stride >= 3: nine offsets per unit -- they are recomputed at the unit's turn instead of riding in the ring)
    constexpr int NO = SC == 3 ? 1 : NT;
    uint32_t xq[D][NT];
    unsigned oq[D][NO], lq[D];
    int f = ts;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      unsigned off[NT];
      locate(f + j * PF_SLOTS, off, &lq[j]);
#pragma unroll
      for (int e = 0; e < NT; ++e) xq[j][e] = __builtin_amdgcn_raw_buffer_load_b32(xrs, off[e], 0, 0);
      if constexpr (SC != 3) {
#pragma unroll
        for (int e = 0; e < NT; ++e) oq[j][e] = off[e];
      }
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D * NT) : "memory");      // the staged planes, the zero pass (everything but the x ring) are complete
    __syncthreads();
    PFSTAMP(1);
    const int steps = (total + PF_SLOTS - 1) / PF_SLOTS;               // (uniform: every thread walks the same number of steps)
    for (int i = 0; i < steps; i += D) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        if (i + j < steps) {
          uint32_t xs0[NT], xs1[NT];
          unsigned off[NT], lb = lq[j];
          float a0[NT], a1[NT];
#pragma unroll
          for (int e = 0; e < NT; ++e) {
            xs0[e] = xq[j][e] & 0xffffu; xs1[e] = xq[j][e] & 0xffff0000u;
            a0[e] = 0.f; a1[e] = 0.f;
          }
          {
            unsigned offn[NT];
            locate(f + D * PF_SLOTS, offn, &lq[j]);
#pragma unroll
            for (int e = 0; e < NT; ++e) xq[j][e] = __builtin_amdgcn_raw_buffer_load_b32(xrs, offn[e], 0, 0);
            if constexpr (SC != 3) {
#pragma unroll
              for (int e = 0; e < NT; ++e) { off[e] = oq[j][e]; oq[j][e] = offn[e]; }
            }
          }
          pf_unit<SC, NT>(lb, plane_b, rowb, xs0, xs1, w0, w1, dw0, dw1, a0, a1);
          if constexpr (SC == 3) {
            unsigned lb2;
            locate(f, off, &lb2);
          }
#pragma unroll
          for (int e = 0; e < NT; ++e) __builtin_amdgcn_raw_buffer_store_b32(pack_bf16x2(a0[e], a1[e]), drs, off[e], 0, 0);
          f += PF_SLOTS;
        }
      }
    }
  }
  PFSTAMP(2);
  // ---- cls / object rows ride on chunk 0: dx[cls] = dpre[cls], dx[obj] = dpre[obj] * g(w), dw += coef * sum dpre * x
  if (chunk == 0) {
    float go0 = 0.f, go1 = 0.f;
    // (four rows per thread in flight: the loads of a row depend on nothing, only their round trips would add up)
    for (int i0 = ts; i0 <= a.n_obj; i0 += 4 * PF_SLOTS) {        // i = 0: cls, i >= 1: object i - 1
      uint32_t dv[4], xv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * PF_SLOTS;
        dv[e] = 0u; xv[e] = 0u;
        if (i <= a.n_obj) {
          dv[e] = *(const uint32_t*)(dsrc + (size_t)(i == 0 ? 0 : Lo + i) * HD + 2 * cp);
          if (i > 0) xv[e] = *(const uint32_t*)(xin + (size_t)(L + i) * tok_stride);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * PF_SLOTS;
        if (i > a.n_obj) continue;
        float d0 = lo_bf16(dv[e]), d1 = hi_bf16(dv[e]);
        if (i > 0) {
          go0 += d0 * lo_bf16(xv[e]); go1 += d1 * hi_bf16(xv[e]);
          d0 *= g0; d1 *= g1;
        }
        *(uint32_t*)(dxo + (size_t)(i == 0 ? 0 : L + i) * tok_stride) = pack_bf16x2(d0, d1);
      }
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const float coef = nt[k / 9] * nh[(k / 3) % 3] * nh[k % 3] * onorm;
      dw0[k] += go0 * coef; dw1[k] += go1 * coef;
    }
  }
  // ---- the 16 unit slots meet: 4 per wave through shuffles, the 4 waves through LDS
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    dw0[k] += __shfl_xor(dw0[k], 16, 64); dw0[k] += __shfl_xor(dw0[k], 32, 64);
    dw1[k] += __shfl_xor(dw1[k], 16, 64); dw1[k] += __shfl_xor(dw1[k], 32, 64);
  }
  __syncthreads();                              // everyone is done reading the planes
  float* red = (float*)smem;                    // [4 waves][16 pairs][54]
  if ((tid & 63) < 16) {
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      red[(wave * 16 + cp) * 54 + k] = dw0[k];
      red[(wave * 16 + cp) * 54 + 27 + k] = dw1[k];
    }
  }
  __syncthreads();
  // one partial row per (batch*head, chunk): [which][c][tap], this workgroup's 32 channels of it
  float* prow = g.partial + (((size_t)bh * g.max_chunks + chunk) * 3 + which) * (27 * HD) + group * 32 * 27;
  for (int o = tid; o < 16 * 54; o += PF_NT)
    prow[o] = red[o] + red[864 + o] + red[2 * 864 + o] + red[3 * 864 + o];     // ([pair][ch 0 taps | ch 1 taps] = [c][tap])
  // rows of chunks this tensor does not have must read as zero in the second-stage sum
  if (chunk == 0)
    for (int ch = g.t_chunks[which] * g.y_chunks[which]; ch < g.max_chunks; ++ch) {
      float* z = g.partial + (((size_t)bh * g.max_chunks + ch) * 3 + which) * (27 * HD) + group * 32 * 27;
      for (int o = tid; o < 32 * 27; o += PF_NT) z[o] = 0.f;
    }
#ifdef SVIT_POOL_STAMPS
  __syncthreads();
  PFSTAMP(3);
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    g_pf_wg[8 * blockIdx.x + 4] = which; g_pf_wg[8 * blockIdx.x + 5] = chunk;
    g_pf_wg[8 * blockIdx.x + 6] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
  }
#endif
}

__global__ __launch_bounds__(PF_NT, 2) void pool_bwd_fused_kernel(PoolBwdFused g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_pf[];
  const int item = blockIdx.x;
  const int j = (item >= g.first_item[1]) + (item >= g.first_item[2]);
  const int which = g.order[j];
  const int local = item - g.first_item[j];
  const int BH = g.d[0].B * g.d[0].heads;
  const int bh = local % BH, rest = local / BH, group = rest % 3, ch = rest / 3;
  const int ychunk = ch % g.y_chunks[which], tchunk = ch / g.y_chunks[which];
  const int s = g.d[which].stride_hw;
  if (s == 1) pool_bwd_fused_body<1>(g, which, bh, group, tchunk, ychunk, smem_pf);
  else if (s == 2) pool_bwd_fused_body<2>(g, which, bh, group, tchunk, ychunk, smem_pf);
  else pool_bwd_fused_body<3>(g, which, bh, group, tchunk, ychunk, smem_pf);
}

// ---------------------------------------------------------------------------------------
// Staged conv FORWARD of the large planes (round 5): the depthwise 3x3x3 conv of q, k, v of a block
// in one launch with the INPUT staged once in LDS -- the mirror image of pool_bwd_fused_kernel -- for the blocks whose
// planes are too large for the slab / MFMA stencils (blocks 0-3 of 16x224^2), where the streaming kernel pulls every tap
// through L2 (FETCH 2.6x its operands; 116 / 105 us at the stride-2 blocks 1 / 3).  LayerNorm stays pool_slab_ln_kernel
// (a second, row-wise launch over `pre`: a 32-channel workgroup cannot normalise 96 channels).
//   * workgroup = (batch*head, tensor, 32-channel group, t-chunk, y-chunk of OUTPUT rows): 64-byte segments of qkv in,
//     64-byte segments of `pre` out -- whole cache lines, nothing shared between workgroups;
//   * the image holds exactly the cells the chunk's windows touch: stride 1 / 2: input rows s*yo0-1 .. s*(yo1-1)+1, every
//     x (pitch W + 1: the left halo column doubles as the previous row's right halo); stride >= 3 (windows do not overlap):
//     only the 3 rows / 3 columns of each window, packed (3 R rows x 3 Wo cells).  Either way the 27 taps of output (yo, xo)
//     are the 3 x 3 cells from base (SE (yo - yo0), SE xo), SE = 1 / 2 / 3, in the slots of planes t-1, t, t+1: ONE code path
//     for every stride, unconditional reads (out-of-volume cells are staged as zeros through the buffer descriptor's end);
//   * thread = (channel pair, unit slot): 27 ds_read_b32 feed 54 v_dot2 (selector weights in registers), one 4-byte store.
#ifndef SVIT_PS_NT
#define SVIT_PS_NT 512
#endif
constexpr int PS_NT = SVIT_PS_NT, PS_SLOTS = PS_NT / 16;
struct PoolFwdStaged {
  svit_pool_args p[3];
  int n_per[3], t_chunks[3], r_per[3], y_chunks[3];
  int order[3], first_item[4];
};
__host__ __device__ inline int ps_plane_bytes(int se, int R, int W, int Wo) {
  return se < 3 ? ((se * (R - 1) + 3) * (W + 1) + 1) * PF_ROWB : (3 * R) * (3 * Wo) * PF_ROWB;
}

template <int SE>
__device__ __forceinline__ void pool_fwd_staged_body(const PoolFwdStaged& g, int which, int bh, int group, int tchunk,
                                                     int ychunk, unsigned char* smem) {
  const svit_pool_args& a = g.p[which];
  const int tid = threadIdx.x, cp = tid & 15, ts = tid >> 4, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = group * 32 + 2 * cp;
  const int s = a.stride_hw, T = a.T, H = a.H, W = a.W;
  const int Ho = pooled(H, s), Wo = pooled(W, s);
  const int L = T * H * W, Lo = T * Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int b = bh / a.heads, head = bh % a.heads;
  const int t0 = tchunk * g.n_per[which], t1 = min(T, t0 + g.n_per[which]), np = t1 - t0;
  const int yo0 = ychunk * g.r_per[which], yo1 = min(Ho, yo0 + g.r_per[which]), Rc = yo1 - yo0;
  const int P = SE < 3 ? W + 1 : 3 * Wo, RR = SE < 3 ? SE * (Rc - 1) + 3 : 3 * Rc;
  const int cells = RR * P + (SE < 3 ? 1 : 0), plane_b = cells * PF_ROWB, rowb = P * PF_ROWB;
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const unsigned stride_b = (unsigned)(tok_stride * 2);
  const size_t span = (size_t)N * tok_stride * 2;
  const unsigned grp_b = (unsigned)((((size_t)a.which * a.heads + head) * HD + group * 32) * 2);
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.qkv + (size_t)b * span), 0, (int)span, 0x00020000);
  // ---- stage input planes t0-1 .. t1 (slot sl = plane t0 - 1 + sl): 1-KiB LDS-DMA pieces, every piece of a wave in flight
  {
    const unsigned mP = fdiv_magic_dev(P), mC = fdiv_magic_dev(cells);
    const int pieces = ((np + 2) * plane_b + 1023) >> 10;
    for (int q = wave; q < pieces; q += PS_NT / 64) {
      const int o = q * 1024 + lane * 16;
      const int cell = o >> 6, part = (o >> 4) & 3;
      const int sl = fdiv(cell, mC), cr = cell - sl * cells;
      const int iy = fdiv(cr, mP), ix = cr - iy * P;
      int y, x;
      if (SE < 3) { y = s * yo0 - 1 + iy; x = ix - 1; }
      else { const int wy = fdiv(iy, 0x55555556u), wx = fdiv(ix, 0x55555556u); y = s * (yo0 + wy) - 1 + (iy - 3 * wy); x = s * wx - 1 + (ix - 3 * wx); }
      const int t = t0 - 1 + sl;
      const bool ok = sl < np + 2 && iy < RR && t >= 0 && t < T && y >= 0 && y < H && x >= 0 && x < W;
      const unsigned voff = ok ? (unsigned)(1 + (t * H + y) * W + x) * stride_b + grp_b + part * 16 : 0x7ffffff0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(smem + q * 1024), 16, voff, 0, 0, 0);
    }
  }
  // ---- weights: bf16-rounded selectors (like every stencil of this file); object gains from the fp32 values
  uint32_t w0[27], w1[27];
  float nt[3], nh[3], ipt, iph;
  obj_counts(1, nt, &ipt);
  obj_counts(s, nh, &iph);
  const float onorm = ipt * iph * iph;
  float g0 = 0.f, g1 = 0.f;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const float f0 = a.conv_w[(size_t)c * 27 + k], f1 = a.conv_w[(size_t)(c + 1) * 27 + k];
    const float coef = nt[k / 9] * nh[(k / 3) % 3] * nh[k % 3] * onorm;
    g0 += f0 * coef; g1 += f1 * coef;
    w0[k] = (uint32_t)f32_to_bf16(f0);
    w1[k] = (uint32_t)f32_to_bf16(f1) << 16;
  }
  bf16_t* preb = (bf16_t*)a.pre + (size_t)bh * Nout * HD;
  const auto prs = __builtin_amdgcn_make_buffer_rsrc((void*)preb, 0, (int)((size_t)Nout * HD * 2), 0x00020000);
  // cls / object rows ride on chunk 0: pre[cls] = x[cls], pre[obj] = x[obj] * g(w)  (requested before the wait)
  if (tchunk == 0 && ychunk == 0) {
    for (int i = ts; i <= a.n_obj; i += PS_SLOTS) {
      const int tin = i == 0 ? 0 : L + i, tout = i == 0 ? 0 : Lo + i;
      const uint32_t xv = __builtin_amdgcn_raw_buffer_load_b32(xrs, (unsigned)tin * stride_b + grp_b + cp * 4, 0, 0);
      float x0 = lo_bf16(xv), x1 = hi_bf16(xv);
      if (i > 0) { x0 *= g0; x1 *= g1; }
      __builtin_amdgcn_raw_buffer_store_b32(pack_bf16x2(x0, x1), prs, (unsigned)(tout * HD + c) * 2, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ---- the walk over output tokens: unit f = slot + 16 i
  const int U = Rc * Wo, total = np * U;
  const unsigned mU = fdiv_magic_dev(U), mW = fdiv_magic_dev(Wo);
  const unsigned lds0 = (unsigned)(uintptr_t)smem;
  for (int f = ts; f < total; f += PS_SLOTS) {
    const int pl = fdiv(f, mU), u = f - pl * U;
    const int r = fdiv(u, mW), xo = u - r * Wo;
    const unsigned lb = lds0 + (unsigned)(pl * plane_b + (SE * r) * rowb + (SE * xo) * PF_ROWB + cp * 4);
    uint32_t v[27];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          v[(kt * 3 + ky) * 3 + kx] = *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)(
              lb + kt * plane_b + ky * rowb + kx * PF_ROWB);
    __builtin_amdgcn_sched_barrier(0);
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      a0 = dot2_sel(v[k], w0[k], a0);
      a1 = dot2_sel(v[k], w1[k], a1);
    }
    const int tok = 1 + ((t0 + pl) * Ho + yo0 + r) * Wo + xo;
    __builtin_amdgcn_raw_buffer_store_b32(pack_bf16x2(a0, a1), prs, (unsigned)(tok * HD + c) * 2, 0, 0);
  }
}

__global__ __launch_bounds__(PS_NT, PS_NT == 256 ? 3 : PS_NT == 512 ? 4 : 2) void pool_fwd_staged_kernel(PoolFwdStaged g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_ps[];
  const int item = blockIdx.x;
  const int j = (item >= g.first_item[1]) + (item >= g.first_item[2]);
  const int which = g.order[j];
  const int local = item - g.first_item[j];
  const int BH = g.p[0].B * g.p[0].heads;
  const int bh = local % BH, rest = local / BH, group = rest % 3, ch = rest / 3;
  const int ychunk = ch % g.y_chunks[which], tchunk = ch / g.y_chunks[which];
  const int s = g.p[which].stride_hw;
  if (s == 1) pool_fwd_staged_body<1>(g, which, bh, group, tchunk, ychunk, smem_ps);
  else if (s == 2) pool_fwd_staged_body<2>(g, which, bh, group, tchunk, ychunk, smem_ps);
  else pool_fwd_staged_body<3>(g, which, bh, group, tchunk, ychunk, smem_ps);
}

// ---------------------------------------------------------------------------------------
// T = 1 volumes: conv + LayerNorm in ONE launch with the plane staged in LDS (round 5).  Every frame of the no-grad frames
// pass (train_net.py:105-110) and every still of an image rank is a one-plane volume: 9 of the 27 taps exist, and a whole
// 96-channel plane (14x14: 46 KB) or a band of its rows fits LDS -- so the workgroup that convolves also holds whole token
// rows and normalises them itself (the arithmetic and the stores of pool_ln_finish, the streaming kernel's back end).  The
// streaming kernel fetched the 9 taps of every output straight through L2: 97 us per 14x14 block of the frames pass
// (~1 TB/s on its 90 MB), sixteen launches = 1.55 ms of the as-released step.
//   * item = (tensor, head, frame, band of output rows); image as in pool_fwd_staged_kernel (stride 1 / 2: dense rows, pitch
//     W + 1 cells, halo cells from past the end of the buffer descriptor = zeros; stride >= 3: the 3 x 3 cells of each
//     window, packed) with 192-byte cells;
//   * ONE persistent 8-wave workgroup per CU walks items blockIdx.x, + gridDim.x, ... through TWO image buffers: the LDS-DMA
//     of item k + 1 is issued right behind the barrier that says item k has landed and travels under item k's arithmetic
//     (the first version staged, waited, computed: 44 us per 14x14 block, most of it exposed latency);
//   * thread = (token, 12-channel eighth): the 9 x 12 selector weights and the object gains of a lane live in registers
//     (re-read when the tensor changes: items are sorted by tensor) -- LDS serves the 27 eight-byte tap reads only (four
//     24-channel lanes per token with the weights in LDS read three times as many bytes and were LDS-bound);
//   * cls / object rows ride on band 0.  q's rel-pos columns come from the SVIT_EPI_RELQ GEMM launch behind it, as on the
//     streaming path.
struct PoolFrame3 {
  svit_pool_args p[3];
  int r_per[3], y_chunks[3], n_items[3], wg_first[4];     // workgroups [wg_first[i], wg_first[i+1]) walk the items of tensor i
};
constexpr int FR_NT = 512;
constexpr int FR_ROWB = 192;                       // bytes per cell: the 96 channels of a token
constexpr int FR_HEAD = 27 * HD * 4 + 384;         // the fp32 weights of the workgroup's tensor (source of the register copies)
constexpr int FR_IMG_MAX = 74 * 1024;              // 56x56 at stride 1: 6 input rows = 4 output rows per band; x 2 buffers + head <= 160 KB
__host__ __device__ inline int fr_image_bytes(int se, int R, int W, int Wo) {
  return se < 3 ? ((se * (R - 1) + 3) * (W + 1) + 1) * FR_ROWB : (3 * R) * (3 * Wo) * FR_ROWB;
}
struct FrItem { int bh, yo0, Rc, specials; };
#ifdef SVIT_POOL_STAMPS
__device__ unsigned long long g_fr_st[256 * 64];     // workgroup x (4 stamps per item: top, landed, issued, computed)
#define FRSTAMP() do { __builtin_amdgcn_sched_barrier(0); if (threadIdx.x == 0 && blockIdx.x < 256 && fr_si < 64) g_fr_st[64 * blockIdx.x + fr_si++] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define FRSTAMP() do {} while (0)
#endif

// sum over the 8 lanes of a token on the vector pipe (DPP: two quad permutes and a half-row mirror; __shfl_xor compiles to
// ds_bpermute -- six LDS round trips per pass)
__device__ __forceinline__ float oct_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));   // row_half_mirror
  return v;
}

__device__ __forceinline__ FrItem fr_item(const svit_pool_args& a, int chunks, int r_per, int local) {
  FrItem it;
  const int ch = local % chunks, rest = local / chunks;
  const int b = rest % a.B, head = rest / a.B;
  const int Ho = pooled(a.H, a.stride_hw);
  it.bh = b * a.heads + head;
  it.yo0 = ch * r_per;
  it.Rc = min(Ho, it.yo0 + r_per) - it.yo0;
  it.specials = ch == 0;
  return it;
}

// issue the LDS-DMA pieces of one item's image (no wait)
template <int SE>
__device__ __forceinline__ void fr_stage(const svit_pool_args& a, const FrItem& it, unsigned char* img) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = a.stride_hw, H = a.H, W = a.W;
  const int Wo = pooled(W, s);
  const int N = 1 + H * W + a.n_obj;
  const int b = it.bh / a.heads, head = it.bh % a.heads;
  const int P = SE < 3 ? W + 1 : 3 * Wo, RR = SE < 3 ? SE * (it.Rc - 1) + 3 : 3 * it.Rc;
  const int cells = RR * P + (SE < 3 ? 1 : 0);
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const unsigned stride_b = (unsigned)(tok_stride * 2);
  const size_t span = (size_t)N * tok_stride * 2;
  const unsigned chan_b = (unsigned)((((size_t)a.which * a.heads + head) * HD) * 2);
  const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.qkv + (size_t)b * span), 0, (int)span, 0x00020000);
  const unsigned mP = fdiv_magic_dev(P);
  const int pieces = (cells * FR_ROWB + 1023) >> 10;
  for (int q = wave; q < pieces; q += FR_NT / 64) {
    const int slot = q * 64 + lane;                     // 16-byte slot of the image
    const int cell = fdiv(slot, 0x15555556u), part = slot - cell * 12;
    const int iy = fdiv(cell, mP), ix = cell - iy * P;
    int y, x;
    if (SE < 3) { y = s * it.yo0 - 1 + iy; x = ix - 1; }
    else { const int wy = fdiv(iy, 0x55555556u), wx = fdiv(ix, 0x55555556u); y = s * (it.yo0 + wy) - 1 + (iy - 3 * wy); x = s * wx - 1 + (ix - 3 * wx); }
    const bool ok = iy < RR && y >= 0 && y < H && x >= 0 && x < W;
    const unsigned voff = ok ? (unsigned)(1 + y * W + x) * stride_b + chan_b + part * 16 : 0x7ffffff0u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(img + q * 1024), 16, voff, 0, 0, 0);
  }
}

// One tensor's share of the launch: this workgroup walks items first, first + step, ... of tensor `a`
template <int SE>
__device__ __forceinline__ void fr_run(const svit_pool_args& a, int chunks, int r_per, int n_items, int first, int step,
                                       int img_bytes, unsigned char* smem) {
  float* w_raw = (float*)smem;               // [96][27] fp32 weights
  unsigned char* img0 = smem + FR_HEAD;
  const int tid = threadIdx.x, sub = tid & 7, c0 = sub * 12;
  const int s = a.stride_hw, H = a.H, W = a.W;
  const int Ho = pooled(H, s), Wo = pooled(W, s);
  const int L = H * W, Lo = Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int P = SE < 3 ? W + 1 : 3 * Wo;
  const unsigned mW = fdiv_magic_dev(Wo);
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const float osc = a.out_scale != 0.f ? a.out_scale : 1.f;
#ifdef SVIT_POOL_STAMPS
  int fr_si = 0;
#endif
  int local = first;
  if (local >= n_items) return;
  FrItem it = fr_item(a, chunks, r_per, local);
  fr_stage<SE>(a, it, img0);
  // the lane's 9 x 12 selector weights, object gains and LayerNorm parameters (while the first image travels)
  uint32_t wsel[9][12];
  float gain[12], gm[12], bt[12];
  for (int i = tid; i < 27 * HD; i += FR_NT) w_raw[i] = a.conv_w[i];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const float4 g4 = *(const float4*)(a.gamma + c0 + 4 * u), b4 = *(const float4*)(a.beta + c0 + 4 * u);
    gm[4 * u] = g4.x * osc; gm[4 * u + 1] = g4.y * osc; gm[4 * u + 2] = g4.z * osc; gm[4 * u + 3] = g4.w * osc;
    bt[4 * u] = b4.x * osc; bt[4 * u + 1] = b4.y * osc; bt[4 * u + 2] = b4.z * osc; bt[4 * u + 3] = b4.w * osc;
  }
  __syncthreads();
  {
    float nt[3], nh[3], ipt, iph;
    obj_counts(1, nt, &ipt);
    obj_counts(s, nh, &iph);
    const float onorm = ipt * iph * iph;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const float* wc = w_raw + (c0 + j) * 27;
      float gs = 0.f;
#pragma unroll
      for (int t27 = 0; t27 < 27; ++t27) gs += wc[t27] * (nt[t27 / 9] * nh[(t27 / 3) % 3] * nh[t27 % 3]);
      gain[j] = gs * onorm;
#pragma unroll
      for (int k9 = 0; k9 < 9; ++k9) wsel[k9][j] = (uint32_t)f32_to_bf16(wc[9 + k9]) << (16 * (j & 1));
    }
  }
  for (int k = 0; local < n_items; ++k, local += step) {
    const unsigned char* img = img0 + (k & 1) * img_bytes;
    FRSTAMP();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                 // item k has landed; every wave is done with item k - 1 (its buffer is free)
    FRSTAMP();
    // the next item's image travels under item k's arithmetic.  (The LDS-DMA issue itself is paced by the CU's vector-memory
    // path, ~25 ns per 1-KiB piece = 1.2 us for a 14x14 plane; letting the two waves of a SIMD take turns -- waves 0-3 issue
    // here, waves 4-7 behind their first pass -- changed nothing: every wave still issues its share and computes every pass.)
    FrItem nx = it;
    if (local + step < n_items) {
      nx = fr_item(a, chunks, r_per, local + step);
      fr_stage<SE>(a, nx, img0 + ((k + 1) & 1) * img_bytes);
    }
    FRSTAMP();
    // ---- the outputs of item k: 64 tokens per pass, thread = (token, 12 channels)
    const int bh = it.bh, b = bh / a.heads, head = bh % a.heads;
    const int U = it.Rc * Wo, total = U + (it.specials ? 1 + a.n_obj : 0);
    const bf16_t* gbase = (const bf16_t*)a.qkv + (size_t)b * N * tok_stride + ((size_t)a.which * a.heads + head) * HD + c0;
    for (int base = 0; base < total; base += FR_NT / 8) {
      const int idx = base + (tid >> 3);
      const bool live = idx < total, is_patch = idx < U;
      float acc[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[i] = 0.f;
      int py = 0, px = 0, tok = 0;
      if (is_patch) {
        const int r = fdiv(idx, mW), xo = idx - r * Wo;
        py = it.yo0 + r; px = xo; tok = 1 + py * Wo + xo;
        const unsigned char* lb = img + ((SE * r) * P + SE * xo) * FR_ROWB + sub * 24;
        uint2 v[9][3];
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9)
#pragma unroll
          for (int u = 0; u < 3; ++u) v[k9][u] = *(const uint2*)(lb + ((k9 / 3) * P + (k9 % 3)) * FR_ROWB + u * 8);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9)
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            acc[4 * u + 0] = dot2_sel(v[k9][u].x, wsel[k9][4 * u + 0], acc[4 * u + 0]);
            acc[4 * u + 1] = dot2_sel(v[k9][u].x, wsel[k9][4 * u + 1], acc[4 * u + 1]);
            acc[4 * u + 2] = dot2_sel(v[k9][u].y, wsel[k9][4 * u + 2], acc[4 * u + 2]);
            acc[4 * u + 3] = dot2_sel(v[k9][u].y, wsel[k9][4 * u + 3], acc[4 * u + 3]);
          }
      } else if (live) {
        const int j = idx - U;
        const int src = j == 0 ? 0 : L + j;
        tok = j == 0 ? 0 : Lo + j;
        const bf16_t* p = gbase + (size_t)src * tok_stride;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const uint2 h = *(const uint2*)(p + u * 4);
          const float f[4] = {lo_bf16(h.x), hi_bf16(h.x), lo_bf16(h.y), hi_bf16(h.y)};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[4 * u + e] = j == 0 ? f[e] : f[e] * gain[4 * u + e];
        }
      }
      // LayerNorm(96) over the 8 lanes of a token + stores (the arithmetic of pool_ln_finish with 12 channels per lane)
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[i] = bf16_to_f32(f32_to_bf16(acc[i]));
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 12; ++i) sum += acc[i];
      const float mean = oct_sum(sum) * (1.f / HD);
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < 12; ++i) sq += (acc[i] - mean) * (acc[i] - mean);
      const float rstd = rsqrtf(oct_sum(sq) * (1.f / HD) + a.eps);
      if (live) {
      const size_t orow = (size_t)bh * Nout + tok;
      if (sub == 0 && a.mean) { a.mean[orow] = mean; a.rstd[orow] = rstd; }
      bf16_t* outp = (bf16_t*)a.out + orow * a.ld_out + c0;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        uint2 o;
        o.x = pack_bf16x2((acc[4 * u + 0] - mean) * rstd * gm[4 * u + 0] + bt[4 * u + 0], (acc[4 * u + 1] - mean) * rstd * gm[4 * u + 1] + bt[4 * u + 1]);
        o.y = pack_bf16x2((acc[4 * u + 2] - mean) * rstd * gm[4 * u + 2] + bt[4 * u + 2], (acc[4 * u + 3] - mean) * rstd * gm[4 * u + 3] + bt[4 * u + 3]);
        *(uint2*)(outp + 4 * u) = o;
      }
      if (a.pre) {
        bf16_t* prep = (bf16_t*)a.pre + orow * HD + c0;
#pragma unroll
        for (int u = 0; u < 3; ++u)
          *(uint2*)(prep + 4 * u) = make_uint2(pack_bf16x2(acc[4 * u], acc[4 * u + 1]), pack_bf16x2(acc[4 * u + 2], acc[4 * u + 3]));
      }
      if (a.mode == 1) {  // one-hot key coordinates [y | kh+x | kh+kw+t], zeros elsewhere (t = 0)
        const int extra = a.ld_out - HD, per = extra / 8;       // 4 or 8 columns per lane
        bf16_t* ex = (bf16_t*)a.out + orow * a.ld_out + HD + sub * per;
        for (int v4 = 0; v4 < per; v4 += 4) {
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = sub * per + v4 + e;
            o[e] = (is_patch && (j == py || j == Ho + px || j == Ho + Wo)) ? 1.f : 0.f;
          }
          *(uint2*)(ex + v4) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        }
      }
      }
    }
    FRSTAMP();
    it = nx;
  }
}

__global__ __launch_bounds__(FR_NT, 1) void pool_frame_fwd_kernel(PoolFrame3 g, int img_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_fr[];
  const int wg = blockIdx.x;
  const int which = (wg >= g.wg_first[1]) + (wg >= g.wg_first[2]);
  const svit_pool_args& a = g.p[which];
  const int first = wg - g.wg_first[which], step = g.wg_first[which + 1] - g.wg_first[which];
  const int s = a.stride_hw;
  if (s == 1) fr_run<1>(a, g.y_chunks[which], g.r_per[which], g.n_items[which], first, step, img_bytes, smem_fr);
  else if (s == 2) fr_run<2>(a, g.y_chunks[which], g.r_per[which], g.n_items[which], first, step, img_bytes, smem_fr);
  else fr_run<3>(a, g.y_chunks[which], g.r_per[which], g.n_items[which], first, step, img_bytes, smem_fr);
}

// ---------------------------------------------------------------------------------------
// query side of the decomposed relative-position bias
__global__ __launch_bounds__(256) void relq_fwd_kernel(svit_relq_args a) {
  const int extra = a.ld - HD;               // 32 or 64 columns
  const int Lq = a.qt * a.qh * a.qw, Nq = 1 + Lq + a.n_obj;
  const int J = a.kh + a.kw + a.kt;
  const int tok_per_block = 256 / extra;
  const int64_t total = (int64_t)a.B * a.heads * Nq;
  const int64_t row = (int64_t)blockIdx.x * tok_per_block + threadIdx.x / extra;
  const int j = threadIdx.x % extra;
  if (row >= total) return;
  bf16_t* qrow = (bf16_t*)a.qa + row * a.ld;
  const int tok = (int)(row % Nq);
  float val = 0.f;
  if (tok >= 1 && tok <= Lq && j < J) {
    const int p = tok - 1, x = p % a.qw, y = (p / a.qw) % a.qh, t = p / (a.qw * a.qh);
    const float* R;
    if (j < a.kh) R = a.rel_h + (size_t)a.idx_h[y * a.kh + j] * HD;
    else if (j < a.kh + a.kw) R = a.rel_w + (size_t)a.idx_w[x * a.kw + (j - a.kh)] * HD;
    else R = a.rel_t + (size_t)a.idx_t[t * a.kt + (j - a.kh - a.kw)] * HD;
#pragma unroll
    for (int v = 0; v < 12; ++v) {
      float f[8];
      unpack8(*(const uint4*)(qrow + v * 8), f);
      const float4 r0 = *(const float4*)(R + v * 8), r1 = *(const float4*)(R + v * 8 + 4);
      val += f[0] * r0.x + f[1] * r0.y + f[2] * r0.z + f[3] * r0.w + f[4] * r1.x + f[5] * r1.y +
             f[6] * r1.z + f[7] * r1.w;
    }
    val *= a.inv_scale;
  }
  qrow[HD + j] = f32_to_bf16(val);
}

// forward as a GEMM + gather: P = q . Rcat^T (svit_gemm_nt, all table rows at once), then each
// (query, j) picks P[query, section_row_offset + idx] -- 2 bytes read instead of a 96-long dot
__global__ __launch_bounds__(256) void relq_gather_kernel(svit_relq_gather_args a) {
  const int extra = a.ld - HD;
  const int Lq = a.qt * a.qh * a.qw, Nq = 1 + Lq + a.n_obj;
  const int J = a.kh + a.kw + a.kt;
  const int tok_per_block = 256 / extra;
  const int64_t total = (int64_t)a.B * a.heads * Nq;
  const int64_t row = (int64_t)blockIdx.x * tok_per_block + threadIdx.x / extra;
  const int j = threadIdx.x % extra;
  if (row >= total) return;
  const int tok = (int)(row % Nq);
  float val = 0.f;
  if (tok >= 1 && tok <= Lq && j < J) {
    const int p = tok - 1, x = p % a.qw, y = (p / a.qw) % a.qh, t = p / (a.qw * a.qh);
    int col;
    if (j < a.kh) col = a.row_h + a.idx_h[y * a.kh + j];
    else if (j < a.kh + a.kw) col = a.row_w + a.idx_w[x * a.kw + (j - a.kh)];
    else col = a.row_t + a.idx_t[t * a.kt + (j - a.kh - a.kw)];
    val = bf16_to_f32(((const bf16_t*)a.P)[row * a.ldp + col]) * a.inv_scale;
  }
  ((bf16_t*)a.qa)[row * a.ld + HD + j] = f32_to_bf16(val);
}

// backward as GEMMs: scatter d(relq) into the dense-but-sparse matrix D [tokens, Lpad] whose
// column sections are the rows of the h / w / t tables; then dR = D^T q (svit_gemm_tn) and
// dq = D R (svit_gemm_nt).  D is zero-filled by the same kernel.
__global__ __launch_bounds__(256) void relq_scatter_kernel(svit_relq_scatter_args a) {
  const int extra = a.ld - HD;
  const int Lq = a.qt * a.qh * a.qw, Nq = 1 + Lq + a.n_obj;
  const int J = a.kh + a.kw + a.kt;
  const int tok_per_block = 256 / extra;
  const int64_t total = (int64_t)a.B * a.heads * Nq;
  const int64_t row0 = (int64_t)blockIdx.x * tok_per_block;
  // the block's rows of D are one contiguous chunk: zero it with 16-byte stores, then scatter
  // (a row holds only J non-zeros at distinct columns)
  {
    const int64_t rows_here = min((int64_t)tok_per_block, total - row0);
    uint4* chunk = (uint4*)((bf16_t*)a.D + row0 * a.ldd);
    const int n16 = (int)(rows_here * a.ldd / 8);
    for (int i = threadIdx.x; i < n16; i += 256) chunk[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const int64_t row = row0 + threadIdx.x / extra;
  const int j = threadIdx.x % extra;
  if (row >= total || j >= J) return;
  const int tok = (int)(row % Nq);
  if (tok < 1 || tok > Lq) return;
  const int p = tok - 1, x = p % a.qw, y = (p / a.qw) % a.qh, t = p / (a.qw * a.qh);
  int col;
  if (j < a.kh) col = a.off_h + a.idx_h[y * a.kh + j];
  else if (j < a.kh + a.kw) col = a.off_w + a.idx_w[x * a.kw + (j - a.kh)];
  else col = a.off_t + a.idx_t[t * a.kt + (j - a.kh - a.kw)];
  const float d = bf16_to_f32(((const bf16_t*)a.dqa)[row * a.ld + HD + j]) * a.inv_scale;
  ((bf16_t*)a.D)[row * a.ldd + col] = f32_to_bf16(d);
}

__global__ __launch_bounds__(256) void relq_bwd_kernel(svit_relq_bwd_args a) {
  extern __shared__ __attribute__((aligned(16))) float tabs[];  // dRh | dRw | dRt
  float* th = tabs;
  float* tw = th + a.rows_h * HD;
  float* tt = tw + a.rows_w * HD;
  const int tab_n = (a.rows_h + a.rows_w + a.rows_t) * HD;
  for (int i = threadIdx.x; i < tab_n; i += blockDim.x) tabs[i] = 0.f;
  __syncthreads();
  const int Lq = a.qt * a.qh * a.qw, Nq = 1 + Lq + a.n_obj;
  const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;  // 8 tokens per block
  const int64_t total = (int64_t)a.B * a.heads * Nq;
  for (int64_t row = (int64_t)blockIdx.x * 8 + slot; row < total; row += (int64_t)gridDim.x * 8) {
    const int tok = (int)(row % Nq);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    if (tok >= 1 && tok <= Lq) {
      const int p = tok - 1, x = p % a.qw, y = (p / a.qw) % a.qh, t = p / (a.qw * a.qh);
      const bf16_t* qrow = (const bf16_t*)a.qa + row * a.ld;
      const bf16_t* drow = (const bf16_t*)a.dqa + row * a.ld + HD;
      const float q0 = bf16_to_f32(qrow[l32]), q1 = bf16_to_f32(qrow[l32 + 32]),
                  q2 = bf16_to_f32(qrow[l32 + 64]);
      for (int j = 0; j < a.kh; ++j) {
        const float d = bf16_to_f32(drow[j]) * a.inv_scale;
        const int r = a.idx_h[y * a.kh + j];
        const float* R = a.rel_h + (size_t)r * HD;
        o0 += d * R[l32]; o1 += d * R[l32 + 32]; o2 += d * R[l32 + 64];
        atomicAdd(&th[r * HD + l32], d * q0);
        atomicAdd(&th[r * HD + l32 + 32], d * q1);
        atomicAdd(&th[r * HD + l32 + 64], d * q2);
      }
      for (int j = 0; j < a.kw; ++j) {
        const float d = bf16_to_f32(drow[a.kh + j]) * a.inv_scale;
        const int r = a.idx_w[x * a.kw + j];
        const float* R = a.rel_w + (size_t)r * HD;
        o0 += d * R[l32]; o1 += d * R[l32 + 32]; o2 += d * R[l32 + 64];
        atomicAdd(&tw[r * HD + l32], d * q0);
        atomicAdd(&tw[r * HD + l32 + 32], d * q1);
        atomicAdd(&tw[r * HD + l32 + 64], d * q2);
      }
      for (int j = 0; j < a.kt; ++j) {
        const float d = bf16_to_f32(drow[a.kh + a.kw + j]) * a.inv_scale;
        const int r = a.idx_t[t * a.kt + j];
        const float* R = a.rel_t + (size_t)r * HD;
        o0 += d * R[l32]; o1 += d * R[l32 + 32]; o2 += d * R[l32 + 64];
        atomicAdd(&tt[r * HD + l32], d * q0);
        atomicAdd(&tt[r * HD + l32 + 32], d * q1);
        atomicAdd(&tt[r * HD + l32 + 64], d * q2);
      }
    }
    float* o = a.dq_extra + row * HD;
    o[l32] = o0; o[l32 + 32] = o1; o[l32 + 64] = o2;
  }
  __syncthreads();
  float* prow = a.workspace + (size_t)blockIdx.x * tab_n;
  for (int i = threadIdx.x; i < tab_n; i += blockDim.x) prow[i] = tabs[i];
}

#ifdef SVIT_POOL_STAMPS
__device__ unsigned long long g_pm_wg[4 * 2048];      // per workgroup of pool_mfma_fwd_kernel: start, end, kind, hw id
__device__ unsigned long long g_slab_stamps[16];
#define PSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (pst) g_slab_stamps[i] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PSTAMP(i) do {} while (0)
#endif
// ---------------------------------------------------------------------------------------
// MFMA stencil (round 4): the forward depthwise 3x3x3 conv of the small planes (W <= 14, T % 4 == 0, strides 1 / 2)
// on the matrix pipe, as banded-Toeplitz products of v_mfma_f32_4x4x4_16b_bf16 -- one wave-instruction = 16
// independent 4x4x4 products, one per CHANNEL (a depthwise conv mixes nothing across channels, which is why the big
// MFMA shapes do not apply and why the VALU forms above pay one instruction per MAC).  Per block (= channel):
//     D[i][j] += sum_k A[i][k] B[k][j]
//       i = 4 output positions along x,  k = 4 consecutive INPUT slots along x,  j = 4 t-planes of a "t-quad"
//       A = the (kt, ky) row of the channel's weights laid out as a band (Toeplitz) matrix: A[i][k] = w[kx(i, k)] or 0
//       B = 4 input slots x 4 planes, read with ONE ds_read_b64 per lane from a planar image [channel][plane][row][slot]
// 4 outputs x 3 taps need 6 inputs (stride 1) or 9 (stride 2), i.e. 2 or 3 k-steps: 12 of 32 / 48 products carry
// data -- 37 % / 25 % of a pipe that does 1024 MACs per 8 cycles per SIMD, against 64 useful MACs per 4-cycle
// v_dot2 of the slab kernel: ~3x the MACs per cycle, and no VALU work at all in the loop.
//   * LDS image: slot = x + 1 (slot 0 and the slots past W hold zeros = the conv's zero padding in x), 16 slots = 32
//     bytes per row, planes t = -1 .. T as zero halos (the 4 planes of a quad sit on different lanes, so the t boundary
//     cannot be a uniform branch; the y boundary can: a whole (kt, ky) row is skipped), channel stride padded so that
//     the 32 lanes of a ds_read_b64 half (8 channels x 4 planes) hit 32 different bank pairs.
//   * fill = the transpose: a lane fetches the 8 channels of TWO x-neighbours (16 bytes each, zeros outside the row)
//     and writes 8 dwords (x, x+1) -- slot pairs (2m, 2m+1) = x (2m-1, 2m), so the x halos are written by the fill.
//   * a workgroup = one (batch, head, tensor, 16-channel block), 4 waves; a wave takes (t-quad, output row) units,
//     keeps the Toeplitz fragments of all 9 (kt, ky) rows in 36 / 54 registers, and sends a finished unit through a
//     2-KiB LDS transpose so that `pre` gets 16-byte stores.  LayerNorm stays pool_slab_ln_kernel.
// Arithmetic: bf16 inputs and bf16-rounded weights (as the selector tables), fp32 accumulation in the order the
// matrix pipe adds (k ascending inside a product, products in (kt, ky, k-step) order): the same values as the slab
// kernel up to fp32 summation order.
__device__ __forceinline__ f32x4_t mfma4(s16x4_t a, s16x4_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, c, 0, 0, 0);
}
constexpr int PM_SLOTS = 16, PM_ROWB = PM_SLOTS * 2;          // slots / bytes per image row
constexpr int PM_NT = 512, PM_NW = PM_NT / 64;                  // threads / waves per workgroup: 4 waves per SIMD at 2 per CU
__host__ __device__ inline int pm_plane_bytes(int H) { return H * PM_ROWB; }
__host__ __device__ inline int pm_chan_bytes(int T, int H) { return (T + 2) * H * PM_ROWB + 8; }
__host__ __device__ inline size_t pm_lds_bytes(int T, int H) { return (size_t)16 * pm_chan_bytes(T, H) + PM_NW * 1024 + 64 + 16 * 27 * 4; }

// G = output groups of 4 along x that are computed (a group past the row multiplies zero slots; nothing of it is stored)
template <int S, int G>
__device__ __forceinline__ void pool_mfma_body(const svit_pool_args& a, int which, int bh, int cb, unsigned char* lds) {
  constexpr int NA = S == 1 ? 2 : 3;                 // Toeplitz fragments per (kt, ky) row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, H = a.H, W = a.W;
  const int Ho = pooled(H, S), Wo = pooled(W, S);
  const int L = T * H * W, Lo = T * Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int b = bh / a.heads, head = bh % a.heads;
  const int PP = pm_plane_bytes(H), CS = pm_chan_bytes(T, H);
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const bf16_t* src = (const bf16_t*)a.qkv + (size_t)b * N * tok_stride + ((size_t)which * a.heads + head) * HD + cb * 16;
  unsigned char* ostage = lds + 16 * CS;             // PM_NW x 1 KiB output transposes, then the object gains
  float* g_lds = (float*)(ostage + PM_NW * 1024);
#ifdef SVIT_POOL_STAMPS
  const bool pst = which == 0 && cb == 0 && bh == 3 && tid == 0;
#endif
  PSTAMP(8);

  // ---- requests first: the 16 x 27 weights of the channel block go to LDS (one coalesced load) while the image fills
  const int blk = lane >> 2, li = lane & 3;
  float* w_lds = g_lds + 16;
  if (tid < 16 * 27) w_lds[tid] = a.conv_w[(size_t)cb * 16 * 27 + tid];
  // ---- zero halo planes t = -1 and t = T of the 16 channels -------------------------------------------
  // (8-byte stores: the channel stride CS = (T + 2) * H * 32 + 8 is a multiple of 8, NOT of 16 -- the +8 skew that
  //  spreads a half-wave's channels over the bank pairs -- so a 16-byte store would be misaligned for odd channels)
  const int ppc = PP / 8;                            // 8-byte chunks per plane
  for (int i = tid; i < 16 * 2 * ppc; i += PM_NT) {
    const int c = i / (2 * ppc), r = i % (2 * ppc);
    *(uint2*)(lds + c * CS + (r < ppc ? 0 : (T + 1) * PP) + (r % ppc) * 8) = make_uint2(0u, 0u);
  }
  // ---- fill: task = (row of the volume, slot pair m, channel half); the loads of FB tasks per thread are requested
  // together (one memory round trip per batch instead of one per task) ------------------------------------------
  const int ntask = T * H * 16;
  const unsigned mH = fdiv_magic_dev(H);
  constexpr int FB = 4;
  for (int q0 = tid; q0 < ntask; q0 += FB * PM_NT) {
    uint4 v0[FB], v1[FB];
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      const int q = q0 + f * PM_NT;
      const int half = q & 1, m = (q >> 1) & 7, row = q >> 4;
      const int x0 = 2 * m - 1, x1 = 2 * m;
      v0[f] = make_uint4(0u, 0u, 0u, 0u);
      v1[f] = make_uint4(0u, 0u, 0u, 0u);
      if (q < ntask && x0 >= 0 && x0 < W) v0[f] = *(const uint4*)(src + (size_t)(1 + row * W + x0) * tok_stride + half * 8);
      if (q < ntask && x1 < W) v1[f] = *(const uint4*)(src + (size_t)(1 + row * W + x1) * tok_stride + half * 8);
    }
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      const int q = q0 + f * PM_NT;
      if (q >= ntask) break;
      const int half = q & 1, m = (q >> 1) & 7, row = q >> 4;
      const int t = fdiv(row, mH), y = row - t * H;
      unsigned char* dst = lds + (half * 8) * CS + (t + 1) * PP + y * PM_ROWB + m * 4;
      const uint32_t w0[4] = {v0[f].x, v0[f].y, v0[f].z, v0[f].w}, w1[4] = {v1[f].x, v1[f].y, v1[f].z, v1[f].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *(uint32_t*)(dst + (2 * e) * CS) = (w0[e] & 0xffffu) | (w1[e] << 16);
        *(uint32_t*)(dst + (2 * e + 1) * CS) = (w0[e] >> 16) | (w1[e] & 0xffff0000u);
      }
    }
  }
  PSTAMP(9);
  // ---- object gain of the 16 channels (closed form of the cube branch), read by the cls /
  // object pass at the end: written before the barrier -----------------------------------------------------------
  if (tid < 16) {
    float nt3[3], nh3[3], ipt, iph;
    obj_counts(1, nt3, &ipt);
    obj_counts(S, nh3, &iph);
    const float* cw = a.conv_w + (size_t)(cb * 16 + tid) * 27;
    float gsum = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) gsum += cw[k] * nt3[k / 9] * nh3[(k / 3) % 3] * nh3[k % 3];
    g_lds[tid] = gsum * ipt * iph * iph;
  }
  __syncthreads();
  // ---- Toeplitz fragments: lane 4 blk + i holds row i of the band matrices of channel blk ----------------
  s16x4_t afr[9][NA];
#pragma unroll
  for (int p = 0; p < 9; ++p) {
    const bf16_t w3[3] = {f32_to_bf16(w_lds[blk * 27 + p * 3]), f32_to_bf16(w_lds[blk * 27 + p * 3 + 1]),
                          f32_to_bf16(w_lds[blk * 27 + p * 3 + 2])};
#pragma unroll
    for (int n = 0; n < NA; ++n)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // input slot 4 (S g + n) + k against output position 4 g + li, whose first tap sits at slot S (4 g + li)
        const int kx = 4 * n + k - S * li;
        afr[p][n][k] = (short)((kx >= 0 && kx <= 2) ? w3[kx] : (bf16_t)0);
      }
  }
  PSTAMP(10);
  PSTAMP(11);

  // ---- units: (t-quad, output row) ---------------------------------------------------------------------------
  const unsigned lb = (unsigned)(blk * CS + li * PP);             // B operand: lane 4 blk + j reads plane j of the quad
  unsigned char* ost = ostage + wave * 1024;
  // transposed staging: [plane j (4)][x (8)][channel (16)] bf16 = 1 KiB, two x phases per unit; on the way out lane
  // (token = lane >> 1, half = lane & 1) owns one 16-byte chunk
  unsigned char* owr = ost + ((li * 8) * 16 + blk) * 2;
  const int o_tt = lane >> 1, o_half = lane & 1, o_jj = o_tt >> 3, o_x = o_tt & 7;
  const unsigned char* ord = ost + (o_tt * 16 + o_half * 8) * 2;
  bf16_t* pre = (bf16_t*)a.pre + ((size_t)bh * Nout + 1) * HD + cb * 16 + o_half * 8;
  const int nunit = (T >> 2) * Ho;
  int tq = 0, yo = wave;
  while (yo >= Ho) { yo -= Ho; ++tq; }
  for (int u = wave; u < nunit; u += PM_NW) {
    f32x4_t acc[G];
#pragma unroll
    for (int g2 = 0; g2 < G; ++g2) acc[g2] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // all 36 fragment reads of the unit are independent of the MFMAs: one basic block, no branch -- a (kt, ky) row
    // outside the plane (the conv's zero padding in y, uniform over the wave) reads the zero halo plane instead
    s16x4_t bf[9][4];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yi = S * yo + ky - 1;
        const bool ok = yi >= 0 && yi < H;
        const unsigned char* rowp = ok ? lds + lb + (4 * tq + kt) * PP + yi * PM_ROWB      // plane index = t + 1
                                       : lds + blk * CS;                                     // plane t = -1: zeros
#pragma unroll
        for (int m = 0; m < 4; ++m) bf[kt * 3 + ky][m] = *(const s16x4_t*)(rowp + 8 * m);
      }
#pragma unroll
    for (int p = 0; p < 9; ++p) {
      if constexpr (S == 1) {
#pragma unroll
        for (int g2 = 0; g2 < G; ++g2) acc[g2] = mfma4(afr[p][0], bf[p][g2], acc[g2]);
#pragma unroll
        for (int g2 = 0; g2 < G && g2 < 3; ++g2) acc[g2] = mfma4(afr[p][1], bf[p][g2 + 1], acc[g2]);
      } else {
#pragma unroll
        for (int g2 = 0; g2 < G; ++g2) acc[g2] = mfma4(afr[p][0], bf[p][2 * g2], acc[g2]);
#pragma unroll
        for (int g2 = 0; g2 < G; ++g2) acc[g2] = mfma4(afr[p][1], bf[p][2 * g2 + 1], acc[g2]);
        acc[0] = mfma4(afr[p][2], bf[p][2], acc[0]);
      }
    }
    // D[i][j]: lane 4 blk + j holds the outputs x = 4 g + i (register i) of plane 4 tq + j, channel blk.
    // Transpose through LDS, 8 x positions (two groups) per phase.
    bf16_t* prow = pre + (size_t)(((4 * tq + o_jj) * Ho + yo) * Wo) * HD;
#pragma unroll
    for (int ph = 0; ph < (G + 1) / 2; ++ph) {
#pragma unroll
      for (int g2 = 2 * ph; g2 < 2 * ph + 2 && g2 < G; ++g2)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *(bf16_t*)(owr + ((4 * (g2 - 2 * ph) + i) * 16) * 2) = f32_to_bf16(acc[g2][i]);
      asm volatile("" ::: "memory");     // (the wave's own LDS operations complete in order; keep the compiler's order too)
      const uint4 v = *(const uint4*)ord;
      const int xo = 8 * ph + o_x;
      if (xo < Wo) *(uint4*)(prow + (size_t)xo * HD) = v;
      asm volatile("" ::: "memory");
    }
    yo += PM_NW;
    while (yo >= Ho) { yo -= Ho; ++tq; }
  }
  PSTAMP(12);
  // ---- cls and object tokens: pre = x, x * g(w) ------------------------------------------------------------------
  for (int i = tid; i < (1 + a.n_obj) * 2; i += PM_NT) {
    const int idx = i >> 1, half = i & 1;
    const int tin = idx == 0 ? 0 : L + idx, tout = idx == 0 ? 0 : Lo + idx;
    float f[8];
    unpack8(*(const uint4*)(src + (size_t)tin * tok_stride + half * 8), f);
    if (idx > 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] *= g_lds[half * 8 + e];
    }
    *(uint4*)((bf16_t*)a.pre + ((size_t)bh * Nout + tout) * HD + cb * 16 + half * 8) = pack8(f);
  }
  PSTAMP(13);
}

struct PoolMfma3 { svit_pool_args p[3]; };
__global__ __launch_bounds__(PM_NT, 4) void pool_mfma_fwd_kernel(PoolMfma3 g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
  // 1-D grid, XCD-aware like the slab kernel: consecutive logical ids run on one XCD, and the six channel
  // blocks of a (batch, head, tensor) are consecutive logical ids -- they read interleaved 32-byte pieces of
  // the same lines.  Two kinds of workgroup: the q tensor (one fill, the long stride-1 sweep at blocks 4-13), and
  // k followed by v (two fills, two short sweeps): 2 x 6 x B x heads workgroups -- 384 at the 14x14 stage, ONE
  // round at two workgroups per CU (one workgroup per tensor gave 576: a second round for an eighth of them).
  const int nwg = gridDim.x, lin = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  int lg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int cb = lg % 6; lg /= 6;
  const int nbh = g.p[0].B * g.p[0].heads;
  const int bh = lg % nbh, kind = lg / nbh;
#ifdef SVIT_POOL_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    g_pm_wg[4 * blockIdx.x] = wall_clock64();
    g_pm_wg[4 * blockIdx.x + 2] = kind;
    g_pm_wg[4 * blockIdx.x + 3] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_ID
  }
#endif
  for (int which = kind; which <= 2 * kind; ++which) {         // kind 0: q; kind 1: k, v
    const svit_pool_args& a = g.p[which];
    if (which == 2) __syncthreads();                             // every wave is done with k's image
    const int Wo = pooled(a.W, a.stride_hw);
    if (a.stride_hw == 1) {
      if (Wo > 8) pool_mfma_body<1, 4>(a, which, bh, cb, pm_lds);
      else pool_mfma_body<1, 2>(a, which, bh, cb, pm_lds);
    } else {
      if (Wo > 4) pool_mfma_body<2, 2>(a, which, bh, cb, pm_lds);
      else pool_mfma_body<2, 1>(a, which, bh, cb, pm_lds);
    }
  }
#ifdef SVIT_POOL_STAMPS
  __syncthreads();
  if (threadIdx.x == 0 && blockIdx.x < 2048) g_pm_wg[4 * blockIdx.x + 1] = wall_clock64();
#endif
}

// ---------------------------------------------------------------------------------------
// Slab stencils (round 3): the forward depthwise conv of one (batch, head, tensor) for ONE group of
// 24 channels, with the input "slab" it needs (a range of t-planes and y-rows, every x; 48 bytes
// per token) resident in LDS.
//   * The slab is fetched ONCE with LDS-DMA (global_load_lds, 16 bytes per lane, lanes = (token,
//     chunk) so the LDS image is simply [token][24 channels]); the 27 taps are then LDS reads -- the
//     streaming kernels above pull every tap through the texture path (27x re-reads, rocprof round
//     2: 2.7x read amplification, the launches of the 14x14 stage 45 us for 45 MB).
//   * lane = output token, the workgroup = one channel group: the 24 x 27 selector weights are
//     uniform over the WHOLE workgroup and are read as scalar operands straight from the selector
//     table (svit_pool_weight_sel) -- no LDS traffic, no vector registers for weights; a tap costs
//     three conflict-free ds_read_b128 (consecutive tokens are 48 bytes apart: 16 lanes hit 16
//     distinct 16-byte slots of the bank row) and 24 v_dot2.  ~75 VGPRs: 6 waves per SIMD.
//   * LayerNorm(96) spans four channel groups, i.e. four workgroups: the conv writes `pre` (the
//     bf16 pre-LN value, saved for the backward anyway) and a second, row-wise launch
//     (pool_slab_ln_kernel -> pool_ln_finish) normalises.  The tap order and the arithmetic are those
//     of pool_ln_fwd_body: the results are bit-identical to the streaming kernel's.
struct SlabPlan { int on, TC, YC, nt, ny; };
constexpr int SLAB_NT = 1024;                 // threads per slab workgroup: every wave does at most one 64-token unit
struct PoolSlab3 { svit_pool_args p[3]; SlabPlan plan[3]; const uint32_t* sel[3]; int max_chunks; };
constexpr int SLAB_MAXTOK = 1600;

__global__ __launch_bounds__(SLAB_NT) void pool_slab_fwd_kernel(PoolSlab3 g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char slab[];
  // 1-D grid, XCD-aware: consecutive logical ids run on ONE XCD, and the four channel groups of a slab
  // are consecutive logical ids -- they read interleaved 48-byte pieces of the same 128-byte lines, which
  // then come from HBM once and from that XCD's L2 three times (dealt round-robin the four landed on
  // four XCDs: 3.3x over-fetch, the 14x14 launch 30 us instead of ~12)
  const int nwg = gridDim.x, lin = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  int lg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int cg = lg & 3; lg >>= 2;
  const int wg = lg % g.max_chunks; lg /= g.max_chunks;
  const int which = lg % 3, bh = lg / 3;
  const svit_pool_args& a = g.p[which];
  const SlabPlan& pl = g.plan[which];
  if (!pl.on || wg >= pl.nt * pl.ny) return;
  const int tid = threadIdx.x, wave = tid >> 6;
#ifdef SVIT_POOL_STAMPS
  const bool pst = which == 0 && cg == 0 && wg == 0 && bh == 3 && tid == 0;
#endif
  PSTAMP(0);
  const int s = a.stride_hw, T = a.T, H = a.H, W = a.W;
  const int Ho = pooled(H, s), Wo = pooled(W, s);
  const int L = T * H * W, Lo = T * Ho * Wo;
  const int N = 1 + L + a.n_obj, Nout = 1 + Lo + a.n_obj;
  const int b = bh / a.heads, head = bh % a.heads;
  const int tci = wg / pl.ny, yci = wg % pl.ny;
  const int to0 = tci * pl.TC, to1 = min(T, to0 + pl.TC);          // output planes
  const int yo0 = yci * pl.YC, yo1 = min(Ho, yo0 + pl.YC);         // output rows
  const int t_lo = max(0, to0 - 1), t_hi = min(T, to1 + 1);        // input slab, clipped to the volume
  const int y_lo = max(0, s * yo0 - 1), y_hi = min(H, s * (yo1 - 1) + 2);
  const int RT = t_hi - t_lo, RY = y_hi - y_lo, ntok = RT * RY * W;
  const size_t tok_stride = (size_t)3 * a.heads * HD;
  const bf16_t* src = (const bf16_t*)a.qkv + (size_t)b * N * tok_stride + ((size_t)which * a.heads + head) * HD + cg * 24;
  // ---- fill: chunk q = 16 bytes at LDS offset 16 q = channels 8 (q % 3) .. of slab token q / 3
  const int nchunks = ntok * 3;
  const unsigned mW = fdiv_magic_dev(W), mRY = fdiv_magic_dev(RY), mWo = fdiv_magic_dev(Wo);
  for (int q0 = 0; q0 < nchunks; q0 += SLAB_NT) {
    if (q0 + wave * 64 >= nchunks) break;          // (whole wave past the end: nothing to fetch)
    const int q = min(q0 + tid, nchunks - 1);      // lanes past the end re-read the last chunk (into the pad)
    const int j = fdiv(q, 0x55555556u), ch = q - 3 * j;
    size_t tok;
    if (RY == H) {                 // whole planes (what plan_slab picks): slab tokens are consecutive input tokens
      tok = 1 + (size_t)t_lo * H * W + j;
    } else {
      const int r = fdiv(j, mW), xj = j - r * W, tj = fdiv(r, mRY), yj = r - tj * RY;
      tok = 1 + (size_t)((t_lo + tj) * H + (y_lo + yj)) * W + xj;
    }
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(src + tok * tok_stride + ch * 8),
        (__attribute__((address_space(3))) void*)(slab + (size_t)(q0 + wave * 64) * 16), 16, 0, 0);
  }
  PSTAMP(1);
  const int zero_off = ((nchunks * 16 + 1023) / 1024) * 1024;      // behind the image, padded to whole wave-instructions
  if (tid < 3) *(uint4*)(slab + zero_off + tid * 16) = make_uint4(0, 0, 0, 0);
  float* g_lds = (float*)(slab + zero_off + 64);                   // object gain of the 24 channels
  if (wg == 0 && tid < 24) {     // (27 independent loads per thread: one memory round trip)
    float nt3[3], nh3[3], ipt, iph;
    obj_counts(1, nt3, &ipt);
    obj_counts(s, nh3, &iph);
    const float* cw = a.conv_w + (size_t)(cg * 24 + tid) * 27;
    float gsum = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) gsum += cw[k] * nt3[k / 9] * nh3[(k / 3) % 3] * nh3[k % 3];
    g_lds[tid] = gsum * ipt * iph * iph;
  }
  PSTAMP(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PSTAMP(3);
  __syncthreads();
  PSTAMP(4);

  // selector dwords [27][96] read through the constant address space: uniform addresses there
  // become s_load (scalar operands of the v_dot2), not vector loads
  typedef const __attribute__((address_space(4))) uint32_t* cptr_t;
  const cptr_t selw = (cptr_t)(g.sel[which] + cg * 24);
  const int ny_o = yo1 - yo0, n_out = (to1 - to0) * ny_o * Wo;
  bf16_t* pre = (bf16_t*)a.pre + ((size_t)bh * Nout + 1) * HD + cg * 24;
  const unsigned mNY = fdiv_magic_dev(ny_o);
  for (int o = tid; o < n_out; o += SLAB_NT) {
    const int r = fdiv(o, mWo), xo = o - r * Wo, tq = fdiv(r, mNY), yo = yo0 + r - tq * ny_o, to = to0 + tq;
    const int yi = s * yo, xi = s * xo;
    bool vx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vx[k] = xi - 1 + k >= 0 && xi - 1 + k < W;
    const int ib = ((to - 1 - t_lo) * RY + (yi - 1 - y_lo)) * W + (xi - 1);
    float acc[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0.f;
    // (kt, ky) stay loops: one row of three taps = 72 scalar weights at a time
#pragma unroll 1
    for (int kt = 0; kt < 3; ++kt) {
      const bool vtk = to - 1 + kt >= 0 && to - 1 + kt < T;
#pragma unroll 1
      for (int ky = 0; ky < 3; ++ky) {
        const bool vyk = vtk && yi - 1 + ky >= 0 && yi - 1 + ky < H;
        const int rowoff = ib + (kt * RY + ky) * W;
        const cptr_t wrow = selw + (kt * 3 + ky) * 3 * HD;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool ok = vyk && vx[kx];
          const int off = ok ? (rowoff + kx) * 48 : zero_off;
          const uint4 v0 = *(const uint4*)(slab + off), v1 = *(const uint4*)(slab + off + 16),
                      v2 = *(const uint4*)(slab + off + 32);
          const cptr_t w = wrow + kx * HD;
          acc[0] = dot2_sel(v0.x, w[0], acc[0]);   acc[1] = dot2_sel(v0.x, w[1], acc[1]);
          acc[2] = dot2_sel(v0.y, w[2], acc[2]);   acc[3] = dot2_sel(v0.y, w[3], acc[3]);
          acc[4] = dot2_sel(v0.z, w[4], acc[4]);   acc[5] = dot2_sel(v0.z, w[5], acc[5]);
          acc[6] = dot2_sel(v0.w, w[6], acc[6]);   acc[7] = dot2_sel(v0.w, w[7], acc[7]);
          acc[8] = dot2_sel(v1.x, w[8], acc[8]);   acc[9] = dot2_sel(v1.x, w[9], acc[9]);
          acc[10] = dot2_sel(v1.y, w[10], acc[10]); acc[11] = dot2_sel(v1.y, w[11], acc[11]);
          acc[12] = dot2_sel(v1.z, w[12], acc[12]); acc[13] = dot2_sel(v1.z, w[13], acc[13]);
          acc[14] = dot2_sel(v1.w, w[14], acc[14]); acc[15] = dot2_sel(v1.w, w[15], acc[15]);
          acc[16] = dot2_sel(v2.x, w[16], acc[16]); acc[17] = dot2_sel(v2.x, w[17], acc[17]);
          acc[18] = dot2_sel(v2.y, w[18], acc[18]); acc[19] = dot2_sel(v2.y, w[19], acc[19]);
          acc[20] = dot2_sel(v2.z, w[20], acc[20]); acc[21] = dot2_sel(v2.z, w[21], acc[21]);
          acc[22] = dot2_sel(v2.w, w[22], acc[22]); acc[23] = dot2_sel(v2.w, w[23], acc[23]);
        }
      }
    }
    bf16_t* dst = pre + (size_t)((to * Ho + yo) * Wo + xo) * HD;
    *(uint4*)(dst) = pack8(&acc[0]);
    *(uint4*)(dst + 8) = pack8(&acc[8]);
    *(uint4*)(dst + 16) = pack8(&acc[16]);
  }
  PSTAMP(5);
  // ---- cls and object tokens (first workgroup of the tensor): pre = x, x * g(w) (the closed form
  // of the cube branch), 8 channels per thread
  if (wg == 0) {
    for (int i = tid; i < (1 + a.n_obj) * 3; i += SLAB_NT) {
      const int idx = i / 3, ch = i - 3 * idx;
      const int tin = idx == 0 ? 0 : L + idx, tout = idx == 0 ? 0 : Lo + idx;
      float f[8];
      unpack8(*(const uint4*)(src + (size_t)tin * tok_stride + ch * 8), f);
      if (idx > 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= g_lds[ch * 8 + e];
      }
      *(uint4*)((bf16_t*)a.pre + ((size_t)bh * Nout + tout) * HD + cg * 24 + ch * 8) = pack8(f);
    }
  }
  PSTAMP(6);
}
#ifdef SVIT_POOL_STAMPS
extern "C" int svit_debug_pool_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_slab_stamps), sizeof(unsigned long long) * n);
}
extern "C" int svit_debug_pool_wg_times(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pm_wg), sizeof(unsigned long long) * n);
}
extern "C" int svit_debug_pool_bwd_wg_times(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pf_wg), sizeof(unsigned long long) * n);
}
extern "C" int svit_debug_pool_frame_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_fr_st), sizeof(unsigned long long) * n);
}
#endif

// LayerNorm(96) + one-hot key coordinates over the `pre` rows the slab conv wrote (pool_ln_finish).
// For the q tensor with relq_R set, the rel-pos query-side columns ride along (svit_pool_args.relq_*): the 64
// normalised rows of a pass stay in LDS as bf16, the four waves multiply them with the concatenated tables on
// the matrix pipe (P = q . R^T, table fragments straight from L2, swapped operands: a lane owns a token), P goes
// back through LDS rounded to bf16, and every (token, j) picks its table row through the map -- the same two
// roundings as svit_gemm_nt + SVIT_EPI_RELQ, which this replaces for the slab blocks.
constexpr int SLN_QROW = 208;      // LDS bytes per staged q row (192 + 16 pad)
__global__ __launch_bounds__(256) void pool_slab_ln_kernel(PoolSlab3 g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sln[];
  const int which = blockIdx.z;
  if (!g.plan[which].on) return;
  svit_pool_args a = g.p[which];
  const int s = a.stride_hw, Ho = pooled(a.H, s), Wo = pooled(a.W, s), Lo = a.T * Ho * Wo;
  const int Nout = 1 + Lo + a.n_obj, bh = blockIdx.y;
  const bf16_t* prep = (const bf16_t*)a.pre;
  a.pre = nullptr;                                  // (do not write back what is being read)
  const int sub = threadIdx.x & 3, c0 = sub * 24, tl = threadIdx.x >> 2;
  const bool relq = which == 0 && a.relq_R != nullptr;     // (uniform over the block)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
  const int lpad = a.relq_lpad, extra = a.ld_out - HD, per = extra >> 2;    // rel-pos columns per lane: 8 or 16
  unsigned char* qt = sln;                                   // [64][SLN_QROW] bf16 rows
  bf16_t* pt_ = (bf16_t*)(sln + 64 * SLN_QROW);              // [64][lpad] bf16 products
  bf16x8_t rf0[6];                                          // table fragments of this wave's first table block
  if (relq) {
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
      rf0[ks] = (wave << 5) < lpad ? *(const bf16x8_t*)((const bf16_t*)a.relq_R + (size_t)(wave * 32 + l31) * HD + 16 * ks + 8 * hh)
                                   : bf16x8_t{};
  }
  for (int tb = blockIdx.x; tb * 64 < Nout; tb += gridDim.x) {
    const int tok = tb * 64 + tl;
    const bool live = tok < Nout;
    float acc[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0.f;
    int py = 0, px = 0, pt = 0;
    bool is_patch = false;
    int4 mp[4];                                      // this lane's map entries, requested before the LayerNorm
    if (relq) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        mp[v] = (live && v * 4 < per) ? *(const int4*)(a.relq_map + (size_t)tok * extra + sub * per + v * 4)
                                      : make_int4(-1, -1, -1, -1);
    }
    if (live) {
      const bf16_t* p = prep + ((size_t)bh * Nout + tok) * HD + c0;
#pragma unroll
      for (int v = 0; v < 3; ++v) unpack8(*(const uint4*)(p + v * 8), &acc[v * 8]);
      if (tok >= 1 && tok <= Lo) {
        is_patch = true;
        const int q = tok - 1;
        px = q % Wo; py = (q / Wo) % Ho; pt = q / (Wo * Ho);
      }
    }
    if (relq) {
      __syncthreads();                              // the previous pass's readers are done with the tiles
      if (!live) {
#pragma unroll
        for (int v = 0; v < 3; ++v) *(uint4*)(qt + tl * SLN_QROW + (c0 + v * 8) * 2) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    pool_ln_finish(a, acc, live, tok, is_patch, py, px, pt, bh, Nout, Ho, Wo,
                   relq ? (bf16_t*)(qt + tl * SLN_QROW) : nullptr);
    if (!relq) continue;
    __syncthreads();
    // P[token, table row] for the 64 tokens: 2 token blocks x lpad/32 table blocks of 32 x 32, 6 k-steps each.
    // A wave owns table blocks (wave, wave + 4, ...) and both token blocks of each; the fragments of its FIRST
    // table block are pass-invariant and stay in registers (rf0, loaded once in front of the loop).
    const int ncb = lpad >> 5;
    const bf16_t* R = (const bf16_t*)a.relq_R;
    for (int cb = wave; cb < ncb; cb += 4) {
      bf16x8_t rf[6];
#pragma unroll
      for (int ks = 0; ks < 6; ++ks)
        rf[ks] = cb == wave ? rf0[ks] : *(const bf16x8_t*)(R + (size_t)(cb * 32 + l31) * HD + 16 * ks + 8 * hh);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        f32x16_t c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
          const bf16x8_t qf = *(const bf16x8_t*)(qt + (rb * 32 + l31) * SLN_QROW + (16 * ks + 8 * hh) * 2);
          c = mfma32(rf[ks], qf, c);                // c[r] = P[token rb*32 + l31][table row cb*32 + acc_row(r)]
        }
        bf16_t* prow = pt_ + (size_t)(rb * 32 + l31) * lpad + cb * 32 + 4 * hh;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          uint2 pk;
          pk.x = pack_bf16x2(c[4 * gq], c[4 * gq + 1]);
          pk.y = pack_bf16x2(c[4 * gq + 2], c[4 * gq + 3]);
          *(uint2*)(prow + 8 * gq) = pk;
        }
      }
    }
    __syncthreads();
    if (live) {
      bf16_t* ex = (bf16_t*)a.out + ((size_t)bh * Nout + tok) * a.ld_out + HD + sub * per;
      const bf16_t* prow = pt_ + (size_t)tl * lpad;
#pragma unroll
      for (int v8 = 0; v8 < 2; ++v8) {
        if (v8 * 8 >= per) break;
        const int cc[8] = {mp[2 * v8].x, mp[2 * v8].y, mp[2 * v8].z, mp[2 * v8].w,
                           mp[2 * v8 + 1].x, mp[2 * v8 + 1].y, mp[2 * v8 + 1].z, mp[2 * v8 + 1].w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = cc[e] < 0 ? 0.f : bf16_to_f32(prow[cc[e]]) * a.relq_scale;
        *(uint4*)(ex + v8 * 8) = pack8(o);
      }
    }
  }
}
}  // namespace

// grid.x of the persistent stencil kernels: token blocks are dealt round-robin to workgroups so
// that about 1024 workgroups (2 per CU on two resident rounds) exist in total
static unsigned persistent_x(int token_blocks, int other_dims, long want_override = 0) {
  const long want = want_override > 0 ? want_override : 1024;      // (512 / 1024 / 2048 swept inside the step in round 4)
  const long total = (long)token_blocks * other_dims;
  const long chunks = (total + want - 1) / want;
  long x = (token_blocks + chunks - 1) / chunks;
  if (x < 1) x = 1;
  return (unsigned)x;
}

static int check_pool_dims(int B, int heads, int T, int H, int W, int n_obj, int s) {
  if (B <= 0 || heads <= 0 || T <= 0 || H <= 0 || W <= 0 || n_obj < 0 || s < 1) return SVIT_ERR_SHAPE;
  return SVIT_OK;
}

// pooled plane and token count of one tensor: Nout = 1 (cls) + T * Ho * Wo + n_obj
struct PoolOut { int Ho, Wo, Nout; };
static PoolOut pool_out(int T, int H, int W, int n_obj, int s) {
  const int Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
  return {Ho, Wo, 1 + T * Ho * Wo + n_obj};
}
static PoolOut pool_out(const svit_pool_args& a) { return pool_out(a.T, a.H, a.W, a.n_obj, a.stride_hw); }

static int check_pool_fwd(const svit_pool_args* a) {
  if (!a->qkv || !a->conv_w || !a->gamma || !a->beta || !a->out) return SVIT_ERR_ARG;
  if ((a->pre == nullptr) != (a->mean == nullptr) || (a->mean == nullptr) != (a->rstd == nullptr))
    return SVIT_ERR_ARG;     // the saved-for-backward trio is all-or-nothing
  if (int rc = check_pool_dims(a->B, a->heads, a->T, a->H, a->W, a->n_obj, a->stride_hw)) return rc;
  if (a->which < 0 || a->which > 2 || a->ld_out < HD || a->ld_out % 8 != 0) return SVIT_ERR_ARG;
  if (a->mode == 1) {
    const PoolOut o = pool_out(*a);
    const int extra = a->ld_out - HD;
    if (extra % 32 != 0 || extra < o.Ho + o.Wo + a->T) return SVIT_ERR_SHAPE;
  }
  return SVIT_OK;
}

extern "C" int svit_pool_ln_fwd(const svit_pool_args* a, void* stream) {
  if (!a || !a->pre || !a->mean || !a->rstd) return SVIT_ERR_ARG;      // (the single-tensor kernel always saves the trio)
  if (int rc = check_pool_fwd(a)) return rc;
  hipLaunchKernelGGL(pool_ln_fwd_kernel, dim3(persistent_x((pool_out(*a).Nout + 63) / 64, a->B * a->heads),
                                              a->B * a->heads), dim3(256), 0, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

// What the host decides from, for a q / k / v pooling call: plain integers, filled from the argument blocks (pool_geom) or by
// the plan query (svit_debug_pool_plan).  T / H / W / n_obj are per tensor because the forward entry points have never
// refused tensors that differ in them; every caller passes one volume three times.
struct PoolGeom {
  int B, heads, T[3], H[3], W[3], n_obj[3], s[3];
  int pre[3];        // the tensor saves pre / mean / rstd
  int sel;           // selector tables were given
  int relq_lpad;     // q's rel-pos columns are wanted: rows of the concatenated tables (svit_pool_args.relq_lpad), else 0
};
static PoolGeom pool_geom(int B, int heads, int T, int H, int W, int n_obj, int sq, int sk, int sv) {
  PoolGeom g = {};
  g.B = B; g.heads = heads;
  for (int i = 0; i < 3; ++i) { g.T[i] = T; g.H[i] = H; g.W[i] = W; g.n_obj[i] = n_obj; g.s[i] = i == 0 ? sq : i == 1 ? sk : sv; }
  return g;
}
static PoolGeom pool_geom(const svit_pool_args* a3, bool sel) {
  PoolGeom g = {};
  g.B = a3[0].B; g.heads = a3[0].heads;
  for (int i = 0; i < 3; ++i) {
    g.T[i] = a3[i].T; g.H[i] = a3[i].H; g.W[i] = a3[i].W; g.n_obj[i] = a3[i].n_obj; g.s[i] = a3[i].stride_hw;
    g.pre[i] = a3[i].pre != nullptr;
  }
  g.sel = sel;
  g.relq_lpad = a3[0].relq_R ? a3[0].relq_lpad : 0;
  return g;
}
static PoolGeom pool_geom(const svit_pool_dgrad_args* d3) {
  return pool_geom(d3[0].B, d3[0].heads, d3[0].T, d3[0].H, d3[0].W, d3[0].n_obj, d3[0].stride_hw, d3[1].stride_hw, d3[2].stride_hw);
}
static PoolOut pool_out(const PoolGeom& g, int i) { return pool_out(g.T[i], g.H[i], g.W[i], g.n_obj[i], g.s[i]); }

// plan of the LDS-tiled stride-1 stencil for one tensor (see pool_tiled_body)
static PoolTilePlan plan_tiled(int T, int H, int W, int n_obj, int bh) {
  PoolTilePlan pl;
  const int TX = W > 8 ? 16 : 8, TY = W > 8 ? 4 : 8;
  pl.tiled = 1;
  pl.tiles_x = (W + TX - 1) / TX;
  pl.tiles_y = (H + TY - 1) / TY;
  int tch = 1;           // cut the t walk while the (y, x) tiling alone leaves CUs idle
  while (tch * 2 <= T && (long)pl.tiles_x * pl.tiles_y * tch * bh < 384 && T / (tch * 2) >= 1) tch *= 2;
  pl.tch = tch;
  pl.tlen = (T + tch - 1) / tch;
  pl.n_wgs = pl.tiles_x * pl.tiles_y * tch;
  pl.n_special = (1 + n_obj + 63) / 64;
  return pl;
}
static size_t tiled_lds_bytes(int W) {
  const int htok = W > 8 ? 6 * 18 : 10 * 10;
  return 512 * sizeof(float) + 3 * (size_t)htok * TL_ROW;
}

// Slab plan of one tensor (pool_slab_fwd_kernel): output t-planes (TC) x output rows (YC) per
// workgroup such that the input slab -- min(T, TC + 2) planes x min(H, s (YC - 1) + 3) rows x W --
// fits SLAB_MAXTOK tokens; among those the one that re-reads the input least, then cut in t until the
// launch has >= 256 workgroups.  Strides 1 and 2 only (a stride-4 / -8 stencil touches a small part
// of the planes a slab would load), and only where `pre` is given (the LayerNorm launch reads it).
// SVIT_K_POOL_FWD of the knob table (common.h): 0 = streaming kernels, 1 = VALU slab conv, 2 = MFMA conv where it is ahead,
// 3 = MFMA conv wherever its geometry holds.  Whole planes only: the y-chunked planner for 28x28 planes (rounds 3-4)
// measured level with the streaming kernel inside the step (profiles/r04_in_step_sweeps.txt) and was removed in round 5.
static SlabPlan plan_slab(const PoolGeom& g, int i) {
  SlabPlan pl = {0, 0, 0, 0, 0};
  const int s = g.s[i], T = g.T[i], H = g.H[i], W = g.W[i];
  // measured (tools/pool_one.py under rocprofv3, profiles/r03_pool_slab.txt): ahead of the streaming
  // kernel on the 14x14 and 7x7 planes (12 of 16 blocks), behind it on 28x28 and behind the tiled
  // stencil on 56x56 -- the conv phase is VALU-bound (27 v_dot2 per output channel) and a slab
  // workgroup serialises fill -> conv -> store with one 16-wave workgroup per CU (106 SGPRs)
  if (!svit_knob(SVIT_K_POOL_FWD) || s > 2 || !g.pre[i] || H * W > 196) return pl;
  const PoolOut o = pool_out(g, i);
  double best = 1e30;
  const int yc = o.Ho;                          // whole planes: the planes this path is used on (<= 14x14) fit
  for (int tc = 1; tc <= T; ++tc) {
    const int pin = std::min(T, tc + 2), rin = std::min(H, s * (yc - 1) + 3);
    if ((long)pin * rin * W > SLAB_MAXTOK) continue;
    const double cost = ((double)pin / tc) * ((double)rin / (s * yc)) - 1e-6 * tc * yc;
    if (cost < best) { best = cost; pl.TC = tc; pl.YC = yc; }
  }
  if (pl.TC == 0) return pl;
  pl.ny = (o.Ho + pl.YC - 1) / pl.YC;
  // at most one 64-token unit per wave (the conv phase of a workgroup is then ONE pass of ~750 VALU
  // instructions per wave), then cut in t until the tensor alone gives the chip >= 128 workgroups
  while (pl.TC > 1 && (long)pl.TC * pl.YC * o.Wo > SLAB_NT) pl.TC = (pl.TC + 1) / 2;
  while (pl.TC > 1 && (long)((T + pl.TC - 1) / pl.TC) * pl.ny * g.B * g.heads * 4 < 128) pl.TC = (pl.TC + 1) / 2;
  pl.nt = (T + pl.TC - 1) / pl.TC;
  pl.on = 1;
  return pl;
}

// The LDS-staged kernels address a clip of qkv / dqkv through a buffer descriptor: num_records = the clip's bytes as an int,
// per-lane 32-bit byte offsets, 0x7ffffff0 as the "past the end" sentinel.  A clip that large takes the 64-bit streaming paths.
static bool pool_clip_span_ok(int T, int H, int W, int n_obj, int heads) {
  const size_t span = (size_t)(1 + (size_t)T * H * W + n_obj) * 3 * heads * HD * 2;
  return span < 0x7ffffff0u;
}
// ---- chunk plans of the two LDS-staged kernels (pool_fwd_staged_kernel, pool_bwd_fused_kernel) ----
// Both cut every tensor into chunks of n planes x r rows: an item (one per batch*head, tensor, channel group, t-chunk, y-chunk)
// stages the (n + 2)-plane image of its chunk in LDS.  One search picks (n, r) for q and one pair for k and v together (same
// stride in every block of the model) so that the items are about equally long and fill the chip's slots.  Estimate of the
// launch = the longest item if everything is resident at once, else the average load of a slot plus half an item.  What
// differs between the kernels comes in as a model: the row extent and stride class per tensor, lds_of(i, n, r), item_us(i, n, r),
// cost(i, plan, t_chunks, y_chunks, &sum, &longest) and admit(q's plan, kv's plan).
struct PfTensorPlan { int n, r; };
struct PoolChunkPlan {
  int ok;
  int n_per[3], r_per[3];        // planes / rows per chunk, per tensor
  int t_chunks[3], y_chunks[3];  // chunks along t / y
  int order[3], first_item[4];   // tensors in launch order (longest items first: the dispatcher fills the second slot of every
                                 //  CU with the shorter ones) / item ranges of order[0..2]
  int lds, max_chunks;           // dynamic LDS bytes of the launch / max over the tensors of t_chunks * y_chunks
};
template <class K> static void chunk_plan_into(const PoolChunkPlan& p, K* k) {
  for (int i = 0; i < 3; ++i) {
    k->n_per[i] = p.n_per[i]; k->r_per[i] = p.r_per[i]; k->t_chunks[i] = p.t_chunks[i]; k->y_chunks[i] = p.y_chunks[i];
    k->order[i] = p.order[i];
  }
  for (int j = 0; j < 4; ++j) k->first_item[j] = p.first_item[j];
}

template <class M> static PoolChunkPlan pool_chunk_search(const M& m, int T, int BH, size_t lds_max, size_t lds_min, double slots) {
  PoolChunkPlan p = {};
  // candidate (n, r) per tensor: every n, r = ceil(extent / k)
  auto candidates = [&](int i, std::vector<PfTensorPlan>* out) {
    for (int n = 1; n <= T; ++n) {
      int last_r = -1;
      for (int k = 1; k <= m.ext[i]; ++k) {
        const int r = (m.ext[i] + k - 1) / k;
        if (r == last_r) continue;
        last_r = r;
        if (m.lds_of(i, n, r) <= lds_max) out->push_back({n, r});
      }
    }
  };
  std::vector<PfTensorPlan> cq, c1, c2, ckv;
  candidates(0, &cq);
  candidates(1, &c1);
  candidates(2, &c2);
  for (const auto& x : c1)
    for (const auto& y : c2)
      if (x.n == y.n && x.r == y.r) ckv.push_back(x);
  if (m.cls[1] != m.cls[2] || m.ext[1] != m.ext[2]) ckv = c1.size() < c2.size() ? c1 : c2;      // (not the model's case: take the tighter list)
  if (cq.empty() || ckv.empty()) return p;
  double best = 1e300;
  PfTensorPlan bq = cq[0], bkv = ckv[0];
  for (const auto& pq : cq)
    for (const auto& pkv : ckv) {
      const PfTensorPlan pl[3] = {pq, pkv, pkv};
      double items = 0, sum = 0, longest = 0;
      bool fits = true;
      for (int i = 0; i < 3 && fits; ++i) {
        if (m.lds_of(i, pl[i].n, pl[i].r) > lds_max) { fits = false; break; }
        const int tc = (T + pl[i].n - 1) / pl[i].n, yc = (m.ext[i] + pl[i].r - 1) / pl[i].r;
        items += 3.0 * BH * tc * yc;
        m.cost(i, pl[i], tc, yc, &sum, &longest);
      }
      if (!fits || !m.admit(pq, pkv)) continue;
      const double est = items <= slots ? std::max(longest, sum / slots) : sum / slots + 0.5 * longest;
      if (est < best) { best = est; bq = pq; bkv = pkv; }
    }
  if (best >= 1e300) return p;
  const PfTensorPlan pl[3] = {bq, bkv, bkv};
  size_t lds = lds_min;
  double len[3];
  p.max_chunks = 1;
  for (int i = 0; i < 3; ++i) {
    p.n_per[i] = pl[i].n;
    p.r_per[i] = pl[i].r;
    p.t_chunks[i] = (T + pl[i].n - 1) / pl[i].n;
    p.y_chunks[i] = (m.ext[i] + pl[i].r - 1) / pl[i].r;
    p.max_chunks = std::max(p.max_chunks, p.t_chunks[i] * p.y_chunks[i]);
    lds = std::max(lds, m.lds_of(i, pl[i].n, pl[i].r));
    len[i] = m.item_us(i, pl[i].n, pl[i].r);
  }
  int ord[3] = {0, 1, 2};
  std::sort(ord, ord + 3, [&](int x, int y) { return len[x] > len[y] || (len[x] == len[y] && x < y); });
  int first = 0;
  for (int j = 0; j < 3; ++j) {
    p.order[j] = ord[j];
    p.first_item[j] = first;
    first += 3 * BH * p.t_chunks[ord[j]] * p.y_chunks[ord[j]];
  }
  p.first_item[3] = first;
  p.lds = (int)lds;
  p.ok = 1;
  return p;
}

// Staged conv forward: output planes (n) and output rows (r) per chunk so that (n + 2) planes of the r-row image fit LDS.
// Item time: staging 3 us + 0.08 us per 1-KiB piece and wave, 0.27 us per 16-output step (27 reads + 54 dot2), ~1 us of tail.
#ifndef SVIT_PS_LDS_KB      // LDS budget of a staged-forward workgroup / resident workgroups the planner counts on.  Swept in
#define SVIT_PS_LDS_KB 79   // diagnostic builds (profiles/r05_pool_fwd_staged.txt): 256 threads x 52 KB x 3 per CU 255 us over blocks 0-3,
#define SVIT_PS_SLOTS 512   // 256 x 79 KB x 2: 238, 512 x 79 KB x 2: 232 (default), 1024 x 156 KB x 1: 287
#endif
struct PsChunkModel {
  int BH, W, cls[3], ext[3], Wo[3];      // cls: stride class (1, 2, 3 = any stride >= 3); ext: output rows
  size_t lds_of(int i, int n, int r) const { return ((size_t)(n + 2) * ps_plane_bytes(cls[i], r, W, Wo[i]) + 1023) / 1024 * 1024; }
  double item_us(int i, int n, int r) const {
    return 3.0 + 0.08 * (double)(lds_of(i, n, r) / 1024) / 4.0 + std::ceil((double)n * r * Wo[i] / PS_SLOTS) * 0.27 + 1.0;
  }
  void cost(int i, PfTensorPlan p, int tc, int yc, double* sum, double* longest) const {
    *sum += 3.0 * BH * tc * yc * item_us(i, p.n, p.r);
    *longest = std::max(*longest, item_us(i, p.n, p.r));
  }
  bool admit(PfTensorPlan, PfTensorPlan) const { return true; }
};
static PoolChunkPlan search_fwd_staged(const PoolGeom& g) {
  PsChunkModel m = {g.B * g.heads, g.W[0]};
  for (int i = 0; i < 3; ++i) {
    const PoolOut o = pool_out(g.T[0], g.H[0], g.W[0], g.n_obj[0], g.s[i]);
    m.cls[i] = pf_class(g.s[i]);
    m.ext[i] = o.Ho;
    m.Wo[i] = o.Wo;
  }
  return pool_chunk_search(m, g.T[0], m.BH, SVIT_PS_LDS_KB * 1024, 0, SVIT_PS_SLOTS);
}

// Fused conv backward: input planes (n) and unit rows (r) per chunk, two workgroups per CU.  Item time, from the in-kernel
// stamps of round 5 (profiles/r05_pool_bwd_stamps.txt, MI355X): staging 3 us + 0.08 us per 1-KiB piece and wave, then
// ceil(planes x units / 16 thread slots) steps of 0.47 us (stride 1: one token per unit), 0.96 us (stride 2: four tokens -- four
// loads and four stores -- per unit) or ~2 us (stride >= 3: nine), 2.5 us of tail (+ 1.5 us for the cls / object rows of chunk 0).
// The last chunk along t and along y is ragged and costed as such.  No plan where not even one unit row of three planes fits;
// a candidate past 4096 partial rows per tensor (batch*heads x chunks) is not admitted.
struct PfChunkModel {
  int T, BH, cls[3], ext[3], UC[3], Wo[3];           // ext / UC: rows / columns of units of a plane
  double step_us[3];
  size_t lds_of(int i, int n, int r) const { return ((size_t)(n + 2) * pf_plane_bytes(pf_image_rows(cls[i], r), Wo[i]) + 1023) / 1024 * 1024; }
  double item_us(int i, int n, int r, bool first = false) const {
    return 3.0 + 0.08 * (double)(lds_of(i, n, r) / 1024) / 4.0 + std::ceil((double)n * r * UC[i] / PF_SLOTS) * step_us[i] + 2.5 +
           (first ? 1.5 : 0.0);
  }
  void cost(int i, PfTensorPlan p, int tc, int yc, double* sum, double* longest) const {
    const int nl = T - (tc - 1) * p.n, rl = ext[i] - (yc - 1) * p.r;
    *sum += 3.0 * BH * ((tc - 1) * (yc - 1) * item_us(i, p.n, p.r, false) + (tc - 1) * item_us(i, p.n, rl, false) +
                        (yc - 1) * item_us(i, nl, p.r, false) + item_us(i, nl, rl, false) + 1.5);
    *longest = std::max(*longest, item_us(i, p.n, p.r, tc * yc == 1));
  }
  bool admit(PfTensorPlan pq, PfTensorPlan pkv) const {
    return (long)BH * std::max((T + pq.n - 1) / pq.n * ((ext[0] + pq.r - 1) / pq.r),
                               (T + pkv.n - 1) / pkv.n * ((ext[1] + pkv.r - 1) / pkv.r)) <= 4096;
  }
};
static PoolChunkPlan search_bwd_fused(const PoolGeom& g) {
  constexpr size_t LDS_MAX = 79 * 1024;       // two workgroups per CU (the image is staged in whole 1-KiB pieces)
  PfChunkModel m = {g.T[0], g.B * g.heads};
  for (int i = 0; i < 3; ++i) {
    const PoolOut o = pool_out(g.T[0], g.H[0], g.W[0], g.n_obj[0], g.s[i]);
    m.Wo[i] = o.Wo;
    m.cls[i] = pf_class(g.s[i]);
    m.ext[i] = pf_unit_rows(m.cls[i], g.H[0], o.Ho);
    m.UC[i] = m.cls[i] == 1 ? g.W[0] : m.cls[i] == 2 ? (g.W[0] + 1) / 2 : o.Wo;
    m.step_us[i] = m.cls[i] == 1 ? 0.47 : m.cls[i] == 2 ? 0.96 : 2.0;
    if (3 * (size_t)pf_plane_bytes(pf_image_rows(m.cls[i], 1), o.Wo) + 1023 > LDS_MAX) return PoolChunkPlan{};
  }
  return pool_chunk_search(m, m.T, m.BH, LDS_MAX, 4 * 16 * 54 * sizeof(float), 512.0);
}

// A search costs ~1 ms of host time and its result is a pure function of the key -- batch*heads, T, H, W, the three strides,
// kind -- so it is memoised (a training step has at most 16 distinct geometries per kind; the table is append-only,
// mutex-guarded, and holds no device state).  false: no plan (a clip past the descriptor span, an image that does not fit).
enum { POOL_PLAN_BWD = 0, POOL_PLAN_STAGED = 1 };
struct PfPlanKey { int v[8]; bool operator==(const PfPlanKey& o) const { for (int i = 0; i < 8; ++i) if (v[i] != o.v[i]) return false; return true; } };
struct PfPlanEntry { PfPlanKey key; PoolChunkPlan plan; };
static std::mutex g_pf_plan_mu;
static std::vector<PfPlanEntry> g_pf_plans;
static bool pool_chunk_plan(const PoolGeom& g, int kind, PoolChunkPlan* out) {
  *out = {};
  if (!pool_clip_span_ok(g.T[0], g.H[0], g.W[0], g.n_obj[0], g.heads)) return false;
  const PfPlanKey key = {{g.B * g.heads, g.T[0], g.H[0], g.W[0], g.s[0], g.s[1], g.s[2], kind}};
  {
    std::lock_guard<std::mutex> lk(g_pf_plan_mu);
    for (const auto& e : g_pf_plans)
      if (e.key == key) { *out = e.plan; return out->ok; }
  }
  *out = kind == POOL_PLAN_STAGED ? search_fwd_staged(g) : search_bwd_fused(g);
  std::lock_guard<std::mutex> lk(g_pf_plan_mu);
  if (g_pf_plans.size() < 256) g_pf_plans.push_back({key, *out});
  return out->ok;
}

// ---- forward of q, k, v: geometry -> choice -> launches ----
enum { POOL_PATH_FRAME = 0, POOL_PATH_MFMA, POOL_PATH_SLAB, POOL_PATH_STAGED, POOL_PATH_STREAM };     // PoolFwdChoice.path
enum { POOL_RELQ_NOBODY = 0, POOL_RELQ_SLAB_LN, POOL_RELQ_GEMM };                                       // PoolFwdChoice.relq
enum { POOL_KERNEL_FRAME = 0, POOL_KERNEL_MFMA, POOL_KERNEL_SLAB, POOL_KERNEL_SLAB_LN, POOL_KERNEL_STAGED, POOL_KERNEL_FWD3 };
struct PoolLaunch { int kernel; unsigned gx, gy, gz, block, lds; };
// the kernel structs hold what the chooser decides (plans, skip flags); their pointers are the launch functions' to fill
struct PoolFwdChoice {
  int path;
  int relq;                  // who writes q's rel-pos columns: nobody, pool_slab_ln_kernel, the trailing SVIT_EPI_RELQ GEMM
  int n_launch;
  PoolLaunch launch[3];
  PoolFrame3 frame;
  int frame_img_bytes;
  PoolSlab3 slab;            // plan[i].on: pool_slab_ln_kernel normalises tensor i (slab and staged paths)
  PoolFwdStaged staged;
  PoolFwd3 fwd3;             // skip[i] = slab.plan[i].on
};
static void add_launch(PoolFwdChoice* c, int kernel, dim3 grid, unsigned block, size_t lds) {
  c->launch[c->n_launch++] = {kernel, grid.x, grid.y, grid.z, block, (unsigned)lds};
}

// pool_frame_fwd_kernel: bands of R output rows whose image fits FR_IMG_MAX; false where one row does not fit
static bool choose_frame(const PoolGeom& g, PoolFwdChoice* c) {
  PoolFrame3& fg = c->frame;
  size_t img = 0;
  double cost[3], cost_sum = 0.0;
  for (int i = 0; i < 3; ++i) {
    const int se = pf_class(g.s[i]);
    const PoolOut o = pool_out(g, i);
    int R = o.Ho;
    while (R > 1 && fr_image_bytes(se, R, g.W[i], o.Wo) > FR_IMG_MAX) --R;
    if (fr_image_bytes(se, R, g.W[i], o.Wo) > FR_IMG_MAX) return false;
    const int chunks = (o.Ho + R - 1) / R;
    R = (o.Ho + chunks - 1) / chunks;
    fg.r_per[i] = R;
    fg.y_chunks[i] = chunks;
    fg.n_items[i] = g.B * g.heads * chunks;
    const size_t ib = fr_image_bytes(se, R, g.W[i], o.Wo);
    img = std::max(img, ib);
    // item time (tools/pool_frame_stamps.py): ~0.03 us per 1-KiB piece to issue, ~0.7 us at the barrier, ~1 us per 64-token pass
    const int passes = (R * o.Wo + 1 + g.n_obj[i] + 63) / 64;
    cost[i] = fg.n_items[i] * (0.7 + 0.03 * (double)(ib >> 10) + 1.0 * passes);
    cost_sum += cost[i];
  }
  // workgroups per tensor in proportion to its work (one persistent workgroup per CU; each reads ONE tensor's weights)
  int wgs[3], total_wgs = 256;
  for (int i = 0; i < 3; ++i) wgs[i] = std::max(1, std::min(fg.n_items[i], (int)(total_wgs * cost[i] / cost_sum + 0.5)));
  while (wgs[0] + wgs[1] + wgs[2] > total_wgs) {
    int big = 0;
    for (int i = 1; i < 3; ++i) if (wgs[i] > wgs[big]) big = i;
    --wgs[big];
  }
  for (int i = 0; i < 3; ++i) fg.wg_first[i + 1] = fg.wg_first[i] + wgs[i];
  c->frame_img_bytes = (int)((img + 1023) / 1024 * 1024);
  add_launch(c, POOL_KERNEL_FRAME, dim3((unsigned)fg.wg_first[3]), FR_NT, FR_HEAD + 2 * (size_t)c->frame_img_bytes);
  return true;
}

// pool_slab_ln_kernel over the tensors with slab.plan[i].on
#ifndef SVIT_SLAB_LN_WANT
#define SVIT_SLAB_LN_WANT 2048      // (in-step A/B of round 4: 1024 -> 2048 is -0.02..-0.04 ms)
#endif
static void add_slab_ln(const PoolGeom& g, PoolFwdChoice* c) {
  int blocks = 1;
  for (int i = 0; i < 3; ++i)
    if (c->slab.plan[i].on) blocks = std::max(blocks, (int)persistent_x((pool_out(g, i).Nout + 63) / 64, g.B * g.heads * 3, SVIT_SLAB_LN_WANT));
  const size_t lds = c->relq == POOL_RELQ_SLAB_LN ? (size_t)64 * SLN_QROW + (size_t)64 * g.relq_lpad * 2 : 0;
  add_launch(c, POOL_KERNEL_SLAB_LN, dim3(blocks, g.B * g.heads, 3), 256, lds);
}

// pool_ln_fwd3_kernel over the other tensors: streaming, or the LDS-tiled stencil at stride 1 where tables were given
static void add_fwd3(const PoolGeom& g, PoolFwdChoice* c) {
  unsigned gx = 1;
  size_t lds = 0;
  for (int i = 0; i < 3; ++i) {
    if ((c->fwd3.skip[i] = c->slab.plan[i].on)) continue;
    unsigned x = persistent_x((pool_out(g, i).Nout + 63) / 64, g.B * g.heads * 3);
    if (g.s[i] == 1 && g.sel) {
      c->fwd3.plan[i] = plan_tiled(g.T[i], g.H[i], g.W[i], g.n_obj[i], g.B * g.heads);
      x = (unsigned)(c->fwd3.plan[i].n_wgs + c->fwd3.plan[i].n_special);
      lds = std::max(lds, tiled_lds_bytes(g.W[i]));
    }
    gx = std::max(gx, x);
  }
  add_launch(c, POOL_KERNEL_FWD3, dim3(gx, g.B * g.heads, 3), 256, lds);
}

// Reads nothing but the geometry and the knobs.  Precedence: frame; slab, with pool_ln_fwd3_kernel for the tensors that are
// not on the slab; staged; pool_ln_fwd3_kernel.  q's rel-pos columns: pool_slab_ln_kernel writes them where it normalises q and
// the product tile of 64 tokens fits LDS (relq_lpad <= 288), else svit_gemm_nt with SVIT_EPI_RELQ right behind the pooling.
static PoolFwdChoice pool_fwd_choose(const PoolGeom& g) {
  PoolFwdChoice c = {};
  const int BH = g.B * g.heads;
  const int relq_gemm = g.relq_lpad ? POOL_RELQ_GEMM : POOL_RELQ_NOBODY;
  const int relq_ln = g.relq_lpad && g.relq_lpad <= 288 ? POOL_RELQ_SLAB_LN : relq_gemm;
  c.path = POOL_PATH_STREAM;
  c.relq = relq_gemm;
  // round 5: one-plane volumes (frames pass, image ranks): conv + LayerNorm in one launch from an LDS-staged plane;
  // svit_debug_set_pool(3, 0) keeps the paths below (A/B)
  // (round 6: default 2 = every T = 1 pass, training steps of the image ranks included.  Round 5 kept those on the streaming
  //  kernels because the image-rank test's worst gradient tensor (rel_pos_t: one table row shared by every query) read 0.9893
  //  against a flat 0.99 bar with this kernel and 0.9915 without -- same arithmetic, another summation order of the row
  //  statistics.  The golden manifest's bf16 yardstick -- the REFERENCE's own backward with bf16 matrix operands -- scores
  //  0.9789 on that tensor (profiles/r06_yardstick.txt): both orders sit well inside what a correct bf16 implementation
  //  produces, and the test now measures against the yardstick.  1 = no-grad passes only, 0 = never.)
  const int fr_mode = svit_knob(SVIT_K_POOL_FRAME);
  if (g.T[0] == 1 && g.T[1] == 1 && g.T[2] == 1 && (fr_mode == 2 || (fr_mode == 1 && !g.pre[0] && !g.pre[1] && !g.pre[2])) &&
      pool_clip_span_ok(1, g.H[0], g.W[0], g.n_obj[0], g.heads) && choose_frame(g, &c)) {
    c.path = POOL_PATH_FRAME;
    return c;
  }
  int n_slab = 0;
  for (int i = 0; i < 3; ++i) {
    if (g.sel) c.slab.plan[i] = plan_slab(g, i);
    n_slab += c.slab.plan[i].on;
  }
  if (n_slab) {
    // round 4: the conv of the slab planes on the matrix pipe (pool_mfma_fwd_kernel) where its geometry holds for
    // all three tensors: W <= 14 (16 slots per image row with both x halos), T a multiple of 4 (t-quads), the
    // 16-channel image within the LDS of a CU; svit_debug_set_pool(0, 1) keeps the VALU slab kernel (A/B)
    bool mfma = n_slab == 3 && svit_knob(SVIT_K_POOL_FWD) != 1;
    size_t mlds = 0, slds = 0;
    for (int i = 0; i < 3 && mfma; ++i) {
      mfma = g.W[i] <= 14 && g.T[i] % 4 == 0 && g.T[i] == g.T[0] && g.H[i] == g.H[0];
      mlds = std::max(mlds, pm_lds_bytes(g.T[i], g.H[i]));
    }
    if (mfma && mlds > 160 * 1024) mfma = false;
    // measured (tools/diag/pool_fwd_ab.sh, profiles/r04_pool_mfma_stencil.txt): ahead of the VALU slab kernel where its
    // 12 B heads workgroups are ONE round at two per CU (blocks 4-13 of 16x224^2: 24.6 against 28.4 us), level or
    // behind with more (blocks 14 / 15, 8 heads); svit_debug_set_pool(0, 3) forces it everywhere its geometry holds
    if (mfma && svit_knob(SVIT_K_POOL_FWD) != 3 && ((long)BH * 12 > 512 || 2 * mlds > 160 * 1024)) mfma = false;
    for (int i = 0; i < 3; ++i) {
      const SlabPlan& pl = c.slab.plan[i];
      if (!pl.on) continue;
      const int pin = std::min(g.T[i], pl.TC + 2), rin = std::min(g.H[i], g.s[i] * (pl.YC - 1) + 3);
      slds = std::max(slds, ((size_t)pin * rin * g.W[i] * 48 + 1023) / 1024 * 1024 + 64 + 96);
      c.slab.max_chunks = std::max(c.slab.max_chunks, pl.nt * pl.ny);
    }
    c.path = mfma ? POOL_PATH_MFMA : POOL_PATH_SLAB;
    if (mfma) add_launch(&c, POOL_KERNEL_MFMA, dim3(BH * 2 * 6), PM_NT, mlds);
    else add_launch(&c, POOL_KERNEL_SLAB, dim3(c.slab.max_chunks * BH * 12), SLAB_NT, slds);
    if (c.slab.plan[0].on) c.relq = relq_ln;
    add_slab_ln(g, &c);
    if (n_slab < 3) add_fwd3(g, &c);
    return c;
  }
  // round 5: no tensor took the slab path (planes past 14x14: blocks 0-3) and every tensor saves `pre` (a training step):
  // the staged conv forward (input staged once in LDS, every stride) + the row-wise LayerNorm launch of the slab path;
  // svit_debug_set_pool(2, 0) keeps the streaming kernel below (A/B)
  PoolChunkPlan cp;
  if (g.H[0] * g.W[0] > 196 && svit_knob(SVIT_K_POOL_FWD_LARGE) != 0 && g.pre[0] && g.pre[1] && g.pre[2] &&
      g.T[1] == g.T[0] && g.T[2] == g.T[0] && g.H[1] == g.H[0] && g.H[2] == g.H[0] && g.W[1] == g.W[0] &&
      g.W[2] == g.W[0] && g.n_obj[1] == g.n_obj[0] && g.n_obj[2] == g.n_obj[0] && pool_chunk_plan(g, POOL_PLAN_STAGED, &cp)) {
    c.path = POOL_PATH_STAGED;
    c.relq = relq_ln;
    chunk_plan_into(cp, &c.staged);
    add_launch(&c, POOL_KERNEL_STAGED, dim3((unsigned)cp.first_item[3]), PS_NT, cp.lds);
    for (int i = 0; i < 3; ++i) c.slab.plan[i].on = 1;
    add_slab_ln(g, &c);
    return c;
  }
  add_fwd3(g, &c);
  return c;
}

// the launch functions execute a choice (svit_max_lds_once: the largest dynamic LDS a kernel is ever launched with)
struct PoolCall { const svit_pool_args* a3; const uint32_t* const* sel3; hipStream_t stream; };
template <class K> static K with_args(K k, const PoolCall& call) {
  for (int i = 0; i < 3; ++i) k.p[i] = call.a3[i];
  return k;
}
template <class K> static K with_args_sel(K k, const PoolCall& call) {
  for (int i = 0; i < 3; ++i) k.sel[i] = call.sel3 ? call.sel3[i] : nullptr;
  return with_args(k, call);
}
template <class K, class... A>
static int pool_launch(K kernel, SvitOnce* once, size_t max_lds, const PoolLaunch& l, const PoolCall& call, const A&... args) {
  if (int rc = once ? svit_max_lds_once(*once, (const void*)kernel, max_lds) : 0) return rc;
  hipLaunchKernelGGL(kernel, dim3(l.gx, l.gy, l.gz), dim3(l.block), l.lds, call.stream, args...);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
static int launch_frame(const PoolFwdChoice& c, const PoolLaunch& l, const PoolCall& call) {
  static SvitOnce once;
  return pool_launch(pool_frame_fwd_kernel, &once, FR_HEAD + 2 * FR_IMG_MAX, l, call, with_args(c.frame, call), c.frame_img_bytes);
}
static PoolSlab3 slab_args(const PoolFwdChoice& c, const PoolCall& call) {
  PoolSlab3 sg = with_args_sel(c.slab, call);
  if (c.relq != POOL_RELQ_SLAB_LN) sg.p[0].relq_R = nullptr;
  return sg;
}
static int launch_slab_conv(const PoolFwdChoice& c, const PoolLaunch& l, const PoolCall& call) {      // MFMA or VALU
  static SvitOnce once_mfma, once_slab;
  if (l.kernel == POOL_KERNEL_MFMA) return pool_launch(pool_mfma_fwd_kernel, &once_mfma, 160 * 1024, l, call, with_args(PoolMfma3{}, call));
  return pool_launch(pool_slab_fwd_kernel, &once_slab, 80 * 1024, l, call, slab_args(c, call));
}
static int launch_slab_ln(const PoolFwdChoice& c, const PoolLaunch& l, const PoolCall& call) {
  return pool_launch(pool_slab_ln_kernel, nullptr, 0, l, call, slab_args(c, call));      // (at most 50 KiB: within the default limit)
}
static int launch_staged(const PoolFwdChoice& c, const PoolLaunch& l, const PoolCall& call) {
  static SvitOnce once;
  return pool_launch(pool_fwd_staged_kernel, &once, SVIT_PS_LDS_KB * 1024, l, call, with_args(c.staged, call));
}
static int launch_fwd3(const PoolFwdChoice& c, const PoolLaunch& l, const PoolCall& call) {
  static SvitOnce once;
  return pool_launch(pool_ln_fwd3_kernel, &once, 64 * 1024, l, call, with_args_sel(c.fwd3, call));
}

static int pool_ln_fwd_qkv_impl(const svit_pool_args* a3, const uint32_t* const* sel3, void* stream) {
  if (!a3) return SVIT_ERR_ARG;
  const svit_pool_args& q = a3[0];
  if (q.relq_R) {
    if (!q.relq_map || q.relq_lpad <= 0 || q.relq_lpad % 96 != 0 || q.which != 0 || q.mode != 0 ||
        (q.ld_out != 128 && q.ld_out != 160) || (((uintptr_t)q.relq_R | (uintptr_t)q.relq_map) & 15))
      return SVIT_ERR_ARG;
  }
  for (int i = 0; i < 3; ++i) {
    if (int rc = check_pool_fwd(&a3[i])) return rc;
    if (a3[i].B != a3[0].B || a3[i].heads != a3[0].heads) return SVIT_ERR_SHAPE;
  }
  const PoolFwdChoice c = pool_fwd_choose(pool_geom(a3, sel3 != nullptr));
  const PoolCall call = {a3, sel3, (hipStream_t)stream};
  for (int k = 0; k < c.n_launch; ++k) {
    const PoolLaunch& l = c.launch[k];
    const int rc = l.kernel == POOL_KERNEL_FRAME ? launch_frame(c, l, call)
                 : l.kernel == POOL_KERNEL_SLAB_LN ? launch_slab_ln(c, l, call)
                 : l.kernel == POOL_KERNEL_STAGED ? launch_staged(c, l, call)
                 : l.kernel == POOL_KERNEL_FWD3 ? launch_fwd3(c, l, call) : launch_slab_conv(c, l, call);
    if (rc) return rc;
  }
  if (c.relq != POOL_RELQ_GEMM) return SVIT_OK;
  // rel-pos columns of the q tensor (svit_pool_args.relq_*): the product + gather as its own launch right behind the pooling
  const int Nout = pool_out(q).Nout;
  svit_gemm_args g = {};
  g.A = q.out; g.lda = q.ld_out;
  g.W = q.relq_R; g.ldw = HD;
  g.M = q.B * q.heads * Nout; g.N = (q.relq_lpad + 95) / 96 * 96; g.K = HD;
  g.epilogue = SVIT_EPI_RELQ;
  g.relq_map = q.relq_map; g.relq_out = q.out; g.relq_ld = q.ld_out;
  g.relq_extra = q.ld_out - HD; g.relq_rows = Nout; g.relq_scale = q.relq_scale;
  return svit_gemm_nt(&g, stream);
}

// Host-only plan query (include/svit_hip.h, diagnostics): what the chooser and the chunk search above answer for a geometry.
extern "C" int svit_debug_pool_plan(int kind, int B, int heads, int T, int H, int W, int n_obj, int sq, int sk, int sv,
                                    int save_mask, int sel, int relq_lpad, int32_t* out, int n_out) {
  if (!out || n_out < 24 || kind < 0 || kind > 2 || relq_lpad < 0) return SVIT_ERR_ARG;
  PoolGeom g = pool_geom(B, heads, T, H, W, n_obj, sq, sk, sv);
  for (int i = 0; i < 3; ++i) {
    if (check_pool_dims(B, heads, T, H, W, n_obj, g.s[i])) return SVIT_ERR_SHAPE;
    g.pre[i] = (save_mask >> i) & 1;
  }
  g.sel = sel != 0;
  g.relq_lpad = relq_lpad;
  if (kind == 0) {       // path, relq, n_launch, then per launch: kernel, grid x / y / z, block, dynamic LDS bytes
    const PoolFwdChoice c = pool_fwd_choose(g);
    static_assert(offsetof(PoolFwdChoice, frame) >= 21 * sizeof(int32_t) && sizeof(PoolLaunch) == 6 * sizeof(int32_t), "layout");
    memcpy(out, &c, 21 * sizeof(int32_t));
    return 3 + 6 * c.n_launch;
  }
  PoolChunkPlan p;       // the fields of PoolChunkPlan in their order
  static_assert(sizeof p == 22 * sizeof(int32_t), "layout");
  pool_chunk_plan(g, kind == 1 ? POOL_PLAN_STAGED : POOL_PLAN_BWD, &p);
  memcpy(out, &p, sizeof p);
  return 22;
}

extern "C" int svit_pool_ln_fwd_qkv(const svit_pool_args* a3, void* stream) {
  return pool_ln_fwd_qkv_impl(a3, nullptr, stream);
}
// the same with the selector tables of the three depthwise weights (svit_pool_weight_sel): tensors
// with stride 1 run the LDS-tiled stencil
extern "C" int svit_pool_ln_fwd_qkv_sel(const svit_pool_args* a3, const uint32_t* const* sel3, void* stream) {
  if (!sel3) return SVIT_ERR_ARG;
  return pool_ln_fwd_qkv_impl(a3, sel3, stream);
}

extern "C" int svit_pool_weight_sel(const float* src_base, const int64_t* src_off, uint32_t* dst,
                                    int n_tables, void* stream) {
  if (!src_base || !src_off || !dst || n_tables <= 0) return SVIT_ERR_ARG;
  hipLaunchKernelGGL(pool_weight_sel_kernel, dim3(4, n_tables), dim3(256), 0, (hipStream_t)stream,
                     src_base, src_off, dst, n_tables);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

static int check_pool_ln_bwd(const svit_pool_ln_bwd_args* a) {
  if (!a->pre || !a->mean || !a->rstd || !a->gamma || !a->dpre || !a->dgamma || !a->dbeta)
    return SVIT_ERR_ARG;
  if (a->B <= 0 || a->heads <= 0 || a->Nout <= 0) return SVIT_ERR_SHAPE;
  if (a->d_main && (a->ld_main < HD || a->ld_main % 8 != 0)) return SVIT_ERR_ALIGN;
  return SVIT_OK;
}

// workgroups of the LayerNorm backward: >= 4 token groups each, 128..1024, and no more partial rows than the workspace holds
static int64_t pool_ln_bwd_blocks(int64_t total, int64_t workspace_floats, int row_floats) {
  int64_t blocks = (total + 255) / 256;
  if (blocks < 128) blocks = (total + 63) / 64 < 128 ? (total + 63) / 64 : 128;
  if (blocks > 1024) blocks = 1024;
  return std::min(blocks, workspace_floats / row_floats);
}

extern "C" int svit_pool_ln_bwd_qkv(const svit_pool_ln_bwd_args* a3, void* stream) {
  if (!a3 || !a3[0].workspace) return SVIT_ERR_ARG;
  PoolLnBwd3 g;
  int64_t max_total = 0;
  for (int i = 0; i < 3; ++i) {
    const int rc = check_pool_ln_bwd(&a3[i]);
    if (rc) return rc;
    g.p[i] = a3[i];
    const int64_t total = (int64_t)a3[i].B * a3[i].heads * a3[i].Nout;
    if (total > max_total) max_total = total;
  }
  const int64_t blocks = pool_ln_bwd_blocks(max_total, a3[0].workspace_floats, 6 * HD);
  if (blocks < 1) return SVIT_ERR_ARG;
  hipLaunchKernelGGL(pool_ln_bwd3_kernel, dim3((unsigned)blocks, 3), dim3(256), 0,
                     (hipStream_t)stream, g);
  SVIT_LAUNCH_CHECK();
  SvitReduceDst dst = {{a3[0].dgamma, a3[0].dbeta, a3[1].dgamma, a3[1].dbeta, a3[2].dgamma, a3[2].dbeta},
                       {HD, 2 * HD, 3 * HD, 4 * HD, 5 * HD, 6 * HD}};
  svit_launch_reduce(a3[0].workspace, (int)blocks, 6 * HD, dst, (hipStream_t)stream);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

#ifdef SVIT_DIAG_POOL_STREAMING
#define SVIT_POOL_STREAMING_PART 2
#include "../../tools/diag/variants/pool_streaming.inc"
#undef SVIT_POOL_STREAMING_PART
#endif

// floats of workspace svit_pool_conv_bwd_qkv needs for these three tensors (one partial row of the three dw per (batch, head, chunk) of
// its plan); -1 where the fused kernel has no plan.  Callers with a fixed scratch region ask first and bring a larger buffer when the
// batch outgrows it (the entry point refuses a workspace that is too small: the product library has no other conv backward).
extern "C" int64_t svit_pool_conv_bwd_workspace(const svit_pool_dgrad_args* d3) {
  if (!d3) return SVIT_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (check_pool_dims(d3[i].B, d3[i].heads, d3[i].T, d3[i].H, d3[i].W, d3[i].n_obj, d3[i].stride_hw)) return SVIT_ERR_SHAPE;
  PoolChunkPlan cp;
  if (!pool_chunk_plan(pool_geom(d3), POOL_PLAN_BWD, &cp)) return -1;
  return (int64_t)d3[0].B * d3[0].heads * cp.max_chunks * 3 * 27 * HD;
}

// which path the last svit_pool_conv_bwd_qkv call of this process took: 1 the fused plane-walk kernel, 0 the two streaming launches
// (planes that do not fit, a workspace smaller than the plan's partial rows, the knob), -1 none yet.  Diagnostics / tests: a parity
// test of the fused kernel must not pass on a silent fallback.
static int g_pool_bwd_last_path = -1;
extern "C" int svit_debug_pool_bwd_path(void) { return __atomic_load_n(&g_pool_bwd_last_path, __ATOMIC_RELAXED); }

extern "C" int svit_pool_conv_bwd_qkv(const svit_pool_dgrad_args* d3, const svit_pool_wgrad_args* w3, void* stream) {
  if (!d3 || !w3) return SVIT_ERR_ARG;
  for (int i = 0; i < 3; ++i) {
    const svit_pool_dgrad_args& d = d3[i];
    const svit_pool_wgrad_args& w = w3[i];
    if (!d.dpre || !d.conv_w || !d.dqkv || !w.qkv || !w.dw || d.which != i || w.which != i)
      return SVIT_ERR_ARG;
    const int rc = check_pool_dims(d.B, d.heads, d.T, d.H, d.W, d.n_obj, d.stride_hw);
    if (rc) return rc;
    if (w.dpre != d.dpre || w.stride_hw != d.stride_hw || w.qkv != w3[0].qkv) return SVIT_ERR_ARG;
    if (d.B != d3[0].B || d.heads != d3[0].heads || d.T != d3[0].T || d.H != d3[0].H || d.W != d3[0].W ||
        d.n_obj != d3[0].n_obj)
      return SVIT_ERR_SHAPE;
  }
  PoolChunkPlan cp;
  bool fused = svit_knob(SVIT_K_POOL_BWD) != 0 && pool_chunk_plan(pool_geom(d3), POOL_PLAN_BWD, &cp);
  const int64_t prows = fused ? (int64_t)d3[0].B * d3[0].heads * cp.max_chunks : 0;
  if (fused && (!w3[0].workspace || w3[0].workspace_floats < prows * 3 * 27 * HD || prows > 65536)) fused = false;
  __atomic_store_n(&g_pool_bwd_last_path, fused ? 1 : 0, __ATOMIC_RELAXED);
  if (!fused) {
#ifdef SVIT_DIAG_POOL_STREAMING      // (diagnostic build: the two streaming launches of rounds 1-4, also the knob-off arm)
    int rc = svit_pool_conv_dgrad_qkv(d3, stream);
    if (rc) return rc;
    return svit_pool_conv_wgrad_qkv(w3, stream);
#else
    // no plan (a volume whose unit row of three planes does not fit 79 KB of LDS, a clip past the 2-GiB descriptor span), a
    // workspace smaller than the plan's partial rows, or key 1 = 0: the product library has no other conv backward -- fail loudly
    return SVIT_ERR_SHAPE;
#endif
  }
  PoolBwdFused g;
  chunk_plan_into(cp, &g);
  g.max_chunks = cp.max_chunks;
  for (int i = 0; i < 3; ++i) g.d[i] = d3[i];
  g.qkv = w3[0].qkv;
  g.partial = w3[0].workspace;
  static SvitOnce once;
  if (int rc = svit_max_lds_once(once, (const void*)pool_bwd_fused_kernel, 80 * 1024)) return rc;
  hipLaunchKernelGGL(pool_bwd_fused_kernel, dim3((unsigned)g.first_item[3]), dim3(PF_NT), cp.lds, (hipStream_t)stream, g);
  SVIT_LAUNCH_CHECK();
  SvitReduceDst dst = {{w3[0].dw, w3[1].dw, w3[2].dw, w3[2].dw, w3[2].dw, w3[2].dw},
                       {27 * HD, 2 * 27 * HD, 3 * 27 * HD, 3 * 27 * HD, 3 * 27 * HD, 3 * 27 * HD}};
  svit_launch_reduce(w3[0].workspace, (int)prows, 3 * 27 * HD, dst, (hipStream_t)stream);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_pool_ln_bwd(const svit_pool_ln_bwd_args* a, void* stream) {
  if (!a) return SVIT_ERR_ARG;
  if (int rc = check_pool_ln_bwd(a)) return rc;
  if (!a->workspace) return SVIT_ERR_ARG;
  const int64_t blocks = pool_ln_bwd_blocks((int64_t)a->B * a->heads * a->Nout, a->workspace_floats, 2 * HD);
  if (blocks < 1) return SVIT_ERR_ARG;
  hipLaunchKernelGGL(pool_ln_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  SvitReduceDst dst = {{a->dgamma, a->dbeta, a->dbeta, a->dbeta, a->dbeta, a->dbeta}, {HD, 2 * HD, 2 * HD, 2 * HD, 2 * HD, 2 * HD}};
  svit_launch_reduce(a->workspace, (int)blocks, 2 * HD, dst, (hipStream_t)stream);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

#ifdef SVIT_DIAG_POOL_STREAMING
#define SVIT_POOL_STREAMING_PART 3
#include "../../tools/diag/variants/pool_streaming.inc"
#undef SVIT_POOL_STREAMING_PART
#endif

static int check_relq(int ld, int kh, int kw, int kt) {
  const int extra = ld - HD;
  if (extra != 32 && extra != 64) return SVIT_ERR_SHAPE;
  if (kh + kw + kt > extra) return SVIT_ERR_SHAPE;
  return SVIT_OK;
}
// tokens of a rel-pos launch, and the grid of its per-token kernels: 256 / extra tokens per workgroup
template <class A> static int64_t relq_tokens(const A* a) { return (int64_t)a->B * a->heads * (1 + a->qt * a->qh * a->qw + a->n_obj); }
template <class A> static dim3 relq_grid(const A* a) {
  const int tpb = 256 / (a->ld - HD);
  return dim3((unsigned)((relq_tokens(a) + tpb - 1) / tpb));
}

extern "C" int svit_relpos_q_fwd(const svit_relq_args* a, void* stream) {
  if (!a || !a->qa || !a->rel_h || !a->rel_w || !a->rel_t || !a->idx_h || !a->idx_w || !a->idx_t)
    return SVIT_ERR_ARG;
  if (int rc = check_relq(a->ld, a->kh, a->kw, a->kt)) return rc;
  hipLaunchKernelGGL(relq_fwd_kernel, relq_grid(a), dim3(256), 0, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_relpos_gather(const svit_relq_gather_args* a, void* stream) {
  if (!a || !a->P || !a->qa || !a->idx_h || !a->idx_w || !a->idx_t) return SVIT_ERR_ARG;
  if (int rc = check_relq(a->ld, a->kh, a->kw, a->kt)) return rc;
  hipLaunchKernelGGL(relq_gather_kernel, relq_grid(a), dim3(256), 0, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_relpos_scatter(const svit_relq_scatter_args* a, void* stream) {
  if (!a || !a->dqa || !a->D || !a->idx_h || !a->idx_w || !a->idx_t) return SVIT_ERR_ARG;
  if (int rc = check_relq(a->ld, a->kh, a->kw, a->kt)) return rc;
  if (a->ldd % 8 != 0 || a->off_h < 0 || a->off_w < a->off_h || a->off_t < a->off_w) return SVIT_ERR_ARG;
  if ((uintptr_t)a->D & 15) return SVIT_ERR_ALIGN;
  hipLaunchKernelGGL(relq_scatter_kernel, relq_grid(a), dim3(256), 0, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_relpos_q_bwd(const svit_relq_bwd_args* a, void* stream) {
  if (!a || !a->qa || !a->dqa || !a->dq_extra || !a->drel_h || !a->drel_w || !a->drel_t)
    return SVIT_ERR_ARG;
  if (int rc = check_relq(a->ld, a->kh, a->kw, a->kt)) return rc;
  const size_t lds = (size_t)(a->rows_h + a->rows_w + a->rows_t) * HD * sizeof(float);
  if (lds > 150 * 1024) return SVIT_ERR_SHAPE;
  static SvitOnce once;      // sized for the largest table set the shape check admits
  if (int rc = svit_max_lds_once(once, (const void*)relq_bwd_kernel, 150 * 1024)) return rc;
  const int64_t total = relq_tokens(a);
  if (!a->workspace) return SVIT_ERR_ARG;
  const int tab_n = (a->rows_h + a->rows_w + a->rows_t) * HD;
  int64_t blocks = (total + 7) / 8;
  if (blocks > 512) blocks = 512;
  if (blocks > a->workspace_floats / tab_n) blocks = a->workspace_floats / tab_n;
  if (blocks < 1) return SVIT_ERR_ARG;
  hipLaunchKernelGGL(relq_bwd_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, *a);
  SVIT_LAUNCH_CHECK();
  SvitReduceDst dst = {{a->drel_h, a->drel_w, a->drel_t, a->drel_t, a->drel_t, a->drel_t},
                       {a->rows_h * HD, (a->rows_h + a->rows_w) * HD, tab_n, tab_n, tab_n, tab_n}};
  svit_launch_reduce(a->workspace, (int)blocks, tab_n, dst, (hipStream_t)stream);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
