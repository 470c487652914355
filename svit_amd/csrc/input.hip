// Input pipeline fused into the patch embedding -- gfx950.
//
// The reference normalises decoded uint8 frames on the host ((u/255 - mean)/std,
// slowfast/datasets/utils.py:287-303), permutes T H W C -> C T H W, crops (transform.py:288-348)
// and ships fp32 clips to the GPU (misc.iter_to_cuda, slowfast/utils/misc.py:374-387): 4 bytes
// per sample over PCIe and HBM, plus a materialised copy per spatial crop.  Here the clip stays
// uint8 [V,T,Hs,Ws,3] in HBM and is normalised (a 3 x 256-entry table built with the reference's
// own fp32 operation order, so the values are bit-identical), cropped, augmented and mixed while
// the im2col rows of Conv3d(3->96, k(3,7,7), s(2,4,4), p(1,3,3)) (stem_helper.py:309-320) are
// assembled -- same [rows, 448] bf16 operand as svit_im2col_patch, a quarter of the input bytes,
// no per-crop copy.
//
// The skeleton, shared by the three im2col kernels: a block owns one output row (clip, to, yo) and
// walks it in chunks of XO output positions.  Per chunk it FILLS the LDS image
// img[(c*3+kt)*7+ky][x - x_start] -- the 21 (kt, ky) lines x 3 channels x COLS clip columns the
// chunk's patches read, as bf16, 0 = padding -- and then STORES it (store_chunk): 56 uint4 per
// output position.  Frame bytes come in aligned words through load_word, which alone knows about
// the end of the buffer; walk_span hands a contiguous byte span out byte by byte.  What a fill does:
//   svit_im2col_patch_u8       a line is one byte span of the clip's crop row (CropRow: video,
//                              y0, x0); each byte goes through the bf16 table.
//   svit_im2col_patch_u8_mix   Mixup / CutMix (cfg.MIXUP; slowfast/datasets/mixup.py,
//                              tools/train_net.py:63-71,92-94) between the fp32 normalisation and
//                              the bf16 rounding: the same span of the partner clip B-1-b is
//                              dropped into LDS first, then the clip's own span is walked and
//                              every byte blended with / replaced by the partner's.
//   svit_im2col_patch_u8_aug[_frames]  every pixel of the lines is aug_pixel (resized crop, flip,
//                              erasing per the clip's SvitAug record) of the clip, mixed with
//                              aug_pixel of the partner; the taps come from a staged copy of the
//                              source rectangle where it fits LDS.
// Every kernel of the mix feature reads ONE 32-byte record from device memory (SvitMix below), so a
// captured step holds the same launches whatever was drawn for it; `svit_mixup_clips` blends /
// swaps the fp32 clips of a batch in place against the batch reversed (uint8 frames cannot be
// blended in place without losing the fp32 arithmetic).
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
// the mix record: [0] mode (0 none, 1 mixup, 2 CutMix), [1] lam, [2] oml = float(1.0 - lam) (the
// subtraction in double, as torch does with the Python scalar), [3..6] yl, yh, xl, xh, [7] 0
struct SvitMix {
  int mode;
  float lam, oml;
  int yl, yh, xl, xh, pad;
};

// a * lam + b * oml with two roundings of the products and one of the sum -- what torch's
// mul_ / add_ sequence gives.  The library is built with -ffast-math, under which the backend
// fuses a multiply into the add that consumes it whatever the source says (__fmul_rn is a plain
// `*` here, and `#pragma clang fp contract(off)` still came out as v_fmac_f32): the empty asm
// makes each rounded product opaque, so there is nothing left to fuse.
__device__ __forceinline__ float mix_blend(float a, float b, float lam, float oml) {
  float p = __fmul_rn(a, lam), q = __fmul_rn(b, oml);
  __asm__("" : "+v"(p));
  __asm__("" : "+v"(q));
  return __fadd_rn(p, q);
}

// One thread owns a pair (element e of clip b, element e of clip B-1-b): it reads both and writes
// both, so the in-place update has no ordering problem.  For odd B the middle clip pairs with
// itself and goes through the same formula (x*lam + x*oml is not x in fp32).
template <bool VEC>
__global__ __launch_bounds__(256) void mixup_clips_kernel(float* __restrict__ x, const SvitMix* __restrict__ mix,
                                                          int B, uint32_t n, uint32_t H, uint32_t W) {
  const SvitMix m = *mix;
  if (m.mode != 1 && m.mode != 2) return;             // (uniform) mode 0: the data stays bit-unchanged
  const int b = blockIdx.y, pb = B - 1 - b;
  if (m.mode == 2 && pb == b) return;                 // CutMix of the middle clip with itself
  float* xa = x + (int64_t)b * n;
  float* xb = x + (int64_t)pb * n;
  constexpr int V = VEC ? 4 : 1;
  const uint32_t nv = n / V, stride = gridDim.x * blockDim.x;     // (n < 2^31, checked by the host: 32-bit divisions)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const uint32_t e = i * V, row = e / W;
    const int xc = (int)(e - row * W), yc = (int)(row % H);
    if (m.mode == 2 && (yc < m.yl || yc >= m.yh || xc + V <= m.xl || xc >= m.xh)) continue;
    if (VEC) {
      const float4 a = *(const float4*)(xa + e), c = *(const float4*)(xb + e);
      float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w}, ao[4], co[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (m.mode == 1) {
          ao[k] = mix_blend(av[k], cv[k], m.lam, m.oml);
          co[k] = mix_blend(cv[k], av[k], m.lam, m.oml);
        } else {
          const bool in = xc + k >= m.xl && xc + k < m.xh;
          ao[k] = in ? cv[k] : av[k];
          co[k] = in ? av[k] : cv[k];
        }
      }
      *(float4*)(xa + e) = make_float4(ao[0], ao[1], ao[2], ao[3]);
      if (pb != b) *(float4*)(xb + e) = make_float4(co[0], co[1], co[2], co[3]);
    } else {
      const float a = xa[e], c = xb[e];
      if (m.mode == 1) {
        xa[e] = mix_blend(a, c, m.lam, m.oml);
        if (pb != b) xb[e] = mix_blend(c, a, m.lam, m.oml);
      } else {                                          // (inside the box: checked above)
        xa[e] = c;
        xb[e] = a;
      }
    }
  }
}

constexpr int XO = 62;                  // output positions per chunk
constexpr int COLS = XO * 4 + 4;        // clip columns held per chunk: x in [xc0*4 - 4, xc0*4 + 248)

// the aligned word at byte `addr` of the frames; where the buffer ends inside it, the bytes that exist
__device__ __forceinline__ uint32_t load_word(const uint8_t* __restrict__ frames, int64_t frames_bytes, int64_t addr) {
  uint32_t word = 0;
  if (addr + 4 <= frames_bytes) {
    word = *(const uint32_t*)(frames + addr);
  } else {                              // last bytes of the buffer
    for (int k = 0; k < 4; ++k)
      if (addr + k < frames_bytes) word |= (uint32_t)frames[addr + k] << (8 * k);
  }
  return word;
}

// The block walks the byte span [base, base + nbytes) of the frames in aligned 4-byte words, one word per thread and
// turn: f(j, byte) for every byte 0 <= j < nbytes of the span, each exactly once over the block.
template <class F>
__device__ __forceinline__ void walk_span(const uint8_t* __restrict__ frames, int64_t frames_bytes, int64_t base,
                                          int nbytes, const F& f) {
  const int64_t a0 = base & ~(int64_t)3;
  const int nwords = (int)((base + nbytes - a0 + 3) >> 2);
  for (int w = threadIdx.x; w < nwords; w += 256) {
    const int64_t addr = a0 + 4 * (int64_t)w;
    const uint32_t word = load_word(frames, frames_bytes, addr);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = (int)(addr + k - base);
      if (j < 0 || j >= nbytes) continue;
      f(j, (word >> (8 * k)) & 255u);
    }
  }
}

__device__ __forceinline__ void zero_image(bf16_t (*img)[COLS + 4]) {
  for (int i = threadIdx.x; i < 63 * (COLS + 4) / 2; i += 256) ((uint32_t*)img)[i] = 0u;
}

// the store phase: the image of the chunk that starts at output position xc0 -> 56 uint4 per position of the output
// row `out` (441 patch elements + 7 zeros; element (r, kx) of position xl is img[r][xl*4 + 1 + kx], x = xo*4 - 3 + kx)
__device__ __forceinline__ void store_chunk(const bf16_t (*img)[COLS + 4], bf16_t* __restrict__ out, int xc0, int Wo) {
  const int n_xo = min(XO, Wo - xc0);
  for (int i = threadIdx.x; i < n_xo * 56; i += 256) {
    const int xl = i / 56, chunk = i % 56;
    bf16_t e8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = chunk * 8 + e;
      const int kx = col % 7, r = col / 7;
      e8[e] = col < 441 ? img[r][xl * 4 + 1 + kx] : (bf16_t)0;
    }
    uint4 o;
    o.x = (uint32_t)e8[0] | ((uint32_t)e8[1] << 16); o.y = (uint32_t)e8[2] | ((uint32_t)e8[3] << 16);
    o.z = (uint32_t)e8[4] | ((uint32_t)e8[5] << 16); o.w = (uint32_t)e8[6] | ((uint32_t)e8[7] << 16);
    ((uint4*)out)[(size_t)(xc0 + xl) * 56 + chunk] = o;
  }
}

// Row b of the crop table (video, y0, x0); a null table is the identity (clip b = video b, no offset).  The host
// validates the table when it is built (svit_amd/input.py); a table rewritten on the device later is clamped into the
// frames here, so no entry can address outside them.
struct CropRow {
  int v, y0, x0;
  // byte offset of pixel (t, y, x) of the crop
  __device__ __forceinline__ int64_t byte_of(int T, int Hs, int Ws, int t, int y, int x) const {
    return ((((int64_t)v * T + t) * Hs + (y0 + y)) * Ws + (x0 + x)) * 3;
  }
};

__device__ __forceinline__ CropRow crop_row(const int32_t* __restrict__ crops, int b, int64_t frames_bytes, int T, int Hs,
                                            int Ws, int S) {
  const int64_t n_videos = frames_bytes / ((int64_t)T * Hs * Ws * 3);
  CropRow r = {crops ? crops[b * 3] : b, crops ? crops[b * 3 + 1] : 0, crops ? crops[b * 3 + 2] : 0};
  r.v = max(0, min(r.v, (int)n_videos - 1));
  r.y0 = max(0, min(r.y0, Hs - S));
  r.x0 = max(0, min(r.x0, Ws - S));
  return r;
}

__global__ __launch_bounds__(256) void im2col_patch_u8_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const bf16_t* __restrict__ lut,
    const int32_t* __restrict__ crops, bf16_t* __restrict__ cols, int T, int Hs, int Ws, int S,
    int To, int Ho, int Wo) {
  __shared__ bf16_t img[63][COLS + 4];  // normalised
  __shared__ bf16_t tab[768];
  const int yo = blockIdx.x % Ho, to = (blockIdx.x / Ho) % To, b = blockIdx.x / (Ho * To);
  const CropRow crop = crop_row(crops, b, frames_bytes, T, Hs, Ws, S);
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  bf16_t* out = cols + (((int64_t)b * To + to) * Ho + yo) * Wo * 448;
  for (int xc0 = 0; xc0 < Wo; xc0 += XO) {
    const int x_start = xc0 * 4 - 4;
    __syncthreads();                    // table ready / previous chunk's readers done
    // zero the image (padding), then drop the in-frame bytes of each (kt, ky) line: the three
    // channels of a pixel are adjacent bytes, so a line is one contiguous span of COLS*3 bytes
    zero_image(img);
    __syncthreads();
    for (int line = 0; line < 21; ++line) {
      const int ky = line % 7, kt = line / 7;
      const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
      if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
      const int xa = max(x_start, 0), xb = min(x_start + COLS, S);   // clip columns in the frame
      if (xb <= xa) continue;
      walk_span(frames, frames_bytes, crop.byte_of(T, Hs, Ws, t, y, xa), (xb - xa) * 3, [&](int j, uint32_t byte) {
        const int px = j / 3, c = j - px * 3;
        img[(c * 3 + kt) * 7 + ky][xa - x_start + px] = tab[c * 256 + byte];
      });
    }
    __syncthreads();
    store_chunk(img, out, xc0, Wo);
  }
}

// The partner of clip b is clip B-1-b, read through ITS crop row at the same (t, y, x) of the crop; its byte span has
// its own alignment (other x0, other base & 3), so phase A drops the partner's raw bytes of all 21 lines into LDS
// indexed by the byte position inside the span -- which is the same for both clips -- and phase B walks the clip's own
// words as the plain kernel does.
__global__ __launch_bounds__(256) void im2col_patch_u8_mix_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const float* __restrict__ lut,
    const int32_t* __restrict__ crops, const SvitMix* __restrict__ mix, bf16_t* __restrict__ cols,
    int B, int T, int Hs, int Ws, int S, int To, int Ho, int Wo) {
  __shared__ bf16_t img[63][COLS + 4];  // mixed + rounded
  __shared__ float tab[768];
  __shared__ uint8_t pbytes[21][COLS * 3];   // the partner's bytes of every (kt, ky) line
  const SvitMix m = *mix;
  const bool mixing = m.mode == 1 || m.mode == 2;
  const int yo = blockIdx.x % Ho, to = (blockIdx.x / Ho) % To, b = blockIdx.x / (Ho * To);
  const CropRow crop = crop_row(crops, b, frames_bytes, T, Hs, Ws, S);
  const CropRow crop2 = crop_row(crops, B - 1 - b, frames_bytes, T, Hs, Ws, S);
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  bf16_t* out = cols + (((int64_t)b * To + to) * Ho + yo) * Wo * 448;
  for (int xc0 = 0; xc0 < Wo; xc0 += XO) {
    const int x_start = xc0 * 4 - 4;
    const int xa = max(x_start, 0), xb = min(x_start + COLS, S);   // clip columns in the frame
    const int nbytes = (xb - xa) * 3;
    __syncthreads();                    // table ready / previous chunk's readers done
    zero_image(img);
    if (mixing && xb > xa) {
      for (int line = 0; line < 21; ++line) {
        const int ky = line % 7, kt = line / 7;
        const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
        if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
        walk_span(frames, frames_bytes, crop2.byte_of(T, Hs, Ws, t, y, xa), nbytes,
                  [&](int j, uint32_t byte) { pbytes[line][j] = (uint8_t)byte; });
      }
    }
    __syncthreads();
    for (int line = 0; line < 21; ++line) {
      const int ky = line % 7, kt = line / 7;
      const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
      if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
      if (xb <= xa) continue;
      const bool y_in = y >= m.yl && y < m.yh;
      walk_span(frames, frames_bytes, crop.byte_of(T, Hs, Ws, t, y, xa), nbytes, [&](int j, uint32_t byte) {
        const int px = j / 3, c = j - px * 3;
        float val = tab[c * 256 + byte];
        if (mixing) {
          const float other = tab[c * 256 + pbytes[line][j]];
          const int x = xa + px;
          if (m.mode == 1) val = mix_blend(val, other, m.lam, m.oml);
          else if (y_in && x >= m.xl && x < m.xh) val = other;
        }
        img[(c * 3 + kt) * 7 + ky][xa - x_start + px] = f32_to_bf16(val);
      });
    }
    __syncthreads();
    store_chunk(img, out, xc0, Wo);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Training augmentation on the uint8 route (svit_amd/augment.py): the reference's post-normalisation spatial pipeline
// -- random-resized crop or short-side jitter + crop with bilinear resampling (datasets/transform.py:47-105,154-191,
// 596-683), horizontal flip (transform.py:248-285) and random erasing of a cube (datasets/random_erasing.py) -- as a
// pure function of the output coordinate, driven by one 64-byte record per clip in device memory (SvitAug,
// include/svit_hip.h).  `aug_pixel` below is that function; svit_u8_clips_render writes its fp32 values,
// svit_im2col_patch_u8_aug rounds them once to bf16 while it assembles the patch-embedding operand, and
// svit_im2col_patch_u8_aug_frames does the same for the frames pass (every frame as a single-frame clip).
struct SvitAug {
  int video, i, j, h, w, out_h, out_w, oy, ox, flip, erase_mode, et, el, eh, ew, seed;
};

// a record clamped into its video's extent (the host validates at construction, svit_amd/augment.py; a record rewritten
// on the device can then still never address outside `frames_bytes`) + the two resampling scales.  `extents` int32
// [V,2] = (h_v, w_v), itself clamped into [1,Hs] x [1,Ws]: video v is the top-left h_v x w_v of each of its frames, the
// pitch stays Ws; null = every video fills the buffer.
struct AugGeom {
  int64_t vbase;                        // byte offset of the source video
  int i, j, h, w, oy, ox, flip, mode;
  int et, eb, el, er;                   // erase box [et, eb) x [el, er) in output coordinates
  float sy, sx;                         // float(in) / float(out), as F.interpolate(size=...) computes it
  uint32_t seed;
};
constexpr int AUG_MAX_OUT = 1 << 24;    // resampled sizes stay exact in fp32

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return max(lo, min(v, hi)); }

__device__ __forceinline__ AugGeom aug_geom(const SvitAug* __restrict__ aug, const int32_t* __restrict__ extents, int b,
                                            int64_t n_videos, int T, int Hs, int Ws, int S) {
  const SvitAug r = aug[b];
  AugGeom g;
  const int v = clampi(r.video, 0, (int)n_videos - 1);
  g.vbase = (int64_t)v * T * Hs * Ws * 3;
  const int hv = extents ? clampi(extents[2 * v], 1, Hs) : Hs, wv = extents ? clampi(extents[2 * v + 1], 1, Ws) : Ws;
  g.h = clampi(r.h, 1, hv);
  g.w = clampi(r.w, 1, wv);
  g.i = clampi(r.i, 0, hv - g.h);
  g.j = clampi(r.j, 0, wv - g.w);
  const int out_h = clampi(r.out_h, 1, AUG_MAX_OUT), out_w = clampi(r.out_w, 1, AUG_MAX_OUT);
  g.oy = clampi(r.oy, 0, max(out_h - S, 0));
  g.ox = clampi(r.ox, 0, max(out_w - S, 0));
  g.flip = r.flip != 0;
  g.mode = (r.erase_mode >= 1 && r.erase_mode <= 3) ? r.erase_mode : 0;
  g.et = clampi(r.et, 0, S);
  g.el = clampi(r.el, 0, S);
  g.eb = g.et + clampi(r.eh, 0, S - g.et);
  g.er = g.el + clampi(r.ew, 0, S - g.el);
  // the quotient in double, rounded once: the library is built with -ffast-math, whose fp32 division is a reciprocal
  // and a multiply -- up to 2 ulp off what the host computes
  g.sy = (float)((double)g.h / (double)out_h);
  g.sx = (float)((double)g.w / (double)out_w);
  g.seed = (uint32_t)r.seed;
  return g;
}

// One axis of F.interpolate(mode="bilinear", align_corners=False): destination index -> the two source indices and their
// weights (ATen area_pixel_compute_source_index + guard_index_and_lambda).  The weights are made opaque so that
// -ffast-math cannot rewrite the lerps that consume them differently in the two kernels that inline this.
__device__ __forceinline__ void aug_axis(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  l0 = 1.f - l1;
  __asm__("" : "+v"(l0));
  __asm__("" : "+v"(l1));
}

// (aug_noise, the N(0,1) of the erasing noise, lives in common.h: csrc/attrib.hip draws the same field)

// taps straight from global memory: pixel (r, col) of the record's rectangle in frame t -> its three bytes
struct AugGlobalFetch {
  const uint8_t* __restrict__ frames;
  int64_t vbase;
  int Hs, Ws, i, j;
  __device__ __forceinline__ uint32_t operator()(int t, int r, int col) const {
    const uint8_t* p = frames + vbase + (((int64_t)t * Hs + (i + r)) * Ws + (j + col)) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
};

// The fp32 value of output pixel (t, y, x) of clip b, all three channels: erased (inside the box, on every frame), or
// the bilinear resample of the normalised source rectangle.  `tab` f32 [3][256] is the normalisation table.  With
// in == out the weights are exactly 1 and 0 and the value is the tap itself.
template <class Fetch>
__device__ __forceinline__ void aug_pixel(const AugGeom& g, const float* tab, const Fetch& fetch, int b, int t, int y,
                                          int x, int T, int S, float (&v)[3]) {
  if (g.mode && y >= g.et && y < g.eb && x >= g.el && x < g.er) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[c] = g.mode == 1 ? 0.f : aug_noise(g.seed, b, c * T + t, g.mode == 3 ? (uint32_t)(y * S + x) : 0xFFFFFFFFu);
    return;
  }
  const int xs = g.flip ? S - 1 - x : x;
  int r0, r1, c0, c1;
  float l0y, l1y, l0x, l1x;
  aug_axis(g.oy + y, g.h, g.sy, r0, r1, l0y, l1y);
  aug_axis(g.ox + xs, g.w, g.sx, c0, c1, l0x, l1x);
  const uint32_t pa = fetch(t, r0, c0), pb = fetch(t, r0, c1), pc = fetch(t, r1, c0), pd = fetch(t, r1, c1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = tab[c * 256 + ((pa >> (8 * c)) & 255u)], bb = tab[c * 256 + ((pb >> (8 * c)) & 255u)];
    const float cc = tab[c * 256 + ((pc >> (8 * c)) & 255u)], d = tab[c * 256 + ((pd >> (8 * c)) & 255u)];
    float p = l1x * bb, q = l1x * d;
    __asm__("" : "+v"(p));
    __asm__("" : "+v"(q));
    const float top = __builtin_fmaf(l0x, a, p), bot = __builtin_fmaf(l0x, cc, q);
    float s = l1y * bot;
    __asm__("" : "+v"(s));
    v[c] = __builtin_fmaf(l0y, top, s);
  }
}

__global__ __launch_bounds__(256) void u8_clips_render_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const float* __restrict__ lut,
    const SvitAug* __restrict__ aug, const int32_t* __restrict__ extents, float* __restrict__ out, int T, int Hs, int Ws,
    int S) {
  __shared__ float tab[768];
  const int b = blockIdx.y / T, t = blockIdx.y % T;
  const int64_t n_videos = frames_bytes / ((int64_t)T * Hs * Ws * 3);
  const AugGeom g = aug_geom(aug, extents, b, n_videos, T, Hs, Ws, S);
  const AugGlobalFetch fetch{frames, g.vbase, Hs, Ws, g.i, g.j};
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  __syncthreads();
  const int n = S * S;
  float* o = out + ((int64_t)b * 3 * T + t) * n;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    float v[3];
    aug_pixel(g, tab, fetch, b, t, p / S, p % S, T, S, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(int64_t)c * T * n + p] = v[c];
  }
}

// svit_im2col_patch_u8 with the fill phase going through aug_pixel.  Same grid, same LDS image and the same store phase.
// Per chunk the block needs, of each of its three frames, the source rows [r_lo, r_hi] x columns [c_lo, c_hi] that the
// 7 output rows x COLS output columns resample from; where that rectangle fits AUG_STAGE bytes (img + tab + stage =
// 51.5 KB, three blocks per CU like the mix kernel) it is staged into LDS with aligned word loads -- every source byte
// is then fetched from memory once per block instead of once per tap -- otherwise the taps are gathered from global
// memory.  The mix partner (clip B-1-b through its own record) is always gathered: it is needed on mixing steps only.
//
// FRAMES = true is the frames pass (svit_im2col_patch_u8_aug_frames): the operand of the B*T single-frame clips
// [B*T,3,1,S,S], frame n = b*T + t.  A block is (n, yo); To = 1, so of the 21 (kt, ky) lines only the seven kt = 1
// lines hold a frame -- frame t of clip b, through aug_pixel with the clip's own (b, t, T), so geometry, erase noise and
// mix partner (frame t of clip B-1-b) are the clip pass's -- and the other fourteen are the temporal padding: the image
// is zeroed once and the fill writes the kt = 1 lines only.  One frame's rectangle is staged instead of three, within
// AUG_STAGE_FRAMES = AUG_STAGE / 3: the rectangle that fits is the one that fits the clip kernel, so a record takes the
// same path in both passes, and img + tab + stage = 39.8 KB goes four times into a CU's 160 KB instead of three (the
// block fills a third of the clip kernel's pixels and stores as much: more resident waves behind the stores).
constexpr int AUG_STAGE = 16384;
constexpr int AUG_STAGE_FRAMES = 5460;

// taps from the staged rectangle: row (kt, r) starts at the byte its global address has modulo 4, so the staging
// copies whole words
struct AugStageFetch {
  const uint8_t* st;
  int t0, r_lo, c_lo, nrows, pitch;
  uint32_t rowbase;                     // (video*T*Hs + i) modulo 2^32: only the address modulo 4 is needed
  int Hs, Ws, jc;                       // jc = j + c_lo
  __device__ __forceinline__ uint32_t operator()(int t, int r, int col) const {
    const uint32_t mis = (((rowbase + (uint32_t)t * Hs + r) * Ws + jc) * 3u) & 3u;
    const uint8_t* p = st + ((t - t0) * nrows + (r - r_lo)) * pitch + mis + (col - c_lo) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
};

template <bool FRAMES>
__global__ __launch_bounds__(256) void im2col_patch_u8_aug_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const float* __restrict__ lut,
    const SvitAug* __restrict__ aug, const int32_t* __restrict__ extents, const SvitMix* __restrict__ mix,
    bf16_t* __restrict__ cols, int B, int T, int Hs, int Ws, int S, int To, int Ho, int Wo) {
  constexpr int KT = FRAMES ? 1 : 3;             // frames a block reads
  constexpr int LINE0 = FRAMES ? 7 : 0;          // first (kt, ky) line the fill writes, KT * 7 of them
  constexpr int STAGE = FRAMES ? AUG_STAGE_FRAMES : AUG_STAGE;
  __shared__ bf16_t img[63][COLS + 4];  // augmented + mixed + rounded
  __shared__ float tab[768];
  __shared__ uint32_t stage[STAGE / 4];
  SvitMix m = {0, 1.f, 0.f, 0, 0, 0, 0, 0};
  if (mix) m = *mix;
  const bool mixing = m.mode == 1 || m.mode == 2;
  // clip n = b*To + to of the output (FRAMES: To = 1 and n = b*T + t, one single-frame clip per frame)
  const int yo = blockIdx.x % Ho, n = blockIdx.x / Ho;
  const int b = FRAMES ? n / T : n / To;
  const int pb = B - 1 - b;
  const int64_t n_videos = frames_bytes / ((int64_t)T * Hs * Ws * 3);
  const AugGeom g = aug_geom(aug, extents, b, n_videos, T, Hs, Ws, S);
  const AugGeom g2 = aug_geom(aug, extents, pb, n_videos, T, Hs, Ws, S);
  const AugGlobalFetch gfetch{frames, g.vbase, Hs, Ws, g.i, g.j};
  const AugGlobalFetch gfetch2{frames, g2.vbase, Hs, Ws, g2.i, g2.j};
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  if (FRAMES) zero_image(img);          // the kt = 0 and kt = 2 lines stay zero: no chunk writes them
  bf16_t* out = cols + ((int64_t)n * Ho + yo) * Wo * 448;
  // tap kt is frame t0 + kt (FRAMES: the one tap kt = 1 is frame n - b*T); the staged frames start at ts
  const int t0 = FRAMES ? n - b * T - 1 : (n - b * To) * 2 - 1, ts = FRAMES ? t0 + 1 : t0, y0 = yo * 4 - 3;
  // the source rows of the block's output rows (the same for every chunk)
  const int ya = max(y0, 0), yb = min(y0 + 7, S);
  int r_lo, r_hi, tmp;
  float f0, f1;
  aug_axis(g.oy + ya, g.h, g.sy, r_lo, tmp, f0, f1);
  aug_axis(g.oy + yb - 1, g.h, g.sy, tmp, r_hi, f0, f1);
  const int nrows = r_hi - r_lo + 1;
  for (int xc0 = 0; xc0 < Wo; xc0 += XO) {
    const int x_start = xc0 * 4 - 4;
    const int xa = max(x_start, 0), xb = min(x_start + COLS, S);   // clip columns in the frame
    // the source columns of this chunk's output columns (xs = S-1-x under the flip: the range is mirrored)
    int c_lo = 0, c_hi = 0;
    if (xb > xa) {
      aug_axis(g.ox + (g.flip ? S - xb : xa), g.w, g.sx, c_lo, tmp, f0, f1);
      aug_axis(g.ox + (g.flip ? S - 1 - xa : xb - 1), g.w, g.sx, tmp, c_hi, f0, f1);
    }
    const int rowbytes = (c_hi - c_lo + 1) * 3, pitch = (rowbytes + 6) & ~3;
    const bool staged = xb > xa && (int64_t)KT * nrows * pitch <= STAGE;
    __syncthreads();                    // table ready / previous chunk's readers done
    if (staged) {
      for (int kr = 0; kr < KT * nrows; ++kr) {
        const int kt = kr / nrows, r = r_lo + kr - kt * nrows, t = ts + kt;
        if (t < 0 || t >= T) continue;                               // uniform over the block
        const int64_t base = g.vbase + (((int64_t)t * Hs + (g.i + r)) * Ws + (g.j + c_lo)) * 3;
        const int64_t a0 = base & ~(int64_t)3;                       // aligned 4-byte words
        const int nwords = (int)((base + rowbytes - a0 + 3) >> 2);   // <= pitch / 4
        uint32_t* dst = stage + kr * (pitch >> 2);
        for (int w = threadIdx.x; w < nwords; w += 256) dst[w] = load_word(frames, frames_bytes, a0 + 4 * (int64_t)w);
      }
      __syncthreads();
    }
    const AugStageFetch sfetch{(const uint8_t*)stage, ts, r_lo, c_lo, nrows, pitch,
                               (uint32_t)(g.vbase / ((int64_t)Ws * 3)) + (uint32_t)g.i, Hs, Ws, g.j + c_lo};
    // every element of the KT * 7 lines is written here (0 outside the clip): no separate zero pass
    for (int p = threadIdx.x; p < KT * 7 * COLS; p += 256) {
      const int line = LINE0 + p / COLS, px = p - (line - LINE0) * COLS;
      const int ky = line % 7, kt = line / 7;
      const int t = t0 + kt, y = y0 + ky, x = x_start + px;
      float v[3] = {0.f, 0.f, 0.f};
      if (t >= 0 && t < T && y >= 0 && y < S && x >= 0 && x < S) {
        if (staged) aug_pixel(g, tab, sfetch, b, t, y, x, T, S, v);
        else aug_pixel(g, tab, gfetch, b, t, y, x, T, S, v);
        if (mixing && (m.mode == 1 || (y >= m.yl && y < m.yh && x >= m.xl && x < m.xh))) {
          float o[3];
          aug_pixel(g2, tab, gfetch2, pb, t, y, x, T, S, o);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c] = m.mode == 1 ? mix_blend(v[c], o[c], m.lam, m.oml) : o[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) img[(c * 3 + kt) * 7 + ky][px] = f32_to_bf16(v[c]);
    }
    __syncthreads();
    store_chunk(img, out, xc0, Wo);
  }
}
}  // namespace

// the output grid of the patch embedding Conv3d(k(3,7,7), s(2,4,4), p(1,3,3)) over T frames of S x S
struct PatchGrid {
  int To, Ho, Wo;
};
static PatchGrid patch_grid(int T, int S) { return {(T + 2 - 3) / 2 + 1, (S + 6 - 7) / 4 + 1, (S + 6 - 7) / 4 + 1}; }

extern "C" int svit_im2col_patch_u8(const uint8_t* frames, int64_t frames_bytes, const void* lut,
                                    const int32_t* crops, void* cols, int B, int T, int Hs,
                                    int Ws, int S, void* stream) {
  if (!frames || !lut || !cols) return SVIT_ERR_ARG;
  if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || S > Hs || S > Ws) return SVIT_ERR_SHAPE;
  if ((uintptr_t)frames & 3) return SVIT_ERR_ALIGN;
  const PatchGrid g = patch_grid(T, S);
  hipLaunchKernelGGL(im2col_patch_u8_kernel, dim3((unsigned)(B * g.To * g.Ho)), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, (const bf16_t*)lut, crops,
                     (bf16_t*)cols, T, Hs, Ws, S, g.To, g.Ho, g.Wo);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_im2col_patch_u8_mix(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                        const int32_t* crops, const void* mix, void* cols, int B, int T,
                                        int Hs, int Ws, int S, void* stream) {
  if (!frames || !lut_f32 || !mix || !cols) return SVIT_ERR_ARG;
  if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || S > Hs || S > Ws) return SVIT_ERR_SHAPE;
  if (frames_bytes < (int64_t)T * Hs * Ws * 3) return SVIT_ERR_SHAPE;
  if (((uintptr_t)frames | (uintptr_t)mix | (uintptr_t)lut_f32) & 3) return SVIT_ERR_ALIGN;
  const PatchGrid g = patch_grid(T, S);
  hipLaunchKernelGGL(im2col_patch_u8_mix_kernel, dim3((unsigned)(B * g.To * g.Ho)), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, lut_f32, crops, (const SvitMix*)mix,
                     (bf16_t*)cols, B, T, Hs, Ws, S, g.To, g.Ho, g.Wo);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_mixup_clips(float* x, const void* mix, int B, int planes, int H, int W, void* stream) {
  if (!x || !mix) return SVIT_ERR_ARG;
  if (B <= 0 || planes <= 0 || H <= 0 || W <= 0) return SVIT_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)mix) & 3) return SVIT_ERR_ALIGN;
  const int64_t n = (int64_t)planes * H * W;          // elements per clip
  if (n >= ((int64_t)1 << 31)) return SVIT_ERR_SHAPE;
  const int pairs = (B + 1) / 2;                      // (odd B: the middle clip is its own partner)
  if (pairs > 65535) return SVIT_ERR_SHAPE;
  const bool vec = !(W & 3) && !((uintptr_t)x & 15);
  const int64_t nv = vec ? n / 4 : n;
  int64_t blocks = (nv + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (vec)
    hipLaunchKernelGGL(mixup_clips_kernel<true>, dim3((unsigned)blocks, (unsigned)pairs), dim3(256), 0,
                       (hipStream_t)stream, x, (const SvitMix*)mix, B, (uint32_t)n, (uint32_t)H, (uint32_t)W);
  else
    hipLaunchKernelGGL(mixup_clips_kernel<false>, dim3((unsigned)blocks, (unsigned)pairs), dim3(256), 0,
                       (hipStream_t)stream, x, (const SvitMix*)mix, B, (uint32_t)n, (uint32_t)H, (uint32_t)W);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

static int aug_args_ok(const void* frames, int64_t frames_bytes, const void* lut_f32, const void* aug,
                       const void* extents, const void* out, int B, int T, int Hs, int Ws, int S) {
  if (!frames || !lut_f32 || !aug || !out) return SVIT_ERR_ARG;
  if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || S > 16384 || Hs > 32768 || Ws > 32768) return SVIT_ERR_SHAPE;
  if (frames_bytes < (int64_t)T * Hs * Ws * 3) return SVIT_ERR_SHAPE;                 // at least one whole video
  if (frames_bytes / ((int64_t)T * Hs * Ws * 3) > 0x7fffffff) return SVIT_ERR_SHAPE;
  if (((uintptr_t)frames | (uintptr_t)lut_f32 | (uintptr_t)aug | (uintptr_t)extents | (uintptr_t)out) & 3)
    return SVIT_ERR_ALIGN;
  return SVIT_OK;
}

// both passes of the augmented im2col: FRAMES = the B*T frames as single-frame clips (To = 1)
template <bool FRAMES>
static int launch_im2col_aug(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                             const int32_t* extents, const void* mix, void* cols, int B, int T, int Hs, int Ws, int S,
                             void* stream) {
  const int rc = aug_args_ok(frames, frames_bytes, lut_f32, aug, extents, cols, B, T, Hs, Ws, S);
  if (rc != SVIT_OK) return rc;
  if (((uintptr_t)mix & 3) || ((uintptr_t)cols & 15)) return SVIT_ERR_ALIGN;
  const PatchGrid g = patch_grid(FRAMES ? 1 : T, S);
  const int64_t blocks = (int64_t)B * (FRAMES ? T : g.To) * g.Ho;
  if (blocks > 0x7fffffff) return SVIT_ERR_SHAPE;
  hipLaunchKernelGGL(im2col_patch_u8_aug_kernel<FRAMES>, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, lut_f32, (const SvitAug*)aug, extents,
                     (const SvitMix*)mix, (bf16_t*)cols, B, T, Hs, Ws, S, g.To, g.Ho, g.Wo);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_im2col_patch_u8_aug_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                            const void* aug, const int32_t* extents, const void* mix, void* cols, int B,
                                            int T, int Hs, int Ws, int S, void* stream) {
  return launch_im2col_aug<false>(frames, frames_bytes, lut_f32, aug, extents, mix, cols, B, T, Hs, Ws, S, stream);
}

extern "C" int svit_im2col_patch_u8_aug_frames_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                                   const void* aug, const int32_t* extents, const void* mix, void* cols,
                                                   int B, int T, int Hs, int Ws, int S, void* stream) {
  return launch_im2col_aug<true>(frames, frames_bytes, lut_f32, aug, extents, mix, cols, B, T, Hs, Ws, S, stream);
}

extern "C" int svit_u8_clips_render_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                        const void* aug, const int32_t* extents, float* out_f32, int B, int T, int Hs,
                                        int Ws, int S, void* stream) {
  const int rc = aug_args_ok(frames, frames_bytes, lut_f32, aug, extents, out_f32, B, T, Hs, Ws, S);
  if (rc != SVIT_OK) return rc;
  if ((int64_t)B * T > 65535) return SVIT_ERR_SHAPE;
  int blocks = (S * S + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(u8_clips_render_kernel, dim3((unsigned)blocks, (unsigned)(B * T)), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, lut_f32, (const SvitAug*)aug, extents, out_f32, T, Hs,
                     Ws, S);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_im2col_patch_u8_aug(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                        const void* aug, const void* mix, void* cols, int B, int T, int Hs,
                                        int Ws, int S, void* stream) {
  return svit_im2col_patch_u8_aug_ext(frames, frames_bytes, lut_f32, aug, nullptr, mix, cols, B, T, Hs, Ws, S, stream);
}

extern "C" int svit_im2col_patch_u8_aug_frames(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                               const void* aug, const void* mix, void* cols, int B, int T, int Hs,
                                               int Ws, int S, void* stream) {
  return svit_im2col_patch_u8_aug_frames_ext(frames, frames_bytes, lut_f32, aug, nullptr, mix, cols, B, T, Hs, Ws, S,
                                             stream);
}

extern "C" int svit_u8_clips_render(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                                    const void* aug, float* out_f32, int B, int T, int Hs, int Ws, int S,
                                    void* stream) {
  return svit_u8_clips_render_ext(frames, frames_bytes, lut_f32, aug, nullptr, out_f32, B, T, Hs, Ws, S, stream);
}
