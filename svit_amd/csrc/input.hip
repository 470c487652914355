// Input pipeline fused into the patch embedding -- gfx950.
//
// The reference normalises decoded uint8 frames on the host ((u/255 - mean)/std,
// slowfast/datasets/utils.py:287-303), permutes T H W C -> C T H W, crops (transform.py:288-348)
// and ships fp32 clips to the GPU (misc.iter_to_cuda, slowfast/utils/misc.py:374-387): 4 bytes
// per sample over PCIe and HBM, plus a materialised copy per spatial crop.  Here the clip stays
// uint8 [V,T,Hs,Ws,3] in HBM; normalisation is a 3 x 256-entry table (built with the reference's
// own fp32 operation order, so the values are bit-identical), the crop is an (y0, x0) offset per
// output clip, and both are applied while the im2col rows of Conv3d(3->96, k(3,7,7), s(2,4,4),
// p(1,3,3)) (stem_helper.py:309-320) are assembled -- same [rows, 448] bf16 operand as
// svit_im2col_patch, a quarter of the input bytes, no per-crop copy.
//
// Mixup / CutMix (cfg.MIXUP; slowfast/datasets/mixup.py, tools/train_net.py:63-71,92-94) lives here too.
// Every kernel of the feature reads ONE 32-byte record from device memory (SvitMix below), so a
// captured step holds the same launches whatever was drawn for it: `svit_mixup_clips` blends /
// swaps the fp32 clips of a batch in place against the batch reversed, and
// `svit_im2col_patch_u8_mix` does the same on the uint8 route between the fp32 normalisation and
// the bf16 rounding (uint8 frames cannot be blended in place without losing the fp32 arithmetic).
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

__global__ __launch_bounds__(256) void im2col_patch_u8_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const bf16_t* __restrict__ lut,
    const int32_t* __restrict__ crops, bf16_t* __restrict__ cols, int T, int Hs, int Ws, int S,
    int To, int Ho, int Wo) {
  __shared__ bf16_t img[63][COLS + 4];  // [(c*3+kt)*7+ky][x - x_start], normalised, 0 = padding
  __shared__ bf16_t tab[768];
  const int yo = blockIdx.x % Ho, to = (blockIdx.x / Ho) % To, b = blockIdx.x / (Ho * To);
  // the host validates the crop table when it is built (svit_amd/input.py); a table rewritten
  // on the device later is clamped into the frames here, so no entry can address outside them
  int v = crops ? crops[b * 3] : b, y0 = crops ? crops[b * 3 + 1] : 0,
      x0 = crops ? crops[b * 3 + 2] : 0;
  const int64_t n_videos = frames_bytes / ((int64_t)T * Hs * Ws * 3);
  v = max(0, min(v, (int)n_videos - 1));
  y0 = max(0, min(y0, Hs - S));
  x0 = max(0, min(x0, Ws - S));
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  bf16_t* out = cols + (((int64_t)b * To + to) * Ho + yo) * Wo * 448;
  for (int xc0 = 0; xc0 < Wo; xc0 += XO) {
    const int x_start = xc0 * 4 - 4;
    __syncthreads();                    // table ready / previous chunk's readers done
    // zero the image (padding), then drop the in-frame bytes of each (kt, ky) line: the three
    // channels of a pixel are adjacent bytes, so a line is one contiguous span of COLS*3 bytes
    for (int i = threadIdx.x; i < 63 * (COLS + 4) / 2; i += 256) ((uint32_t*)img)[i] = 0u;
    __syncthreads();
    for (int line = 0; line < 21; ++line) {
      const int ky = line % 7, kt = line / 7;
      const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
      if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
      const int xa = max(x_start, 0), xb = min(x_start + COLS, S);   // clip columns in the frame
      if (xb <= xa) continue;
      const int64_t base = ((((int64_t)v * T + t) * Hs + (y0 + y)) * Ws + (x0 + xa)) * 3;
      const int nbytes = (xb - xa) * 3;
      const int64_t a0 = base & ~(int64_t)3;                       // aligned 4-byte words
      const int nwords = (int)((base + nbytes - a0 + 3) >> 2);
      for (int w = threadIdx.x; w < nwords; w += 256) {
        const int64_t addr = a0 + 4 * (int64_t)w;
        uint32_t word = 0;
        if (addr + 4 <= frames_bytes) {
          word = *(const uint32_t*)(frames + addr);
        } else {                                                    // last bytes of the buffer
          for (int k = 0; k < 4; ++k)
            if (addr + k < frames_bytes) word |= (uint32_t)frames[addr + k] << (8 * k);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = (int)(addr + k - base);                    // byte index inside the span
          if (j < 0 || j >= nbytes) continue;
          const int px = j / 3, c = j - px * 3;
          img[(c * 3 + kt) * 7 + ky][xa - x_start + px] = tab[c * 256 + ((word >> (8 * k)) & 255u)];
        }
      }
    }
    __syncthreads();
    const int n_xo = min(XO, Wo - xc0);
    for (int i = threadIdx.x; i < n_xo * 56; i += 256) {
      const int xl = i / 56, chunk = i % 56;
      bf16_t e8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = chunk * 8 + e;
        const int kx = col % 7, r = col / 7;
        e8[e] = col < 441 ? img[r][xl * 4 + 1 + kx] : (bf16_t)0;   // x = xo*4 - 3 + kx
      }
      uint4 o;
      o.x = (uint32_t)e8[0] | ((uint32_t)e8[1] << 16); o.y = (uint32_t)e8[2] | ((uint32_t)e8[3] << 16);
      o.z = (uint32_t)e8[4] | ((uint32_t)e8[5] << 16); o.w = (uint32_t)e8[6] | ((uint32_t)e8[7] << 16);
      ((uint4*)out)[(size_t)(xc0 + xl) * 56 + chunk] = o;
    }
  }
}
// svit_im2col_patch_u8 with the mix between the normalisation and the bf16 rounding.  The partner
// of clip b is clip B-1-b, read through ITS crop row at the same (t, y, x) of the crop; its byte
// span has its own alignment (other x0, other base & 3), so phase A drops the partner's raw bytes
// of all 21 lines into LDS indexed by the byte position inside the span -- which is the same for
// both clips -- and phase B walks the clip's own words as the plain kernel does.
__global__ __launch_bounds__(256) void im2col_patch_u8_mix_kernel(
    const uint8_t* __restrict__ frames, int64_t frames_bytes, const float* __restrict__ lut,
    const int32_t* __restrict__ crops, const SvitMix* __restrict__ mix, bf16_t* __restrict__ cols,
    int B, int T, int Hs, int Ws, int S, int To, int Ho, int Wo) {
  __shared__ bf16_t img[63][COLS + 4];  // [(c*3+kt)*7+ky][x - x_start], mixed + rounded, 0 = padding
  __shared__ float tab[768];
  __shared__ uint8_t pbytes[21][COLS * 3];   // the partner's bytes of every (kt, ky) line
  const SvitMix m = *mix;
  const bool mixing = m.mode == 1 || m.mode == 2;
  const int yo = blockIdx.x % Ho, to = (blockIdx.x / Ho) % To, b = blockIdx.x / (Ho * To);
  const int pb = B - 1 - b;
  const int64_t n_videos = frames_bytes / ((int64_t)T * Hs * Ws * 3);
  int v = crops ? crops[b * 3] : b, y0 = crops ? crops[b * 3 + 1] : 0, x0 = crops ? crops[b * 3 + 2] : 0;
  int v2 = crops ? crops[pb * 3] : pb, y02 = crops ? crops[pb * 3 + 1] : 0, x02 = crops ? crops[pb * 3 + 2] : 0;
  v = max(0, min(v, (int)n_videos - 1));
  y0 = max(0, min(y0, Hs - S));
  x0 = max(0, min(x0, Ws - S));
  v2 = max(0, min(v2, (int)n_videos - 1));
  y02 = max(0, min(y02, Hs - S));
  x02 = max(0, min(x02, Ws - S));
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  bf16_t* out = cols + (((int64_t)b * To + to) * Ho + yo) * Wo * 448;
  for (int xc0 = 0; xc0 < Wo; xc0 += XO) {
    const int x_start = xc0 * 4 - 4;
    const int xa = max(x_start, 0), xb = min(x_start + COLS, S);   // clip columns in the frame
    const int nbytes = (xb - xa) * 3;
    __syncthreads();                    // table ready / previous chunk's readers done
    for (int i = threadIdx.x; i < 63 * (COLS + 4) / 2; i += 256) ((uint32_t*)img)[i] = 0u;
    if (mixing && xb > xa) {
      for (int line = 0; line < 21; ++line) {
        const int ky = line % 7, kt = line / 7;
        const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
        if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
        const int64_t base = ((((int64_t)v2 * T + t) * Hs + (y02 + y)) * Ws + (x02 + xa)) * 3;
        const int64_t a0 = base & ~(int64_t)3;
        const int nwords = (int)((base + nbytes - a0 + 3) >> 2);
        for (int w = threadIdx.x; w < nwords; w += 256) {
          const int64_t addr = a0 + 4 * (int64_t)w;
          uint32_t word = 0;
          if (addr + 4 <= frames_bytes) {
            word = *(const uint32_t*)(frames + addr);
          } else {
            for (int k = 0; k < 4; ++k)
              if (addr + k < frames_bytes) word |= (uint32_t)frames[addr + k] << (8 * k);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int j = (int)(addr + k - base);
            if (j >= 0 && j < nbytes) pbytes[line][j] = (uint8_t)((word >> (8 * k)) & 255u);
          }
        }
      }
    }
    __syncthreads();
    for (int line = 0; line < 21; ++line) {
      const int ky = line % 7, kt = line / 7;
      const int t = to * 2 - 1 + kt, y = yo * 4 - 3 + ky;
      if (t < 0 || t >= T || y < 0 || y >= S) continue;          // uniform over the block
      if (xb <= xa) continue;
      const int64_t base = ((((int64_t)v * T + t) * Hs + (y0 + y)) * Ws + (x0 + xa)) * 3;
      const int64_t a0 = base & ~(int64_t)3;                       // aligned 4-byte words
      const int nwords = (int)((base + nbytes - a0 + 3) >> 2);
      const bool y_in = y >= m.yl && y < m.yh;
      for (int w = threadIdx.x; w < nwords; w += 256) {
        const int64_t addr = a0 + 4 * (int64_t)w;
        uint32_t word = 0;
        if (addr + 4 <= frames_bytes) {
          word = *(const uint32_t*)(frames + addr);
        } else {                                                    // last bytes of the buffer
          for (int k = 0; k < 4; ++k)
            if (addr + k < frames_bytes) word |= (uint32_t)frames[addr + k] << (8 * k);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = (int)(addr + k - base);                    // byte index inside the span
          if (j < 0 || j >= nbytes) continue;
          const int px = j / 3, c = j - px * 3;
          float val = tab[c * 256 + ((word >> (8 * k)) & 255u)];
          if (mixing) {
            const float other = tab[c * 256 + pbytes[line][j]];
            const int x = xa + px;
            if (m.mode == 1) val = mix_blend(val, other, m.lam, m.oml);
            else if (y_in && x >= m.xl && x < m.xh) val = other;
          }
          img[(c * 3 + kt) * 7 + ky][xa - x_start + px] = f32_to_bf16(val);
        }
      }
    }
    __syncthreads();
    const int n_xo = min(XO, Wo - xc0);
    for (int i = threadIdx.x; i < n_xo * 56; i += 256) {
      const int xl = i / 56, chunk = i % 56;
      bf16_t e8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = chunk * 8 + e;
        const int kx = col % 7, r = col / 7;
        e8[e] = col < 441 ? img[r][xl * 4 + 1 + kx] : (bf16_t)0;   // x = xo*4 - 3 + kx
      }
      uint4 o;
      o.x = (uint32_t)e8[0] | ((uint32_t)e8[1] << 16); o.y = (uint32_t)e8[2] | ((uint32_t)e8[3] << 16);
      o.z = (uint32_t)e8[4] | ((uint32_t)e8[5] << 16); o.w = (uint32_t)e8[6] | ((uint32_t)e8[7] << 16);
      ((uint4*)out)[(size_t)(xc0 + xl) * 56 + chunk] = o;
    }
  }
}
}  // namespace

extern "C" int svit_im2col_patch_u8(const uint8_t* frames, int64_t frames_bytes, const void* lut,
                                    const int32_t* crops, void* cols, int B, int T, int Hs,
                                    int Ws, int S, void* stream) {
  if (!frames || !lut || !cols) return SVIT_ERR_ARG;
  if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || S > Hs || S > Ws) return SVIT_ERR_SHAPE;
  if ((uintptr_t)frames & 3) return SVIT_ERR_ALIGN;
  const int To = (T + 2 - 3) / 2 + 1, Ho = (S + 6 - 7) / 4 + 1, Wo = (S + 6 - 7) / 4 + 1;
  hipLaunchKernelGGL(im2col_patch_u8_kernel, dim3((unsigned)(B * To * Ho)), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, (const bf16_t*)lut, crops,
                     (bf16_t*)cols, T, Hs, Ws, S, To, Ho, Wo);
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
  const int To = (T + 2 - 3) / 2 + 1, Ho = (S + 6 - 7) / 4 + 1, Wo = (S + 6 - 7) / 4 + 1;
  hipLaunchKernelGGL(im2col_patch_u8_mix_kernel, dim3((unsigned)(B * To * Ho)), dim3(256), 0,
                     (hipStream_t)stream, frames, frames_bytes, lut_f32, crops, (const SvitMix*)mix,
                     (bf16_t*)cols, B, T, Hs, Ws, S, To, Ho, Wo);
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
