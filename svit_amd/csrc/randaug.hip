// RandAugment on uint8 frames where they lie (cfg.AUG.AA_TYPE; svit_amd/randaug.py) -- gfx950.
//
// The reference's loader runs `create_random_augment(...)` on every training clip before anything else
// (slowfast/datasets/ssv2.py:345-375, rand_augment.py): N randomly chosen PIL operations on each uint8 frame at
// source resolution.  Here the frames are u8 [V,T,Hs,Ws,3] in HBM and what was drawn is one 64-byte record per
// (video, layer) in DEVICE memory (SvitRandAugOp, include/svit_hip.h), so a captured step holds the same 2N
// launches for every draw.  Per layer: `svit_randaug_stats` (histogram -> AutoContrast / Equalize table, Contrast
// mean; per FRAME, as PIL sees one image at a time) and `svit_randaug_apply` (src -> dst, every byte written).
//
// Per-video extents (the `_ext` entry points; include/svit_hip.h): the buffer is padded, video v is the tight
// h_v x w_v image in the top-left corner of each of its frames, row pitch Ws.  Statistics, the affine in-range test,
// the tap clamps and the Sharpness interior all see that image; the padding is copied.  The grid stays over Hs*Ws.
//
// The bar is PIL's bytes, so every operation keeps PIL's arithmetic and its ORDER: integer tables, the fp32 blend of
// ImagingBlend and the fp32 3x3 smooth of ImagingFilter with product and sum rounded separately, the fp64
// coordinates and bilinear / bicubic filters of ImagingGenericTransform.  This file is therefore compiled WITHOUT
// -ffast-math and with -ffp-contract=off (svit_amd/build.py, SOURCE_FLAGS): under the library's common flags the
// backend fuses a multiply into the add that consumes it whatever the source says (csrc/input.hip, mix_blend).
#include "common.h"
#include "../../include/svit_hip.h"

static_assert(sizeof(SvitRandAugOp) == 64, "one record is 64 bytes");

namespace {
enum { RA_NONE = 0, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR,
       RA_CONTRAST, RA_BRIGHTNESS, RA_SHARPNESS, RA_AFFINE };
constexpr int RA_SLOT = 1024;        // workspace bytes per (video, frame): 3 x 256 table, the mean as int32 at 768
constexpr int RA_MEAN_AT = 768;
constexpr int RA_FILL = 128;

__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ra_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// PIL's clip8: 0 up to 0 (and for a NaN), 255 from 255, truncation between
__device__ __forceinline__ int ra_clip8(float t) { return !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t); }
__device__ __forceinline__ int ra_clip8(double t) { return !(t > 0.0) ? 0 : (t >= 255.0 ? 255 : (int)t); }

// the extent of video v clamped into the buffer (a table rewritten on the device never addresses outside it); a null
// table is the whole frame
__device__ __forceinline__ void ra_extent(const int32_t* __restrict__ extents, int v, int Hs, int Ws, int& h, int& w) {
  h = Hs, w = Ws;
  if (extents) {
    h = ra_clampi(extents[2 * v], 1, Hs);
    w = ra_clampi(extents[2 * v + 1], 1, Ws);
  }
}

// ---- per-frame statistics ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void randaug_stats_kernel(const uint8_t* __restrict__ frames,
                                                            const SvitRandAugOp* __restrict__ recs,
                                                            const int32_t* __restrict__ extents, int layer,
                                                            uint8_t* __restrict__ ws, int T, int Hs, int Ws, int N) {
  const int vt = blockIdx.x, tid = threadIdx.x;
  const int op = recs[(size_t)(vt / T) * N + layer].op;
  if (op != RA_AUTOCONTRAST && op != RA_EQUALIZE && op != RA_CONTRAST) return;      // (uniform: before any barrier)
  __shared__ uint32_t hist[768];
  __shared__ unsigned long long part[256];
  __shared__ int lohi[6];
  for (int i = tid; i < 768; i += 256) hist[i] = 0;
  __syncthreads();
  int h, w;
  ra_extent(extents, vt / T, Hs, Ws, h, w);
  const int npix = h * w;
  const uint8_t* f = frames + (size_t)vt * Hs * Ws * 3;
  // every pixel of the extent once; full-width rows are one contiguous run of pixels (the loop of the plain entry points)
  const auto walk = [&](const auto& count) {
    if (w == Ws) {
      for (int p = tid; p < npix; p += 256) count(f + (size_t)p * 3);
    } else {
      for (int p = tid; p < npix; p += 256) {
        const int y = p / w, x = p - y * w;
        count(f + ((size_t)y * Ws + x) * 3);
      }
    }
  };
  if (op == RA_CONTRAST) {
    walk([&](const uint8_t* q) { atomicAdd(&hist[ra_luma(q[0], q[1], q[2])], 1u); });
  } else {
    walk([&](const uint8_t* q) {
      atomicAdd(&hist[q[0]], 1u);
      atomicAdd(&hist[256 + q[1]], 1u);
      atomicAdd(&hist[512 + q[2]], 1u);
    });
  }
  __syncthreads();
  uint8_t* slot = ws + (size_t)vt * RA_SLOT;
  if (op == RA_CONTRAST) {
    // mean = int(sum(L) / count + 0.5), the quotient in fp64 as Python divides the two integers
    part[tid] = (unsigned long long)tid * hist[tid];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    if (tid == 0) *(int32_t*)(slot + RA_MEAN_AT) = (int32_t)((double)part[0] / (double)npix + 0.5);
    return;
  }
  if (op == RA_AUTOCONTRAST) {
    if (tid < 3) {
      const uint32_t* h = hist + tid * 256;
      int lo = 0, hi = 255;
      while (lo < 255 && h[lo] == 0) ++lo;
      while (hi > 0 && h[hi] == 0) --hi;
      lohi[tid * 2] = lo;
      lohi[tid * 2 + 1] = hi;
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
      const int lo = lohi[c * 2], hi = lohi[c * 2 + 1];
      int out = tid;
      if (hi > lo) {
        const double scale = 255.0 / (double)(hi - lo);
        const double off = -(double)lo * scale;
        const double val = (double)tid * scale + off;       // (no contraction: product and sum rounded separately)
        out = val < 0.0 ? 0 : (val > 255.0 ? 255 : (int)val);
      }
      slot[c * 256 + tid] = (uint8_t)out;
    }
    return;
  }
  // RA_EQUALIZE: ImageOps.equalize, all in integers; the quotient can reach 256, which PIL's table clamps
  if (tid < 3) {
    const uint32_t* h = hist + tid * 256;
    uint8_t* lut = slot + tid * 256;
    int nonzero = 0, last = 0;
    for (int i = 0; i < 256; ++i)
      if (h[i]) {
        ++nonzero;
        last = i;
      }
    const uint32_t step = nonzero <= 1 ? 0u : ((uint32_t)npix - h[last]) / 255u;
    if (step == 0) {
      for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)i;
    } else {
      uint32_t n = step / 2;
      for (int i = 0; i < 256; ++i) {
        const uint32_t q = n / step;
        lut[i] = (uint8_t)(q > 255u ? 255u : q);
        n += h[i];
      }
    }
  }
}

// ---- one layer: src -> dst ------------------------------------------------------------------------------------------
__device__ __forceinline__ int ra_blend(int a, int b, float f, bool in_range) {
  const float t = (float)a + f * (float)(b - a);
  return in_range ? (int)t : ra_clip8(t);
}

__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

__global__ __launch_bounds__(256) void randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const SvitRandAugOp* __restrict__ recs,
                                                            const int32_t* __restrict__ extents, int layer,
                                                            const uint8_t* __restrict__ ws, int T, int Hb, int Wb, int N,
                                                            int blocks_per_frame) {
  const int vt = blockIdx.x / blocks_per_frame, blk = blockIdx.x % blocks_per_frame, tid = threadIdx.x;
  const int t = vt % T;
  const SvitRandAugOp* rec = recs + (size_t)(vt / T) * N + layer;
  const int op = rec->op;
  const uint8_t* slot = ws + (size_t)vt * RA_SLOT;
  __shared__ uint8_t lut[768];
  if (op == RA_AUTOCONTRAST || op == RA_EQUALIZE) {          // (uniform per block)
    for (int i = tid; i < 768; i += 256) lut[i] = slot[i];
    __syncthreads();
  }
  const int npix = Hb * Wb;                                  // the grid is over the padded buffer Hb x Wb, pitch Wb
  const int p = blk * 256 + tid;
  if (p >= npix) return;
  const int y = p / Wb, x = p - y * Wb;
  const uint8_t* f = src + (size_t)vt * npix * 3;
  const uint8_t* q = f + (size_t)p * 3;
  uint8_t* o = dst + (size_t)vt * npix * 3 + (size_t)p * 3;
  int c0 = q[0], c1 = q[1], c2 = q[2];
  int Hs, Ws;                                                // the video's own image; outside it dst is a copy
  ra_extent(extents, vt / T, Hb, Wb, Hs, Ws);
  if (y >= Hs || x >= Ws) {                                  // (no barrier below; `op` stays uniform for the switch)
    o[0] = (uint8_t)c0, o[1] = (uint8_t)c1, o[2] = (uint8_t)c2;
    return;
  }
  switch (op) {
    case RA_AUTOCONTRAST:
    case RA_EQUALIZE:
      c0 = lut[c0], c1 = lut[256 + c1], c2 = lut[512 + c2];
      break;
    case RA_INVERT:
      c0 = 255 - c0, c1 = 255 - c1, c2 = 255 - c2;
      break;
    case RA_POSTERIZE: {
      const int mask = ~((1 << (8 - ra_clampi(rec->arg_i, 0, 8))) - 1);
      c0 &= mask, c1 &= mask, c2 &= mask;
      break;
    }
    case RA_SOLARIZE: {
      const int thr = rec->arg_i;
      c0 = c0 < thr ? c0 : 255 - c0, c1 = c1 < thr ? c1 : 255 - c1, c2 = c2 < thr ? c2 : 255 - c2;
      break;
    }
    case RA_SOLARIZE_ADD: {
      const int add = ra_clampi(rec->arg_i, -255, 255);
      c0 = c0 < 128 ? ra_clampi(c0 + add, 0, 255) : c0;
      c1 = c1 < 128 ? ra_clampi(c1 + add, 0, 255) : c1;
      c2 = c2 < 128 ? ra_clampi(c2 + add, 0, 255) : c2;
      break;
    }
    case RA_COLOR:
    case RA_CONTRAST:
    case RA_BRIGHTNESS:
    case RA_SHARPNESS: {
      // ImagingBlend(degenerate a, image b, factor): (float)a + factor * (float)(b - a), truncated inside [0, 1],
      // clipped outside
      const float fac = rec->arg_f;
      const bool in_range = fac >= 0.0f && fac <= 1.0f;
      int a0 = 0, a1 = 0, a2 = 0;                            // BRIGHTNESS: black
      if (op == RA_COLOR) {
        a0 = a1 = a2 = ra_luma(c0, c1, c2);
      } else if (op == RA_CONTRAST) {
        a0 = a1 = a2 = ra_clampi(*(const int32_t*)(slot + RA_MEAN_AT), 0, 255);
      } else if (op == RA_SHARPNESS) {
        a0 = c0, a1 = c1, a2 = c2;                           // the border ring of ImageFilter.SMOOTH is the source
        if (y > 0 && y < Hs - 1 && x > 0 && x < Ws - 1) {
          constexpr float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
          float ss[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
          for (int r = 1; r >= -1; --r) {                    // rows y+1, y, y-1 as ImagingFilter3x3 adds them
            const uint8_t* row = q + (ptrdiff_t)r * Wb * 3;
            const float kc = r == 0 ? k5 : k1;
#pragma unroll
            for (int c = 0; c < 3; ++c)
              ss[c] = ss[c] + (((float)row[c - 3] * k1 + (float)row[c] * kc) + (float)row[c + 3] * k1);
          }
          a0 = ra_clip8(ss[0]), a1 = ra_clip8(ss[1]), a2 = ra_clip8(ss[2]);
        }
      }
      c0 = ra_blend(a0, c0, fac, in_range), c1 = ra_blend(a1, c1, fac, in_range), c2 = ra_blend(a2, c2, fac, in_range);
      break;
    }
    case RA_AFFINE: {
      // ImagingGenericTransform: affine_transform's coordinates, then the filter; fp64 throughout
      const double xin = (double)x + 0.5, yin = (double)y + 0.5;
      double xo = rec->m[0] * xin + rec->m[1] * yin + rec->m[2];
      double yo = rec->m[3] * xin + rec->m[4] * yin + rec->m[5];
      // the positive form: a NaN lands on the fill.  (affine_transform admits xo == Ws, the filters refuse it)
      if (!(xo >= 0.0 && xo < (double)Ws && yo >= 0.0 && yo < (double)Hs)) {
        c0 = c1 = c2 = RA_FILL;
        break;
      }
      xo -= 0.5, yo -= 0.5;
      const double fx = floor(xo), fy = floor(yo);
      const double dx = xo - fx, dy = yo - fy;
      const int ix = (int)fx, iy = (int)fy;                  // in [-1, Ws-1] x [-1, Hs-1]
      int out[3];
      if ((rec->bicubic_mask >> (t & 31)) & 1u) {
        const int xa = ra_clampi(ix - 1, 0, Ws - 1) * 3, xb = ra_clampi(ix, 0, Ws - 1) * 3,
                  xc = ra_clampi(ix + 1, 0, Ws - 1) * 3, xd = ra_clampi(ix + 2, 0, Ws - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int yy = iy - 1 + r;
            if (r == 0 || (yy >= 0 && yy < Hs)) {
              const uint8_t* row = f + (size_t)ra_clampi(yy, 0, Hs - 1) * Wb * 3 + c;
              v[r] = ra_cubic((double)row[xa], (double)row[xb], (double)row[xc], (double)row[xd], dx);
            } else {
              v[r] = v[r - 1];
            }
          }
          out[c] = ra_clip8(ra_cubic(v[0], v[1], v[2], v[3], dy));
        }
      } else {
        const int xa = ra_clampi(ix, 0, Ws - 1) * 3, xb = ra_clampi(ix + 1, 0, Ws - 1) * 3;
        const uint8_t* row0 = f + (size_t)ra_clampi(iy, 0, Hs - 1) * Wb * 3;
        const bool second = iy + 1 >= 0 && iy + 1 < Hs;
        const uint8_t* row1 = f + (size_t)ra_clampi(iy + 1, 0, Hs - 1) * Wb * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int a = row0[xa + c], b = row0[xb + c];
          const double v1 = (double)a + (double)(b - a) * dx;
          double v2 = v1;
          if (second) {
            const int a2 = row1[xa + c], b2 = row1[xb + c];
            v2 = (double)a2 + (double)(b2 - a2) * dx;
          }
          out[c] = ra_clampi((int)(v1 + (v2 - v1) * dy), 0, 255);
        }
      }
      c0 = out[0], c1 = out[1], c2 = out[2];
      break;
    }
    default:
      break;                                                 // NONE and anything unknown: a copy
  }
  o[0] = (uint8_t)c0;
  o[1] = (uint8_t)c1;
  o[2] = (uint8_t)c2;
}

int ra_args_ok(const void* frames, const void* recs, int layer, const void* ws, int V, int T, int Hs, int Ws, int N) {
  if (!frames || !recs || !ws) return SVIT_ERR_ARG;
  if (V < 1 || T < 1 || N < 1 || Hs < 3 || Ws < 3) return SVIT_ERR_SHAPE;
  if (layer < 0 || layer >= N) return SVIT_ERR_ARG;
  if ((int64_t)Hs * Ws > (1 << 28) || (int64_t)V * T > (1 << 20)) return SVIT_ERR_SHAPE;
  if ((int64_t)V * T * (((int64_t)Hs * Ws + 255) / 256) > 0x7fffffffLL) return SVIT_ERR_SHAPE;
  if ((uintptr_t)recs % 8 || (uintptr_t)ws % 4) return SVIT_ERR_ALIGN;
  return SVIT_OK;
}
}  // namespace

extern "C" int svit_randaug_stats_ext(const uint8_t* frames, const void* records, const int32_t* extents, int layer,
                                      void* workspace, int V, int T, int Hs, int Ws, int N, void* stream) {
  const int rc = ra_args_ok(frames, records, layer, workspace, V, T, Hs, Ws, N);
  if (rc != SVIT_OK) return rc;
  if ((uintptr_t)extents % 4) return SVIT_ERR_ALIGN;
  hipLaunchKernelGGL(randaug_stats_kernel, dim3((unsigned)(V * T)), dim3(256), 0, (hipStream_t)stream, frames,
                     (const SvitRandAugOp*)records, extents, layer, (uint8_t*)workspace, T, Hs, Ws, N);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_randaug_apply_ext(const uint8_t* src, uint8_t* dst, const void* records, const int32_t* extents,
                                      int layer, const void* workspace, int V, int T, int Hs, int Ws, int N,
                                      void* stream) {
  const int rc = ra_args_ok(src, records, layer, workspace, V, T, Hs, Ws, N);
  if (rc != SVIT_OK) return rc;
  if (!dst || dst == src) return SVIT_ERR_ARG;
  if ((uintptr_t)extents % 4) return SVIT_ERR_ALIGN;
  const int bpf = (Hs * Ws + 255) / 256;
  hipLaunchKernelGGL(randaug_apply_kernel, dim3((unsigned)(V * T * bpf)), dim3(256), 0, (hipStream_t)stream, src, dst,
                     (const SvitRandAugOp*)records, extents, layer, (const uint8_t*)workspace, T, Hs, Ws, N, bpf);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_randaug_stats(const uint8_t* frames, const void* records, int layer, void* workspace, int V, int T,
                                  int Hs, int Ws, int N, void* stream) {
  return svit_randaug_stats_ext(frames, records, nullptr, layer, workspace, V, T, Hs, Ws, N, stream);
}

extern "C" int svit_randaug_apply(const uint8_t* src, uint8_t* dst, const void* records, int layer, const void* workspace,
                                  int V, int T, int Hs, int Ws, int N, void* stream) {
  return svit_randaug_apply_ext(src, dst, records, nullptr, layer, workspace, V, T, Hs, Ws, N, stream);
}
