// Data gradient of the patch-embedding stem, Conv3d(3->96, k(3,7,7), s(2,4,4), p(1,3,3)) (svit_patch_embed_dgrad) --
// gfx950.
//
//   dvideo[b,c,t,y,x] = sum over (to,kt), (yo,ky), (xo,kx) with t = 2to-1+kt, y = 4yo-3+ky, x = 4xo-3+kx
//                       of sum_{n<96} dtok[(b,to,yo,xo), n] * w16[n, ((c*3+kt)*7+ky)*7+kx]
//
// from the two bf16 operands the backward already holds: dtok [B*To*Ho*Wo, 96], the patch rows of block 0's dx, and
// w16 [96, 448], the forward GEMM's weight (columns 441..447 are its zero pad and are never read here: the largest
// column a tap names is 440).  The yardstick is svit_amd/saliency.py dgrad_host.
//
// GATHER form: every input element is computed and stored once, by the thread that owns it -- no atomics, no ticket,
// nothing to zero beforehand, the same bits from run to run and from the eager pass to a replay.
//
// The strides make the taps of a pixel a function of its coordinates' residues: an odd t meets kt = 0 and 2 (two
// output frames), an even t only kt = 1; y = 4j + r meets (yo, ky) = (j, 3 + r) and, for r > 0, (j + 1, r - 1); x
// likewise.  So a whole input line (t, y) shares at most 2 x 2 "pairs" (to, kt, yo, ky), and under one pair the
// four pixels x = 4j .. 4j + 3 need the tokens xo = j (kx = 3, 4, 5, 6) and xo = j + 1 (kx = -, 0, 1, 2).
//
// One workgroup owns the line (t, y) of every clip of its batch slice (blockIdx.y, blockIdx.y + gridDim.y, ...): the
// weight slices of its pairs -- [pair][c*7 + kx][96], 4 KB per pair, n contiguous -- are gathered from w16 ONCE into LDS
// and serve all those clips.  Per clip and per chunk of 56 pixel quads (one chunk at W = 224) the pairs' token lines
// are staged by coalesced 16-byte loads into rows padded to 208 bytes (13 16-byte units, odd: the lanes' ds_read_b128
// of their own rows meet no bank conflict); rows past Wo are zero, which is the right border.  Wave c of the three
// computes channel c, lane l the quad j0 + l: per pair and per 8 values of n it reads its two token rows and the seven
// weight rows (wave-uniform addresses: broadcasts) and issues 28 v_dot2_f32_bf16 into four accumulators.  The products
// bf16 x bf16 are exact in fp32; the sum runs in fp32 in the fixed order (pair, n, token j before token j + 1).  The
// quad is stored as one 16-byte vector where W % 4 == 0 and dvideo is 16-byte aligned, else pixel by pixel.
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int kThreads = 192;              // three waves: one per input channel
constexpr int kQuads = 56;                 // pixel quads (= tokens) of a chunk: 224 pixels
constexpr int kTokRows = kQuads + 1;       // + the right neighbour of the last quad
constexpr int kTokPitch = 104;             // bf16 per staged token row: 96 + 8 (208 bytes)
constexpr int kPairs = 4;
constexpr int kEmbed = 96;

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), acc, false);
}
__device__ __forceinline__ float dot8(const uint4 a, const uint4 w, float acc) {
  acc = dot2(a.x, w.x, acc);
  acc = dot2(a.y, w.y, acc);
  acc = dot2(a.z, w.z, acc);
  return dot2(a.w, w.w, acc);
}

__global__ __launch_bounds__(kThreads) void patch_embed_dgrad_kernel(const bf16_t* __restrict__ dtok,
                                                                     const bf16_t* __restrict__ w16,
                                                                     float* __restrict__ dvideo, int B, int T, int H,
                                                                     int W, int To, int Ho, int Wo) {
  __shared__ __attribute__((aligned(16))) bf16_t wl[kPairs * 21 * kEmbed];               // [pair][c*7 + kx][n]
  __shared__ __attribute__((aligned(16))) bf16_t tk[kPairs * kTokRows * kTokPitch];      // [pair][token - j0][n | pad]
  const int tid = threadIdx.x, lane = tid & 63, c = tid >> 6;
  const int t = blockIdx.x / H, y = blockIdx.x - t * H;
  // the pairs of this line: to, yo and the weight column of (c = 0, kx = 0); at least one, at most 2 x 2
  __shared__ int p_to[kPairs], p_yo[kPairs], p_col[kPairs], p_count;
  if (tid == 0) {
    int k = 0;
    for (int kt = 0; kt < 3; ++kt) {
      const int tt = t + 1 - kt;
      if (tt < 0 || (tt & 1) || (tt >> 1) >= To) continue;
      for (int ky = 0; ky < 7; ++ky) {
        const int yy = y + 3 - ky;
        if (yy < 0 || (yy & 3) || (yy >> 2) >= Ho) continue;
        p_to[k] = tt >> 1; p_yo[k] = yy >> 2; p_col[k] = (kt * 7 + ky) * 7;
        ++k;
      }
    }
    p_count = k;
  }
  __syncthreads();
  const int np = p_count;
  // weight slices: wl[p][c*7 + kx][n] = w16[n, (c*3 + kt)*49 + ky*7 + kx]; (c, kx) fastest, so a wave's loads fall
  // into three rows of w16
  for (int i = tid; i < np * 21 * kEmbed; i += kThreads) {
    const int ck = i % 21, n = (i / 21) % kEmbed, p = i / (21 * kEmbed);
    const int cc = ck / 7, kx = ck - cc * 7;
    wl[(p * 21 + ck) * kEmbed + n] = w16[n * 448 + cc * 147 + p_col[p] + kx];
  }
  const bool vec = !(W & 3) && !((uintptr_t)dvideo & 15);
  const int rl = lane < kQuads ? lane : kQuads - 1;        // (lanes 56..63 read a valid row and store nothing)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    for (int j0 = 0; j0 < Wo; j0 += kQuads) {
      __syncthreads();                                     // the previous chunk's readers are done
      const int have = min(kTokRows, Wo - j0);             // token rows of this chunk that exist
      for (int i = tid; i < np * kTokRows * 12; i += kThreads) {
        const int s = i % 12, r = (i / 12) % kTokRows, p = i / (12 * kTokRows);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r < have) {
          const int64_t row = (((int64_t)b * To + p_to[p]) * Ho + p_yo[p]) * Wo + j0 + r;
          v = *(const uint4*)(dtok + row * kEmbed + s * 8);
        }
        *(uint4*)(tk + (p * kTokRows + r) * kTokPitch + s * 8) = v;
      }
      __syncthreads();
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < np; ++p) {
        const uint4* ta = (const uint4*)(tk + (p * kTokRows + rl) * kTokPitch);
        const uint4* tb = ta + kTokPitch / 8;
        const uint4* wr = (const uint4*)(wl + (p * 21 + c * 7) * kEmbed);
#pragma unroll 4
        for (int s = 0; s < 12; ++s) {      // (by four: the LDS reads of later steps issue under the dot2s of earlier ones)
          const uint4 a = ta[s], n1 = tb[s];
          acc[0] = dot8(a, wr[3 * 12 + s], acc[0]);
          acc[1] = dot8(a, wr[4 * 12 + s], acc[1]);
          acc[1] = dot8(n1, wr[0 * 12 + s], acc[1]);
          acc[2] = dot8(a, wr[5 * 12 + s], acc[2]);
          acc[2] = dot8(n1, wr[1 * 12 + s], acc[2]);
          acc[3] = dot8(a, wr[6 * 12 + s], acc[3]);
          acc[3] = dot8(n1, wr[2 * 12 + s], acc[3]);
        }
      }
      const int x0 = (j0 + lane) * 4;
      if (lane < kQuads && x0 < W) {
        float* out = dvideo + ((((int64_t)b * 3 + c) * T + t) * H + y) * W + x0;
        if (vec) {
          *(float4*)out = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (x0 + r < W) out[r] = acc[r];
        }
      }
    }
  }
}

}  // namespace

extern "C" int svit_patch_embed_dgrad(const void* dtok, const void* w16, float* dvideo, int B, int T, int H, int W,
                                      void* stream) {
  if (!dtok || !w16 || !dvideo || B < 1 || T < 1 || H < 1 || W < 1) return SVIT_ERR_ARG;
  if (((uintptr_t)dtok & 15) || ((uintptr_t)w16 & 15) || ((uintptr_t)dvideo & 3)) return SVIT_ERR_ALIGN;
  const int To = (T - 1) / 2 + 1, Ho = (H - 1) / 4 + 1, Wo = (W - 1) / 4 + 1;
  if ((int64_t)B * To * Ho * Wo >= (int64_t)1 << 31 || (int64_t)T * H >= (int64_t)1 << 31) return SVIT_ERR_SHAPE;
  // the lines (t, y) in x; in y as many batch slices (at most 65535) as bring the grid to ~2048 workgroups
  const int64_t lines = (int64_t)T * H;
  int slices = (int)((2048 + lines - 1) / lines);
  slices = slices < 1 ? 1 : (slices > B ? B : slices);
  if (slices > 65535) slices = 65535;
  hipLaunchKernelGGL(patch_embed_dgrad_kernel, dim3((unsigned)lines, (unsigned)slices), dim3(kThreads), 0,
                     (hipStream_t)stream, (const bf16_t*)dtok, (const bf16_t*)w16, dvideo, B, T, H, W, To, Ho, Wo);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
