// SViT head in eval mode, one launch (slowfast/models/video_model_builder.py:408-551 under `not self.training`) -- gfx950.
//
// What SViTHead.forward does with stock ATen ops when the model evaluates: three Linears, a softmax (or sigmoid) over
// the classes, a sigmoid on the objectness logit, a softmax over the five contact states, slices, reshapes, a cat --
// and in front of it the cat of the cls and object rows.  About twenty launches of ~5 us for < 1 MFLOP; the captured
// evaluation step (svit_amd/graph.py, GraphedEvalStep) replaces them by this kernel, which reads the final norm's
// output tokens where they lie.  The dot products are fp32, as the stock head's; every exponential, the softmax sums and
// every division run in fp64 and are rounded to fp32 once (a few hundred of them per clip: no time).
//
// Why fp64, and what it does and does not buy.  This file is compiled with the library's common flags, -ffast-math among
// them (svit_amd/build.py: randaug.hip alone has flags of its own, and tests/test_randaug_cpu.py holds the build to that).
// Under them fp32 expf is the bare v_exp_f32 form and an fp32 division a v_rcp_f32 product, each good to about 1e-7
// relative: of the size of the whole error budget.  The fp64 forms under the SAME flags: exp is the library's polynomial
// (there is no approximate fp64 exp), and a division is v_rcp_f64 + Newton steps WITHOUT the scale / fixup sequence of
// an IEEE division -- accurate to a few fp64 ulps for ordinary operands, wrong (NaN) for an infinite or denormal
// divisor.  So every division here is written to have a numerator in [0, 1] and a divisor in [1, n_cls], and every
// exponential an argument <= 0:
//   sigmoid(z) = 1 / (1 + exp(-z)) for z >= 0, exp(z) / (1 + exp(z)) for z < 0   -> divisor in [1, 2], no overflow for any z
//   softmax: exp(z - max) in [0, 1], the max's own term is exactly 1              -> divisor in [1, n_cls]
// (tests/test_eval_u8_gpu.py carries logits of +120 and -800 through both.)  The fast-math flags also let the compiler
// reassociate and contract the fp32 dot products: their summation order is the compiler's, fixed when the library is built.
//
// Workgroup roles by blockIdx.x:
//   [0, B)   one cls row each: n_cls dot products, a wave per output (two outputs in flight per wave), logits into an
//            LDS row; then the activation inside the workgroup -- softmax: max, exp(z - max), sum, one divide per class
//   rest     HE_NW object rows each, a wave per row: x is read once for the five outputs of every object and the five
//            contact logits of objects 0 and 1 of a frame; the contact softmax runs in registers
// No atomics and nothing that depends on dispatch order (per-lane chunks, xor butterfly, waves in index order): one
// build gives equal bits for equal inputs, captured or eager.
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int HE_NT = 512, HE_NW = HE_NT / 64, HE_CLS_MAX = 1024;

__device__ __forceinline__ float dot4(const float4& x, const float4& w) {
  return x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
}
// exp's argument is <= 0 and the divisor in [1, 2] for every z, +-inf included (header comment)
__device__ __forceinline__ float sigmoid_acc(float z) {
  const double en = exp(-fabs((double)z));
  return (float)((z >= 0.f ? 1.0 : en) / (1.0 + en));
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(HE_NT) void head_eval_kernel(svit_head_args a, int act) {
  __shared__ float z[HE_CLS_MAX];
  __shared__ double e[HE_CLS_MAX];
  __shared__ float red[HE_NW];
  __shared__ double red_sum[HE_NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_obj = a.T * a.O;
  if ((int)blockIdx.x < a.B) {
    // ---- cls row of clip b
    const int b = blockIdx.x;
    const float* x = a.tokens + (size_t)b * a.N * a.C;
    for (int k0 = wave; k0 < a.n_cls; k0 += 2 * HE_NW) {
      const int k1 = k0 + HE_NW;
      const bool two = k1 < a.n_cls;
      const float* w0 = a.w_proj + (size_t)k0 * a.C;
      const float* w1 = a.w_proj + (size_t)(two ? k1 : k0) * a.C;
      float s0 = 0.f, s1 = 0.f;
      for (int c = lane * 4; c < a.C; c += 256) {
        const float4 xv = *(const float4*)(x + c);
        s0 += dot4(xv, *(const float4*)(w0 + c));
        s1 += dot4(xv, *(const float4*)(w1 + c));
      }
      s0 = wave_sum(s0);
      s1 = wave_sum(s1);
      if (lane == 0) {
        z[k0] = s0 + a.b_proj[k0];
        if (two) z[k1] = s1 + a.b_proj[k1];
      }
    }
    __syncthreads();
    float* out = a.logits + (size_t)b * a.n_cls;
    if (act == 1) {
      for (int i = threadIdx.x; i < a.n_cls; i += HE_NT) out[i] = sigmoid_acc(z[i]);
      return;
    }
    float m = z[0];
    for (int i = threadIdx.x; i < a.n_cls; i += HE_NT) m = fmaxf(m, z[i]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < HE_NW; ++w) m = fmaxf(m, red[w]);
    double s = 0.0;
    for (int i = threadIdx.x; i < a.n_cls; i += HE_NT) {
      const double ei = exp((double)z[i] - (double)m);
      e[i] = ei;                            // (read back by the thread that wrote it)
      s += ei;
    }
    s = wave_sum_f64(s);
    if (lane == 0) red_sum[wave] = s;
    __syncthreads();
    s = red_sum[0];
#pragma unroll
    for (int w = 1; w < HE_NW; ++w) s += red_sum[w];
    for (int i = threadIdx.x; i < a.n_cls; i += HE_NT) out[i] = (float)(e[i] / s);
    return;
  }
  // ---- object rows: wave -> (b, t, o)
  const int row = ((int)blockIdx.x - a.B) * HE_NW + wave;
  if (row >= a.B * n_obj) return;
  const int b = row / n_obj, j = row % n_obj, t = j / a.O, o = j % a.O;
  const bool con = o < 2;                   // (wave-uniform)
  const float* x = a.tokens + ((size_t)b * a.N + (a.N - n_obj + j)) * a.C;
  float* xo = a.xobj ? a.xobj + (size_t)row * a.C : nullptr;
  float s[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = 0.f;
  for (int c = lane * 4; c < a.C; c += 256) {
    const float4 xv = *(const float4*)(x + c);
    s[0] += dot4(xv, *(const float4*)(a.w_bce + c));
#pragma unroll
    for (int k = 0; k < 4; ++k) s[1 + k] += dot4(xv, *(const float4*)(a.w_box + (size_t)k * a.C + c));
    if (con) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s[5 + k] += dot4(xv, *(const float4*)(a.w_con + (size_t)k * a.C + c));
    }
    if (xo) *(float4*)(xo + c) = xv;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0) {
    float* bx = a.boxes + (size_t)row * 5;
    bx[0] = sigmoid_acc(s[0] + a.b_bce[0]);
#pragma unroll
    for (int k = 0; k < 4; ++k) bx[1 + k] = sigmoid_acc(s[1 + k] + a.b_box[k]);
    if (con) {
      float zc[5], m;
      double ec[5], sum = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) zc[k] = s[5 + k] + a.b_con[k];
      m = zc[0];
#pragma unroll
      for (int k = 1; k < 5; ++k) m = fmaxf(m, zc[k]);
#pragma unroll
      for (int k = 0; k < 5; ++k) { ec[k] = exp((double)zc[k] - (double)m); sum += ec[k]; }
      float* cs = a.contact + (((size_t)b * a.T + t) * 2 + o) * 5;
#pragma unroll
      for (int k = 0; k < 5; ++k) cs[k] = (float)(ec[k] / sum);
    }
  }
}
}  // namespace

extern "C" int svit_head_eval(const svit_head_args* a, int act, void* stream) {
  if (!a) return SVIT_ERR_ARG;
  if (a->keep) return SVIT_ERR_ARG;         // evaluation has no dropout: a mask here is a caller's mistake
  if (!a->tokens || !a->w_proj || !a->b_proj || !a->w_box || !a->b_box || !a->w_bce || !a->b_bce || !a->w_con ||
      !a->b_con || !a->logits || !a->boxes || !a->contact)
    return SVIT_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->O < 2 || a->C <= 0 || a->C % 4 != 0 || a->n_cls < 1 || a->n_cls > HE_CLS_MAX ||
      (int64_t)a->N < 1 + (int64_t)a->T * a->O || (act != 0 && act != 1))
    return SVIT_ERR_SHAPE;
  if (((uintptr_t)a->tokens | (uintptr_t)a->w_proj | (uintptr_t)a->w_box | (uintptr_t)a->w_bce | (uintptr_t)a->w_con |
       (uintptr_t)a->xobj) & 15)
    return SVIT_ERR_ALIGN;
  const int64_t rows = (int64_t)a->B * a->T * a->O;
  const int64_t blocks = a->B + (rows + HE_NW - 1) / HE_NW;
  if (blocks > 0x7fffffff) return SVIT_ERR_SHAPE;
  hipLaunchKernelGGL(head_eval_kernel, dim3((unsigned)blocks), dim3(HE_NT), 0, (hipStream_t)stream, *a, act);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
