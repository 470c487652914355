// The two streaming kernels of the attribution passes (svit_amd/attribution.py: SmoothGrad, integrated gradients) --
// gfx950.
//
//   svit_attr_perturb     out = base + alpha * (x - base) + sigma[b] * n     the clip one pass differentiates
//   svit_attr_accumulate  acc = (pass == 0 ? 0 : acc) + weight * (g or g*g)  its input gradient folded into the sum
//
// Both read ONE 32-byte record (svit_attr_pass) from DEVICE memory at run time, so a captured pass body holds the same
// two launches for every alpha, weight, seed and pass number.
//
// Every subtraction, product and sum below is one fp32 operation rounded to nearest, which is what the torch-CPU
// restatements (attribution.perturb_host / accumulate_host) compute -- the tests hold the kernels to them bit for bit.
// The library's common flags include -ffast-math, under which the backend fuses and reassociates whatever the source
// says, so -- as in solver.hip -- the arithmetic goes through helpers whose results pass an empty asm: nothing is left to
// fuse (and a zero stays a signed zero).  The noise is the erasing noise of csrc/input.hip (aug_noise, common.h: Philox
// + Box-Muller on v_log / v_sqrt / v_cos), built with the same flags as there and at the coordinates its pixel mode
// uses: the field svit_u8_clips_render draws into a fully erased window.
//
// Plain streaming kernels: a grid-stride loop over 16-byte vectors, the grid sized from the CU count.  The vector body
// starts at the first 16-byte boundary of the output; the elements in front of it and behind the last whole vector are
// handled one by one, so any element count and any 4-byte aligned pointer is legal (operands that are misaligned
// DIFFERENTLY from the output take the element path throughout).  Offsets are 64-bit, nothing is atomic, and every
// output element is stored exactly once.
#include "common.h"
#include "../../include/svit_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerCU = 8;

struct Split {       // [0, head) one by one, [head, head + 4 * nvec) as 16-byte vectors, the rest one by one
  int64_t head, nvec;
};

// the split of n elements at `lead`; every other pointer must sit at the same offset inside its 16 bytes, else no vector
Split split_of(int64_t n, const void* lead, const void* const* others, int n_others) {
  const uintptr_t mis = (uintptr_t)lead & 15;
  bool same = true;
  for (int i = 0; i < n_others; ++i)
    if (others[i] && ((uintptr_t)others[i] & 15) != mis) same = false;
  Split s;
  s.head = same ? (int64_t)(((16 - mis) & 15) / 4) : n;
  if (s.head > n) s.head = n;
  s.nvec = (n - s.head) / 4;
  return s;
}

// CU count of the current device, asked once per device
int cu_count(int* out) {
  static int cached[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  int v = __atomic_load_n(&cached[dev & 63], __ATOMIC_ACQUIRE);
  if (v <= 0) {
    e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    if (v < 1) v = 1;
    __atomic_store_n(&cached[dev & 63], v, __ATOMIC_RELEASE);
  }
  *out = v;
  return 0;
}

unsigned grid_for(int64_t nvec, int64_t n, int cus) {
  int64_t items = nvec > 0 ? nvec : n;      // (all head / tail: the first lanes walk them)
  int64_t blocks = (items + kThreads - 1) / kThreads;
  const int64_t cap = (int64_t)cus * kBlocksPerCU;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ---- fp32 operations rounded once each, whatever the build's floating-point flags (as in solver.hip) ------------------
__device__ __forceinline__ float opaque(float x) {
  __asm__("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float mul_rn(float a, float b) { return opaque(opaque(a) * opaque(b)); }
__device__ __forceinline__ float add_rn(float a, float b) { return opaque(opaque(a) + opaque(b)); }
__device__ __forceinline__ float sub_rn(float a, float b) { return opaque(opaque(a) - opaque(b)); }

// ---- perturb -----------------------------------------------------------------------------------------------------------
struct PerturbGeom {
  int64_t n;         // B * 3 * T * H * W
  int HW, P;         // pixels of a plane; planes of a clip (3 * T)
};

// one element: every operation rounded on its own
__device__ __forceinline__ float perturb_value(float xv, float bv, float alpha, bool noisy, float sg, uint32_t seed,
                                               int b, int plane, uint32_t idx) {
  const float d = sub_rn(xv, bv);
  const float m = mul_rn(alpha, d);
  float p = add_rn(bv, m);
  if (noisy) p = add_rn(p, mul_rn(sg, aug_noise(seed, b, plane, idx)));
  return p;
}

__device__ __forceinline__ void perturb_element(const float* __restrict__ x, const float* __restrict__ base,
                                                const float* __restrict__ sigma, float* __restrict__ out,
                                                const PerturbGeom& g, float alpha, uint32_t seed, int64_t i) {
  const int64_t pg = i / g.HW;
  const uint32_t idx = (uint32_t)(i - pg * g.HW);
  const int b = (int)(pg / g.P), plane = (int)(pg - (int64_t)b * g.P);
  out[i] = perturb_value(x[i], base ? base[i] : 0.f, alpha, sigma != nullptr, sigma ? sigma[b] : 0.f, seed, b, plane, idx);
}

__global__ void __launch_bounds__(kThreads)
attr_perturb_kernel(const float* __restrict__ x, const float* __restrict__ base, const float* __restrict__ sigma,
                    const svit_attr_pass* __restrict__ rec, float* __restrict__ out, PerturbGeom g, Split sp) {
  const float alpha = rec->alpha;
  const uint32_t seed = rec->seed;
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
  const int64_t body_end = sp.head + 4 * sp.nvec;
  for (int64_t v = tid; v < sp.nvec; v += stride) {
    const int64_t i0 = sp.head + 4 * v;
    const float4 xv = *(const float4*)(x + i0);
    const float4 bv = base ? *(const float4*)(base + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, bs[4] = {bv.x, bv.y, bv.z, bv.w};
    float o[4];
    if (sigma) {
      int64_t pg = i0 / g.HW;                  // one division per vector; the four elements step from it
      int idx = (int)(i0 - pg * g.HW);
      int b = (int)(pg / g.P), plane = (int)(pg - (int64_t)b * g.P);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = perturb_value(xs[k], bs[k], alpha, true, sigma[b], seed, b, plane, (uint32_t)idx);
        if (++idx == g.HW) {
          idx = 0;
          if (++plane == g.P) { plane = 0; ++b; }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = perturb_value(xs[k], bs[k], alpha, false, 0.f, seed, 0, 0, 0u);
    }
    *(float4*)(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
  }
  for (int64_t i = tid; i < sp.head; i += stride) perturb_element(x, base, sigma, out, g, alpha, seed, i);
  for (int64_t i = body_end + tid; i < g.n; i += stride) perturb_element(x, base, sigma, out, g, alpha, seed, i);
}

// ---- accumulate --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float accumulate_value(float gv, float av, float weight, bool squared, bool first) {
  const float v = squared ? mul_rn(gv, gv) : gv;
  const float t = mul_rn(weight, v);
  return first ? t : add_rn(av, t);
}

__global__ void __launch_bounds__(kThreads)
attr_accumulate_kernel(const float* __restrict__ gr, float* __restrict__ acc, const svit_attr_pass* __restrict__ rec,
                       const uint32_t* __restrict__ scores_in, uint32_t* __restrict__ scores, int rows, int64_t n, int B,
                       Split sp) {
  const float weight = rec->weight;
  const uint32_t pass = rec->pass;
  const bool squared = (rec->flags & 1u) != 0, first = pass == 0u;
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
  const int64_t body_end = sp.head + 4 * sp.nvec;
  if (scores && blockIdx.x == 0 && pass < (uint32_t)rows)       // this pass's scores, bit for bit, into their row
    for (int b = threadIdx.x; b < B; b += kThreads) scores[(int64_t)pass * B + b] = scores_in[b];
  for (int64_t v = tid; v < sp.nvec; v += stride) {
    const int64_t i0 = sp.head + 4 * v;
    const float4 gv = *(const float4*)(gr + i0);
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!first) av = *(const float4*)(acc + i0);      // (the first pass stores: whatever acc held is never read)
    float4 o;
    o.x = accumulate_value(gv.x, av.x, weight, squared, first);
    o.y = accumulate_value(gv.y, av.y, weight, squared, first);
    o.z = accumulate_value(gv.z, av.z, weight, squared, first);
    o.w = accumulate_value(gv.w, av.w, weight, squared, first);
    *(float4*)(acc + i0) = o;
  }
  for (int64_t i = tid; i < sp.head; i += stride)
    acc[i] = accumulate_value(gr[i], first ? 0.f : acc[i], weight, squared, first);
  for (int64_t i = body_end + tid; i < n; i += stride)
    acc[i] = accumulate_value(gr[i], first ? 0.f : acc[i], weight, squared, first);
}

}  // namespace

extern "C" int svit_attr_perturb(const float* x, const float* base, const float* sigma, const void* rec, float* out,
                                 int B, int T, int H, int W, void* stream) {
  if (!x || !rec || !out || B < 1 || T < 1 || H < 1 || W < 1) return SVIT_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)base & 3) || ((uintptr_t)sigma & 3) || ((uintptr_t)rec & 3) ||
      ((uintptr_t)out & 3))
    return SVIT_ERR_ALIGN;
  if ((int64_t)H * W >= (int64_t)1 << 31 || (int64_t)B * 3 * T >= (int64_t)1 << 31) return SVIT_ERR_SHAPE;
  PerturbGeom g;
  g.HW = H * W;
  g.P = 3 * T;
  g.n = (int64_t)B * g.P * g.HW;
  const void* others[2] = {x, base};
  const Split sp = split_of(g.n, out, others, 2);
  int cus = 0;
  const int rc = cu_count(&cus);
  if (rc) return rc;
  hipLaunchKernelGGL(attr_perturb_kernel, dim3(grid_for(sp.nvec, g.n, cus)), dim3(kThreads), 0, (hipStream_t)stream, x,
                     base, sigma, (const svit_attr_pass*)rec, out, g, sp);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_attr_accumulate(const float* g, float* acc, const void* rec, const float* scores_in, float* scores,
                                    int rows, int64_t n, int B, void* stream) {
  if (!g || !acc || !rec || n < 1 || B < 1) return SVIT_ERR_ARG;
  if (scores && (!scores_in || rows < 1)) return SVIT_ERR_ARG;
  if (((uintptr_t)g & 3) || ((uintptr_t)acc & 3) || ((uintptr_t)rec & 3) || ((uintptr_t)scores_in & 3) ||
      ((uintptr_t)scores & 3))
    return SVIT_ERR_ALIGN;
  const void* others[1] = {g};
  const Split sp = split_of(n, acc, others, 1);
  int cus = 0;
  const int rc = cu_count(&cus);
  if (rc) return rc;
  hipLaunchKernelGGL(attr_accumulate_kernel, dim3(grid_for(sp.nvec, n, cus)), dim3(kThreads), 0, (hipStream_t)stream, g,
                     acc, (const svit_attr_pass*)rec, (const uint32_t*)scores_in, (uint32_t*)scores, rows, n, B, sp);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
