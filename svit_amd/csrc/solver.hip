// SGD and Adam on the guarded optimiser tail (svit_sgd_step_guarded / svit_adam_step_guarded) -- gfx950.
//
// The reference builds torch.optim.SGD, Adam or AdamW from the same cfg keys (slowfast/models/optimizer.py:86-112).
// AdamW lives in misc.hip; these are the other two, on the same step record (include/svit_hip.h: svit_step_host /
// svit_step_dev) behind the same guard (svit_step_guard / svit_step_guard_seg): a step whose gradients are not finite
// returns here before its first load, and the first APPLIED step is the one SGD copies its gradient into the momentum
// buffer on.
//
// The bar is a NumPy float32 restatement (svit_amd/optim.py: sgd_step_host / adam_step_host), bit for bit: every fp32
// operation below is rounded once, in the order written, the square root and the divisions are the correctly rounded
// ones.  The library's common flags include -ffast-math, under which the backend fuses a multiply into the add that
// consumes it whatever the source says (csrc/input.hip, mix_blend) and `/` and sqrtf become approximations.  So the
// arithmetic goes through the helpers below (mul_rn, add_rn, sub_rn, div_rn, sqrt_rn): each result passes an empty asm
// that makes it opaque -- nothing is left to fuse or reassociate -- and division and square root are hipcc's own IEEE
// expansions written out with the hardware's div_scale / div_fmas / div_fixup and sqrt instructions, which no flag
// rewrites.  Nothing here depends on what the compiler contracts.
//
// The walk is adamw_guarded_lr_kernel's (misc.hip): the range table and one scale per range ride in the kernel
// arguments, workgroup b takes the 1024 floats at b * 1024 + pass * gridDim.x * 1024, a cursor that only moves forward
// finds the ranges a window meets, the loop over them is workgroup-uniform and a lane keeps the values of the one range
// that holds its quad.  Bounds are multiples of 4 and no range crosses n_decay: a quad is inside one range whole or
// outside all, and has one learning rate and one weight decay.  Nothing outside the ranges is loaded or stored.
//
// svit_ema_step_guarded is the third kernel on that walk: the exponential moving average of the weights, launched
// behind whichever solver stepped them (AdamW's included), bit for bit svit_amd/ema.py's ema_step_host.
#include <cstring>

#include "common.h"
#include "../../include/svit_hip.h"

namespace {
// ---- fp32 operations rounded once each, whatever the build's floating-point flags --------------------------------
__device__ __forceinline__ float opaque(float x) {
  __asm__("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float mul_rn(float a, float b) { return opaque(a * b); }
__device__ __forceinline__ float add_rn(float a, float b) { return opaque(a + b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return opaque(a - b); }
// a / b correctly rounded: the compiler's expansion of an IEEE fp32 division -- LLVM's SITargetLowering::LowerFDIV32
// (llvm/lib/Target/AMDGPU/SIISelLowering.cpp; AMDGPULegalizerInfo::legalizeFDIV32 under GlobalISel), to be kept in step
// with it -- (fp32 denormals are on in HIP kernels, so no mode switch around it): both operands scaled out of the ranges where the iteration would lose bits, a reciprocal
// refined by one Newton step, the quotient by two, div_fmas undoing the scale, div_fixup the special cases
__device__ __forceinline__ float div_rn(float a, float b) {
  bool scaled;
  const float den = __builtin_amdgcn_div_scalef(a, b, false, &scaled);
  const float num = __builtin_amdgcn_div_scalef(a, b, true, &scaled);
  float r = __builtin_amdgcn_rcpf(den);
  r = __builtin_fmaf(__builtin_fmaf(-den, r, 1.0f), r, r);
  float q = opaque(num * r);
  q = __builtin_fmaf(__builtin_fmaf(-den, q, num), r, q);
  const float rem = __builtin_fmaf(-den, q, num);
  return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(rem, r, q, scaled), b, a);
}
// sqrt(x) correctly rounded, the compiler's expansion again -- SITargetLowering::lowerFSQRTF32 (same file;
// AMDGPULegalizerInfo::legalizeFSQRTF32), its branch for fp32 denormals enabled: the hardware's square root is within one ulp; the two
// neighbours' residuals x - s' * s say whether to step down or up.  Inputs below 2^-96 are scaled by 2^32 first (the
// root by 2^-16 after), zero and +inf pass through.
__device__ __forceinline__ float sqrt_rn(float x) {
  const bool tiny = x < 0x1.0p-96f;
  const float xs = tiny ? opaque(x * 0x1.0p+32f) : x;
  float s = __builtin_amdgcn_sqrtf(xs);
  const float down = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
  const float r_down = __builtin_fmaf(-down, s, xs), r_up = __builtin_fmaf(-up, s, xs);
  s = r_down <= 0.0f ? down : s;
  s = r_up > 0.0f ? up : s;
  s = tiny ? opaque(s * 0x1.0p-16f) : s;
  return (xs == 0.0f || xs == __builtin_inff()) ? xs : s;
}

struct RangeTable {
  int64_t v[SVIT_MAX_SEGS][2];
  float scale[SVIT_MAX_SEGS];
  int32_t S;
};

// the rates of a weight-decay group as the step record holds them
struct GroupRates {
  float lr0, lr1, wd0, wd1;
};

// is the quad at float index i of the window [lo, hi) inside a range?  -> its lr_eff = lr[w] * scale[s] (ONE fp32
// multiply) and its weight decay.  k: first range that ends past lo
__device__ __forceinline__ bool range_rates(const RangeTable& T, int& k, int64_t lo, int64_t hi, int64_t i,
                                            int64_t n_decay, const GroupRates& r, float& lr, float& wd) {
  while (k < T.S && T.v[k][1] <= lo) ++k;
  bool in = false;
  for (int j = k; j < T.S && T.v[j][0] < hi; ++j) {
    const bool dec = T.v[j][0] < n_decay;                                  // the whole range: none crosses n_decay
    const float le = mul_rn(dec ? r.lr0 : r.lr1, T.scale[j]);
    const bool here = (i >= T.v[j][0]) & (i < T.v[j][1]);
    in |= here;
    lr = here ? le : lr;
    wd = here ? (dec ? r.wd0 : r.wd1) : wd;
  }
  return in;
}

// g * coef, clamped to +-cv when clipping by value, plus the coupled L2 term
__device__ __forceinline__ float solver_grad(float pw, float gr, float coef, float cv, float wd) {
  float gi = mul_rn(gr, coef);
  if (cv > 0.f) gi = fminf(fmaxf(gi, -cv), cv);
  if (wd != 0.f) gi = add_rn(gi, mul_rn(pw, wd));
  return gi;
}

// torch.optim.SGD's update of one element.  MOM: momentum != 0 (the buffer exists)
template <bool MOM>
__device__ __forceinline__ void sgd_update(float& pw, float gr, float& bu, float coef, float cv, float lr, float wd,
                                           float momentum, float omd, bool nesterov, bool first) {
  float gi = solver_grad(pw, gr, coef, cv, wd);
  if (MOM) {
    const float b = first ? gi : add_rn(mul_rn(bu, momentum), mul_rn(gi, omd));
    bu = b;
    gi = nesterov ? add_rn(gi, mul_rn(b, momentum)) : b;
  }
  pw = sub_rn(pw, mul_rn(gi, lr));
}

// 12 B per parameter without momentum, 20 B with it.  `first`: this is the first applied step (the guard has already
// advanced `applied`), the one that copies the gradient into the buffer.
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ buf, int64_t n, int64_t n_decay,
                                                          const svit_step_host* __restrict__ h,
                                                          const svit_step_dev* __restrict__ d, float momentum, float omd,
                                                          int nesterov, const RangeTable T) {
  if (d->apply == 0) return;
  const float coef = d->coef;
  const bool first = d->applied == 1, nest = nesterov != 0;
  const float cv = h->clip_value;
  const GroupRates r = {h->lr[0], h->lr[1], h->weight_decay[0], h->weight_decay[1]};
  const int64_t window = (int64_t)blockDim.x * 4, stride = (int64_t)gridDim.x * window;
  int k = 0;
  for (int64_t lo = (int64_t)blockIdx.x * window; lo < n; lo += stride) {
    const int64_t i = lo + (int64_t)threadIdx.x * 4;
    float lr = 0.f, wd = 0.f;
    if (!range_rates(T, k, lo, lo + window, i, n_decay, r, lr, wd)) continue;
    const int64_t q = i >> 2;
    float4 P = ((const float4*)p)[q], B = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 G = ((const float4*)g)[q];
    if (MOM) B = ((const float4*)buf)[q];
    sgd_update<MOM>(P.x, G.x, B.x, coef, cv, lr, wd, momentum, omd, nest, first);
    sgd_update<MOM>(P.y, G.y, B.y, coef, cv, lr, wd, momentum, omd, nest, first);
    sgd_update<MOM>(P.z, G.z, B.z, coef, cv, lr, wd, momentum, omd, nest, first);
    sgd_update<MOM>(P.w, G.w, B.w, coef, cv, lr, wd, momentum, omd, nest, first);
    ((float4*)p)[q] = P;
    if (MOM) ((float4*)buf)[q] = B;
  }
}

// torch.optim.Adam's update of one element (coupled L2, no amsgrad); step = lr_eff / bc1, formed once per quad
__device__ __forceinline__ void adam_update(float& pw, float gr, float& mo, float& va, float coef, float cv, float step,
                                            float wd, float b1, float b2, float omb1, float omb2, float eps,
                                            float bc2_sqrt) {
  const float gi = solver_grad(pw, gr, coef, cv, wd);
  const float mi = add_rn(mul_rn(mo, b1), mul_rn(gi, omb1));
  const float vi = add_rn(mul_rn(va, b2), mul_rn(mul_rn(gi, gi), omb2));
  const float denom = add_rn(div_rn(sqrt_rn(vi), bc2_sqrt), eps);
  pw = sub_rn(pw, mul_rn(step, div_rn(mi, denom)));
  mo = mi;
  va = vi;
}

// 28 B per parameter, as the AdamW tail
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           int64_t n_decay, const svit_step_host* __restrict__ h,
                                                           const svit_step_dev* __restrict__ d, float b1, float b2,
                                                           float eps, const RangeTable T) {
  if (d->apply == 0) return;
  const float coef = d->coef, bc1 = d->bc1, bc2_sqrt = d->bc2_sqrt;
  const float cv = h->clip_value;
  const float omb1 = sub_rn(1.f, b1), omb2 = sub_rn(1.f, b2);
  const GroupRates r = {h->lr[0], h->lr[1], h->weight_decay[0], h->weight_decay[1]};
  const int64_t window = (int64_t)blockDim.x * 4, stride = (int64_t)gridDim.x * window;
  int k = 0;
  for (int64_t lo = (int64_t)blockIdx.x * window; lo < n; lo += stride) {
    const int64_t i = lo + (int64_t)threadIdx.x * 4;
    float lr = 0.f, wd = 0.f;
    if (!range_rates(T, k, lo, lo + window, i, n_decay, r, lr, wd)) continue;
    const float step = div_rn(lr, bc1);
    const int64_t q = i >> 2;
    float4 P = ((const float4*)p)[q], M = ((const float4*)m)[q], V = ((const float4*)v)[q];
    const float4 G = ((const float4*)g)[q];
    adam_update(P.x, G.x, M.x, V.x, coef, cv, step, wd, b1, b2, omb1, omb2, eps, bc2_sqrt);
    adam_update(P.y, G.y, M.y, V.y, coef, cv, step, wd, b1, b2, omb1, omb2, eps, bc2_sqrt);
    adam_update(P.z, G.z, M.z, V.z, coef, cv, step, wd, b1, b2, omb1, omb2, eps, bc2_sqrt);
    adam_update(P.w, G.w, M.w, V.w, coef, cv, step, wd, b1, b2, omb1, omb2, eps, bc2_sqrt);
    ((float4*)p)[q] = P; ((float4*)m)[q] = M; ((float4*)v)[q] = V;
  }
}

// ---- exponential moving average of the weights behind a solver (svit_ema_step_guarded) --------------------------------
// is the quad at float index i of the window [lo, hi) inside a range?  range_rates without the rates
__device__ __forceinline__ bool range_holds(const RangeTable& T, int& k, int64_t lo, int64_t hi, int64_t i) {
  while (k < T.S && T.v[k][1] <= lo) ++k;
  bool in = false;
  for (int j = k; j < T.S && T.v[j][0] < hi; ++j) in |= (i >= T.v[j][0]) & (i < T.v[j][1]);
  return in;
}

__device__ __forceinline__ float ema_update(float e, float pw, float d, float omd) {
  return add_rn(mul_rn(e, d), mul_rn(pw, omd));
}

// 12 B per parameter: p read, ema read and written.  The update number is the guard's counter plus the host's offset:
// no workgroup writes anything its neighbours read.  Record, offset and table entry sit at workgroup-uniform addresses.
__global__ __launch_bounds__(256) void ema_guarded_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n,
                                                          const float* __restrict__ table, int64_t entries, float decay,
                                                          const int64_t* __restrict__ er,
                                                          const svit_step_dev* __restrict__ d, const RangeTable T) {
  if (d->apply == 0) return;
  int64_t upd = d->applied + er[0];
  upd = upd < 1 ? 1 : upd;
  const float dk = upd <= entries ? table[upd - 1] : decay;
  const float omd = sub_rn(1.0f, dk);
  const int64_t window = (int64_t)blockDim.x * 4, stride = (int64_t)gridDim.x * window;
  int k = 0;
  for (int64_t lo = (int64_t)blockIdx.x * window; lo < n; lo += stride) {
    const int64_t i = lo + (int64_t)threadIdx.x * 4;
    if (!range_holds(T, k, lo, lo + window, i)) continue;
    const int64_t q = i >> 2;
    float4 E = ((const float4*)ema)[q];
    const float4 P = ((const float4*)p)[q];
    E.x = ema_update(E.x, P.x, dk, omd);
    E.y = ema_update(E.y, P.y, dk, omd);
    E.z = ema_update(E.z, P.z, dk, omd);
    E.w = ema_update(E.w, P.w, dk, omd);
    ((float4*)ema)[q] = E;
  }
}

// 0 < decay < 1, by the bits (positive floats order as their bit patterns; a NaN, an inf and every negative lie above 1.0)
inline bool ema_decay_ok(float decay) {
  uint32_t bits;
  memcpy(&bits, &decay, sizeof bits);
  return bits > 0u && bits < 0x3f800000u;
}

// entry k - 1 of the warm-up table, on the HOST in IEEE double arithmetic whatever the build's flags
inline float ema_warmup_decay(float decay, int64_t k) {
#pragma float_control(precise, on)
  const double w = (1.0 + (double)k) / (10.0 + (double)k), dd = (double)decay;
  return (float)(dd < w ? dd : w);
}

// the checks of svit_adamw_step_guarded_lr, with its error codes, before any HIP call; the tables in kernel-argument form
// (n_decay < 0: no weight-decay boundary to respect)
int range_table_take(const int64_t* segs, const float* scales, int64_t S, int64_t n, int64_t n_decay, RangeTable* out) {
  if (!segs || S < 1 || S > SVIT_MAX_SEGS) return SVIT_ERR_ARG;
  int64_t prev = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t b = segs[2 * s], e = segs[2 * s + 1];
    if (b < prev || e <= b || e > n) return SVIT_ERR_ARG;                   // unsorted / overlapping, empty, past the buffer
    if (b < n_decay && e > n_decay) return SVIT_ERR_ARG;                    // straddles the weight-decay boundary
    prev = e;
  }
  for (int64_t s = 0; s < 2 * S; ++s)
    if (segs[s] & 3) return SVIT_ERR_ALIGN;
  for (int64_t s = 0; s < SVIT_MAX_SEGS; ++s) {
    out->v[s][0] = s < S ? segs[2 * s] : 0;
    out->v[s][1] = s < S ? segs[2 * s + 1] : 0;
    uint32_t bits = 0x3f800000u;                                            // scales == NULL: every scale is 1.0
    if (s < S && scales) memcpy(&bits, scales + s, sizeof bits);
    // finite and > 0, by the bits
    if (s < S && ((bits & 0x7f800000u) == 0x7f800000u || (bits >> 31) || (bits & 0x7fffffffu) == 0)) return SVIT_ERR_ARG;
    if (s >= S) bits = 0;
    memcpy(&out->scale[s], &bits, sizeof bits);
  }
  out->S = (int32_t)S;
  return SVIT_OK;
}

inline unsigned solver_grid(int64_t span) {
  int64_t b = ((span >> 2) + 255) / 256;          // the grid of svit_adamw_step_guarded_lr: the ranges' extent, capped
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
}  // namespace

extern "C" int svit_sgd_step_guarded(float* p, const float* g, float* buf, int64_t n, int64_t n_decay,
                                     const int64_t* segs, const float* scales, int64_t S,
                                     const svit_step_host* host_rec, const svit_step_dev* dev_rec, float momentum,
                                     float dampening, int nesterov, void* stream) {
  if (!p || !g || !host_rec || !dev_rec || n <= 0 || n_decay < 0 || n_decay > n) return SVIT_ERR_ARG;
  if (nesterov && (!(momentum > 0.f) || dampening != 0.f)) return SVIT_ERR_ARG;
  if (momentum != 0.f && !buf) return SVIT_ERR_ARG;
  RangeTable T;
  if (int rc = range_table_take(segs, scales, S, n, n_decay, &T)) return rc;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)host_rec | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  const float omd = 1.f - dampening;
  const int64_t span = T.v[S - 1][1];
  if (momentum != 0.f)
    hipLaunchKernelGGL(sgd_guarded_kernel<true>, dim3(solver_grid(span)), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                       span, n_decay, host_rec, dev_rec, momentum, omd, nesterov, T);
  else
    hipLaunchKernelGGL(sgd_guarded_kernel<false>, dim3(solver_grid(span)), dim3(256), 0, (hipStream_t)stream, p, g,
                       (float*)nullptr, span, n_decay, host_rec, dev_rec, momentum, omd, nesterov, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_ema_decay_table(float decay, float* table, int64_t capacity, int64_t* n_entries) {
  if (!n_entries || (table && capacity < 0) || !ema_decay_ok(decay)) return SVIT_ERR_ARG;
  constexpr int64_t kMax = 1ll << 20;
  for (int64_t k = 1; k <= kMax; ++k) {
    const float e = ema_warmup_decay(decay, k);
    if (table) {
      if (k > capacity) return SVIT_ERR_ARG;
      table[k - 1] = e;
    }
    if (e == decay) {
      *n_entries = k;
      return SVIT_OK;
    }
  }
  return SVIT_ERR_ARG;
}

extern "C" int svit_ema_step_guarded(float* ema, const float* p, int64_t n, const int64_t* segs, int64_t S,
                                     const float* decay_table, int64_t table_entries, float decay,
                                     const int64_t* ema_rec, const svit_step_dev* dev_rec, void* stream) {
  if (!ema || !p || !ema_rec || !dev_rec || n <= 0 || !ema_decay_ok(decay)) return SVIT_ERR_ARG;
  if (table_entries < 0 || table_entries > (1ll << 20) || (table_entries > 0 && !decay_table)) return SVIT_ERR_ARG;
  RangeTable T;
  if (int rc = range_table_take(segs, nullptr, S, n, -1, &T)) return rc;
  if (((uintptr_t)ema | (uintptr_t)p) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)ema_rec | (uintptr_t)dev_rec) & 7 || ((uintptr_t)decay_table & 3)) return SVIT_ERR_ALIGN;
  const int64_t span = T.v[S - 1][1];
  hipLaunchKernelGGL(ema_guarded_kernel, dim3(solver_grid(span)), dim3(256), 0, (hipStream_t)stream, ema, p, span,
                     decay_table, table_entries, decay, ema_rec, dev_rec, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                                      const int64_t* segs, const float* scales, int64_t S,
                                      const svit_step_host* host_rec, const svit_step_dev* dev_rec, float beta1,
                                      float beta2, float eps, void* stream) {
  if (!p || !g || !m || !v || !host_rec || !dev_rec || n <= 0 || n_decay < 0 || n_decay > n) return SVIT_ERR_ARG;
  RangeTable T;
  if (int rc = range_table_take(segs, scales, S, n, n_decay, &T)) return rc;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return SVIT_ERR_ALIGN;
  if (((uintptr_t)host_rec | (uintptr_t)dev_rec) & 7) return SVIT_ERR_ALIGN;
  const int64_t span = T.v[S - 1][1];
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(solver_grid(span)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, span,
                     n_decay, host_rec, dev_rec, beta1, beta2, eps, T);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
