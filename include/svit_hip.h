/* libsvit_hip.so -- C ABI of the MI355X-native SViT forward/backward kernels.
 *
 * Drop-in boundary: the reference has no native code; every entry point
 * below replaces an ATen op sequence of the reference's Python hot path (file:line cited
 * per function, relative to the reference tree).  The reference-side binding is the
 * `torch.autograd.Function` / ctypes stub shown in INTEGRATION.md.
 *
 * Conventions: all pointers are DEVICE pointers (hipMalloc'ed / torch CUDA tensors) unless
 * marked host; `stream` is a hipStream_t passed as void*; every function only enqueues work
 * on `stream` (no allocation, no synchronisation -> hipGraph-capturable) and returns 0 on
 * success, a negative SVIT_ERR_* for argument errors, or a positive hipError_t.
 * bf16 tensors are raw uint16 bit patterns.  Token order everywhere is
 * [cls | patches (t,y,x row-major) | objects]; head_dim is 96.
 */
#ifndef SVIT_HIP_H
#define SVIT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SVIT_HEAD_DIM 96

int svit_version(void);
const char* svit_arch(void); /* "gfx950" */

/* ---------------------------------------------------------------- GEMM family (K4) ---- */
/* nn.Linear everywhere: slowfast/models/attention.py:228,230,344-349,462,546-547,561;
 * slowfast/models/common.py:20-22,26-34; patch embed conv as implicit GEMM
 * (slowfast/models/stem_helper.py:309-320). */
enum {
  SVIT_EPI_BF16 = 0,   /* out(bf16)  = acc + bias                                   */
  SVIT_EPI_GELU = 1,   /* h = acc + bias; out(bf16) = gelu_erf(h); out2(bf16) = gelu_erf'(h) (out2 may be NULL) */
  SVIT_EPI_RESID = 2,  /* out(f32)   = aux(f32) + row_scale[row/rows_per_sample]*(acc+bias)
                          (proj / fc2 + DropPath + residual, attention.py:565,570)    */
  SVIT_EPI_F32 = 3,    /* out(f32)   = [out +] acc + bias, optional row remap         */
  SVIT_EPI_DGELU = 4,  /* out(bf16)  = acc * aux(bf16), aux = the saved gelu_erf'(h) (fc2 dgrad) */
  SVIT_EPI_RELQ = 5    /* rel-pos query side in ONE launch (round 3; replaces svit_gemm_nt + svit_relpos_gather,
                          attention.py:84-183): acc = q . Rcat^T is not stored; instead
                          relq_out[row, 96 + j] = bf16(bf16(acc[row, relq_map[(row % relq_rows) * relq_extra + j]])
                          * relq_scale) for j < relq_extra, 0 where the map holds -1 (cls / object rows, padding) */
};
typedef struct {
  const void* A; int32_t lda;      /* bf16 [M,K] row-major                             */
  const void* W; int32_t ldw;      /* bf16 [N,K] row-major (nn.Linear weight layout)   */
  const float* bias;               /* f32 [N] or NULL                                  */
  void* out; int32_t ldo;
  void* out2; int32_t ldo2;
  const void* aux; int32_t ldaux;
  const float* row_scale; int32_t rows_per_sample;
  int32_t M, N, K;                 /* N % 96 == 0, K % 32 == 0                         */
  int32_t epilogue; int32_t accumulate;
  int32_t remap_L, remap_N, remap_off; /* EPI_F32: out row = (r/L)*remap_N + remap_off + r%L */
  /* EPI_RELQ only (zero otherwise): */
  const int32_t* relq_map;         /* i32 [relq_rows, relq_extra]: column of acc for (token, j), or -1  */
  void* relq_out; int32_t relq_ld; /* bf16 qa rows [M, relq_ld]; columns 96 .. 96+relq_extra are written */
  int32_t relq_extra, relq_rows;   /* relq_extra = relq_ld - 96 in {32, 64}; relq_rows = tokens per (b, head) */
  float relq_scale;
} svit_gemm_args;
/* C[M,N] = A[M,K] * W[N,K]^T with fused epilogue (forward Linear; dgrad with W^T copy). */
int svit_gemm_nt(const svit_gemm_args* args, void* stream);
/* dW[N,K] (f32, atomically accumulated) += A[M,N]^T * B[M,K]  (Linear wgrad; split over M).
 * lda/ldb multiples of 8; K need not be (patch-embed wgrad: K = 441 inside ldb = 448). */
int svit_gemm_tn(const void* A, int lda, const void* B, int ldb, float* dW, int lddw,
                 int M, int N, int K, int splits, float* dbias /* f32 [N] += colsum(A), or NULL */,
                 void* stream);
/* Several independent wgrad GEMMs in ONE launch (the engine queues a block's Linear and rel-pos
 * weight gradients and flushes them together: the per-launch accumulator flush is amortised).
 * Same operand rules as svit_gemm_tn; any count (launched in groups of SVIT_TN_GROUP_MAX).
 * Replaces the per-layer autograd wgrads of slowfast/models/attention.py:377-409 (qkv, proj),
 * common.py:26-37 (fc1, fc2) and the rel-pos table grads of attention.py:77-139. */
#define SVIT_TN_GROUP_MAX 16
typedef struct {
  const void* A; const void* B; float* dW; float* dbias;   /* dbias may be NULL */
  int32_t lda, ldb, lddw, M, N, K;
} svit_tn_problem;
int svit_gemm_tn_grouped(const svit_tn_problem* probs, int count, void* stream);
/* ordered != 0: no split along the reduction rows -- one atomic add per dW element, i.e.
 * bit-reproducible weight gradients (regression-diff mode; slower). */
int svit_gemm_tn_grouped_ex(const svit_tn_problem* probs, int count, int ordered, void* stream);
/* Slab form of svit_gemm_tn_grouped (same problems, same `dW +=` / `dbias +=`, same row splits and speed class): every
 * row split stores its fp32 tile and bias partials into its own slab of `workspace` with plain stores, and a second
 * launch behind each group's GEMM sums the splits of every element in index order and adds the sum to dW / dbias with
 * one plain read-modify-write -- no atomics.  Guarantee: for fixed shapes and a fixed knob table, the result depends
 * only on the operands (not on scheduling: bit-reproducible run to run).  Groups past SVIT_TN_GROUP_MAX reuse the
 * workspace in stream order, so a workspace belongs to ONE stream at a time.  A NULL workspace or workspace_floats
 * below svit_gemm_tn_grouped_workspace(probs, count) is SVIT_ERR_ARG (-4), a workspace not 16-byte aligned
 * SVIT_ERR_ALIGN, both before any launch. */
int svit_gemm_tn_grouped_slab(const svit_tn_problem* probs, int count, float* workspace,
                              int64_t workspace_floats, void* stream);
/* floats of workspace that call needs (the largest of its groups); host-only arithmetic on the shapes and the knob
 * table (no HIP call: works without a GPU), never smaller than what svit_gemm_tn_grouped_slab checks for; a negative
 * SVIT_ERR_* for the argument errors that entry point reports. */
int64_t svit_gemm_tn_grouped_workspace(const svit_tn_problem* probs, int count);
/* svit_gemm_tn_grouped_slab for the LEADING launch_count problems (1 <= launch_count <= count, else SVIT_ERR_ARG) of a
 * list that is checked and planned whole; the pointers of the rest are never followed (any aligned non-null address).
 * The planner cuts every problem of a launch by one step count found over all its problems, so the leading problems
 * get the row splits -- hence, bit for bit, the results -- they have in svit_gemm_tn_grouped_slab over the whole list.
 * The backward that stops above frozen blocks (svit_amd/engine.py) passes, behind its own problems, the shapes of the
 * problems the full backward queues into the same launch.  Workspace as for the whole list. */
int svit_gemm_tn_grouped_slab_lead(const svit_tn_problem* probs, int count, int launch_count, float* workspace,
                                   int64_t workspace_floats, void* stream);
/* dbias[N] (f32, atomically accumulated) += column sums of bf16 A[M,N]. */
int svit_colsum_bf16(const void* A, int lda, float* out, int M, int N, void* stream);

/* ------------------------------------------------------------- elementwise / casts ---- */
int svit_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
/* Rel-pos tables at another resolution (attention.py:84-137 interpolates rel_pos_h / _w / _t with F.interpolate when the
 * query / key grid differs from the table's): out[r][c] = sum_j M[r][j] * tables[j][c], c < 96, with M [rows, J] the
 * fp32 matrix of linear-interpolation weights (zero rows pad to a multiple of 96) and tables [J, 96] the block's three
 * adjacent fp32 tables.  out32 (fp32 [rows, 96]) and / or out16 (bf16 [rows, 96]) may be NULL (not both). */
int svit_table_interp(const float* M, int rows, int J, const float* tables, float* out32, void* out16, void* stream);
/* The same for every block of a forward pass in one launch: `jobs_dev` = n_jobs descriptors in DEVICE memory (the caller
 * caches the table per input geometry: the pointers are those of its persistent buffers), max_rows = the largest `rows`. */
typedef struct svit_table_interp_job {
  const float* M;        /* [rows, J] interpolation weights */
  const float* tables;   /* [J, 96] */
  float* out32;          /* [rows, 96] or NULL */
  void* out16;           /* bf16 [rows, 96] or NULL */
  int32_t rows, J;
} svit_table_interp_job;
int svit_table_interp_batched(const svit_table_interp_job* jobs_dev, int n_jobs, int max_rows, void* stream);
/* batched fp32 [R,C] -> bf16 [C,R] transposes described by a device table of
 * {src_off, dst_off, R, C, ldd} int64 quintuples: dst[c*ldd + r] (the W^T copies used by
 * dgrad; ldd > R places a table inside a wider row, e.g. the concatenated rel-pos tables). */
int svit_transpose_cast_batched(const float* src_base, void* dst_base, const int64_t* table,
                                int n_mats, int max_tiles, void* stream);
/* the same transposes, bf16 [R,C] -> bf16 [C,R], from the bf16 mirror of the weights (same table; offsets then index
 * the mirror): what the step uses -- half the bytes of the fp32 form, 16-byte accesses both ways.  max_tiles counts
 * 64 x 64 tiles here. */
int svit_transpose_bf16_batched(const void* src_base, void* dst_base, const int64_t* table,
                                int n_mats, int max_tiles, void* stream);
/* dst(bf16)[R,ldd] = [src(f32)[R,C] | 0]: row-padded bf16 copy (patch-embed weight 441 -> 448). */
int svit_pad_cast_rows(const float* src, void* dst, int R, int C, int ldd, void* stream);
/* dst(bf16)[r,:] = scale[r/rows_per_sample] * src(f32)[row(r),:]   (DropPath backward).
 * row(r) = r, or with gather_L > 0 the row gather (r / L) * gather_N + gather_off + r % L
 * (the patch rows [1, 1+L) of every sample of a [B, N, C] token tensor in one launch). */
int svit_scale_cast(const float* src, void* dst, const float* row_scale, int rows_per_sample,
                    int64_t rows, int cols, int gather_L, int gather_N, int gather_off,
                    void* stream);

/* ------------------------------------------- deferred second-stage reductions ---------- */
/* svit_layernorm_bwd, svit_pool_ln_bwd(_qkv) and svit_pool_conv_wgrad(_qkv) finish with a
 * "reduce partial rows" launch.  The queue is PER STREAM: between svit_reduce_defer(1, s) and
 * svit_reduce_flush(s) / svit_reduce_defer(0, s) the reduces launched ON STREAM s are queued
 * (host side) and run as ONE launch on s -- the engine brackets a transformer block's backward
 * with them.  Launches on any other stream are unaffected (they reduce at once on their own
 * stream).  While deferred, every producer must be given its own workspace region (the rows are
 * read at the flush), and the gradients are final only after the flush.  svit_reduce_defer(1)
 * drops leftovers of an aborted bracket; svit_reduce_reset(s) is the error path: forget s's queue
 * and leave deferred mode.  Thread-safe (mutex-guarded map keyed by stream; no other global
 * mutable state in the library). */
int svit_reduce_defer(int on, void* stream);
int svit_reduce_flush(void* stream);
int svit_reduce_reset(void* stream);

/* ---------------------------------------------------------------- LayerNorm (K3) ------ */
/* nn.LayerNorm(eps=1e-6): attention.py:501,531; video_model_builder.py:69,233. */
int svit_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16,
                       float* y_f32, float* mean, float* rstd, int64_t rows, int C, float eps,
                       void* stream);
/* dx = [dres +] LN'(dy); dgamma/dbeta += column sums (two-stage: per-block partial rows in
 * `workspace`, then one reduce launch -- no same-address atomics). dy is f32 or bf16.
 * dx_bf16 (optional): also bf16(row_scale[row / rows_per_sample] * dx) -- the DropPath-scaled
 * operand of the next backward GEMM (common.py:46-59), fused instead of a separate cast pass;
 * row_scale may be NULL (scale 1). */
int svit_layernorm_bwd(const void* dy /* f32, or bf16 when dy_is_bf16 */, int dy_is_bf16,
                       const float* x, const float* gamma, const float* mean,
                       const float* rstd, const float* dres, float* dx, void* dx_bf16,
                       const float* row_scale, int rows_per_sample, float* dgamma,
                       float* dbeta, int64_t rows, int C, float* workspace,
                       int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------ patch embedding (K1/K2) - */
/* im2col for Conv3d(3->96, k(3,7,7), s(2,4,4), p(1,3,3)) (stem_helper.py:309-320):
 * video f32 [B,3,T,H,W] -> cols bf16 [B*T'*H'*W', 448] (441 taps, zero-padded to 448). */
int svit_im2col_patch(const float* video, void* cols, int B, int T, int H, int W, void* stream);
/* Data gradient of that convolution (csrc/dgrad.hip): the gradient of the loss with respect to the input clip, from the
 * two bf16 operands the backward already holds.  With To = (T-1)/2 + 1, Ho = (H-1)/4 + 1, Wo = (W-1)/4 + 1:
 *   dvideo[b,c,t,y,x] = sum over (to,kt), (yo,ky), (xo,kx) with t = 2to-1+kt, y = 4yo-3+ky, x = 4xo-3+kx, kt in [0,3),
 *                       ky, kx in [0,7), (to,yo,xo) inside [0,To) x [0,Ho) x [0,Wo), of
 *                       sum_{n<96} dtok[(b,to,yo,xo), n] * w16[n, ((c*3+kt)*7+ky)*7+kx]
 * -- at most 2 x 2 x 2 output positions reach a pixel, so at most 768 products, each exact in fp32, summed in fp32 in
 * a fixed order.  w16 is the forward GEMM's operand in svit_im2col_patch's column order; its pad columns 441..447 are
 * never read.  Gather form: every element of dvideo is stored exactly once by the thread that owns it (no atomics,
 * nothing to zero beforehand, nothing outside [B,3,T,H,W] touched), so the result is bit-identical from run to run and
 * from an eager pass to a graph replay.  Any T, H, W >= 1 (T = 1: the stills, only kt = 1 exists).  Checked before any
 * HIP call: a null pointer or a size < 1 is SVIT_ERR_ARG; dtok or w16 not 16-byte aligned, or dvideo not 4-byte
 * aligned, SVIT_ERR_ALIGN; B*To*Ho*Wo >= 2^31 (or T*H >= 2^31) SVIT_ERR_SHAPE.  Element offsets are 64-bit. */
int svit_patch_embed_dgrad(const void* dtok /* bf16 [B*To*Ho*Wo, 96] */, const void* w16 /* bf16 [96, 448] */,
                           float* dvideo /* f32 [B,3,T,H,W] */, int B, int T, int H, int W, void* stream);
/* ------------------------------------------------------------ attribution passes (csrc/attrib.hip) - */
/* SmoothGrad / integrated gradients (svit_amd/attribution.py) run one input-gradient pass per sample point; these two
 * streaming kernels stand in front of and behind the pass.  Both read ONE 32-byte record from DEVICE memory at run time,
 * so a captured pass body holds the same launches for every pass:
 *   alpha   the point on the path base -> x (1 = the clip itself)      weight  what this pass's gradient is scaled by
 *   seed    31-bit seed of this pass's noise field                     pass    0-based pass number; 0 STORES the sum
 *   flags   bit 0: accumulate g*g instead of g                         pad     0
 * Every fp32 operation named below is rounded once, on its own (helpers that keep the compiler from fusing them).
 * svit_attr_perturb: x, out f32 [B,3,T,H,W] (out may not alias x or base); base the same shape or NULL (zeros); sigma f32
 * [B] or NULL.  Per element  d = x - base;  p = base + alpha*d;  out = p + sigma[b]*n  -- the sigma term is SKIPPED for a
 * NULL sigma (not multiplied by 0), and n = N(0,1) is the erasing noise of svit_u8_clips_render's pixel mode: Philox keyed
 * by `seed`, counter (y*W + x, clip b, plane c*T + t), Box-Muller; |n| <= 5.77, a pure function of (seed, b, c, t, y, x).
 * svit_attr_accumulate: g, acc f32 [n].  v = (flags & 1) ? g*g : g;  t = weight*v;  acc = (pass == 0) ? t : acc + t -- the
 * first pass never reads acc, so nothing has to be zeroed.  With `scores` f32 [rows, B] the B values of `scores_in` f32
 * [B] (this pass's per-sample scores) are copied bit for bit into row `pass`; a pass >= rows writes no score.
 * Both: grid-stride over 16-byte vectors from the output's first 16-byte boundary, single elements in front and behind (any
 * n, any 4-byte aligned pointers; inputs misaligned differently from the output are walked element by element), 64-bit
 * offsets, no atomics, every output element stored exactly once, nothing outside the outputs touched.  Checked before any
 * HIP call: a null x / rec / out (g / acc / rec), a size < 1, or scores without scores_in or with rows < 1 is
 * SVIT_ERR_ARG; a pointer not 4-byte aligned SVIT_ERR_ALIGN; H*W or B*3*T of 2^31 or more SVIT_ERR_SHAPE. */
typedef struct {
  float alpha, weight;
  uint32_t seed, pass, flags, pad[3];
} svit_attr_pass;
int svit_attr_perturb(const float* x, const float* base /* or NULL */, const float* sigma /* f32 [B] or NULL */,
                      const void* rec /* svit_attr_pass, device */, float* out, int B, int T, int H, int W, void* stream);
int svit_attr_accumulate(const float* g, float* acc, const void* rec /* svit_attr_pass, device */,
                         const float* scores_in /* f32 [B] or NULL */, float* scores /* f32 [rows, B] or NULL */, int rows,
                         int64_t n, int B, void* stream);
/* The same operand straight from decoded uint8 frames: frames u8
 * [V,T,Hs,Ws,3] (T H W C per video, `frames_bytes` = size of the buffer), lut bf16 [3,256] =
 * bf16((u/255 - mean[c]) / std[c]) (datasets/utils.py:287-303), crops int32 [B,3] = (source video,
 * y0, x0) per output clip (transform.py:327-342; NULL: clip b = video b at (0,0)); the S x S
 * window is normalised, zero-padded and laid out as cols bf16 [B*T'*S'*S', 448]. The crop table
 * is NOT range-checked on the device: the caller guarantees y0 + S <= Hs, x0 + S <= Ws, v < V. */
int svit_im2col_patch_u8(const uint8_t* frames, int64_t frames_bytes, const void* lut,
                         const int32_t* crops, void* cols, int B, int T, int Hs, int Ws, int S,
                         void* stream);
/* Mixup / CutMix of a batch (cfg.MIXUP; slowfast/datasets/mixup.py, tools/train_net.py:63-71,92-94).  All three
 * entry points of the feature read ONE 32-byte record `mix` from DEVICE memory, so a captured step holds the same
 * launches for every draw:
 *   word [0] int32 mode: 0 none, 1 mixup, 2 CutMix        [1] float lam        [2] float oml = (float)(1.0 - lam), the
 *   subtraction in double (what torch does with the Python scalar; NOT 1 - (float)lam)      [3..6] int32 yl, yh, xl, xh
 *   [7] 0.        For CutMix `lam` is the area-corrected value and only the soft target uses it.
 * svit_mixup_clips: x f32 contiguous [B, planes, H, W] (planes = 3*T of a [B,3,T,H,W] batch), IN PLACE; clip b is paired
 * with clip B-1-b.  mixup: x[b] = x[b]*lam + x[B-1-b]*oml, products and sum each rounded to nearest (no fma), bit-equal to
 * torch's mul_/add_ sequence; for odd B the middle clip blends with itself through the same formula.  CutMix: the two
 * clips are swapped inside [yl,yh) x [xl,xh) of every plane (an empty box is legal).  Mode 0 leaves x bit-unchanged.
 * float4 accesses when W % 4 == 0 and x is 16-byte aligned, scalar otherwise. */
int svit_mixup_clips(float* x, const void* mix, int B, int planes, int H, int W, void* stream);
/* svit_im2col_patch_u8 with the mix applied between the normalisation and the bf16 rounding: lut_f32 f32 [3,256] =
 * (u/255 - mean[c]) / std[c] unrounded; the partner of clip b is clip B-1-b, read through ITS crop row at the same
 * (t, y, x) of the crop; values are blended (mode 1) or selected by the box in crop coordinates (mode 2) with the
 * formulas above and only then rounded to bf16.  Mode 0 gives exactly the bytes of svit_im2col_patch_u8. */
int svit_im2col_patch_u8_mix(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32,
                             const int32_t* crops, const void* mix, void* cols, int B, int T, int Hs,
                             int Ws, int S, void* stream);
/* Training augmentation on the uint8 route (svit_amd/augment.py): the reference's post-normalisation spatial pipeline of
 * `spatial_sampling` + `RandomErasing` (slowfast/datasets/utils.py:110-192, transform.py:47-105,154-191,248-285,596-683,
 * random_erasing.py) applied while the clip is read.  One 64-byte record per output clip, in DEVICE memory (so a captured
 * step serves every draw):
 *   struct SvitAug { int32 video, i, j, h, w, out_h, out_w, oy, ox, flip, erase_mode, et, el, eh, ew, seed; }
 *   video          source video index
 *   i, j, h, w     source rectangle inside the frame (top, left, height, width)
 *   out_h, out_w   size the rectangle is resampled to (bilinear, F.interpolate(..., align_corners=False) given size=)
 *   oy, ox         offset of the S x S window inside that resampled image
 *   flip           horizontal flip of the window (non-zero = on)
 *   erase_mode     0 none, 1 const (0), 2 rand (one N(0,1) per clip, channel, frame), 3 pixel (one per element)
 *   et, el, eh, ew erase box (top, left, height, width) in output coordinates, on every frame
 *   seed           noise seed: Philox-4x32-10 keyed by it, counter (y*S + x, clip, channel*T + frame), Box-Muller
 * random-resized crop: out = S, o = 0; short-side jitter + crop (train or test): i = j = 0, (h, w) = (Hs, Ws), out = the
 * rescaled size, o = the crop offset.  Output pixel (c, t, y, x): xs = flip ? S-1-x : x; per axis scale = float(in) /
 * float(out), src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min(int(src), in-1), i1 = i0 + (i0 < in-1), l1 = clamp(src - i0,
 * 0, 1), l0 = 1 - l1; the four taps come from lut_f32 and are combined as l0y*(l0x*a + l1x*b) + l1y*(l0x*c + l1x*d) in fp32.
 * The kernels clamp every record into the buffer (video into [0, V), h / w into [1, Hs] / [1, Ws], i / j so that the
 * rectangle lies in the frame, out into [1, 2^24], o into [0, max(out - S, 0)], the box into the window; erase modes
 * outside 1..3 are 0), so a record rewritten on the device never addresses outside `frames_bytes`.
 * svit_im2col_patch_u8_aug: the [B*T'*S'*S', 448] bf16 operand of svit_im2col_patch_u8 from those values, rounded ONCE;
 * `mix` (NULL or the record of svit_mixup_clips) blends / swaps clip b with clip B-1-b -- sampled through ITS record at
 * the same (t, y, x) -- before the rounding, as svit_im2col_patch_u8_mix does.  With in == out, no flip and no erase the
 * bytes are those of svit_im2col_patch_u8 (_mix) with the crop table (video, i + oy, j + ox).  S need not fit the frames.
 * svit_u8_clips_render: the same values unrounded, out f32 [B,3,T,S,S].
 * svit_im2col_patch_u8_aug_frames: the operand of the FRAMES PASS (the no-grad forward of every clip as B*T single
 * frames, tools/train_net.py:105-110) from the same frames and records: cols bf16 [B*T*S'*S', 448], what
 * svit_im2col_patch gives for the fp32 tensor [B*T,3,1,S,S] whose frame n = b*T + t is frame t of clip b (T' = 1: the
 * temporal taps kt = 0 and kt = 2 are padding and zero, kt = 1 holds the frame).  Every pixel is evaluated with the
 * clip's own (b, t, T), so the erase noise is the clip pass's; with `mix` the partner of frame (b, t) is frame (B-1-b, t)
 * through that clip's record, mixed before the one rounding.  For T = 1 the bytes are svit_im2col_patch_u8_aug's.  Same
 * clamping and the same argument checks as svit_im2col_patch_u8_aug (cols 16-byte aligned, B*T*S' below 2^31), all made
 * before the launch. */
int svit_im2col_patch_u8_aug(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                             const void* mix, void* cols, int B, int T, int Hs, int Ws, int S, void* stream);
int svit_im2col_patch_u8_aug_frames(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                                    const void* mix, void* cols, int B, int T, int Hs, int Ws, int S, void* stream);
int svit_u8_clips_render(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                         float* out_f32, int B, int T, int Hs, int Ws, int S, void* stream);
/* PER-VIDEO EXTENTS: clips of different source sizes in one batch.  The batch is still one padded buffer u8
 * [V,T,Hs,Ws,3]; `extents` int32 [V,2] = (h_v, w_v) in DEVICE memory (4-byte aligned) holds each video's true size: video
 * v occupies rows [0, h_v) and columns [0, w_v) of each of its frames, the row pitch stays Ws and the rest of the frame is
 * padding nobody interprets.  The table is read at run time, like the records, so one captured step serves batches of any
 * mix of sizes up to (Hs, Ws).  Every kernel clamps an extent into [1,Hs] x [1,Ws] before use, so no table addresses
 * outside the buffer.  NULL: every video fills the buffer -- the `_ext` entry points then run exactly what the plain ones
 * run (the plain ones forward NULL).
 * The three kernels above clamp a record's rectangle into ITS VIDEO'S extent instead of the buffer (h into [1, h_v], i
 * into [0, h_v - h], likewise the width); the mix partner's record is clamped with the partner video's extent.  Nothing
 * else changes. */
int svit_im2col_patch_u8_aug_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                                 const int32_t* extents, const void* mix, void* cols, int B, int T, int Hs, int Ws, int S,
                                 void* stream);
int svit_im2col_patch_u8_aug_frames_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                                        const int32_t* extents, const void* mix, void* cols, int B, int T, int Hs, int Ws,
                                        int S, void* stream);
int svit_u8_clips_render_ext(const uint8_t* frames, int64_t frames_bytes, const float* lut_f32, const void* aug,
                             const int32_t* extents, float* out_f32, int B, int T, int Hs, int Ws, int S, void* stream);
/* RandAugment on the uint8 frames (cfg.AUG.AA_TYPE / INTERPOLATION; svit_amd/randaug.py, csrc/randaug.hip): the reference's
 * `create_random_augment` (slowfast/datasets/ssv2.py:345-375, rand_augment.py) -- N PIL operations per clip on every frame
 * at source resolution, before normalisation -- with PIL's bytes.  frames u8 [V,T,Hs,Ws,3]; `records` is the table
 * SvitRandAugOp [V,N] in DEVICE memory (8-byte aligned), read at run time, so one captured step serves every draw.  The
 * same operation and arguments apply to every frame of a video; statistics are per frame.
 *   op            0 NONE, 1 AUTOCONTRAST, 2 EQUALIZE, 3 INVERT, 4 POSTERIZE, 5 SOLARIZE, 6 SOLARIZE_ADD, 7 COLOR, 8 CONTRAST,
 *                 9 BRIGHTNESS, 10 SHARPNESS, 11 AFFINE; anything else is NONE
 *   arg_i         bits kept (POSTERIZE; >= 8 is the identity), threshold 0..256 (SOLARIZE), addend (SOLARIZE_ADD, below 128)
 *   arg_f         the enhancement factor (ops 7-10): out = degenerate + arg_f * (source - degenerate) in fp32, product and
 *                 sum rounded separately; truncated for 0 <= arg_f <= 1, else clipped to [0, 255] and truncated
 *   bicubic_mask  AFFINE: bit (t mod 32) set = frame t is resampled bicubically, clear = bilinearly
 *   m[6]          AFFINE: the output -> input map, xo = m0*(x+.5) + m1*(y+.5) + m2, yo = m3*(x+.5) + m4*(y+.5) + m5 in fp64
 *                 without contraction; a pixel outside 0 <= xo < Ws, 0 <= yo < Hs (or NaN) is the fill (128,128,128);
 *                 the filters are ImagingGenericTransform's, every tap index clamped into the frame
 * svit_randaug_stats: one block per (video, frame); returns at once unless the video's op in `layer` is AUTOCONTRAST,
 * EQUALIZE or CONTRAST, else builds the frame's 3 x 256 histogram in LDS (integer counts: order-independent) and writes
 * the 1 KiB slot of that frame in `workspace` (V*T KiB, 4-byte aligned): bytes 0..767 the per-channel table, int32 at
 * byte 768 the Contrast mean.  svit_randaug_apply: layer `layer` of every video from src to dst (same shape, src != dst),
 * EVERY byte of dst written (NONE is a copy).  Both are stream-ordered with no host synchronisation; no record can make
 * either address outside its buffers.  Hs, Ws >= 3. */
typedef struct SvitRandAugOp {
  int32_t op, arg_i;
  float arg_f;
  uint32_t bicubic_mask;
  double m[6];
} SvitRandAugOp;
int svit_randaug_stats(const uint8_t* frames, const void* records, int layer, void* workspace, int V, int T, int Hs,
                       int Ws, int N, void* stream);
int svit_randaug_apply(const uint8_t* src, uint8_t* dst, const void* records, int layer, const void* workspace, int V,
                       int T, int Hs, int Ws, int N, void* stream);
/* The same with per-video extents (the table defined at svit_im2col_patch_u8_aug_ext; NULL = the plain entry points).
 * Inside its extent a video is treated as the tight h_v x w_v image: histograms and the Contrast mean run over h_v*w_v
 * pixels, the AFFINE in-range test and every tap clamp use (w_v, h_v) -- the matrix is the caller's, built for the video's
 * own size -- and the SHARPNESS border ring is row 0, row h_v-1, column 0 and column w_v-1.  Bytes of dst outside the
 * extent are copies of src, so every byte of dst is still written; the grid stays over Hs*Ws and addressing uses the
 * pitch Ws (w_v*3 need not be a multiple of anything). */
int svit_randaug_stats_ext(const uint8_t* frames, const void* records, const int32_t* extents, int layer, void* workspace,
                           int V, int T, int Hs, int Ws, int N, void* stream);
int svit_randaug_apply_ext(const uint8_t* src, uint8_t* dst, const void* records, const int32_t* extents, int layer,
                           const void* workspace, int V, int T, int Hs, int Ws, int N, void* stream);
/* THE BATCH FEEDER's device half (svit_amd/feeder.py, csrc/feed.hip): one uploaded slot -> the buffers a captured step reads,
 * in ONE launch.  The host packs a batch TIGHTLY into a slot -- video v as its own u8 [T,h_v,w_v,3], no padding rows, no
 * zero fill, the small tables behind the videos -- and uploads it with one copy; this launch writes the padded buffer
 * `frames` u8 [V,T,Hs,Ws,3] (the layout of the PER-VIDEO EXTENTS above) and copies up to eight segments.
 *   slot, slot_bytes  the uploaded bytes, DEVICE memory, 16-byte aligned, slot_bytes a positive multiple of 16
 *   offsets           DEVICE int64 [V] (8-byte aligned): byte offset of video v inside the slot; NULL: v*T*Hs*Ws*3
 *   extents           DEVICE int32 [V,2] = (h_v, w_v) (4-byte aligned); NULL: every video is Hs x Ws
 *   frames            DEVICE u8 [V,T,Hs,Ws,3], 16-byte aligned; T*Hs*Ws*3 below 2^31
 *   fill 0..255, swap_rb (any non-zero value is 1), n_seg 0..8
 * The frames.  Both tables are read on the device at run time.  Per video (h, w) is the extent clamped into [1,Hs] x [1,Ws]
 * and n_v = T*h*w*3 (int64).  offsets[v] < 0 or offsets[v] > slot_bytes - n_v: the video is ABSENT and its whole T x Hs x Ws
 * x 3 block becomes `fill`.  Otherwise frames[v,t,y,x,c] = slot[offsets[v] + ((t*h + y)*w + x)*3 + (swap_rb ? 2-c : c)] for
 * y < h, x < w, and `fill` elsewhere (swap_rb: a decoder that yields RGB feeds weights trained on the reference's BGR,
 * slowfast/datasets/utils.py:37).  Every byte of `frames` is written exactly once per launch; an offset may be any byte
 * address (rows of 33 or 57 bytes, videos of 54), the row pitch Ws*3 need not be a multiple of anything.  NOTHING outside
 * [slot, slot + slot_bytes) is ever read, whatever the tables hold: the kernel loads aligned dwords that hold at least one
 * byte of a video lying inside the slot, which is what the alignment rule is for.
 * The segments.  seg[s], s < n_seg: `bytes` bytes from slot + src_off to dst (records, extents, RandAugment table, labels),
 * by extra blocks of the same launch.  src_off is a multiple of 16, dst is 4-byte aligned, bytes >= 0 and need not be a
 * multiple of anything (exactly `bytes` bytes of dst are written), src_off + bytes <= slot_bytes.  A segment must not
 * overlap `frames`, another segment's dst or the slot.
 * Checked on the host before the launch: SVIT_ERR_ARG for a null args / slot / frames / segment dst, fill outside 0..255,
 * n_seg outside 0..8, a segment with negative bytes or src_off or one that leaves the slot; SVIT_ERR_ALIGN for a
 * misaligned slot / frames / offsets / extents / segment dst, slot_bytes or a src_off not a multiple of 16; SVIT_ERR_SHAPE
 * for V, T, Hs or Ws below 1, slot_bytes below 16 or T*Hs*Ws*3 of 2^31 or more.  Stream-ordered, no host synchronisation. */
typedef struct { int64_t src_off; void* dst; int64_t bytes; } svit_feed_seg;
typedef struct {
  const uint8_t* slot; int64_t slot_bytes;
  const int64_t* offsets;
  const int32_t* extents;
  uint8_t* frames;
  int V, T, Hs, Ws, fill, swap_rb, n_seg;
  svit_feed_seg seg[8];
} svit_feed_args;
int svit_feed_unpack(const svit_feed_args* a, void* stream);
/* cls / object token rows of the block-0 input (video_model_builder.py:326-363). */
int svit_fill_special_tokens(float* x, const float* cls, const float* objq, const float* pos_t,
                             int B, int N, int L, int Tx, int O, int C, int add_pos, void* stream);
/* its backward in one launch: g_cls [C] += sum_b dx[b,0]; g_obj [O,C] += sum_{b,t} dx[b,1+L+t*O+o];
 * g_pos [Tx,C] += sum_{b,o} of the same rows (add_pos) -- dx f32 [B,N,C]. */
int svit_special_token_grads(const float* dx, float* g_cls, float* g_obj, float* g_pos, int B, int N,
                             int L, int Tx, int O, int C, int add_pos, void* stream);

/* ------------------------------------------------- pooled q/k/v (K5, K6, K3 fused) ---- */
/* attention_pool with depthwise Conv3d(96,96,3^3,stride (1,s,s),pad 1) + object gain +
 * LayerNorm(96) on every token (attention.py:13-65, 263-304).
 * in : qkv bf16 [B, N, 3, h, 96]  (which = 0/1/2 selects q/k/v)
 * out: bf16 [B, h, Nout, ld_out] columns 0..95 = LN(pooled); pre: bf16 [B,h,Nout,96]
 *      pre-LN pooled values (saved for backward); mean/rstd f32 [B*h*Nout]; pre, mean and rstd
 *      may all be NULL (no-grad passes: nothing is saved).
 * mode 1 (keys) additionally writes the one-hot key coordinates at columns
 *      96 + [y | kh + x | kh + kw + t] used by the in-MFMA relative-position bias. */
typedef struct {
  const void* qkv; int32_t which;
  const float* conv_w;            /* f32 [96, 27]                                      */
  const float* gamma; const float* beta;
  void* out; int32_t ld_out;
  void* pre; float* mean; float* rstd;
  int32_t B, heads, T, H, W, n_obj; /* input tokens N = 1 + T*H*W + n_obj               */
  int32_t stride_hw;               /* spatial stride s (temporal stride is 1)          */
  int32_t mode;                    /* 0 = plain (q, v), 1 = keys (+one-hot)            */
  float eps;
  float out_scale;                 /* columns 0..95 of out = LN(pooled) * out_scale (0 = 1): the keys
                                    * carry scale * log2(e) so that qa . ka^T is the score in the
                                    * log2 domain (svit_attn_fwd)                          */
  /* optional, the q tensor of the *_qkv entry points only (round 3; NULL = off): also write the rel-pos columns
   * out[:, 96 + j] = bf16(bf16(LN(q) . relq_R[relq_map[token, j]]) * relq_scale), 0 where the map is -1 --
   * what svit_gemm_nt with SVIT_EPI_RELQ does in a launch of its own.  relq_R bf16 [relq_lpad, 96] (the
   * concatenated tables, relq_lpad % 96 == 0), relq_map i32 [Nout, ld_out - 96].  The slab LayerNorm
   * kernel multiplies it on the matrix pipe from the rows it has just normalised; when the tensor takes
   * another path the entry point runs the GEMM itself, so the columns are written either way. */
  const void* relq_R; const int32_t* relq_map; int32_t relq_lpad; float relq_scale;
} svit_pool_args;
int svit_pool_ln_fwd(const svit_pool_args* a, void* stream);

/* backward, step 1: LayerNorm(96) backward per pooled token.
 * dout: up to three addends: d_main (bf16 or f32, row stride ld_main), d_res (bf16 ctx grad for
 * the residual-pooling path, rows [B, Nout, h*96], skipped for cls), d_extra (f32, or bf16 with extra_is_bf16, [..,96]).
 * writes dpre bf16 [B,h,Nout,96]; dgamma/dbeta accumulated (two-stage via workspace). */
typedef struct {
  const void* d_main; int32_t main_is_f32; int32_t ld_main;
  const void* d_res; const void* d_extra;
  const void* pre; const float* mean; const float* rstd; const float* gamma;
  void* dpre; float* dgamma; float* dbeta;
  int32_t B, heads, Nout;
  float* workspace; int64_t workspace_floats;   /* scratch for the two-stage dgamma/dbeta sum */
  int32_t main_parts; int64_t main_part_stride; /* f32 d_main only: sum of main_parts planes, main_part_stride
                                                 * floats apart (svit_attn_bwd's dk / dv); 0 / 1 = one plane */
  int32_t extra_is_bf16;                        /* d_extra holds bf16 (the rel-pos D . R^T GEMM's bf16 epilogue: half the bytes) */
} svit_pool_ln_bwd_args;
int svit_pool_ln_bwd(const svit_pool_ln_bwd_args* a, void* stream);
/* backward, step 2: depthwise-conv dgrad + cls/object rows -> dqkv bf16 [B,N,3,h,96] slice `which`;
 * step 3: depthwise-conv wgrad incl. the object-gain path; dw f32 [96,27] accumulated.
 * (argument blocks of svit_pool_conv_bwd_qkv below, one pair per tensor) */
typedef struct {
  const void* dpre; const float* conv_w; void* dqkv; int32_t which;
  int32_t B, heads, T, H, W, n_obj, stride_hw;
} svit_pool_dgrad_args;
typedef struct {
  const void* dpre; const void* qkv; int32_t which; float* dw;
  int32_t B, heads, T, H, W, n_obj, stride_hw;
  float* workspace; int64_t workspace_floats;
} svit_pool_wgrad_args;
/* The four pooling entry points for q, k and v of one block in ONE launch each (args[0..2] =
 * which 0, 1, 2; same qkv / B / heads / T / H / W / n_obj, individual strides and outputs).
 * This is what the engine calls: at the 14x14 and 7x7 stages each stencil is a short latency
 * chain, so three side by side cost the time of one (attention.py:263-304 runs them serially).
 * The two-stage reductions use args[0].workspace (>= 1024 * 3 * 27 * 96 floats for wgrad). */
int svit_pool_ln_fwd_qkv(const svit_pool_args* args3, void* stream);
/* Stride-1 stencils that keep their input in LDS.  svit_pool_weight_sel turns a list of depthwise weights
 * (fp32 [96][27] each, at src_base + src_off[i]) into "selector" tables dst[i][27][96] (uint32:
 * bf16(w) in the half of the dword that matches the channel's position in a packed bf16 pair); run
 * once per step for all blocks.  The *_sel entry point takes the three tables of a block.  Who reads
 * them: the SLAB forward (round 3; planes of <= 196 tokens, i.e. the 14x14 and 7x7 stages) fetches a
 * channel group's 27 x 24 entries as SCALAR operands (s_load) -- its stencil has no vector weight loads
 * at all; the LDS-tiled kernels of round 2 (56x56 planes; halo ring in LDS) build their own LDS weight
 * image from conv_w and only consult WHETHER a table is given.  Without tables every tensor runs the
 * streaming kernels. */
int svit_pool_weight_sel(const float* src_base, const int64_t* src_off, uint32_t* dst, int n_tables,
                         void* stream);
int svit_pool_ln_fwd_qkv_sel(const svit_pool_args* args3, const uint32_t* const* sel3, void* stream);
int svit_pool_ln_bwd_qkv(const svit_pool_ln_bwd_args* args3, void* stream);
#ifdef SVIT_DIAG_POOL_STREAMING
/* DIAGNOSTIC BUILD ONLY (round 6: csrc/pool.hip compiled with -DSVIT_DIAG_POOL_STREAMING, tools/diag/build_variant.py): the
 * streaming conv backward of rounds 1-4 -- gather-form dgrad and LDS-tiled wgrad, per tensor and for q, k, v in one launch
 * each.  The product library does not export them: svit_pool_conv_bwd_qkv takes every block of every configuration the suite
 * runs (tools/diag/pool_bwd_paths.py) and fails loudly where its plan does not fit. */
int svit_pool_conv_dgrad(const svit_pool_dgrad_args* a, void* stream);
int svit_pool_conv_wgrad(const svit_pool_wgrad_args* a, void* stream);
int svit_pool_conv_dgrad_qkv(const svit_pool_dgrad_args* args3, void* stream);
int svit_pool_conv_wgrad_qkv(const svit_pool_wgrad_args* args3, void* stream);
#endif
/* Steps 2 + 3 together (what the engine calls; round 5): conv dgrad AND conv wgrad of q, k, v in ONE launch for every
 * stride and plane of the model (csrc/pool.hip::pool_bwd_fused_kernel: a workgroup stages the dpre halo of its chunk of
 * planes / rows once in LDS and walks its input tokens once, producing dqkv and per-workgroup partial rows of the three dw
 * that the second-stage reduce sums in a fixed order).  Since round 6 the ONLY conv backward of the product library: where
 * not even one unit row of three padded planes fits LDS, the workspace is smaller than the plan's partial rows, or with
 * svit_debug_set_pool(1, 0), it returns SVIT_ERR_SHAPE (a diagnostic build falls through to the streaming launches).
 * dgrad3[i] / wgrad3[i] describe the same `which` = i (same dpre, stride, dims); wgrad3[0].workspace >=
 * B * heads * chunks * 3 * 27 * 96 floats. */
int svit_pool_conv_bwd_qkv(const svit_pool_dgrad_args* dgrad3, const svit_pool_wgrad_args* wgrad3,
                           void* stream);
/* floats of wgrad3[0].workspace that call needs for these tensors (B * heads * chunks of its plan * 3 * 27 * 96; grows with the
 * batch), -1 = the fused kernel has no plan for them, < -1 = error code.  Only the shape fields of dgrad3 are read. */
int64_t svit_pool_conv_bwd_workspace(const svit_pool_dgrad_args* dgrad3);

/* ------------------------------------------- decomposed rel-pos bias, query side (K9/K10) */
/* cal_rel_pos_spatial / cal_rel_pos_temporal (attention.py:84-183) restated as
 * relq[q, j] = q . R_j(q) with j over [k_h | k_w | k_t]; stored (divided by the softmax
 * scale) in columns 96.. of the augmented query so that the bias is added by the QK^T MFMA
 * against the one-hot key columns.  tables are f32 [rows,96] already resized to
 * 2*max(q,k)-1 rows; idx_* are int32 [q_n, k_n] row tables (dist.long()). */
typedef struct {
  void* qa; int32_t ld;           /* bf16 [B,h,Nq,ld]: reads cols 0..95, writes 96..96+J-1 */
  const float* rel_h; const float* rel_w; const float* rel_t;
  const int32_t* idx_h; const int32_t* idx_w; const int32_t* idx_t;
  int32_t B, heads, qt, qh, qw, kt, kh, kw, n_obj;
  float inv_scale;
} svit_relq_args;
int svit_relpos_q_fwd(const svit_relq_args* a, void* stream);
typedef struct {
  const void* qa; const void* dqa; int32_t ld;   /* bf16; dqa cols 96.. hold d(relq/scale)   */
  const float* rel_h; const float* rel_w; const float* rel_t;
  const int32_t* idx_h; const int32_t* idx_w; const int32_t* idx_t;
  float* dq_extra;                /* f32 [B,h,Nq,96] written (0 for cls/objects)          */
  float* drel_h; float* drel_w; float* drel_t; /* accumulated                           */
  int32_t rows_h, rows_w, rows_t;
  int32_t B, heads, qt, qh, qw, kt, kh, kw, n_obj;
  float inv_scale;
  float* workspace; int64_t workspace_floats;
} svit_relq_bwd_args;
int svit_relpos_q_bwd(const svit_relq_bwd_args* a, void* stream);
/* GEMM formulation of the forward (the one the engine uses): P[tokens, ldp] = q . Rcat^T with
 * svit_gemm_nt over the concatenated tables (rows row_h.., row_w.., row_t..), then this gather
 * writes qa[:, 96 + j] = P[token, row_x + idx] * inv_scale (zeros for cls / objects / j >= J). */
typedef struct {
  const void* P; int32_t ldp; void* qa; int32_t ld;
  const int32_t* idx_h; const int32_t* idx_w; const int32_t* idx_t;
  int32_t row_h, row_w, row_t;
  int32_t B, heads, qt, qh, qw, kt, kh, kw, n_obj;
  float inv_scale;
} svit_relq_gather_args;
int svit_relpos_gather(const svit_relq_gather_args* a, void* stream);
/* GEMM formulation of the same backward (the one the engine uses): D[tokens, ldd] (bf16,
 * zero-filled here) receives d(relq) at column off_{h,w,t} + idx; then
 * drel_x += D[:, sec_x]^T q (svit_gemm_tn) and dq_extra = D Rcat (svit_gemm_nt). */
typedef struct {
  const void* dqa; int32_t ld; void* D; int32_t ldd;
  const int32_t* idx_h; const int32_t* idx_w; const int32_t* idx_t;
  int32_t off_h, off_w, off_t;
  int32_t B, heads, qt, qh, qw, kt, kh, kw, n_obj;
  float inv_scale;
} svit_relq_scatter_args;
int svit_relpos_scatter(const svit_relq_scatter_args* a, void* stream);

/* ------------------------------------------------ fused pooled attention (K8-K12) ------ */
/* (q*scale)@k^T + rel-pos bias -> softmax -> @v -> + pooled q (all tokens but cls) ->
 * merge heads (attention.py:429-461).
 * qa bf16 [B,h,Nq,DA], ka bf16 [B,h,Nk,DA] (DA = 128 or 160), v bf16 [B,h,Nk,96],
 * ctx bf16 [B,Nq,h*96], lse2 f32 [B,h,Nq] (log2-domain log-sum-exp, saved for backward).
 * Operand convention (round 3): qa . ka^T IS the attention score in the log2 domain --
 *   ka[:, 0:96]  = scale * log2(e) * LN(pool(k))   (svit_pool_args.out_scale of the key tensor),
 *   ka[:, 96+j]  = one-hot key coordinates [y | kh + x | kh + kw + t],
 *   qa[:, 0:96]  = LN(pool(q)), qa[:, 96+j] = log2(e) * (q . R_j) (svit_relpos_gather's inv_scale
 *   = log2 e) -- so the kernels exponentiate with exp2 and no multiply.  `scale` is only used to
 *   express dk with respect to the UN-scaled pooled keys: dk = scale * sum_q P (dP - delta) q.
 * bias_cols: how many of the DA - 96 rel-pos columns carry data (kt + kh + kw); the kernel only
 * multiplies the 16-column k-steps that do.  0 = all of them. */
typedef struct {
  const void* qa; const void* ka; const void* v; void* ctx; float* lse2;
  int32_t B, heads, Nq, Nk, DA; float scale; int32_t bias_cols;
} svit_attn_fwd_args;
int svit_attn_fwd(const svit_attn_fwd_args* a, void* stream);
typedef struct {
  const void* qa; const void* ka; const void* v; const void* ctx; const void* dctx;
  const float* lse2; float* delta;  /* delta: f32 [B,h,2,Nq] scratch (-lse2/c and -rowsum(dO*O) planes) */
  void* dqa;                        /* bf16 [B,h,Nq,DA], every column written: dqa = ln 2 * dS ka over ALL DA columns of
                                     * ka, so the columns past 96 + bias_cols are zero exactly when ka carries
                                     * zeros there (as the pooling kernel writes them)   */
  float* dk; float* dv;             /* f32 [parts,B,h,Nk,96], OVERWRITTEN: parts = svit_attn_bwd_parts(args)
                                     * partial planes (one per chunk of the query range) whose SUM is the
                                     * gradient; svit_pool_ln_bwd adds them while it reads (main_parts) */
  int32_t B, heads, Nq, Nk, DA, q_splits; float scale;
  int32_t bias_cols;                /* as in svit_attn_fwd_args: kt + kh + kw, 0 = all DA - 96 */
  /* optional (round 3; NULL / 0 = off): the dq kernel also writes the scattered matrix of the rel-pos backward,
   * relD bf16 [B*h*Nq, relD_ld] = zeros except relD[row, relD_map[(row % Nq) * (DA - 96) + j]] =
   * bf16(dqa[row, 96 + j] * relD_scale) where the map is >= 0 -- what svit_relpos_scatter builds in a launch
   * of its own (bit-identical).  relD_ld % 8 == 0, relD_ld <= 544, relD 16-byte aligned. */
  void* relD; int32_t relD_ld; const int32_t* relD_map; float relD_scale;
  /* and, when relD_ld <= 128 (one 32-row pass), with relR bf16 [96, relD_ld] (the transposed concatenated tables)
   * the rel-pos backward's "dq = D R" GEMM is multiplied by the same kernel from the rows it builds:
   *   relX != NULL: dq_extra f32 [B*h*Nq, 96] = relD . relR^T is written there;
   *   relX == NULL ("fold"): the product is ADDED to dqa[:, 0:96] before it is rounded to bf16 -- dqa then is
   *   the whole gradient of the pooled q and svit_pool_ln_bwd needs no d_extra.
   * relR == NULL = off (the caller runs svit_gemm_nt on relD). */
  const void* relR; float* relX;
} svit_attn_bwd_args;
int svit_attn_bwd(const svit_attn_bwd_args* a, void* stream);
/* number of dk / dv planes svit_attn_bwd will write for these arguments (>= 1; only the shape fields,
 * DA and q_splits are read; q_splits > 0 asks for that many, the result is what is actually used);
 * negative = error code */
int svit_attn_bwd_parts(const svit_attn_bwd_args* a);

/* ---------------------------------------------------------- max-pool skip path (K7) ---- */
/* MaxPool3d((1,3,3),(1,2,2),(0,1,1)) on patch tokens, cls/objects copied
 * (attention.py:549-555,562-564). x f32 [B,N,C] -> y f32 [B,Nout,C]; idx uint8 (tap 0..8). */
int svit_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int T, int H, int W,
                     int n_obj, int C, void* stream);
int svit_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int T, int H, int W,
                     int n_obj, int C, void* stream);
/* the same with dx rounded to bf16 [B,N,C]: what the dim-change projection's backward consumes
 * (attention.py:520-523 under autocast), without the f32 round trip */
int svit_maxpool_bwd_bf16(const float* dy, const uint8_t* idx, void* dx_bf16, int B, int T, int H, int W,
                          int n_obj, int C, void* stream);

/* ------------------------------------------------------------- optimiser tail (K17) ---- */
/* clip_grad_norm_(1.0) + AdamW (tools/train_net.py:144-151, models/optimizer.py:102-108)
 * on flat f32 buffers.  sumsq is a device scalar (pre-zeroed). */
/* sumsq += sum(g^2), deterministic (two-stage through `workspace`, >= 1024 floats): replicas
 * of a data-parallel job must derive the bit-identical clip coefficient. */
int svit_sumsq(const float* g, int64_t n, float* sumsq, float* workspace,
               int64_t workspace_floats, void* stream);
int svit_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq,
                    float max_norm, float lr, float beta1, float beta2, float eps, float wd,
                    int step, float grad_scale, void* stream);

/* Guarded optimiser tail: the same clip + AdamW, but a step whose gradients hold an inf or a NaN is DROPPED on the
 * device, as GradScaler.step drops it (tools/train_net.py:134-151): weights, moments and AdamW's step counter stay as
 * they were.  Every scalar of the step lives in a step record in device memory, so the launches below are the same for
 * every step and can sit inside a captured graph.  The record has two parts in two SEPARATE buffers, so that an upload
 * never overwrites what the device owns.
 *
 * svit_step_host (32 bytes, 8-byte aligned): written by the host before every step, only read by kernels.
 *   offset  0  float lr[2]            learning rate of [0] the decayed range [0, n_decay), [1] the rest [n_decay, n)
 *   offset  8  float weight_decay[2]  weight decay of the same two groups
 *   offset 16  float max_norm         clip_grad_norm_ bound; <= 0: no norm clipping
 *   offset 20  float clip_value       clip_grad_value_ bound; > 0: g * grad_scale is clamped to +-clip_value element by
 *                                     element and norm clipping is OFF (the reference's precedence, train_net.py:139-147)
 *   offset 24  float grad_scale       factor applied to every gradient (1 / loss scale)
 *   offset 28  float reserved         0
 * svit_step_dev (48 bytes, 8-byte aligned): written only by kernels (the host zeroes it once, and may set `applied`
 * when it loads a checkpoint).
 *   offset  0  int64 applied          steps applied so far = AdamW's step counter
 *   offset  8  int64 skipped          steps dropped so far
 *   offset 16  int32 consecutive      steps dropped in a row, 0 after every applied step
 *   offset 20  int32 apply            this step: 1 applied, 0 dropped
 *   offset 24  float coef             this step's gradient coefficient (clip coefficient * grad_scale)
 *   offset 28  float bc1              this step's 1 - beta1^applied
 *   offset 32  float bc2_sqrt         this step's sqrt(1 - beta2^applied)
 *   offset 36  float sumsq            sum(g^2) of the last applied step
 *   offset 40  float grad_norm        sqrt(sumsq) * grad_scale of the last applied step: the last finite gradient norm
 *   offset 44  float reserved
 * A dropped step changes `skipped`, `consecutive` and `apply` and nothing else. */
typedef struct {
  float lr[2], weight_decay[2];
  float max_norm, clip_value, grad_scale, reserved;
} svit_step_host;
typedef struct {
  int64_t applied, skipped;
  int32_t consecutive, apply;
  float coef, bc1, bc2_sqrt, sumsq, grad_norm, reserved;
} svit_step_dev;

/* Per-tensor statistics of the flat gradient and weight buffers, taken INSIDE the step (svit_amd/monitor.py): two
 * launches between the guard and the solver's launch, so g and dev_rec are this step's and p still holds the weights the
 * gradient was taken at.  They write one row of a ring in device memory; the host reads the ring once per logging period.
 *
 * The ring is plain memory, R rows of 16 + 32 * Tn bytes, 16-byte aligned; the HOST writes all of it when it is created
 * and when it is reset (step = -1, n_bad = -1, first_bad = -1, everything else 0), the kernels write recorded rows.
 *   row header, 16 bytes
 *     offset  0  int64 step        the step the row holds, s below; -1: never written
 *     offset  8  int32 apply       dev_rec->apply of that step: 1 applied, 0 dropped
 *     offset 12  int32 reserved    0
 *   entry of tensor t at offset 16 + 32 * t, 32 bytes
 *     offset  0  double sumsq_g    sum of g^2 over the tensor's FINITE elements, accumulated in fp64
 *     offset  8  double sumsq_p    sum of p^2 over the tensor, accumulated in fp64
 *     offset 16  float absmax_g    largest |g| among the finite elements, 0 when there is none
 *     offset 20  int32 n_bad       number of non-finite elements of g (NaN, +inf, -inf); -1: the tensor is frozen and the
 *                                  entry has never been written
 *     offset 24  int32 first_bad   smallest in-tensor offset of a non-finite element of g, -1 when there is none
 *     offset 28  int32 reserved    0
 * A finite gradient whose fp32 sum of squares overflows (the guard then drops the step) still has a finite sumsq_g.
 *
 * The tensor table: int64 [Tn][2] of (begin, end) float positions, one row per tensor, 1 <= Tn <= 4096, ascending and
 * disjoint (begin >= the previous end), no empty tensor, fewer than 2^31 elements each, end <= n, every begin a multiple
 * of 4 (the flat layout aligns slots to 8 floats; an end may be anything).  What lies between two tensors is alignment
 * padding and is never counted.  svit_tensor_table_check, HOST ONLY (no stream, no launch), checks a table in host
 * memory: SVIT_ERR_ARG for a NULL table, Tn or n out of range, an unsorted, overlapping, empty or oversized tensor or an
 * end past n; SVIT_ERR_ALIGN for a begin that is not a multiple of 4.
 *
 * svit_tensor_stats: g, p f32 [n], 16-byte aligned.  table_dev is the table in DEVICE memory (405 pairs and more do not
 * fit the kernel arguments), written once by the caller; table_host is the same table in host memory, checked here by
 * svit_tensor_table_check before any HIP call and not kept.  segs / S: the optimizer's trainable segments IN HOST MEMORY
 * (svit_adamw_step_guarded_seg's table, its rules and error codes, carried in the kernel arguments); S == 0, segs then
 * ignored: the whole buffer.  A tensor whose begin lies in no segment is frozen: neither loaded nor written, its entry
 * keeps what the host wrote.  EXACTLY two launches, no allocation, copy or synchronisation: capturable.
 *   step index   s = dev_rec->applied + dev_rec->skipped - 1, read on the device from the record the guard in front has
 *                already advanced: no kernel here advances a counter that its own workgroups read.
 *   recorded     when s % every == 0 or dev_rec->apply == 0 (a dropped step is always recorded), into row s % R.
 *                Otherwise every workgroup of both launches returns before its first load of g or p and the ring is
 *                untouched.
 *   stage 1      one workgroup per window of svit_tensor_stats_window() = 4096 floats, 16-byte loads (issued first, for
 *                the quads inside a segment: segments hold whole tensors), then a workgroup-uniform walk of the table
 *                from the first tensor that ends past the window's begin (found by bisection) with a cursor that only
 *                moves forward.  Every (window, tensor) piece leaves ONE 32-byte partial in `workspace`
 *                at slot window + tensor, which no other piece shares; svit_tensor_stats_workspace(n, Tn), HOST ONLY,
 *                returns the bytes of the ceil(n / 4096) + Tn slots (SVIT_ERR_ARG, negative, for n or Tn out of range).
 *   stage 2      one wave per tensor: lane l adds the partials of the tensor's windows l, l + 64, ... in ascending
 *                order, the 64 lanes combine in a fixed butterfly, lane 0 writes the entry; the wave of tensor 0 also
 *                writes the header.
 * An element of g is non-finite when its exponent bits are all ones; such an element enters neither sumsq_g nor absmax_g.
 * The maximum is taken on the integer image of |g|.  (double) x * (double) x is exact, only the fp64 additions round:
 * against svit_amd/monitor.py stats_host both sums of squares agree to 2^-30 relative, everything else exactly.  No
 * atomics and no ticket: the row is bit-identical from run to run and from the eager step to a replay.
 * SVIT_ERR_ARG besides the tables': a NULL g, p, table_dev, dev_rec, ring or workspace; R < 1; every < 1; workspace_bytes
 * below svit_tensor_stats_workspace(n, Tn).  SVIT_ERR_ALIGN: g, p, ring or workspace not 16-byte aligned, table_dev or
 * dev_rec not 8-byte aligned.  All checked before any HIP call.  The ring's size is the caller's to get right. */
int svit_tensor_stats_window(void);
int svit_tensor_table_check(const int64_t* table, int64_t Tn, int64_t n);
int64_t svit_tensor_stats_workspace(int64_t n, int64_t Tn);
int svit_tensor_stats(const float* g, const float* p, int64_t n, const int64_t* table_dev, const int64_t* table_host,
                      int64_t Tn, const int64_t* segs, int64_t S, const svit_step_dev* dev_rec, void* ring, int64_t R,
                      int64_t every, void* workspace, int64_t workspace_bytes, void* stream);

/* What the solver did to every tensor, measured INSIDE the step (svit_amd/updmon.py): one launch in front of the solver's
 * launch copies the weights into a shadow buffer, two launches behind it compare the weights with the shadow.  No update
 * rule is restated: the numbers are those of whatever solver ran in between.  All three launches read the guard's record,
 * which no solver kernel writes, and so agree on whether the step is due:
 *   step index   s = dev_rec->applied + dev_rec->skipped - 1, svit_tensor_stats' index: rows of both rings join by step.
 *   due          when dev_rec->apply == 1 and s % every == 0 (a dropped step moves nothing and is never recorded).
 *                Otherwise every workgroup of the three launches returns before its first load; shadow, workspace and
 *                ring keep their bytes.
 *
 * svit_update_snapshot: p, shadow f32 [n], 16-byte aligned.  ONE launch.  On a due step shadow = p over the trainable
 * segments, 16 bytes at a time; segs / S: svit_adamw_step_guarded_seg's table IN HOST MEMORY with its rules and error
 * codes, carried in the kernel arguments and walked with a workgroup-uniform cursor that only moves forward; S == 0, segs
 * then ignored: the whole buffer (its last n % 4 elements one by one).  Nothing outside the segments is read or written.
 * SVIT_ERR_ARG besides the table's: a NULL p, shadow or dev_rec, n <= 0, every < 1.  SVIT_ERR_ALIGN: p or shadow not
 * 16-byte aligned, dev_rec not 8-byte aligned.
 *
 * svit_update_stats: p (the weights behind the solver), shadow (the weights in front of it), g f32 [n]; m, v f32 [n] or
 * NULL (SGD: its momentum buffer or NULL for m, NULL for v), all 16-byte aligned.  table_dev / table_host / Tn: the
 * tensor table of svit_tensor_stats, checked by svit_tensor_table_check; segs / S as above, segments hold whole tensors.
 * A tensor whose begin lies in no segment is frozen: neither loaded nor written, its entry keeps what the host wrote.
 * EXACTLY two launches, no atomics, no ticket, no allocation, copy or synchronisation: capturable, and a row is
 * bit-identical from run to run and from the eager step to a replay.
 *   stage 1      one workgroup per window of svit_tensor_stats_window() = 4096 floats, loads issued first, then the
 *                bisection and the forward-only walk of svit_tensor_stats; ONE 64-byte partial per (window, tensor) piece
 *                at slot window + tensor.  svit_update_stats_workspace(n, Tn), HOST ONLY, returns the bytes of the
 *                ceil(n / 4096) + Tn slots (SVIT_ERR_ARG, negative, for n or Tn out of range).
 *   stage 2      one wave per tensor: lane l adds the partials of the tensor's windows l, l + 64, ... in ascending
 *                order, the 64 lanes combine in a fixed butterfly, lane 0 writes the entry; the wave of tensor 0 also
 *                writes the header.
 * The ring: R rows of 16 + 64 * Tn bytes, 16-byte aligned; the HOST writes all of it when it is created and when it is
 * reset (step = -1, n_still = -1, everything else 0), the kernels write the rows of due steps, row s % R.
 *   row header, 16 bytes
 *     offset  0  int64 step        the step the row holds; -1: never written
 *     offset  8  int32 flags       bit 0: m was present, bit 1: v was present
 *     offset 12  int32 reserved    0
 *   entry of tensor t at offset 16 + 64 * t, 64 bytes, with Delta = (double) p_new - (double) p_old per element
 *     offset  0  double sumsq_d    sum of Delta^2
 *     offset  8  double sumsq_p    sum of p_new^2
 *     offset 16  double dot_dg     sum of Delta * g, signed
 *     offset 24  double sumsq_g    sum of g^2
 *     offset 32  double sumsq_m    sum of m^2; 0 without m
 *     offset 40  double sum_v      sum of v; 0 without v
 *     offset 48  float absmax_d    largest (float) |Delta|, the maximum taken on the integer image
 *     offset 52  int32 n_still     elements whose 32 bits did not change; -1: the tensor is frozen and the entry has
 *                                  never been written
 *     offset 56  int32 n_one_ulp   elements that moved to an adjacent float: |key(new) - key(old)| == 1 in int64, with
 *                                  key(i) = i ^ ((i >> 31) & 0x7fffffff) on the signed 32-bit image (+0.0 -> -0.0 is one)
 *     offset 60  int32 reserved    0
 * The counts compare integer images, never floats.  A due step was applied, so g is finite inside the segments.
 * Non-finite p, m or v are NOT filtered: the sums, the maximum and n_one_ulp of such a tensor are unspecified; no address
 * outside the buffers is touched for any input.  Against svit_amd/updmon.py update_host: Delta is one IEEE subtraction on
 * both sides; a product may be fused into the following addition here (2^-53 relative per term); either side sums at
 * most 2^22 terms per tensor: each of the six sums agrees within 2^-29 * sum |term|, everything else exactly.
 * SVIT_ERR_ARG besides the tables': a NULL p, shadow, g, table_dev, dev_rec, ring or workspace; R < 1; every < 1;
 * workspace_bytes below svit_update_stats_workspace(n, Tn).  SVIT_ERR_ALIGN: p, shadow, g, m, v, ring or workspace not
 * 16-byte aligned, table_dev or dev_rec not 8-byte aligned.  All checked before any HIP call.  The ring's size is the
 * caller's to get right. */
int svit_update_snapshot(const float* p, float* shadow, int64_t n, const int64_t* segs, int64_t S,
                         const svit_step_dev* dev_rec, int64_t every, void* stream);
int64_t svit_update_stats_workspace(int64_t n, int64_t Tn);
int svit_update_stats(const float* p, const float* shadow, const float* g, const float* m, const float* v, int64_t n,
                      const int64_t* table_dev, const int64_t* table_host, int64_t Tn, const int64_t* segs, int64_t S,
                      const svit_step_dev* dev_rec, void* ring, int64_t R, int64_t every, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Per-block FORWARD statistics, read from what a training forward keeps for its backward and never from the activations
 * (svit_amd/actmon.py): the per-row LayerNorm statistics in front of each block's attention branch, in front of its MLP
 * and in front of the final norm, and the attention's log-sum-exp (log2 domain) per (sample, head, query).
 * svit_layernorm_fwd forms `mean` as a plain sum and `rstd` from the two-pass variance without a clamp, so a non-finite
 * element of a row shows in that row's mean or rstd, and for a finite row mean^2 + 1 / rstd^2 - eps is its mean square.
 * Two launches at the end of a saving forward write one row of a ring in device memory.
 *
 * A site: one array pair (LayerNorm: a = mean, b = rstd, f32 [rows]) or one array (lse: a = lse2, b = NULL), 4-byte
 * aligned, 1 <= rows <= 2^24.  `first_window` is filled in by the library in its own copy; the caller's value is
 * ignored.  The table and `slots` (int32 [n_sites]: the ring slot of each site) are HOST memory and travel in the kernel
 * arguments, so an eager pass may name fresh arrays every time and a capture bakes its pool's addresses:
 * 1 <= n_sites <= SVIT_ACT_MAX_SITES, 1 <= n_slots <= 1024, slots distinct and inside [0, n_slots).
 *
 * The ring: R rows of SVIT_ACT_HEADER_BYTES + 32 * n_slots bytes, 16-byte aligned; the HOST writes all of it when it is
 * created or reset (pass = -1, step = -1, arg = n_bad = first_bad = -1, everything else 0).
 *   row header, 48 bytes
 *     offset  0  int64 pass        the counter's value when the row was written, from 0; -1: never written
 *     offset  8  int64 step        dev_rec->applied + dev_rec->skipped: the index of the optimizer step this pass feeds
 *                                  (what svit_tensor_stats rows carry); -1 without a dev_rec
 *     offset 16  int32 B, Tx, T0, H0, W0   the pass's geometry, copied from `geom` (host, int32 [5]): batch, frames of the
 *                                  clip, and the token grid in front of block 0 -- what unravels a row index
 *     offset 36  int32 n_sites     sites of this pass
 *     offset 40  int32 reserved[2] 0
 *   entry of slot k at offset 48 + 32 * k, 32 bytes
 *     offset  0  double sum        LayerNorm: sum over the good rows of (double) mean * mean + 1 / ((double) rstd * rstd),
 *                                  each term within 2^-40 relative; lse: sum of (double) lse2 over the good rows
 *     offset  8  float ext         LayerNorm: the smallest rstd (the widest token); lse: the largest value
 *     offset 12  float ext2        LayerNorm: the largest |mean|; lse: 0
 *     offset 16  int32 arg         the row of `ext`, the smallest such row among ties
 *     offset 20  int32 n_bad       bad rows; -1: no site of this pass named the slot (the rest of the entry is then the
 *                                  empty entry: zeros, arg = first_bad = -1)
 *     offset 24  int32 first_bad   smallest bad row, -1 when there is none
 *     offset 28  int32 rows        the site's rows
 * A LayerNorm row is bad when mean or rstd has all exponent bits set or rstd is zero or negative (sign bit set); an lse
 * row when its exponent bits are all set.  Bad rows enter neither the sum nor the extrema; with no good row
 * ext = ext2 = 0 and arg = -1.  Extrema are taken on integer keys monotone in the float order (-0.0 below +0.0).
 *
 *   stage 1   one workgroup of 256 threads per window of svit_act_stats_window() = 4096 rows of ONE site (found by
 *             bisection over first_window in the arguments, workgroup-uniform); loads first, then a fixed-order
 *             reduction; ONE 32-byte partial at slot `window` of the workspace.  svit_act_stats_workspace(windows),
 *             HOST ONLY, returns the bytes (SVIT_ERR_ARG, negative, for windows < 1 or above 96 * 4096).
 *   stage 2   ONE workgroup: folds every site's partials in window order, writes the entries and the empty entries of
 *             ring row (pass % R) and the header, then advances the pass counter state[0] (int64, device memory, zeroed
 *             by the host) -- svit_meter_push's contract: one workgroup reads it at entry and writes it at exit; stage 1
 *             never reads it.
 * EXACTLY two launches; no float atomics, no ticket, no allocation, copy or synchronisation: capturable, and a row is
 * bit-identical from run to run and from the eager pass to a replay.  Nothing but the ring row, the workspace and state
 * is written.  Against svit_amd/actmon.py acts_host: |sum - host| <= 2^-27 * sum |term| (a site sums at most 2^24 terms
 * on either side, each sum within 2^-29 of sum |term|, each term within 2^-40); everything else exactly.
 *
 * svit_act_sites_check, HOST ONLY, and svit_act_stats before any HIP call: SVIT_ERR_ARG for a NULL table / slots,
 * n_sites or n_slots out of range, a NULL `a`, rows outside 1..2^24, a slot outside [0, n_slots) or named twice;
 * SVIT_ERR_ALIGN for an `a` or `b` not 4-byte aligned; *total_windows (may be NULL) receives the windows of the table.
 * svit_act_stats besides: SVIT_ERR_ARG for a NULL geom, ring, state or workspace, R < 1, workspace_bytes below
 * svit_act_stats_workspace(windows); SVIT_ERR_ALIGN for a ring or workspace not 16-byte aligned, state or dev_rec not
 * 8-byte aligned.  dev_rec may be NULL.  The ring's size is the caller's to get right. */
#define SVIT_ACT_MAX_SITES 96
#define SVIT_ACT_HEADER_BYTES 48
typedef struct {
  const float* a;
  const float* b;
  int32_t rows, first_window;
} svit_act_site;
int svit_act_stats_window(void);
int64_t svit_act_stats_workspace(int64_t total_windows);
int svit_act_sites_check(const svit_act_site* sites, const int32_t* slots, int64_t n_sites, int64_t n_slots,
                         int64_t* total_windows);
int svit_act_stats(const svit_act_site* sites, const int32_t* slots, int64_t n_sites, int64_t n_slots,
                   const int32_t* geom, const svit_step_dev* dev_rec, void* ring, int64_t R, int64_t* state,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* Per-head ATTENTION statistics of chosen query rows, from the operands a saving forward keeps for its backward
 * (svit_amd/attnmon.py): by the operand convention of svit_attn_fwd, qa . ka^T over columns [0, 96 + J) is the score in
 * the log2 domain with the relative-position bias folded in, so
 *     p[q, k] = exp2( sum_j qa[q, j] * ka[k, j] - lse2[q] )
 * and no table, index map or interpolation is restated.  Two launches at the end of a saving forward write one row of a
 * ring in device memory; the attention kernels are not touched.
 *
 * A site (one kept block; HOST memory, the table travels in the kernel arguments, 1 <= n_sites <= SVIT_ATTN_MAX_SITES):
 *   qa bf16 [B,heads,Nq,DA], ka bf16 [B,heads,Nk,DA] (16-byte aligned), lse2 f32 [B,heads,Nq] (4-byte aligned),
 *   maps f32 [maps_samples,heads,n_probe,Nk] or NULL (4-byte aligned); DA = 128 or 160; bias_cols = J, 0 = all DA - 96;
 *   Lq / Lk: the patch tokens of the query / key grid, n_obj the object tokens: Nq = 1 + Lq + n_obj, Nk = 1 + Lk + n_obj
 *   (token 0 is cls, tokens 1 .. L the patches, the rest the objects); slot: the site's ring slot, distinct, inside
 *   [0, n_slots); ent_base: its first entry in a ring row -- it owns entries ent_base + head * n_groups + group, inside
 *   [0, ent_slots), shared with no other site; first_wg is filled in by the library in its own copy.
 * The probe (HOST memory): 1 <= n_groups <= 3 query groups of distinct kinds, in entry order --
 *   SVIT_ATTN_CLS    row 0;
 *   SVIT_ATTN_OBJ    rows 1 + Lq .. Nq - 1 (none when n_obj = 0);
 *   SVIT_ATTN_PATCH  rows 1 + ((2 i + 1) * Lq) / (2 K) for i < K, integer division, or all Lq patch rows when Lq <= K
 *                    (1 <= K <= 256);
 * n_probe of a site is the sum of its groups' rows, and a map holds them in that order.  every >= 1; maps_samples >= 0
 * (samples past B are not stored).
 *
 * Per probe row: s_k = sum over columns j < 96 + J of qa[q, j] * ka[k, j], accumulated in fp32 in column order over
 * products that are exact (bf16 x bf16); d_k = s_k - lse2[q] in fp32; p_k = exp2(d_k) by the hardware's fp32 exp2
 * (results below 2^-126 may be flushed to zero).  Columns >= 96 + J are never multiplied: what they hold, NaN included,
 * changes nothing.  In fp64: sum_p = sum_k p_k, H = - sum_k p_k d_k (bits), m_cls = p_0, m_obj = sum_{k > Lk} p_k, and
 * pmax = max_k p_k.  A row is BAD when lse2[q] or any s_k has all exponent bits set (integer images, never a float
 * compare); bad rows enter no sum, and their map rows hold no meaning.
 *
 * The ring: R rows of SVIT_ATTN_HEADER_BYTES + 64 * ent_slots bytes, 16-byte aligned; the HOST writes all of it when it
 * is created or reset (pass = step = -1, every entry the empty entry).
 *   row header, 48 bytes
 *     offset  0  int64 pass        the pass counter's value when the row was written, from 0; -1: never written
 *     offset  8  int64 step        dev_rec->applied + dev_rec->skipped, the optimizer step this pass feeds; -1 without
 *     offset 16  int32 B, Tx, T0, H0, W0, n_sites   as svit_act_stats' header
 *     offset 40  int32 row         the rows-written counter's value when the row was written (it lies at row % R)
 *     offset 44  int32 reserved    0
 *   entry e at offset 48 + 64 * e, 64 bytes: the good probe rows of one (slot, head, group) over all samples
 *     offset  0  double sum_H, sum_pmax, sum_cls, sum_obj, sum_p   sums of H, pmax, m_cls, m_obj and sum_p
 *     offset 40  float  min_H      the smallest (float) H; 0 when there is no good row
 *     offset 44  int32  min_row    its row code b * Nq + q, the smallest code among ties; -1 when there is none
 *     offset 48  float  sum_dev    the largest (float) |sum_p - 1|: how far the probe's sum lies from svit_attn_fwd's lse2
 *     offset 52  int32  rows       probe rows, good and bad
 *     offset 56  int32  n_bad      bad rows; -1: no site of this pass owns the entry (the rest is then the empty entry:
 *                                  zeros, min_row = first_bad = -1)
 *     offset 60  int32  first_bad  the smallest row code b * Nq + q among the bad rows, -1 when there is none
 * state: int64 [4] in device memory, written by the host when it is created or reset: [0] passes so far (0), [1] rows
 * written so far (0), [2] the pass whose probabilities the maps hold (-1: none yet), [3] reserved (0).
 *
 * A pass is DUE when (dev_rec->applied + dev_rec->skipped) % every == 0, read on the device; without a dev_rec when
 * pass % every == 0.
 *   stage 1   one workgroup of 256 threads per (site, sample, head, group), found by bisection over first_wg in the
 *             arguments (workgroup-uniform; the library's copy of the table is ordered by falling Nk * DA, ties in table
 *             order, so that the long workgroups start first -- entries and slots do not depend on it); rows over its 4
 *             waves, keys over lanes, 64 keys at a time staged in LDS; a fixed-order reduction and ONE 64-byte partial
 *             at slot `workgroup` of the workspace; with a map pointer and sample < maps_samples also the
 *             probabilities of its rows.  With a dev_rec whose step is not due it returns before any load of qa, ka or
 *             lse2.  It never reads `state`: WITHOUT a dev_rec it therefore works on every pass, and `every` then only
 *             thins the ring.  svit_attn_stats_workspace(workgroups), HOST ONLY, returns the bytes (SVIT_ERR_ARG,
 *             negative, for workgroups < 1 or above 2^20).
 *   stage 2   ONE workgroup under svit_meter_push's contract for the counters: due -- folds the partials of every entry
 *             in sample order, writes the entries, the empty entries and the header of ring row state[1] % R, sets
 *             state[2] = pass when a site has a map and advances state[1]; always -- advances state[0] (without a
 *             dev_rec, a pass that is not due still sets state[2], since stage 1 stored its maps).
 * EXACTLY two launches; no atomics, no ticket, no allocation, copy or synchronisation: capturable, and a row is
 * bit-identical from run to run and from the eager pass to a replay.  Nothing but the ring row, the workspace, the maps
 * and state is written.
 *
 * svit_attn_sites_check, HOST ONLY, and svit_attn_stats before any HIP call: SVIT_ERR_ARG for a NULL table or probe,
 * n_sites, n_slots (1 .. 1024) or ent_slots (1 .. 1024) out of range, a probe with no or more than 3 groups, an unknown
 * or repeated kind, K outside 1 .. 256, every < 1 or maps_samples < 0; per site a NULL qa, ka or lse2, B, heads, Lq or
 * Lk < 1, n_obj < 0, DA not 128 or 160, bias_cols outside [0, DA - 96], 1 + Lq + n_obj != Nq, 1 + Lk + n_obj != Nk,
 * B * heads * max(Nq, Nk) above 2^31 - 1, a slot outside [0, n_slots) or named twice, entries outside [0, ent_slots) or
 * owned twice; SVIT_ERR_ALIGN for a qa or ka not 16-byte or an lse2 or maps not 4-byte aligned.  *total_wgs (may be
 * NULL) receives the workgroups of stage 1.  svit_attn_stats besides: SVIT_ERR_ARG for a NULL geom, ring, state or
 * workspace, R < 1, workspace_bytes below svit_attn_stats_workspace(workgroups); SVIT_ERR_ALIGN for a ring or workspace
 * not 16-byte aligned, state or dev_rec not 8-byte aligned.  dev_rec may be NULL.  The sizes of the ring and of the maps
 * are the caller's to get right. */
#define SVIT_ATTN_MAX_SITES 32
#define SVIT_ATTN_HEADER_BYTES 48
#define SVIT_ATTN_ENTRY_BYTES 64
#define SVIT_ATTN_CLS 0
#define SVIT_ATTN_OBJ 1
#define SVIT_ATTN_PATCH 2
typedef struct {
  const void* qa; const void* ka; const float* lse2; float* maps;
  int32_t B, heads, Nq, Nk, DA, bias_cols, Lq, Lk, n_obj, slot, ent_base, first_wg;
} svit_attn_site;
typedef struct {
  int32_t n_groups, kind[3], K, every, maps_samples, reserved;
} svit_attn_probe;
int64_t svit_attn_stats_workspace(int64_t total_wgs);
int svit_attn_sites_check(const svit_attn_site* sites, int64_t n_sites, int64_t n_slots, int64_t ent_slots,
                          const svit_attn_probe* probe, int64_t* total_wgs);
int svit_attn_stats(const svit_attn_site* sites, int64_t n_sites, int64_t n_slots, int64_t ent_slots,
                    const svit_attn_probe* probe, const int32_t* geom, const svit_step_dev* dev_rec, void* ring,
                    int64_t R, int64_t* state, void* workspace, int64_t workspace_bytes, void* stream);

/* HOST ONLY (no stream, no launch): the bias corrections svit_adamw_step derives from its `step` argument, by the very
 * same host code: pair k-1 = (1 - powf(beta1, k), sqrtf(1 - powf(beta2, k))) for steps k = 1, 2, ... up to and including
 * the first step at which both values are exactly 1.0f; past the table both are 1.0f.  *n_entries receives that length
 * (17321 pairs for betas (0.9, 0.999)).  table (2 floats per pair, room for `capacity` pairs) may be NULL to ask for the
 * length alone.  SVIT_ERR_ARG: n_entries NULL, a table shorter than the length, or a length above 2^20 (betas that
 * never reach 1.0f, or not below 1, included).  The device never calls pow: the guard looks the pair up. */
int svit_adamw_bias_table(float beta1, float beta2, float* table, int64_t capacity, int64_t* n_entries);

/* The guard: svit_sumsq's two-stage deterministic sum of squares (same kernel, same partial layout through `workspace`,
 * >= 1 float, 1024 for the full grid) whose final one-wave stage also takes the step's decision:
 *   total = sqrtf(sumsq) * grad_scale;  apply = isfinite(total)
 *   apply: applied += 1, consecutive = 0, coef = svit_adamw_step's coefficient (grad_scale * min(max_norm / (total + 1e-6),
 *          1) when max_norm > 0 and clip_value <= 0, grad_scale otherwise), (bc1, bc2_sqrt) = pair `applied` of
 *          bias_table (1.0f past its `table_entries` pairs), sumsq and grad_norm recorded;
 *   drop:  skipped += 1, consecutive += 1.
 * A step of finite gradients whose sum of squares overflows fp32 (a norm above ~1.8e19) counts as non-finite and is
 * dropped.  The guard runs with norm clipping off too: it is what detects the non-finite step.  Two launches, no
 * allocation, copy or synchronisation: capturable.  records not 8-byte aligned: SVIT_ERR_ALIGN. */
int svit_step_guard(const float* g, int64_t n, const svit_step_host* host_rec, svit_step_dev* dev_rec,
                    const float* bias_table, int64_t table_entries, float* workspace, int64_t workspace_floats,
                    void* stream);
/* svit_adamw_step's arithmetic in the same order on p, g, m, v f32 [n] (16-byte aligned, else SVIT_ERR_ALIGN), every
 * scalar read from the step record the guard left: ONE launch for both weight-decay groups ([0, n_decay) takes lr[0] /
 * weight_decay[0], [n_decay, n) takes [1]; 0 <= n_decay <= n), 16-byte accesses with a scalar tail for n % 4.  On a
 * dropped step (apply == 0) every workgroup returns before its first load of p, g, m or v. */
int svit_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                            const svit_step_host* host_rec, const svit_step_dev* dev_rec, float beta1, float beta2,
                            float eps, void* stream);

/* The guarded tail over the TRAINABLE part of the flat buffers (parameters with requires_grad = False are frozen:
 * never read, never written, not counted in the norm).  The trainable set is a segment table: `segs` = int64 [S][2] of
 * (begin, end) float indices IN HOST MEMORY, 1 <= S <= SVIT_MAX_SEGS, ascending and disjoint (begin >= the previous
 * end), no empty segment, end <= n, every bound a multiple of 4 (the flat layout aligns slots to 8 floats).  The table
 * is checked on the host before any HIP call and travels to the device inside the kernel arguments (1 KB, read by
 * scalar loads at workgroup-uniform indices; a captured graph keeps its copy), so the caller may free it after the call.
 * SVIT_ERR_ARG: S out of range, NULL table, an unsorted, overlapping or empty segment, end > n, and for the AdamW entry
 * point a segment that straddles n_decay; SVIT_ERR_ALIGN: a bound not a multiple of 4, g / p / m / v not 16-byte aligned.
 *
 * svit_step_guard_seg: svit_step_guard over the segments.  Elements keep svit_sumsq's assignment to partial sums by
 * absolute position; one outside every segment contributes 0 and is not loaded.  The record it leaves is therefore bit
 * for bit svit_step_guard's on a buffer whose other ranges hold zeros (data-parallel replicas keep deriving the same
 * coefficient), and a NaN or inf outside the segments does not drop the step.
 * svit_adamw_step_guarded_seg: svit_adamw_step_guarded's arithmetic in its order on the elements inside a segment, ONE
 * launch; no load or store of p, g, m or v outside the segments; returns early on a dropped step. */
#define SVIT_MAX_SEGS 64
int svit_step_guard_seg(const float* g, int64_t n, const int64_t* segs, int64_t S, const svit_step_host* host_rec,
                        svit_step_dev* dev_rec, const float* bias_table, int64_t table_entries, float* workspace,
                        int64_t workspace_floats, void* stream);
int svit_adamw_step_guarded_seg(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                                const int64_t* segs, int64_t S, const svit_step_host* host_rec,
                                const svit_step_dev* dev_rec, float beta1, float beta2, float eps, void* stream);

/* svit_adamw_step_guarded_seg with a learning-rate scale per segment (layer-wise lr decay, per-range multipliers):
 * `scales` = float [S] IN HOST MEMORY beside `segs`, every scale finite and > 0 (else SVIT_ERR_ARG).  Both are checked
 * on the host before any HIP call -- the table by svit_adamw_step_guarded_seg's rules, with its error codes -- and travel
 * in the kernel arguments (1.3 KB; a captured graph keeps its copy).  An element of segment s in weight-decay group w is
 * stepped with lr_eff = lr[w] * scales[s], ONE fp32 multiply on the device, in every place svit_adamw_step_guarded uses
 * lr[w] (the decay factor 1 - lr_eff * weight_decay[w] and the step lr_eff / bc1); the coefficient, the bias corrections
 * and the guard's decision are not scaled.  The results are bit for bit those of svit_adamw_step_guarded_seg run over
 * the segments of one scale with a record that holds the premultiplied lr_eff.  Segments that touch (begin == the
 * previous end) and several segments inside one 1024-float window are the normal case.  The guard in front of it is
 * svit_step_guard, or svit_step_guard_seg when part of the buffer is frozen.  ONE launch; no load or store of p, g, m
 * or v outside the segments; returns early on a dropped step. */
int svit_adamw_step_guarded_lr(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                               const int64_t* segs, const float* scales, int64_t S, const svit_step_host* host_rec,
                               const svit_step_dev* dev_rec, float beta1, float beta2, float eps, void* stream);

/* The reference's other two solvers (slowfast/models/optimizer.py:86-101: torch.optim.SGD, torch.optim.Adam) on the
 * guarded tail: the guard in front is svit_step_guard / svit_step_guard_seg, unchanged, and the record it leaves is
 * read here as svit_adamw_step_guarded_lr reads it.  `segs` / `scales` / S are that entry point's tables IN HOST MEMORY,
 * checked on the host before any HIP call by its rules and with its error codes, and carried in the kernel arguments;
 * scales == NULL: every scale is 1.0.  An element of range s in weight-decay group w has lr_eff = lr[w] * scales[s] (ONE
 * fp32 multiply) and wd = weight_decay[w].  ONE launch; 16-byte accesses; no load or store outside the ranges; every
 * workgroup returns before its first load on a dropped step.  Every fp32 operation is rounded once, in the order
 * written (no contraction, correctly rounded sqrtf and divisions): the results equal the NumPy float32 restatements
 * svit_amd/optim.py sgd_step_host / adam_step_host bit for bit.  With gi = g * coef, clamped to +-clip_value when
 * clip_value > 0, then gi = gi + p * wd when wd != 0 (coupled L2):
 *
 * svit_sgd_step_guarded, p, g, buf f32 [n]:
 *     if momentum != 0:  buf = first ? gi : buf * momentum + gi * (1 - dampening)
 *                        gi  = nesterov ? gi + buf * momentum : buf
 *     p = p - gi * lr_eff
 *   `first` is dev_rec->applied == 1, read on the device: the first APPLIED step copies gi into the buffer, as
 *   torch.optim.SGD does for a momentum_buffer of None (a dropped step does not advance `applied`).  1 - dampening is
 *   formed once on the host in fp32.  With momentum == 0 buf may be NULL and is never touched (12 B per parameter
 *   against 20).  The guard takes a bias table of 0 entries.  SVIT_ERR_ARG besides the tables': nesterov != 0 with
 *   momentum <= 0 or dampening != 0; momentum != 0 with buf == NULL.
 * svit_adam_step_guarded, p, g, m, v f32 [n] (28 B per parameter):
 *     m = m * beta1 + gi * (1 - beta1);  v = v * beta2 + (gi * gi) * (1 - beta2)
 *     p = p - (lr_eff / bc1) * (m / (sqrtf(v) / bc2_sqrt + eps))
 *   with (bc1, bc2_sqrt) the pair the guard looked up in svit_adamw_bias_table(beta1, beta2). */
int svit_sgd_step_guarded(float* p, const float* g, float* buf, int64_t n, int64_t n_decay, const int64_t* segs,
                          const float* scales, int64_t S, const svit_step_host* host_rec, const svit_step_dev* dev_rec,
                          float momentum, float dampening, int nesterov, void* stream);
int svit_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_decay,
                           const int64_t* segs, const float* scales, int64_t S, const svit_step_host* host_rec,
                           const svit_step_dev* dev_rec, float beta1, float beta2, float eps, void* stream);

/* Exponential moving average of the weights behind a guarded solver (timm's ModelEma, in the captured step): ema, p f32
 * [n], 16-byte aligned (else SVIT_ERR_ALIGN),
 *     ema = ema * d + p * (1 - d)
 * on the elements inside the ranges of `segs` (the table of svit_adamw_step_guarded_seg IN HOST MEMORY, checked on the
 * host before any HIP call by its rules and with its error codes -- there is no weight-decay boundary here -- and
 * carried in the kernel arguments).  ONE launch on svit_sgd_step_guarded's walk; 16-byte accesses; no load or store of
 * ema or p outside the ranges; every workgroup returns before its first load of p or ema when dev_rec->apply == 0, so
 * a dropped step leaves the average bit for bit as it was.  Nothing but ema is written: no counter, no record.
 *   update number  k = max(dev_rec->applied + ema_rec[0], 1), read on the device.  `ema_rec` = int64 [2] in device memory,
 *                  {offset, reserved}, 8-byte aligned, written by the host alone (when the average is created, reset or
 *                  loaded from a checkpoint): the count is DERIVED from the guard's counter, which the guard in front
 *                  has already advanced, so no workgroup advances anything another reads; the offset keeps the count
 *                  across a resume of a solver that does not checkpoint `applied`.
 *   decay          d = k <= table_entries ? decay_table[k - 1] : decay.  decay_table = float [table_entries] in device
 *                  memory (svit_ema_decay_table's warm-up), NULL with 0 entries for a constant decay; `decay` travels as
 *                  a kernel argument and is fixed for the life of a captured graph.
 *   arithmetic     1 - d, e * d, p * (1 - d) and their sum are each rounded once, in that order, whatever the build's
 *                  floating-point flags: the result equals svit_amd/ema.py ema_step_host bit for bit.
 * SVIT_ERR_ARG besides the table's: decay not in (0, 1); table_entries < 0 or above 2^20; a NULL table with entries > 0;
 * a NULL ema, p, ema_rec or dev_rec.  All checked before any HIP call.
 *
 * svit_ema_decay_table, HOST ONLY (no stream, no launch), the contract of svit_adamw_bias_table: entry k-1 =
 * (float) min((double) decay, (1.0 + k) / (10.0 + k)) for updates k = 1, 2, ... up to and including the first k whose
 * entry equals `decay` (89 949 entries at 0.9999, 8 990 at 0.999); past the table the decay is `decay`.  *n_entries receives that
 * length; table (room for `capacity` floats) may be NULL to ask for the length alone.  SVIT_ERR_ARG: n_entries NULL, a
 * table shorter than the length, decay not in (0, 1), or a length above 2^20. */
int svit_ema_decay_table(float decay, float* table, int64_t capacity, int64_t* n_entries);
int svit_ema_step_guarded(float* ema, const float* p, int64_t n, const int64_t* segs, int64_t S,
                          const float* decay_table, int64_t table_entries, float decay, const int64_t* ema_rec,
                          const svit_step_dev* dev_rec, void* stream);

/* ------------------------------------------------------------------ head (K15) ---------- */
/* SViT head (slowfast/models/video_model_builder.py:408-551) in one launch each way, fp32: dropout factors
 * applied to the cls / object rows of the final norm's output, class logits from the cls row, box MLP +
 * sigmoid and objectness logit from every object row, contact-state logits from the first two objects of a
 * frame.  tokens f32 [B,N,C]: row 0 = cls, the last T*O rows = objects (t-major).  keep f32 [B,1+T*O,C]
 * (mask / (1-p)) or NULL.  Outputs: logits [B,n_cls]; boxes [B,T,O,5] (col 0 objectness logit, 1..4 sigmoid
 * boxes = the reference's pred_bboxes); contact [B,T,2,5]; xobj [B,T*O,C] (optional: the dropped object
 * features = the reference's obj_desc). */
typedef struct {
  const float* tokens; int32_t B, N, C, T, O;
  const float* keep;
  const float* w_proj; const float* b_proj; int32_t n_cls;
  const float* w_box; const float* b_box;
  const float* w_bce; const float* b_bce;
  const float* w_con; const float* b_con;
  float* logits; float* boxes; float* contact; float* xobj;
} svit_head_args;
int svit_head_fwd(const svit_head_args* a, void* stream);
/* Backward: any of dlogits / dboxes / dcontact / dxobj may be NULL (no gradient).  dtokens f32 [B,N,C] is
 * OVERWRITTEN (zero rows for the patch tokens); the eight parameter gradients are ACCUMULATED (+=) -- they are
 * meant to be the views of the flat gradient buffer. */
typedef struct {
  svit_head_args f;
  const float* dlogits; const float* dboxes; const float* dcontact; const float* dxobj;
  float* dtokens;
  float* gw_proj; float* gb_proj; float* gw_box; float* gb_box; float* gw_bce; float* gb_bce; float* gw_con; float* gb_con;
  int32_t ordered;   /* != 0: the box / objectness / contact gradients of ALL object rows are summed by one block per channel
                        chunk in row order (no atomics: bit-reproducible when B*T*O exceeds one 32-row chunk); 0: a block per row chunk */
} svit_head_bwd_args;
int svit_head_bwd(const svit_head_bwd_args* g, void* stream);
/* The head in EVAL mode, one launch (csrc/head_eval.hip; what SViTHead.forward returns when `not self.training`).  Same
 * argument block; `tokens` is the final norm's output as it lies (row 0 = cls, the last T*O rows = objects: no
 * concatenation in front), `keep` must be NULL.  Outputs: logits [B,n_cls] holds PROBABILITIES -- act 0: softmax over
 * the classes, act 1: sigmoid per class (exponentials, sums and divisions in fp64, rounded to fp32 once; every
 * exponential has an argument <= 0 and every divisor lies in [1, n_cls], so no logit, however large, overflows: a
 * sigmoid of -800 is 0, not NaN); boxes [B,T,O,5]:
 * column 0 the SIGMOID of the objectness logit, 1..4 the sigmoid boxes; contact [B,T,2,5]: softmax over the last axis;
 * xobj [B,T*O,C] (optional, may be NULL): the object rows.  Workgroups [0,B) own one cls row each and run the softmax
 * in LDS; the others take eight object rows each.  Plain vector stores only; no atomics, so one build gives equal bits
 * for equal inputs.  Refused before any launch: SVIT_ERR_ARG -- keep != NULL, or NULL tokens / weights / biases /
 * logits / boxes / contact; SVIT_ERR_SHAPE -- C % 4 != 0, n_cls < 1, n_cls > 1024 (the LDS row), N < 1 + T*O, O < 2,
 * B or T < 1, act outside {0, 1}; SVIT_ERR_ALIGN -- tokens, a weight matrix or xobj not 16-byte aligned. */
int svit_head_eval(const svit_head_args* a, int act, void* stream);

/* ------------------------------------------------ image-rank HAOG losses ---- */
/* boxes_loss_ + contact-state CE of VideoImageLoss._haog_loss (slowfast/models/losses.py:50-93,
 * 138-155; slowfast/utils/box_ops.py:10-77) without the reference's boolean-index host syncs:
 * masks stay arithmetic, shapes fixed, so the image rank's step replays as a HIP graph.
 * pred f32 [R,5] (objectness logit, sigmoid cx,cy,w,h), tar f32 [R,4] (all-zero row = empty),
 * contact f32 [Rc,5] logits, contact_tar int64 [Rc] (<0 ignored).  One launch writes
 * losses f32 [8] = {l1, bce, giou, contact CE, #boxes, #contacts, #targets>4, 0} and the unit
 * gradients g_l1/g_giou f32 [R,4], g_bce f32 [R], g_contact f32 [Rc,5]. */
int svit_haog_loss(const float* pred, const float* tar, const float* contact,
                   const int64_t* contact_tar, float* losses, float* g_l1, float* g_bce,
                   float* g_giou, float* g_contact, int R, int Rc, void* stream);
/* dpred [R,5] = up[1]*g_bce | up[0]*g_l1 + up[2]*g_giou ; dcontact = up[3]*g_contact, with
 * `upstream` f32 [4] on the device (d total / d {l1, bce, giou, contact}). */
int svit_haog_loss_bwd(const float* upstream, const float* g_l1, const float* g_bce,
                       const float* g_giou, const float* g_contact, float* dpred,
                       float* dcontact, int R, int Rc, void* stream);

/* Video-rank classification loss (round 6): nn.CrossEntropyLoss(reduction="mean") of VideoImageLoss
 * (slowfast/models/losses.py:121,158) and its unit gradient in one launch -- replaces log_softmax + nll_loss and their
 * backward kernels.  logits f32 [B,C], labels int64 [B] (-100 = ignored row, as torch's default ignore_index; any other
 * label outside [0,C) makes the loss NaN); loss f32 [1] = mean over the counted rows, dlogits f32 [B,C] = d loss / d logits. */
int svit_ce_loss(const float* logits, const int64_t* labels, int B, int C, float* loss, float* dlogits, void* stream);
/* Cross entropy against a soft target and its unit gradient in one launch (cfg.MIXUP: the reference hands
 * nn.CrossEntropyLoss the float [B,C] target of mixup.py::mixup_target).  One workgroup, a wave per row, row losses added
 * in row order, no atomics.  Exactly one of `target` / `labels` is given:
 *   dense: target f32 [B,C] (mix must be NULL);
 *   fused: labels int64 [B]; t[b,c] = v1*lam + v2*oml (each product and the sum rounded to nearest, as torch does) with
 *          v1 = (c == labels[b]) ? on : off, v2 the same for labels[B-1-b], lam / oml from the record `mix` (see
 *          svit_mixup_clips; NULL: lam = 1, oml = 0).  on / off are the smoothed one-hot values (off = s/C, on = 1 - s + off,
 *          computed in double and cast by the caller).  The target is never stored.
 * loss f32 [1] = (1/B) sum_b sum_c t (logsumexp(x_b) - x_bc); dlogits f32 [B,C] = (softmax(x_b) * sum_c t_bc - t_bc) / B
 * (what autograd of F.cross_entropy gives for probability targets, also when they do not sum to 1).  No ignore index; a
 * label outside [0,C) makes the loss NaN. */
int svit_ce_loss_soft(const float* logits, const float* target, const int64_t* labels, const void* mix, float on,
                      float off, int B, int C, float* loss, float* dlogits, void* stream);
/* The step's random draws in one launch (round 6; replaces torch.rand + add + floor + div of DropPath,
 * slowfast/models/common.py:46-59, and the head's nn.Dropout mask): scales f32 [n_blocks, per_block] =
 * floor(keep[b] + U) / keep[b], drop f32 [n_drop] in {0, 1/(1-p_drop)}.  Philox-4x32-10 keyed by state[0], draw number
 * state[1] advanced by the launch itself (state: uint64 [3] in device memory = {seed, draw, 0}), so a replayed HIP graph
 * draws fresh numbers every replay. */
int svit_step_draws(uint64_t* state, const float* keep, int n_blocks, int per_block, float* scales,
                    int n_drop, float p_drop, float* drop, void* stream);

/* ---------------------------------------- multi-view test ensemble ---------- */
/* TestMeter.update_stats (slowfast/utils/meters.py:303-336) for one batch, on the device: clip n
 * belongs to video clip_ids[n] / num_clips; video_preds[v] (f32 [V,C]) += preds[n] (mode 0, "sum")
 * or = max(.,.) (mode 1, "max") in BATCH ORDER (bit-identical to the reference's sequential
 * loop), video_labels[v] = labels[n], clip_count[v] += 1.  `repeat` folds the batch's clips of a
 * video cyclically that many times (de-duplicated NUM_ENSEMBLE_VIEWS).  err int32 [4]:
 * {clip ids out of range, label conflicts (the reference's assert), labels out of range, 0},
 * incremented, never cleared. */
int svit_ensemble_update(const float* preds, const int64_t* labels, const int64_t* clip_ids,
                         int N, int C, int num_clips, int num_videos, int mode, int repeat,
                         float* video_preds, int64_t* video_labels, int64_t* clip_count,
                         int* err, void* stream);
/* metrics.topks_correct (slowfast/utils/metrics.py:9-50): counts[i] += #videos whose label is
 * among the ks[i] best scores (ties: lower class index first).  ks int32 [nk] on the device,
 * nk <= 8; counts int32 [nk] pre-zeroed. */
int svit_topk_correct(const float* video_preds, const int64_t* video_labels, int V, int C,
                      const int* ks, int nk, int* counts, int* err, void* stream);
/* One iteration of the train / val meters (slowfast/utils/meters.py:454-709; the .item() of every loss in every
 * iteration of tools/train_net.py:153-167 and of the two top-k errors of :325-335) recorded on the device: row
 * state[0] % W of ring (f32 [W,K]) takes the iteration, then state[0] += 1.  state: int64 [2] in device memory, read and
 * written only by the launch itself (a replayed HIP graph walks the rows by itself) = {pushes, labels out of range}.
 * Columns of a row: n_scalars <= SVIT_METER_MAX_SCALARS fp32 scalars fetched through the DEVICE addresses listed in the
 * HOST array `scalars` (read during the call; the 0-d loss tensors; their bits are copied, NaN payloads included), then,
 * if logits (f32 [N,C]) is not NULL, two more: the numbers of rows whose label (int64 [N]) ranks among the first k0 /
 * k1 classes, as fp32 (exact below 2^24).  Ranking is svit_topk_correct's: a class is ahead of the label if its score
 * is larger, or equal with a lower index.  A label outside [0,C) reads nothing, counts as wrong and increments state[1].
 * One workgroup, no float arithmetic.  Before any launch: SVIT_ERR_ARG for a NULL ring / state / listed address (or
 * logits without labels), SVIT_ERR_SHAPE for W <= 0, K != n_scalars + (logits ? 2 : 0), n_scalars > 16 and, with logits,
 * N <= 0, C <= 0 or a k outside [1,C]. */
#define SVIT_METER_MAX_SCALARS 16
int svit_meter_push(float* ring, int W, int K, int64_t* state, const float* const* scalars, int n_scalars,
                    const float* logits, const int64_t* labels, int N, int C, int k0, int k1, void* stream);
/* ------------------------------------------------ diagnostics (tools/ only) ------------------ */
/* Process-wide tuning knobs for the measurement scripts under tools/ and for the variant-parity tests (A/B runs of
 * kernel variants inside one process).  NOT part of the drop-in surface: the product path (svit_amd/engine.py,
 * bench.py) never calls them.  They are the ONLY way to change a heuristic: the library reads no environment
 * variable; all of them write one table (csrc/common.h SvitKnob, csrc/misc.hip), every selectable variant computes the
 * same results (none skips work), out-of-range values return SVIT_ERR_ARG, and svit_debug_reset() restores every
 * default -- tests and tools call it in their `finally`.  They replace nothing in the reference (it has no native
 * code). */
/* NT GEMM (csrc/gemm_nt.hip): key 0 = pipeline stages (2..4, 0 = heuristic), key 1 = forced tile/ring
 * configuration (-1 = heuristic, 0..10; 8 = the pre-ring v2 heuristic), key 2 = forced K-step (32 / 64, 0 = heuristic). */
int svit_debug_set(int key, int val);
/* Which kernel svit_gemm_nt would launch for a shape and an epilogue, and how -- the launch path's own chooser (csrc/gemm_nt.hip,
 * nt_choose), asked with plain integers under the current values of the three keys above.  Launches nothing and needs no
 * device.  The shape is checked as svit_gemm_nt checks it (SVIT_ERR_SHAPE: M, N, K <= 0, K % 32, N % 96; SVIT_ERR_ARG: no
 * such epilogue).  Fills out (n_out >= 13) and returns the number of values written, or an error code:
 *   family (0 gemm_nt_v2_kernel, 1 gemm_nt_ring_kernel); the template parameters RB, NB, WAVES_M, WAVES_N, loader waves
 *   (0 for v2), STAGES, K-step -- the tile is 32 RB WAVES_M rows x 32 NB WAVES_N columns; grid x, grid y; block size;
 *   dynamic LDS bytes; the rule that decided the tile (0 forced by key 1 / 2, 1 ring_few_long_tiles, 2 ring_long_k_narrow,
 *   3 bk64_narrow_long_k, 4 one_round_160x256, 5 one_round_192x192, 6 square_128x128, 7 big_128x192, 8 default_128x96). */
int svit_debug_gemm_nt_plan(int M, int N, int K, int epilogue, int32_t* out, int n_out);
/* grouped TN GEMM (csrc/gemm_tn.hip): cost-model constants of the row-chunk planner (x 0.01: microseconds per
 * k-step, TB/s of the fp32-atomic flush; <= 0 leaves a constant unchanged), and the tile mode (0: 128x96 only,
 * 1: per-problem heuristic fitted on isolated launches, 2: 128x192 everywhere (default), 3: 128x192 where
 * K % 192 == 0). */
int svit_debug_set_tn(int step_us_x100, int atomic_tbs_x100);
int svit_debug_set_tn_tile(int mode);
/* What a TN GEMM call would launch under the current values of the knobs above -- the launch path's own argument check,
 * planners and walk over the problem list (csrc/gemm_tn.hip: tn_check, tn_plan / tn_single_plan, tn_chunks).  Launches
 * nothing, makes no HIP call and needs no device; the pointers of `probs` are only checked (non-NULL, alignment), never
 * followed.  form: 0 svit_gemm_tn_grouped, 1 svit_gemm_tn_grouped_ex with ordered = 1, 2 svit_gemm_tn_grouped_slab,
 * 3 the stand-alone svit_gemm_tn of probs[0] (count must be 1; arg = its `splits`; arg is ignored by the other forms).
 * Returns the number of values written to out, or an error: the entry point's own code for what it refuses in `probs` /
 * `count`, SVIT_ERR_ARG for a form outside 0..3, form 3 with count != 1, a NULL out or an n_out below
 * 2 + 3 groups + 10 count.  Layout of out:
 *   [0] launch groups (ceil(count / SVIT_TN_GROUP_MAX); 1 for form 3)   [1] floats of slab workspace (form 2, else 0:
 *   what svit_gemm_tn_grouped_workspace answers), then per group
 *     problems in the group; grid of the GEMM launch (workgroups); grid of the reduce launch (form 2, else 0), and per problem
 *       tile kind (0 = 128x96, 1 = 128x192); tiles along N; tiles along K; rows_per_split; splits; first_block (the
 *       problem's first logical workgroup: its workgroups are first_block + split * tiles + tile); and, form 2 (else 0):
 *       slab columns w; tile_off; bias_off (float offsets into the workspace); red_first (its first reduce block).
 *   Form 3: the grid is tiles along N x tiles along K x splits, tile kind 0, first_block 0. */
int svit_debug_gemm_tn_plan(const svit_tn_problem* probs, int count, int form, int arg, int64_t* out, int n_out);
/* pooling (csrc/pool.hip): key 0 = forward path of the small planes: 0 streaming kernels, 1 VALU slab conv, 2 (default)
 * MFMA conv where it is ahead (blocks 4-13 of 16x224^2) and the slab elsewhere, 3 MFMA conv wherever its geometry holds;
 * key 1 = conv backward: 1 (default) the fused plane-walk kernel (conv dgrad + conv wgrad in one launch),
 * 0 refuse it (the two streaming launches in a -DSVIT_DIAG_POOL_STREAMING build, SVIT_ERR_SHAPE in the product library); key 2 = forward of the planes past 14x14 (blocks 0-3): 1 (default) the staged conv (input
 * staged once in LDS) + the row-wise LayerNorm launch, 0 the streaming kernel; key 3 = one-plane volumes (T = 1):
 * conv + LayerNorm in one launch from an LDS-staged plane -- 2 (default since round 6) in every T = 1 pass, also where
 * pre / mean / rstd are saved for a backward (image ranks), 1 in no-grad passes only (the frames pass), 0 never. */
int svit_debug_set_pool(int key, int val);
/* which path the last svit_pool_conv_bwd_qkv call took: 1 = the fused plane-walk kernel, 0 = not (planes that do not fit its LDS
 * plan, a workspace smaller than the plan's partial rows, key 1 = 0: SVIT_ERR_SHAPE in the product library, the two streaming
 * launches in a -DSVIT_DIAG_POOL_STREAMING build), -1 = no call yet. */
int svit_debug_pool_bwd_path(void);
/* What the host would decide for a pooling geometry -- the forward's chooser and the chunk search themselves, asked with plain
 * integers.  Launches nothing and needs no device.  save_mask: bit i = tensor i saves pre / mean / rstd; sel: selector tables
 * are given; relq_lpad: svit_pool_args.relq_lpad where q's rel-pos columns are wanted, else 0.  Fills out (n_out >= 24) and
 * returns the number of values written, or an error code.
 * kind 0, the forward (svit_pool_ln_fwd_qkv[_sel]): path (0 frame, 1 MFMA slab, 2 VALU slab, 3 staged, 4 streaming / tiled);
 *   who writes q's rel-pos columns (0 nobody, 1 pool_slab_ln_kernel, 2 the trailing svit_gemm_nt with SVIT_EPI_RELQ); the
 *   number of pooling launches; per launch the kernel (0 pool_frame_fwd, 1 pool_mfma_fwd, 2 pool_slab_fwd, 3 pool_slab_ln,
 *   4 pool_fwd_staged, 5 pool_ln_fwd3), grid x, y, z, block size, dynamic LDS bytes.
 * kind 1 / 2, the chunk plan of the staged forward / of svit_pool_conv_bwd_qkv: ok (0 = no plan), n_per[3], r_per[3],
 *   t_chunks[3], y_chunks[3], order[3], first_item[4], LDS bytes, max_chunks. */
int svit_debug_pool_plan(int kind, int B, int heads, int T, int H, int W, int n_obj, int sq, int sk, int sv, int save_mask,
                         int sel, int relq_lpad, int32_t* out, int n_out);
/* attention: key 0 = dkv kernel form (0 heuristic, 1 four waves, 2 eight waves with query halves), key 3 = the
 * forward's T' = 1 tile for Nk <= 64 (1 on (default), 0 the generic kernel). */
int svit_attn_debug_set(int key, int val);
/* every knob above back to its default */
int svit_debug_reset(void);
#ifdef __cplusplus
}
#endif
#endif
