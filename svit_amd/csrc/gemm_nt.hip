// bf16 MFMA GEMM for the nn.Linear family, forward and dgrad -- gfx950.
//   svit_gemm_nt : C[M,N] = A[M,K] * W[N,K]^T with fused epilogues (bias / GELU / residual +
//                  DropPath / fp32 accumulate + row remap / GELU-backward), gemm_epilogue.h
//
// Main loop: multi-stage direct-to-LDS pipeline.  A/W tiles go HBM/L2 -> LDS with
// global_load_lds_dwordx4 (no VGPR staging, no ds_write), STAGES tiles of BK=32 are kept in
// flight behind a COUNTED s_waitcnt vmcnt(N) and ONE raw s_barrier per K-step, so the prefetch
// distance (STAGES-1 tiles) covers L2/HBM latency instead of the single tile a register-staged
// double buffer can hide (cdna guide: "Pipelining across barriers").  Every wave owns a
// (32*RB) x 96 output tile as 32x32x16 MFMA accumulators; tiles are walked in an XCD-aware
// order (N tiles of one A row panel stay on one XCD's L2).
//
// LDS image of a stage: rows of 64 B (32 bf16), lane-linear as global_load_lds requires
// (wave-uniform base + lane*16); the four 16-B chunks of a row are XOR-swizzled with
// ((row>>2)&3) on the per-lane SOURCE address, and the same XOR is applied on the fragment
// reads -> ds_read_b128 of 16 consecutive rows hits 16 distinct slots of the 256-B bank row.
#include <cstring>
#include "gemm_epilogue.h"
#include "attn_common.h"   // Int / static_for / lds_read128 / lgkm_release1

namespace {

// LDS byte offset of the 16-B chunk `ch` of tile row `r`.  BK = 32: rows of 64 B, chunk XOR
// ((r>>2)&3).  BK = 64: rows of 128 B (a whole 128-B cache line per row and K-step: a 64-B row
// uses half of every line it touches), two tile rows (r, r+8) share a 256-B bank row, chunk XOR
// (r&7) -> the 16 rows of a ds_read_b128 lane group land on 16 distinct 16-B bank slots.
template <int BK>
__device__ __forceinline__ int nt_lds_off(int r, int ch) {
  if constexpr (BK == 32) return r * 64 + 16 * (ch ^ ((r >> 2) & 3));
  else return (r >> 4) * 2048 + (r & 7) * 256 + ((r >> 3) & 1) * 128 + 16 * (ch ^ (r & 7));
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int RB, int NB, int WAVES_M, int WAVES_N, int STAGES, int EPI, int BK2>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, (WAVES_M * WAVES_N > 4 ? 1 : 2)) void
gemm_nt_v2_kernel(svit_gemm_args p) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int BM = 32 * RB * WAVES_M, WN = 32 * NB, BN = WN * WAVES_N;
  // rows per stage, padded so that every wave issues the same number of loads per stage (the
  // counted vmcnt must be the same immediate for all waves); pad rows re-read a valid W row
  constexpr int CPR = BK2 / 8;                // 16-B chunks per tile row
  constexpr int RPR = NT / CPR;               // rows one round of loads (NT x 16 B) covers
  constexpr int ROWS = (BM + BN + RPR - 1) / RPR * RPR;
  constexpr int STAGE_BYTES = ROWS * BK2 * 2;
  constexpr int PER = ROWS * CPR / NT;        // global_load_lds per thread per stage
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  const int wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int m0 = (wgid / gridDim.x) * BM, n0 = (wgid % gridDim.x) * BN;

  // per-lane source pointers of this thread's PER chunks (k offset added per tile)
  const bf16_t* src[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int q = tid + i * NT;              // LDS position q*16 bytes within a stage
    int row, ch;
    if constexpr (BK2 == 32) {
      row = q >> 2;
      ch = (q & 3) ^ ((row >> 2) & 3);
    } else {
      const int line = q >> 4;
      row = (line >> 3) * 16 + ((q >> 3) & 1) * 8 + (line & 7);
      ch = (q & 7) ^ (row & 7);
    }
    if (row < BM) {
      const int gr = min(m0 + row, p.M - 1);
      src[i] = (const bf16_t*)p.A + (size_t)gr * p.lda + ch * 8;
    } else {
      const int gr = min(n0 + row - BM, p.N - 1);
      src[i] = (const bf16_t*)p.W + (size_t)gr * p.ldw + ch * 8;
    }
  }
  auto issue = [&](int kt, int stage) {
    unsigned char* base = smem + stage * STAGE_BYTES + wave * 1024;
#pragma unroll
    for (int i = 0; i < PER; ++i)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(src[i] + kt * BK2),
          (__attribute__((address_space(3))) void*)(base + i * (NT * 16)), 16, 0, 0);
  };

  f32x16_t acc[RB][NB];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.K / BK2;
  // prologue: STAGES-1 tiles in flight
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) issue(s, s);

  const int a_row = wm * 32 * RB + (lane & 31);
  const int w_row = BM + wn * WN + (lane & 31);
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt has landed once at most the (STAGES-2) younger tiles' loads are outstanding
    if (kt + STAGES - 2 < nk) wait_vmcnt<(STAGES - 2) * PER>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // (a) everyone's part of tile kt is in LDS
                                    // (b) everyone finished reading tile kt-1's buffer
    if (kt + STAGES - 1 < nk) issue(kt + STAGES - 1, (kt + STAGES - 1) % STAGES);
    const unsigned char* st = smem + (kt % STAGES) * STAGE_BYTES;
    // all fragment reads of the tile first, then the MFMAs back to back: left to itself the
    // compiler reused two fragment registers and put a full `s_waitcnt lgkmcnt(0)` in front of
    // nearly every MFMA (four exposed LDS round trips per tile)
    bf16x8_t af[BK2 / 16][RB], wf[BK2 / 16][NB];
#pragma unroll
    for (int ks = 0; ks < BK2 / 16; ++ks) {
      const int ch = 2 * ks + (lane >> 5);
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int r = a_row + i * 32;
        af[ks][i] = *(const bf16x8_t*)(st + nt_lds_off<BK2>(r, ch));
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int r = w_row + j * 32;
        wf[ks][j] = *(const bf16x8_t*)(st + nt_lds_off<BK2>(r, ch));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < BK2 / 16; ++ks)
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = mfma32(af[ks][i], wf[ks][j], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();   // all LDS reads of the last tiles done before the epilogue reuses LDS
  // (staging regions are per wave: no workgroup barrier inside the epilogue -- eight of them per 128x128 tile
  // kept the four waves in lock step through their stores)
  nt_epilogue<RB, NB, EPI, true>(p, acc, smem, m0, n0, wm, wn, lane, wave);
}

// ---- ring form: loader waves + MFMA waves (long-K GEMMs) ---------------------------------------------
// What bounds gemm_nt_v2_kernel on the long-K shapes is not a byte rate but the ISSUE of the LDS-DMA
// instructions: a 1-KiB piece holds the issuing wave for 60-185 cycles (MI355X guide, "LDS-DMA piece
// issue cost"), and in the v2 loop those cycles, the fragment reads and the MFMAs of a K-step are
// one wave's serial stream, so the matrix pipe idles while its wave feeds the ring (28 % busy, SQ counters
// of round 2) and only a second resident workgroup fills the holes.  Here the two jobs are different
// waves of one 8-wave workgroup, one of each per SIMD:
//   * waves 4..7 (loaders) do nothing but issue `global_load_lds_dwordx4` pieces (per-lane source pointers
//     fixed, one 64-bit add per piece and K-step) and wait for them with counted vmcnt; STAGES-1 K-steps
//     of 64 stay in flight;
//   * waves 0..3 (MFMA waves) own (32 RB) x (32 NB) accumulators and stream the fragments of one k16
//     sub-step AHEAD of the MFMAs that use them (inline-asm ds_read_b128, two per MFMA gap, released by
//     lgkmcnt(0) three MFMAs later), so neither the LDS latency nor any vector-memory instruction sits
//     in their instruction stream.
// One s_barrier per K-step joins them: B(kt) = "tile kt has landed" (loaders arrive after their vmcnt)
// and "tile kt-1 is read" (MFMA waves arrive after the lgkmcnt(0) of its last fragments) -- it sits
// BEFORE the last sub-step's MFMAs of tile kt-1, whose 32 RB NB cycles cover the first fragment reads of
// tile kt.  Tiles as in v2: BK = 64 rows of 128 B, chunk XOR (r & 7) (nt_lds_off<64>).
// The loader waves' whole life.  (Per-lane 64-bit source pointers + global_load_lds: the buffer-descriptor
// form of the same instruction, called with template-dependent operands from a kernel template, makes
// hipcc's HOST pass drop the kernel's stub without a diagnostic; the one v_lshl_add_u64 per piece this
// costs is nothing to a wave that does nothing else.)
template <int NL, int BM, int BN, int STAGES>
__device__ __forceinline__ void nt_ring_loader(const svit_gemm_args& p, unsigned char* smem, int lw, int lane,
                                               int m0, int n0, int nk) {
  constexpr int PIECES = (BM + BN) / 8;              // 1-KiB pieces of a stage image (8 rows x 128 B each)
  constexpr int PER = (PIECES + NL - 1) / NL;        // per loader wave and K-step (the same count for every
                                                     // wave: a surplus slot re-loads the last piece)
  constexpr int STAGE_BYTES = (BM + BN) * 128;
  // piece q = lane-linear 16-B slots; slot -> (tile row, 16-B chunk) is the inverse of nt_lds_off<64>;
  // a piece lies wholly in A rows or wholly in W rows (BM % 16 == 0)
  const bf16_t* src[PER];
  auto piece_of = [&](int i) { return min(lw + NL * i, PIECES - 1); };
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int q = piece_of(i) * 64 + lane, line = q >> 4;
    const int row = (line >> 3) * 16 + ((q >> 3) & 1) * 8 + (line & 7);
    const int ch = (q & 7) ^ (row & 7);
    if (row < BM) src[i] = (const bf16_t*)p.A + (size_t)min(m0 + row, p.M - 1) * p.lda + ch * 8;
    else src[i] = (const bf16_t*)p.W + (size_t)min(n0 + row - BM, p.N - 1) * p.ldw + ch * 8;
  }
  auto issue = [&](int kt) {
    unsigned char* st = smem + (kt % STAGES) * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < PER; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + kt * 64),
                                       (__attribute__((address_space(3))) void*)(st + piece_of(i) * 1024), 16, 0, 0);
  };
#pragma unroll
  for (int s = 0; s < STAGES; ++s)
    if (s < nk) issue(s);
  // B(kt): tile kt has landed once at most the tiles issued after it are outstanding
  for (int kt = 0; kt < nk; ++kt) {
    // tiles issued after tile kt so far: the prologue's, then one per passed barrier
    const int younger = (kt == 0 ? min(STAGES - 1, nk - 1) : min(kt + STAGES - 2, nk - 1) - kt);
    attn::static_for<0, STAGES>([&](auto Y) {
      if (younger == decltype(Y)::value) wait_vmcnt<decltype(Y)::value * PER>();
    });
    __builtin_amdgcn_s_barrier();
    // the barrier also says tile kt-1 is read: its slot takes tile kt-1+STAGES
    if (kt >= 1 && kt - 1 + STAGES < nk) issue(kt - 1 + STAGES);
  }
}

template <int RB, int NB, int WAVES_M, int WAVES_N, int NL, int STAGES, int EPI>
__global__ __launch_bounds__((WAVES_M * WAVES_N + NL) * 64, 1) void gemm_nt_ring_kernel(svit_gemm_args p) {
  using attn::Int;
  constexpr int NC = WAVES_M * WAVES_N;          // MFMA waves; NL loader waves behind them
  constexpr int BM = 32 * RB * WAVES_M, WN = 32 * NB, BN = WN * WAVES_N;
  static_assert(BM % 16 == 0 && BN % 16 == 0, "a 1-KiB piece must not straddle A and W rows");
  constexpr int STAGE_BYTES = (BM + BN) * 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  const int wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  const int m0 = (wgid / gridDim.x) * BM, n0 = (wgid % gridDim.x) * BN;
  const int nk = p.K / 64;

  if (wave >= NC) {
    nt_ring_loader<NL, BM, BN, STAGES>(p, smem, wave - NC, lane, m0, n0, nk);
    return;
  }

  // -------------------------------------------------- MFMA waves ----------------------------------------
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  f32x16_t acc[RB][NB];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment addresses: row r = 16 g + (lane & 31) (+ 32 per row block), chunk 2 ks + (lane >> 5);
  // chunk ^ (r & 7) = 2 (ks ^ ((r & 7) >> 1)) + ((lane >> 5) ^ (r & 1)): one address per ks, row blocks and
  // the A / W split are immediates or wave constants
  const int l31 = lane & 31, x7 = lane & 7;
  unsigned fa[4], fw[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const unsigned lp = (unsigned)((l31 >> 4) * 2048 + x7 * 256 + ((l31 >> 3) & 1) * 128 +
                                   32 * (ks ^ (x7 >> 1)) + 16 * ((lane >> 5) ^ (x7 & 1)));
    fa[ks] = (unsigned)(size_t)smem + lp + (unsigned)(wm * 2 * RB) * 2048u;
    fw[ks] = (unsigned)(size_t)smem + lp + (unsigned)((BM + wn * WN) / 16) * 2048u;
  }
  bf16x8_t fr[2][RB + NB];       // fragments of two consecutive k16 sub-steps (A row blocks, then W)
  auto reads = [&](auto KS, auto BUF, unsigned so, auto HALF) {
    // HALF 0: the first (RB+NB+1)/2 fragments, HALF 1: the rest -- two reads per MFMA gap
    constexpr int ks = decltype(KS)::value, b = decltype(BUF)::value, h = decltype(HALF)::value;
    attn::static_for<0, RB + NB>([&](auto F) {
      constexpr int f = decltype(F)::value;
      if constexpr ((f / 2) == h) {
        if constexpr (f < RB) attn::lds_read128<f * 4096>(fr[b][f], fa[ks] + so);
        else attn::lds_read128<(f - RB) * 4096>(fr[b][f], fw[ks] + so);
      }
    });
  };
  constexpr int NH = (RB + NB + 1) / 2;       // read groups of two
  auto release = [&](auto BUF) {
    constexpr int b = decltype(BUF)::value;
    attn::static_for<0, RB + NB>([&](auto F) { attn::lgkm_release1<0>(fr[b][decltype(F)::value]); });
  };
  // MFMAs of one sub-step from buffer B, with the reads of the next sub-step (buffer 1-B) in the first gaps
  auto substep = [&](auto BUF, auto NEXT_KS, unsigned next_so, bool do_reads) {
    constexpr int b = decltype(BUF)::value;
    attn::static_for<0, RB * NB>([&](auto Q) {
      constexpr int q = decltype(Q)::value, i = q / NB, j = q % NB;
      acc[i][j] = mfma32(fr[b][i], fr[b][RB + j], acc[i][j]);
      if constexpr (q < NH) {
        if (do_reads) reads(NEXT_KS, Int<1 - b>{}, next_so, Int<q>{});
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  __builtin_amdgcn_s_barrier();                       // B(0)
  attn::static_for<0, NH>([&](auto H) { reads(Int<0>{}, Int<0>{}, 0u, H); });
  release(Int<0>{});
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned so = (unsigned)((kt % STAGES) * STAGE_BYTES);
    const unsigned so_next = (unsigned)(((kt + 1) % STAGES) * STAGE_BYTES);
    const bool more = kt + 1 < nk;
    substep(Int<0>{}, Int<1>{}, so, true);
    release(Int<1>{});
    substep(Int<1>{}, Int<2>{}, so, true);
    release(Int<0>{});
    substep(Int<0>{}, Int<3>{}, so, true);
    release(Int<1>{});                                // every read of tile kt has returned
    if (more) __builtin_amdgcn_s_barrier();           // B(kt+1): tile kt+1 is in LDS, tile kt's slot is free
    substep(Int<1>{}, Int<0>{}, so_next, more);
    if (more) release(Int<0>{});
  }
  // staging for the epilogue: a slot no MFMA wave can still be reading (tile nk-2's; all DMA has landed)
  unsigned char* epi = smem + (nk >= 2 ? (nk - 2) % STAGES : 1) * STAGE_BYTES;
  nt_epilogue<RB, NB, EPI, true>(p, acc, epi, m0, n0, wm, wn, lane, wave);
}

// ---- host side: shape -> choice (nt_choose) -> row of nt_forms -> launch ---------------------------------------
// The template parameters of a kernel as integers: NL loader waves (0: gemm_nt_v2_kernel, else gemm_nt_ring_kernel).
struct NtParams { int family /* 0 v2, 1 ring */, RB, NB, WM, WN, NL, stages, BK; };
// One instantiated form: its kernel per epilogue (nullptr: no ring kernel takes SVIT_EPI_RELQ) and the per-device state
// of svit_max_lds_once.
typedef void (*NtKernel)(svit_gemm_args);
struct NtForm { NtParams p; NtKernel kernel[6]; SvitOnce once[6]; };
template <int RB, int NB, int WM, int WN, int ST, int BK>
constexpr NtForm v2_form() {
  return {{0, RB, NB, WM, WN, 0, ST, BK},
          {gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_BF16, BK>, gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_GELU, BK>,
           gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_RESID, BK>, gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_F32, BK>,
           gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_DGELU, BK>, gemm_nt_v2_kernel<RB, NB, WM, WN, ST, SVIT_EPI_RELQ, BK>}, {}};
}
template <int RB, int NB, int WM, int WN, int NL, int ST>
constexpr NtForm ring_form() {
  constexpr int BM = 32 * RB * WM, BN = 32 * NB * WN;
  static_assert((size_t)WM * WN * 16 * (32 * NB + 4) * sizeof(float) <= (size_t)(BM + BN) * 128, "epilogue staging fits a slot");
  static_assert((size_t)ST * (BM + BN) * 128 <= 160 * 1024, "LDS");
  return {{1, RB, NB, WM, WN, NL, ST, 64},
          {gemm_nt_ring_kernel<RB, NB, WM, WN, NL, ST, SVIT_EPI_BF16>, gemm_nt_ring_kernel<RB, NB, WM, WN, NL, ST, SVIT_EPI_GELU>,
           gemm_nt_ring_kernel<RB, NB, WM, WN, NL, ST, SVIT_EPI_RESID>, gemm_nt_ring_kernel<RB, NB, WM, WN, NL, ST, SVIT_EPI_F32>,
           gemm_nt_ring_kernel<RB, NB, WM, WN, NL, ST, SVIT_EPI_DGELU>, nullptr}, {}};
}
// Every kernel the library holds (29 forms, 165 kernels), in the order nt_choose's rules name the tiles.  Only the knobs
// (tools, variant and parity tests) reach 3 stages on a v2 tile, K-step 64 on any tile but 128x96 at depth 2, the
// 128x128 ring tile and the ring depths a rule does not name.
NtForm nt_forms[] = {
    ring_form<2, 3, 2, 2, 4, 2>(), ring_form<2, 3, 2, 2, 4, 3>(), ring_form<2, 3, 2, 2, 4, 4>(),   // 128x192 ring
    ring_form<1, 3, 4, 1, 4, 2>(), ring_form<1, 3, 4, 1, 4, 3>(), ring_form<1, 3, 4, 1, 4, 4>(),   // 128x96 ring
    ring_form<2, 2, 2, 2, 4, 2>(), ring_form<2, 2, 2, 2, 4, 3>(), ring_form<2, 2, 2, 2, 4, 4>(),   // 128x128 ring
    v2_form<1, 3, 4, 1, 2, 64>(),                                                                  // 128x96, K-step 64
    v2_form<5, 2, 1, 4, 2, 32>(), v2_form<3, 3, 2, 2, 2, 32>(),                                    // 160x256, 192x192
    v2_form<2, 2, 2, 2, 2, 64>(), v2_form<2, 2, 2, 2, 3, 64>(), v2_form<2, 2, 2, 2, 4, 64>(),      // 128x128
    v2_form<2, 2, 2, 2, 2, 32>(), v2_form<2, 2, 2, 2, 3, 32>(), v2_form<2, 2, 2, 2, 4, 32>(),
    v2_form<2, 3, 2, 2, 2, 64>(), v2_form<2, 3, 2, 2, 3, 64>(), v2_form<2, 3, 2, 2, 4, 64>(),      // 128x192
    v2_form<2, 3, 2, 2, 2, 32>(), v2_form<2, 3, 2, 2, 3, 32>(), v2_form<2, 3, 2, 2, 4, 32>(),
    v2_form<1, 3, 4, 1, 3, 64>(), v2_form<1, 3, 4, 1, 4, 64>(),                                    // 128x96
    v2_form<1, 3, 4, 1, 2, 32>(), v2_form<1, 3, 4, 1, 3, 32>(), v2_form<1, 3, 4, 1, 4, 32>(),
};

enum NtRule { NT_FORCED, NT_RING_FEW_LONG_TILES, NT_RING_LONG_K_NARROW, NT_BK64_NARROW_LONG_K, NT_ONE_ROUND_160X256,
              NT_ONE_ROUND_192X192, NT_SQUARE_128X128, NT_BIG_128X192, NT_DEFAULT_128X96 };
struct NtKnobs { int cfg, stages, bk; };      // SVIT_K_NT_CFG / _STAGES / _BK (svit_debug_set; tools and variant tests only)
struct NtChoice { NtParams p; unsigned gx, gy, block; size_t lds; int rule /* the NtRule that decided the tile */; };

// a tile and its launch geometry (stages: anything but 2 / 3 is 4 -- the knob admits 0 and 2..4 only)
NtChoice nt_tile(int family, int RB, int NB, int WM, int WN, int stages, int BK, int rule, int M, int N) {
  NtChoice c = {{family, RB, NB, WM, WN, family ? 4 : 0, stages == 2 || stages == 3 ? stages : 4, BK}};
  const int BM = 32 * RB * WM, BN = 32 * NB * WN, waves = WM * WN;
  c.gx = (N + BN - 1) / BN, c.gy = (M + BM - 1) / BM, c.block = (waves + c.p.NL) * 64, c.rule = rule;
  if (family) {
    c.lds = (size_t)c.p.stages * (BM + BN) * 128;      // (the epilogue's staging fits a slot: ring_form)
  } else {   // rows per stage padded to whole rounds of loads; at least the epilogue's staging
    const int RPR = waves * 64 / (BK / 8);
    c.lds = (size_t)c.p.stages * ((BM + BN + RPR - 1) / RPR * RPR) * BK * 2;
    const size_t lds_epi = (size_t)waves * 16 * (32 * NB + 4) * sizeof(float);
    if (c.lds < lds_epi) c.lds = lds_epi;
  }
  return c;
}

// Which kernel, for a shape that passed nt_check_shape.  Pure: svit_gemm_nt launches what it answers and
// svit_debug_gemm_nt_plan reports it.  The rules stand in their order of precedence; the first that holds returns.
//
// What the tile rules rest on (measured on MI355X, tools/bench_kernels.py ntstages): 128x192 blocks (2x2 waves of 64x96) win
// whenever they still give >= 1 tile per CU; otherwise, and for N = 96 (mod 192), 128x96 blocks (4 waves of 32x96) double
// the number of workgroups.  A 256x192 / 8-wave tile (fewer LDS-fill bytes per flop) was measured too and never won.  At
// M = 13064 every variant lands within 10 % of the others: the bound is the per-CU LDS fill rate (~40 GB/s per CU,
// ~10 TB/s chip-wide for the mix of L2 and Infinity-Cache hits), not the pipeline depth, the fragment-read scheduling or
// the tile shape.  Also measured and rejected:
//  * a persistent form (a workgroup walks several tiles and issues the next tile's first LDS-DMA from inside the epilogue
//    of the current one; commit "experiment: persistent NT GEMM", profiles/r02_nt_persistent_tiles.txt): -10..-17 % on the
//    many-tile K = 384 shapes of the 56x56 stage, +5..10 % wherever the epilogue writes two outputs or fp32 rows -- the
//    next tile's first s_waitcnt vmcnt(0) also waits for this tile's stores, which a finishing workgroup never does.
//    Net zero over the step; not kept.
//  * a register-staged form (global_load_dwordx4 -> VGPR -> ds_write_b128, K-step 64, loads a whole K-step ahead; commit
//    "experiment: register-staged NT GEMM variant", profiles/r02_nt_tile_sweep.txt column REG): 5-10 % slower than
//    LDS-DMA on every shape -- the bound is the CU's vector-memory path itself (SQ counters, profiles/
//    r02_nt_pmc_13064x384x1536.txt: waves spend 51 % of their cycles stalled at instruction issue with the MFMA pipe
//    28 % busy; ~35 cycles per 1-KiB load instruction per CU = 29 B/clk/CU = 56 GB/s/CU), not how the bytes reach LDS.
//  * a row-stationary form for K <= 384 (8-wave workgroups, A rows held in registers as MFMA fragments, only W streamed
//    through a 4-deep LDS ring: 4x fewer fill bytes per flop) -- 0.6-0.9x the speed of these tiles on every shape of
//    the model: one barrier-locked workgroup per CU leaves nothing to overlap its epilogues and barriers with.
NtChoice nt_choose(int M, int N, int K, int epilogue, NtKnobs kn) {
  // cfg: 0 / 2 / 4 = v2 tiles 128x192 / 128x96 / 128x128, 5 / 6 / 7 = the same as ring tiles, 9 / 10 = the one-round
  // tiles, -1 = heuristic.  Knob value 8 is no tile: it means "the v2 heuristic, no ring".
  const int cfg = kn.cfg == 8 ? -1 : kn.cfg;
  const bool heuristic = cfg < 0 && !kn.stages && !kn.bk;   // nothing forced at all
  const long tm = (M + 127) / 128;                           // 128-row tiles along M

  // ---- 1. ring kernels (loader waves + MFMA waves, K-steps of 64) ----------------------------------------------
  // They exist for K % 64 == 0 only, and none has the SVIT_EPI_RELQ epilogue: both fall through to the v2 rules, a
  // forced ring tile included (it then switches rules 3 to 6 off and leaves 7 / 8 to the heuristic).
  if (K % 64 == 0 && epilogue != SVIT_EPI_RELQ) {
    const int rs = kn.stages ? kn.stages : 3;                // a forced ring tile is 3 deep unless told otherwise
    if (cfg == 5) return nt_tile(1, 2, 3, 2, 2, rs, 64, NT_FORCED, M, N);
    if (cfg == 6) return nt_tile(1, 1, 3, 4, 1, rs, 64, NT_FORCED, M, N);
    if (cfg == 7) return nt_tile(1, 2, 2, 2, 2, rs, 64, NT_FORCED, M, N);
    // Which ring kernel, if any.  Two sets of measurements on MI355X decide (profiles/r03_nt_ring.txt): isolated
    // loops per epilogue family (tools/bench_kernels.py ntring <epilogue>), where the ring kernels win almost
    // everywhere K % 64 == 0, and the replayed training step with every NT launch matched by position
    // (tools/nt_by_position.py), where the short-K wins do NOT survive (a launch's neighbours are other kernels, not
    // copies of itself: 128x128 / 2 stages for fc1 was +5 % there, 128x96 / 2 stages at K = 384 +11 %).  Kept are
    // the two rules that win in both.  Knob value 8 switches them off, and so does ANY forced K-step (a set
    // SVIT_K_NT_BK asks for a v2 kernel); a forced stage count does not reach them: they bring their own depth.
    if (cfg < 0 && kn.cfg != 8 && !kn.bk) {
      const long t192 = N % 192 == 0 ? tm * (N / 192) : 0, t96 = tm * ((N + 95) / 96);
      // few, long tiles: every 128x96 tile has a CU to itself -> 4-deep ring (3656 x 768 x 768..3072: -30 %)
      constexpr int k_min5 = 1024, t_max6 = 256, s6 = 4;     // (swept inside the step in round 4: profiles/r04_in_step_sweeps.txt)
      // (> 256 tiles: two workgroups per CU need the 2-stage ring -- an arm no shape takes while t_max6 is 256)
      if (t96 <= t_max6 && K >= 768) return nt_tile(1, 1, 3, 4, 1, t96 > 256 ? 2 : s6, 64, NT_RING_FEW_LONG_TILES, M, N);
      // long K, narrow output, enough 128x192 tiles for most CUs (13064 x 384 x 1152..2304: -6..-10 % in the
      // step, -15..-20 % isolated; on a par with hipBLASLt's 128x160x64 macro-tile)
      if (t192 >= 160 && N <= 768 && K >= k_min5) return nt_tile(1, 2, 3, 2, 2, 3, 64, NT_RING_LONG_K_NARROW, M, N);
    }
  }

  // ---- 2. the v2 kernel's depth and K-step ----------------------------------------------------------------------
  // pipeline depth (measured, tools/bench_kernels.py ntstages): short K loops prefer 2 stages (less LDS -> more resident
  // workgroups), K >= 2048 wants the 4-deep prefetch
  const int stages = kn.stages ? kn.stages : (K >= 2048 ? 4 : 2);
  // K-step of 64 (whole 128-B lines per tile row; half as many barriers): measured 5-14 % faster for the narrow-output,
  // long-K GEMMs (fc2, proj, qkv dgrad: N <= 768, K >= 384) as 128x96 blocks at depth 2, and slower elsewhere -- the 2x LDS
  // per stage costs a resident workgroup (tools/bench_kernels.py ntstages, profiles/r02_nt_tile_sweep.txt).  A forced
  // K-step of 64 is 32 where K % 64 != 0.
  const bool bk64 = kn.bk ? kn.bk == 64 && K % 64 == 0 : K % 64 == 0 && N <= 768 && K >= 384;
  const int BK = bk64 ? 64 : 32;

  // ---- 3. K-step 64 takes the 128x96 tile at depth 2, whatever the tile rules below would say -- unless a tile or a
  // depth is forced (a forced K-step of 64 alone lands here too)
  if (bk64 && cfg < 0 && !kn.stages) return nt_tile(0, 1, 3, 4, 1, 2, 64, kn.bk ? NT_FORCED : NT_BK64_NARROW_LONG_K, M, N);

  // ---- 4. / 5. ONE-ROUND tiles for the wide short-K GEMMs of the 14x14 stage (round 4) ------------------------------
  // At M = 13064 the 128-row tiles below put 824 (128x192) or 1236 (128x128) workgroups on 512-768 slots: a second,
  // part-filled round in which the chip mostly stores.  160x256 (1 x 4 waves of 160x64) covers 13064 x 1536 with
  // 82 x 6 = 492 workgroups, 192x192 (2 x 2 waves of 96x96) covers 13064 x 1152 with 69 x 6 = 414: every workgroup
  // resident at once (two per CU), more flops per LDS-fill byte (91 / 96 against 77 / 64).  Heuristic: only where the
  // grid is one round and the 128-row grid is not, and nothing is forced.  cfg 9 / 10 force them, always at depth 2 and
  // K-step 32 (forced stages / K-step are not looked at); a forced one whose width does not divide N falls through.
  const long t160 = N % 256 == 0 ? (long)((M + 159) / 160) * (N / 256) : 0;
  const long t192 = N % 192 == 0 ? (long)((M + 191) / 192) * (N / 192) : 0;
  const bool auto_ok = heuristic && K <= 512 && tm * ((N + 191) / 192) > 512;
  if (N % 256 == 0 && (cfg == 9 || (auto_ok && t160 > 256 && t160 <= 512)))
    return nt_tile(0, 5, 2, 1, 4, 2, 32, cfg == 9 ? NT_FORCED : NT_ONE_ROUND_160X256, M, N);
  if (N % 192 == 0 && (cfg == 10 || (auto_ok && t192 > 256 && t192 <= 512)))
    return nt_tile(0, 3, 3, 2, 2, 2, 32, cfg == 10 ? NT_FORCED : NT_ONE_ROUND_192X192, M, N);

  // ---- 6. 128x128 blocks (2x2 waves of 64x64): measured ~10 % faster than 128x192 for the wide, short-K
  // GEMMs of the 14x14 stage (M = 13064, N = 1152 / 1536, K = 384: fc1, fc2-dgrad, qkv).  Any forced tile but cfg 4
  // switches the rule off; cfg 4 where 128 does not divide N falls through.
  if (cfg == 4 ? N % 128 == 0 : cfg < 0 && N % 128 == 0 && N >= 1024 && K <= 512 && tm * (N / 128) <= 2048)
    return nt_tile(0, 2, 2, 2, 2, stages, BK, cfg == 4 ? NT_FORCED : NT_SQUARE_128X128, M, N);

  // ---- 7. 128x192 blocks where they give a tile per CU.  cfg 0 forces them where 192 divides N (else it falls through
  // to rule 8); cfg 2 switches the rule off; every other forced tile that came this far (5..7, 9, 10, a 4 that did not
  // divide) leaves it to the heuristic.
  if (N % 192 == 0 && cfg != 2 && (cfg == 0 || tm * (N / 192) >= 256))
    return nt_tile(0, 2, 3, 2, 2, stages, BK, cfg == 0 ? NT_FORCED : NT_BIG_128X192, M, N);

  // ---- 8. 128x96 blocks: every N the entry point accepts
  return nt_tile(0, 1, 3, 4, 1, stages, BK, cfg == 2 ? NT_FORCED : NT_DEFAULT_128X96, M, N);
}

// the row of nt_forms a choice names and its kernel for an epilogue; nullptr: nt_choose and nt_forms disagree
NtForm* nt_form_of(const NtChoice& c, int epilogue) {
  for (NtForm& r : nt_forms)      // (family follows from NL)
    if (r.p.RB == c.p.RB && r.p.NB == c.p.NB && r.p.WM == c.p.WM && r.p.WN == c.p.WN && r.p.NL == c.p.NL &&
        r.p.stages == c.p.stages && r.p.BK == c.p.BK)
      return epilogue >= 0 && epilogue <= SVIT_EPI_RELQ && r.kernel[epilogue] ? &r : nullptr;
  return nullptr;
}

NtKnobs nt_knobs() { return {svit_knob(SVIT_K_NT_CFG), svit_knob(SVIT_K_NT_STAGES), svit_knob(SVIT_K_NT_BK)}; }

int nt_check_shape(int M, int N, int K) {
  return M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || N % 96 != 0 ? SVIT_ERR_SHAPE : SVIT_OK;
}
}  // namespace

extern "C" int svit_gemm_nt(const svit_gemm_args* args, void* stream) {
  if (!args || !args->A || !args->W) return SVIT_ERR_ARG;
  const svit_gemm_args& a = *args;
  const bool relq = a.epilogue == SVIT_EPI_RELQ;
  if (!relq && !a.out) return SVIT_ERR_ARG;
  if (relq) {
    if (!a.relq_map || !a.relq_out || (a.relq_extra != 32 && a.relq_extra != 64) || a.relq_rows < 1 ||
        a.relq_ld < 96 + a.relq_extra || a.bias)
      return SVIT_ERR_ARG;
  }
  if (int rc = nt_check_shape(a.M, a.N, a.K)) return rc;
  if (a.lda % 8 != 0 || a.ldw % 8 != 0 || a.lda < a.K || a.ldw < a.K || (!relq && a.ldo < a.N))
    return SVIT_ERR_ALIGN;
  if (((uintptr_t)a.A | (uintptr_t)a.W) & 15) return SVIT_ERR_ALIGN;
  if (!relq && (a.ldo % 4 != 0 || ((uintptr_t)a.out & 15))) return SVIT_ERR_ALIGN;
  if (a.bias && ((uintptr_t)a.bias & 15)) return SVIT_ERR_ALIGN;
  if (a.aux && (a.ldaux % 4 != 0 || ((uintptr_t)a.aux & 15))) return SVIT_ERR_ALIGN;
  if (a.out2 && (a.ldo2 % 4 != 0 || ((uintptr_t)a.out2 & 15))) return SVIT_ERR_ALIGN;
  if ((a.epilogue == SVIT_EPI_RESID || a.epilogue == SVIT_EPI_DGELU) && !a.aux) return SVIT_ERR_ARG;
  if (a.epilogue == SVIT_EPI_RESID && a.row_scale && a.rows_per_sample <= 0) return SVIT_ERR_ARG;

  const NtChoice c = nt_choose(a.M, a.N, a.K, a.epilogue, nt_knobs());
  NtForm* f = nt_form_of(c, a.epilogue);
  if (!f) return SVIT_ERR_ARG;
  for (int e = 0; e < 6; ++e)       // the form's kernels for every epilogue, on its first launch per device
    if (f->kernel[e])
      if (int rc = svit_max_lds_once(f->once[e], (const void*)f->kernel[e], c.lds)) return rc;
  hipLaunchKernelGGL(f->kernel[a.epilogue], dim3(c.gx, c.gy), dim3(c.block), c.lds, (hipStream_t)stream, a);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

// Host-only plan query (include/svit_hip.h, diagnostics): nt_choose's answer as integers.
extern "C" int svit_debug_gemm_nt_plan(int M, int N, int K, int epilogue, int32_t* out, int n_out) {
  if (!out || n_out < 13) return SVIT_ERR_ARG;
  if (int rc = nt_check_shape(M, N, K)) return rc;
  const NtChoice c = nt_choose(M, N, K, epilogue, nt_knobs());
  if (!nt_form_of(c, epilogue)) return SVIT_ERR_ARG;
  static_assert(sizeof c.p == 8 * sizeof(int32_t), "layout");
  memcpy(out, &c.p, sizeof c.p);       // family, RB, NB, WAVES_M, WAVES_N, loader waves, stages, K-step
  out[8] = (int32_t)c.gx, out[9] = (int32_t)c.gy, out[10] = (int32_t)c.block, out[11] = (int32_t)c.lds, out[12] = c.rule;
  return 13;
}
