// bf16 MFMA weight-gradient GEMM for the nn.Linear family -- gfx950 only.
//   svit_gemm_tn : dW[N,K] += A[M,N]^T * B[M,K]  (reduction over rows, operands consumed
//                  through ds_read_b64_tr_b16 transposed LDS reads; fused bias gradient)
//   svit_gemm_tn_grouped_slab : the grouped form with the row splits stored to slabs and summed in split order by a
//                  second launch instead of meeting in fp32 atomics (bit-reproducible weight gradients)
//   svit_debug_gemm_tn_plan : what any of these calls would launch, from the launch path's own check and planners
// (the forward / dgrad kernel svit_gemm_nt lives in gemm_nt.hip)
#include <algorithm>
#include <type_traits>
#include <vector>
#include "common.h"
#include "../../include/svit_hip.h"

namespace {

template <int B, int E, typename F>
__device__ __forceinline__ void tn_static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    tn_static_for<B + 1, E>(f);
  }
}

// ---------------------------------------------------------------------------------------
// TN kernel.  Both operands are [rows=m][cols] in LDS and read transposed (ds_read_b64_tr_b16).  Two tile shapes,
// TnSmallD / TnBigD = TnDma<RB, WN, WK, BM, NS> below -- the one description the kernels and the host planners read:
//   TnSmallD <1, 4, 1, 64>: out tile 128(n) x 96(k), 4 waves of 32 x 96, 64 reduction rows per step.
//   TnBigD <2, 2, 2, 32> (round 2): out tile 128 x 192, 2 x 2 waves of 64 x 96, 32 rows per step --
//     the same 12 MFMAs per wave and step from 20 KB of staged operands instead of 28 KB
//     (rocprofv3 round 2: the grouped launch fetched 687 MB against ~320 MB of operands and the
//     CU's vector-memory path, not the matrix pipe, sets the pace), and 10 transposed LDS reads
//     per 6 MFMAs instead of 8 per 3.
// ---------------------------------------------------------------------------------------
// One workgroup's share: rows [m_begin, m_end) of the reduction for the TN x TK tile at (n0, k0).
// Round 3: through an LDS-DMA ring.  The round-2 body (git history) staged both operands
// through registers (global_load -> VGPR -> ds_write_b128: 20-28 KB of LDS stores per 12 MFMAs,
// half of them behind bounds-check branches) and takes one __syncthreads per 12 MFMAs with the
// transposed reads left to the compiler.  Here:
//   * A / B stages [m][cols] arrive by buffer-descriptor LDS-DMA (no VGPR staging, no ds_write, no
//     per-piece address arithmetic: per-lane byte offsets are stage-invariant, the stage's first
//     row is the scalar offset), NS stages deep behind a counted vmcnt and ONE raw barrier per stage;
//   * rows are unpadded (a DMA writes 1 KB linearly); the 4 rows x 64 B of a transposed read land on
//     disjoint banks through a swizzle of the 64-byte blocks on the per-lane SOURCE address
//     (A, 256-B rows: block ^ (row & 3); B, 384-B rows: block ^ ((row >> 1) & 1); 192-B rows skew by
//     themselves) and the same swizzle in the read address;
//   * the transposed fragment reads of k-step s+1 are issued (inline asm) before the MFMAs of k-step
//     s and released by counted lgkmcnt waits;
//   * a ragged last stage (rows past m_end) is fetched through clamped rows and its A rows are
//     zeroed in LDS; columns past N / K are clamped in the source address (their products are
//     never stored).
template <int RB_, int WN_, int WK_, int BM_, int NS_>
struct TnDma {
  static constexpr int RB = RB_, WN = WN_, WK = WK_, BM = BM_, NS = NS_;
  static constexpr int TN = 32 * RB * WN, TK = 96 * WK;
  static constexpr int ROWA = TN * 2, ROWB = TK * 2;             // 256 B; 192 / 384 B
  static constexpr int A_BYTES = BM * ROWA, B_BYTES = BM * ROWB, STAGE = A_BYTES + B_BYTES;
  static constexpr int A_INSTR = A_BYTES / 1024, B_INSTR = B_BYTES / 1024;
  static constexpr int NW = WN * WK, NT = NW * 64;               // waves / threads of a workgroup
  static constexpr int PER = (A_INSTR + B_INSTR) / NW;           // DMA instructions per wave and stage
  static_assert((A_INSTR + B_INSTR) % NW == 0, "every wave issues the same number of pieces");
  __host__ __device__ static constexpr int swz_a(int row) { return row & 3; }
  // 384-byte rows alternate between two bank offsets (one swizzle bit), rows that are a multiple of 256 bytes all
  // start on the same bank (two bits, like A), 192-byte rows skew by themselves
  __host__ __device__ static constexpr int swz_b(int row) { return ROWB == 384 ? ((row >> 1) & 1) : (ROWB % 256 == 0 ? (row & 3) : 0); }
};
using TnSmallD = TnDma<1, 4, 1, 64, 2>;     // 128 x 96 tiles, 64 rows per stage, 2 stages (56 KB)
#ifndef SVIT_TN_BIG_NS      // ring depth of the 128 x 192 tile (diagnostic builds: 4 = 80 KB, still two workgroups per CU)
#define SVIT_TN_BIG_NS 3
#endif
#ifndef SVIT_TN_BIG_BM      // reduction rows per stage of the 128 x 192 tile (diagnostic builds: 64 with 2 stages = half the barriers)
#define SVIT_TN_BIG_BM 32
#endif
using TnBigD = TnDma<2, 2, 2, SVIT_TN_BIG_BM, SVIT_TN_BIG_NS>;       // 128 x 192 tiles, 32 rows per stage, 3 stages (60 KB)
constexpr int TN_DMA_LDS = 2 * TnSmallD::STAGE > SVIT_TN_BIG_NS * TnBigD::STAGE ? 2 * TnSmallD::STAGE : SVIT_TN_BIG_NS * TnBigD::STAGE;

template <int OFF>
__device__ __forceinline__ void tn_read_tr(s16x4_t& d, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=&v"(d) : "v"(addr), "i"(OFF) : "memory");
}

// SLAB selects the flush.  false: the fp32 tile (and the bias column sums) meet the other row splits in atomicAdd on
// dW / dbias.  true: dW is this workgroup's OWN slab of TN x lddw floats (lddw = the slab's column count) and dbias
// its own TN bias partials; both are written with plain stores and summed in split order by tn_slab_reduce_kernel.
// Slab element (row, col) of the tile sits at ((row / 4) * lddw + col) * 4 + row % 4: the four accumulator rows a lane
// holds for one column are one 16-byte store, and the lanes of a half-wave cover 32 adjacent columns (512 B).
template <class C, bool SLAB>
__device__ __forceinline__ void tn_tile_dma(unsigned char* lds, const bf16_t* __restrict__ A, int lda,
                                            const bf16_t* __restrict__ B, int ldb,
                                            float* __restrict__ dW, int lddw, int M, int N, int K, int n0,
                                            int k0, int m_begin, int m_end,
                                            float* __restrict__ dbias, bool bias_tile) {
#if __HIP_DEVICE_COMPILE__
  constexpr int RB = C::RB, BM = C::BM, NS = C::NS, PER = C::PER;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave / C::WK, wk = wave % C::WK;
  if (m_begin >= m_end) return;
  // ---- per-lane source offsets of this wave's DMA pieces (stage-invariant)
  // (a wave's first A_INSTR / 4 pieces are A pieces wave, wave + 4, ...; the rest B pieces)
  constexpr int NW = C::NW, NT = C::NT;
  constexpr int PA = C::A_INSTR / NW;
  static_assert(C::A_INSTR % NW == 0 && C::B_INSTR % NW == 0, "pieces split evenly over the waves");
  unsigned voff[PER];
  const int na8 = (N - n0 + 7) / 8, nb8 = (K - k0 + 7) / 8;     // valid 16-byte column chunks of this tile
  auto piece = [&](int i, bool a) { return wave + NW * (a ? i : i - PA); };
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const bool a = i < PA;
    const int o = piece(i, a) * 1024 + lane * 16;                // byte offset inside the A / B image
    const int rowb = a ? C::ROWA : C::ROWB;
    const int row = o / rowb, inrow = o % rowb;
    const int pb = inrow >> 6, c16 = (inrow >> 4) & 3;
    const int lb = pb ^ (a ? C::swz_a(row) : C::swz_b(row));     // logical 64-byte block
    const int ch = min(lb * 4 + c16, (a ? na8 : nb8) - 1);       // logical 16-byte chunk, clamped into the matrix
    voff[i] = (unsigned)(row * (a ? lda : ldb) + (a ? n0 : k0) + ch * 8) * 2u;
  }
  const auto ars = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)std::min<size_t>((size_t)M * lda * 2, 0x7fffffffu), 0x00020000);
  const auto brs = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)std::min<size_t>((size_t)M * ldb * 2, 0x7fffffffu), 0x00020000);
  const int nsteps = (m_end - m_begin + BM - 1) / BM;
  auto issue = [&](int s) {
    unsigned char* st = lds + (s % NS) * C::STAGE;
    const int m0 = m_begin + s * BM;
    const int valid = m_end - m0;               // >= BM except in a ragged last stage (uniform)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const bool a = i < PA;
      unsigned vo = voff[i];
      if (valid < BM) {                         // rows past m_end re-read the last valid row
        const int row = (piece(i, a) * 1024 + lane * 16) / (a ? C::ROWA : C::ROWB);
        vo -= (unsigned)(row - min(row, valid - 1)) * (a ? lda : ldb) * 2u;
      }
      unsigned char* dst = st + (a ? 0 : C::A_BYTES) + piece(i, a) * 1024;
      if (a)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ars, (__attribute__((address_space(3))) void*)dst, 16, vo,
                                                 (unsigned)m0 * lda * 2u, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(brs, (__attribute__((address_space(3))) void*)dst, 16, vo,
                                                 (unsigned)m0 * ldb * 2u, 0, 0);
    }
  };
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nsteps) issue(s);

  f32x16_t acc[RB][3];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // fused bias gradient: column sums of A (= dY) ride along on the k-tile-0 blocks: thread ->
  // (row tid / 16 (+16, ...), logical 16-byte chunk tid % 16), 8 running sums
  const bool do_bias = (dbias != nullptr) && bias_tile;
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // transposed-read addressing: lane -> (half hh, column group cg, (q, pp));
  // rows of one read are 8 hh + q (+ 4 for the second), so the swizzle term is a per-lane constant
  const int hh = lane >> 5, cg = (lane >> 4) & 1, ii = lane & 15, q = ii >> 2, pp = ii & 3;
  const unsigned lds0 = (unsigned)(size_t)lds;
  unsigned a_addr[RB], b_addr[3];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int col = wn * 32 * RB + i * 32 + 16 * cg + 4 * pp;          // n column of the tile
    a_addr[i] = lds0 + (8 * hh + q) * C::ROWA + (((col >> 5) ^ C::swz_a(q)) << 6) + (col & 31) * 2;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int col = wk * 96 + j * 32 + 16 * cg + 4 * pp;               // k column of the tile
    // rows 8 hh + q and 8 hh + q + 4: (row >> 1) & 1 = (q >> 1) & 1 for both
    b_addr[j] = lds0 + C::A_BYTES + (8 * hh + q) * C::ROWB + (((col >> 5) ^ C::swz_b(q)) << 6) + (col & 31) * 2;
  }
  constexpr int KS = BM / 16;
  for (int s = 0; s < nsteps; ++s) {
    if (s + NS - 2 < nsteps - 0 && NS > 2 && s + 1 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * PER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // everyone's share of stage s has landed; everyone is done with stage s-1
    if (s + NS - 1 < nsteps) issue(s + NS - 1);
    const unsigned so = (unsigned)((s % NS) * C::STAGE);
    if (m_begin + (s + 1) * BM > m_end) {      // ragged last stage: the re-read rows count nothing
      const int valid = m_end - (m_begin + s * BM);
      for (int c = tid; c < (BM - valid) * (C::ROWA / 16); c += NT)
        *(uint4*)(lds + so + valid * C::ROWA + c * 16) = make_uint4(0, 0, 0, 0);
      __syncthreads();
    }
    if (do_bias) {
      constexpr int CPR = C::TN / 8, RP = NT / CPR;       // 16-byte chunks per A row; rows per pass of the workgroup
#pragma unroll
      for (int r0 = 0; r0 < BM; r0 += RP) {
        const int row = r0 + tid / CPR, lc = tid % CPR;
        uint4 u;    // (asm: a compiler-visible LDS load behind an LDS-DMA draws an s_waitcnt vmcnt(0))
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(u)
                     : "v"(lds0 + so + row * C::ROWA + ((((lc >> 2) ^ C::swz_a(row))) << 6) + (lc & 3) * 16) : "memory");
        bsum[0] += lo_bf16(u.x); bsum[1] += hi_bf16(u.x);
        bsum[2] += lo_bf16(u.y); bsum[3] += hi_bf16(u.y);
        bsum[4] += lo_bf16(u.z); bsum[5] += hi_bf16(u.z);
        bsum[6] += lo_bf16(u.w); bsum[7] += hi_bf16(u.w);
      }
    }
    // fragments of k-step ks: RB A fragments + 3 B fragments, two transposed reads each
    s16x4_t fl[2][RB + 3], fh[2][RB + 3];
    auto rd = [&](auto KS_, auto BUF_) {
      constexpr int ks = decltype(KS_)::value, buf = decltype(BUF_)::value;
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        tn_read_tr<ks * 16 * C::ROWA>(fl[buf][i], a_addr[i] + so);
        tn_read_tr<(ks * 16 + 4) * C::ROWA>(fh[buf][i], a_addr[i] + so);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        tn_read_tr<ks * 16 * C::ROWB>(fl[buf][RB + j], b_addr[j] + so);
        tn_read_tr<(ks * 16 + 4) * C::ROWB>(fh[buf][RB + j], b_addr[j] + so);
      }
    };
    rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    tn_static_for<0, KS>([&](auto KS_) {
      constexpr int ks = decltype(KS_)::value, cur = ks & 1;
      if constexpr (ks + 1 < KS) {
        rd(std::integral_constant<int, ks + 1>{}, std::integral_constant<int, (cur ^ 1)>{});
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (RB + 3)) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int f = 0; f < RB + 3; ++f) asm volatile("" : "+v"(fl[cur][f]), "+v"(fh[cur][f]));
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < RB; ++i)
          acc[i][j] = mfma32(make_bf16x8(fl[cur][i], fh[cur][i]), make_bf16x8(fl[cur][RB + j], fh[cur][RB + j]), acc[i][j]);
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  if constexpr (SLAB) {
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int tcol = wk * 96 + j * 32 + (lane & 31);
        if (k0 + tcol >= K) continue;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int trow = wn * 32 * RB + i * 32 + acc_row(4 * r4, lane);      // first of four adjacent rows
          if (n0 + trow < N)
            *(float4*)(dW + ((size_t)(trow >> 2) * lddw + tcol) * 4) =
                make_float4(acc[i][j][4 * r4], acc[i][j][4 * r4 + 1], acc[i][j][4 * r4 + 2], acc[i][j][4 * r4 + 3]);
        }
      }
  } else {
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int col = k0 + wk * 96 + j * 32 + (lane & 31);
      if (col >= K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n0 + wn * 32 * RB + i * 32 + acc_row(r, lane);
#ifdef SVIT_TN_FLUSH_PLAIN     // (diagnostic builds, TIMING ONLY: what the fp32 atomic flush costs against plain stores)
        if (row < N) dW[(size_t)row * lddw + col] = acc[i][j][r];
#else
        if (row < N) atomicAdd(dW + (size_t)row * lddw + col, acc[i][j][r]);
#endif
      }
    }
  }
  if (do_bias) {  // RP threads share a column chunk: reduce through LDS, one atomic per column
    constexpr int CPR = C::TN / 8, RP = NT / CPR;
    static_assert(BM % RP == 0, "whole passes over a stage");
    __syncthreads();                  // (the ring is read by nobody any more)
    float* red = (float*)lds;  // [RP][TN]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[(tid / CPR) * C::TN + (tid % CPR) * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < C::TN && n0 + tid < N) {
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < RP; ++g) sum += red[g * C::TN + tid];
      if constexpr (SLAB) dbias[tid] = sum;
      else atomicAdd(dbias + n0 + tid, sum);
    }
  }
#endif
}


// the single-GEMM entry point: 128 x 96 tiles, grid (n tile, k tile, row split)
__global__ __launch_bounds__(256) void gemm_tn_kernel(const bf16_t* __restrict__ A, int lda,
                                                      const bf16_t* __restrict__ B, int ldb,
                                                      float* __restrict__ dW, int lddw, int M,
                                                      int N, int K, int rows_per_split,
                                                      float* __restrict__ dbias) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[TN_DMA_LDS];
  const int m_begin = blockIdx.z * rows_per_split;
  tn_tile_dma<TnSmallD, false>(lds, A, lda, B, ldb, dW, lddw, M, N, K, blockIdx.x * TnSmallD::TN, blockIdx.y * TnSmallD::TK,
                               m_begin, min(M, m_begin + rows_per_split), dbias, blockIdx.y == 0);
}

// Grouped launch: up to SVIT_TN_GROUP_MAX independent weight-gradient GEMMs share one grid, so
// the machine-wide accumulator flush (every resident workgroup atomically adds its 128x96 fp32
// tile: ~25 MB per launch, the dominant cost of a short-reduction wgrad) is paid once per group
// instead of once per GEMM.
struct TnGroup {
  svit_tn_problem p[SVIT_TN_GROUP_MAX];
  int first_block[SVIT_TN_GROUP_MAX + 1];
  int tiles_n[SVIT_TN_GROUP_MAX];
  int tiles[SVIT_TN_GROUP_MAX];
  int rows_per_split[SVIT_TN_GROUP_MAX];
  int big[SVIT_TN_GROUP_MAX];          // 1: 128 x 192 tiles (TnBigD), 0: 128 x 96 (TnSmallD)
  int count;
};

// ---------------------------------------------------------------------------------------
// Slab form (svit_gemm_tn_grouped_slab): the same grid and the same main loop, but no two workgroups
// ever write one address.  Workgroup (problem, split, tile) -- its LOGICAL id, not the XCD-remapped
// block index -- stores its fp32 tile into slab number `local` of its problem and, on k-tile 0 of a
// problem with a bias, its 128 bias partials into the second region; tn_slab_reduce_kernel, launched
// right behind on the same stream, sums the splits of every output element in index order and adds
// the sum to dW / dbias with one plain read-modify-write.  One writer per element: the result does
// not depend on how the workgroups were scheduled.
struct TnSlabs {
  long long tile_off[SVIT_TN_GROUP_MAX];   // float offset of the problem's slab 0 (slab = 128 x w floats)
  long long bias_off[SVIT_TN_GROUP_MAX];   // float offset of its bias partials [split][n tile][128]
  int red_first[SVIT_TN_GROUP_MAX + 1];    // first block of the reduce grid
  int w[SVIT_TN_GROUP_MAX];                // slab columns: min(tile width, K rounded up to 32)
};
constexpr int TN_RED_THREADS = 128;
static_assert(TnSmallD::TN == 128 && TnBigD::TN == 128, "slabs and bias partials are 128 rows");

// One workgroup of a grouped launch, both forms: which (problem, split, tile) it is, where its flush goes, and its tile
// through the body of the problem's tile shape.  SLAB (sl, ws): the flush goes to the workgroup's own slab and bias partials.
template <bool SLAB>
__device__ __forceinline__ void tn_grouped_workgroup(unsigned char* lds, const TnGroup& g, const TnSlabs* sl, float* ws) {
  // Logical ids are (problem, split)-major, tile-minor: the tiles of one split walk the SAME
  // rows in lock-step and re-read each other's A / B column panels (A once per k-tile, B once
  // per n-tile).  Consecutive logical ids are therefore placed on ONE XCD, so those re-reads
  // hit its L2 instead of crossing the fabric (rocprofv3 FETCH_SIZE before: 810 MB per launch
  // against ~230 MB of operands -- the kernel ran at HBM speed).
  const int nwg = gridDim.x, lin = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  int pi = 0;
  const int bid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
#pragma unroll
  for (int i = 1; i < SVIT_TN_GROUP_MAX; ++i)
    if (i < g.count && bid >= g.first_block[i]) pi = i;
  const int local = bid - g.first_block[pi];
  const int tile = local % g.tiles[pi], split = local / g.tiles[pi];
  const svit_tn_problem& p = g.p[pi];
  const int tn = tile % g.tiles_n[pi], tk = tile / g.tiles_n[pi];
  const int m_begin = split * g.rows_per_split[pi];
  float *out, *bias;
  int ld;
  if constexpr (SLAB) {
    ld = sl->w[pi];
    out = ws + sl->tile_off[pi] + (long long)local * (128 * ld);
    bias = p.dbias ? ws + sl->bias_off[pi] + (long long)(split * g.tiles_n[pi] + tn) * 128 : nullptr;
  } else {
    out = p.dW, ld = p.lddw, bias = p.dbias;
  }
  if (g.big[pi])
    tn_tile_dma<TnBigD, SLAB>(lds, (const bf16_t*)p.A, p.lda, (const bf16_t*)p.B, p.ldb, out, ld, p.M, p.N, p.K,
                              tn * TnBigD::TN, tk * TnBigD::TK, m_begin, min(p.M, m_begin + g.rows_per_split[pi]),
                              bias, tk == 0);
  else
    tn_tile_dma<TnSmallD, SLAB>(lds, (const bf16_t*)p.A, p.lda, (const bf16_t*)p.B, p.ldb, out, ld, p.M, p.N, p.K,
                                tn * TnSmallD::TN, tk * TnSmallD::TK, m_begin, min(p.M, m_begin + g.rows_per_split[pi]),
                                bias, tk == 0);
}

#ifndef SVIT_TN_WPE         // waves per SIMD the grouped kernel is compiled for (diagnostic builds: 3 with SVIT_TN_BIG_NS=2 = three workgroups per CU)
#define SVIT_TN_WPE 2
#endif
__global__ __launch_bounds__(256, SVIT_TN_WPE) void gemm_tn_grouped_kernel(const TnGroup g) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[TN_DMA_LDS];
  tn_grouped_workgroup<false>(lds, g, nullptr, nullptr);
}

__global__ __launch_bounds__(256, SVIT_TN_WPE) void gemm_tn_grouped_slab_kernel(const TnGroup g, const TnSlabs sl,
                                                                               float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[TN_DMA_LDS];
  tn_grouped_workgroup<true>(lds, g, &sl, ws);
}

// thread -> (four adjacent rows, one column) of one problem's dW, consecutive lanes on consecutive
// columns; behind the K * ceil(N / 4) matrix threads of a problem with a bias, ceil(N / 4) threads
// take four bias columns each.  Every slab read is one 16-byte load.
__global__ __launch_bounds__(TN_RED_THREADS) void tn_slab_reduce_kernel(const TnGroup g, const TnSlabs sl,
                                                                        const float* __restrict__ ws) {
#pragma clang fp reassociate(off)      // (-ffast-math: the sum below is in split order)
  int pi = 0;
  const int blk = blockIdx.x;
#pragma unroll
  for (int i = 1; i < SVIT_TN_GROUP_MAX; ++i)
    if (i < g.count && blk >= sl.red_first[i]) pi = i;
  const svit_tn_problem& p = g.p[pi];
  const int N = p.N, K = p.K, rg_n = (N + 3) >> 2;
  const int tiles = g.tiles[pi], tiles_n = g.tiles_n[pi];
  const int S = (g.first_block[pi + 1] - g.first_block[pi]) / tiles;
  const long long e = (long long)(blk - sl.red_first[pi]) * TN_RED_THREADS + threadIdx.x;
  const long long nmat = (long long)rg_n * K;
  const float* src;
  long long stride;       // floats between the same element of consecutive splits
  if (e < nmat) {
    const int rg = (int)(e / K), col = (int)(e - (long long)rg * K);
    const int tk_w = g.big[pi] ? TnBigD::TK : TnSmallD::TK, w = sl.w[pi];
    const int tile = (col / tk_w) * tiles_n + rg / 32;
    stride = (long long)tiles * (128 * w);
    src = ws + sl.tile_off[pi] + (long long)tile * (128 * w) + ((long long)(rg % 32) * w + col % tk_w) * 4;
  } else if (p.dbias && e < nmat + rg_n) {
    const int n = (int)(e - nmat) * 4;
    stride = (long long)tiles_n * 128;
    src = ws + sl.bias_off[pi] + (long long)(n / 128) * 128 + n % 128;
  } else {
    return;
  }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int s = 0;
  for (; s + 8 <= S; s += 8) {       // eight loads in flight, added in index order
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(src + (s + u) * stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) { a0 += v[u].x; a1 += v[u].y; a2 += v[u].z; a3 += v[u].w; }
  }
  for (; s < S; ++s) {
    const float4 v = *(const float4*)(src + s * stride);
    a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
  }
  if (e < nmat) {
    const int rg = (int)(e / K), col = (int)(e - (long long)rg * K), row = rg * 4;
    float* d = p.dW + (size_t)row * p.lddw + col;
    d[0] += a0;
    if (row + 1 < N) d[p.lddw] += a1;
    if (row + 2 < N) d[2 * (size_t)p.lddw] += a2;
    if (row + 3 < N) d[3 * (size_t)p.lddw] += a3;
  } else {
    const int n = (int)(e - nmat) * 4;
    float* d = p.dbias + n;
    d[0] += a0;
    if (n + 1 < N) d[1] += a1;
    if (n + 2 < N) d[2] += a2;
    if (n + 3 < N) d[3] += a3;
  }
}

__global__ void colsum_kernel(const bf16_t* __restrict__ A, int lda, float* __restrict__ out,
                              int M, int N, int rows_per_block) {
  // block (64 x 4): lane -> 2 adjacent columns (one dword), 4 row phases; grid.x = column
  // groups of 128, grid.y = row chunks
  const int col = (blockIdx.x * 64 + threadIdx.x) * 2;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  float s0 = 0.f, s1 = 0.f;
  if (col < N) {
    for (int r = r0 + threadIdx.y; r < r1; r += 4) {
      const uint32_t w = *(const uint32_t*)(A + (size_t)r * lda + col);
      s0 += lo_bf16(w);
      s1 += hi_bf16(w);
    }
  }
  __shared__ float red[4][64][2];
  red[threadIdx.y][threadIdx.x][0] = s0;
  red[threadIdx.y][threadIdx.x][1] = s1;
  __syncthreads();
  if (threadIdx.y == 0 && col < N) {
    for (int k = 1; k < 4; ++k) {
      s0 += red[k][threadIdx.x][0];
      s1 += red[k][threadIdx.x][1];
    }
    atomicAdd(out + col, s0);
    if (col + 1 < N) atomicAdd(out + col + 1, s1);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Host side: check -> plan -> launch, once each.  tn_check is the only argument check; tn_single_plan (the stand-alone
// svit_gemm_tn) and tn_plan (every grouped form) are the only planners, pure functions of the shapes and the knob
// table; tn_chunks is the only walk over a problem list.  svit_debug_gemm_tn_plan answers from the same three, so
// what it reports is what a launch runs.
// ---------------------------------------------------------------------------------------
struct TnTileDims { int tn, tk, bm; };       // tile rows (n), tile columns (k), reduction rows per stage
static constexpr TnTileDims tn_dims(int big) {
  return big ? TnTileDims{TnBigD::TN, TnBigD::TK, TnBigD::BM} : TnTileDims{TnSmallD::TN, TnSmallD::TK, TnSmallD::BM};
}
static constexpr int tn_ceil(long a, long b) { return (int)((a + b - 1) / b); }

static int tn_check(const svit_tn_problem& p) {
  if (!p.A || !p.B || !p.dW) return SVIT_ERR_ARG;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return SVIT_ERR_SHAPE;
  if (p.lda % 8 != 0 || p.ldb % 8 != 0 || p.lda < p.N || p.ldb < p.K || p.lddw < p.K)
    return SVIT_ERR_ALIGN;
  if (((uintptr_t)p.A | (uintptr_t)p.B) & 15) return SVIT_ERR_ALIGN;
  return SVIT_OK;
}
static int tn_check_all(const svit_tn_problem* probs, int count) {
  if (!probs || count <= 0) return SVIT_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    const int rc = tn_check(probs[i]);
    if (rc) return rc;
  }
  return SVIT_OK;
}

// ---- the stand-alone GEMM: 128 x 96 tiles, its own split chooser (NOT the grouped planner's: other constants, other
// candidates -- folding the two would move kernels and splits)
struct TnSingle { int tiles_n, tiles_k, splits, rows_per_split; };
static int tn_single_splits(int M, int N, int K) {
  // Cost model fitted on MI355X (tools/bench_kernels.py tnsplit): a block needs ~0.85 us per
  // 64-row step, 512 blocks run concurrently, and every split adds the whole [N,K] fp32 tile
  // set with atomics at ~0.75 TB/s effective.  Take the split count minimising the sum.
  constexpr TnTileDims t = tn_dims(0);
  const int tiles = tn_ceil(N, t.tn) * tn_ceil(K, t.tk);
  const double atom_us = (double)N * K * 4.0 / 0.75e6;
  double best = 1e30;
  int splits = 1;
  static const int cand[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512};
  for (int ci = 0; ci < (int)(sizeof(cand) / sizeof(cand[0])); ++ci) {
    const int s = cand[ci];
    const long steps = ((M + s - 1) / s + t.bm - 1) / t.bm;
    if (steps < 2 && s > 1) break;
    const long rounds = ((long)tiles * s + 511) / 512;
    const double time = (double)rounds * steps * 0.85 + s * atom_us;
    if (time < best) { best = time; splits = s; }
  }
  return splits;
}
static TnSingle tn_single_plan(int M, int N, int K, int splits) {      // splits <= 0: the chooser's
  constexpr TnTileDims t = tn_dims(0);
  if (splits <= 0) splits = tn_single_splits(M, N, K);
  const int rows_per_split = tn_ceil(tn_ceil(M, splits), t.bm) * t.bm;
  return {tn_ceil(N, t.tn), tn_ceil(K, t.tk), tn_ceil(M, rows_per_split), rows_per_split};
}

extern "C" int svit_gemm_tn(const void* A, int lda, const void* B, int ldb, float* dW, int lddw,
                            int M, int N, int K, int splits, float* dbias, void* stream) {
  const svit_tn_problem p = {A, B, dW, dbias, lda, ldb, lddw, M, N, K};
  const int rc = tn_check(p);
  if (rc) return rc;
  const TnSingle s = tn_single_plan(M, N, K, splits);
  hipLaunchKernelGGL(gemm_tn_kernel, dim3(s.tiles_n, s.tiles_k, s.splits), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)A, lda, (const bf16_t*)B, ldb, dW, lddw, M, N, K, s.rows_per_split, dbias);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

// ---- the grouped forms: tn_plan = tile rule per problem -> chunk-length search over the group -> fill.
// The knobs: SVIT_K_TN_TILE (the tile mode), SVIT_K_TN_STEP_US_X100 (one 64-row step of a workgroup, 512 resident) and
// SVIT_K_TN_ATOMIC_TBS_X100 (effective fp32 atomic flush rate) of the knob table in common.h.

// Tile mode 2 = 128x192 everywhere since the in-step A/B of round 3 (13.46 -> 13.30 ms per step,
// profiles/r03_tn_tile_modes.txt: inside the step the operands come from HBM, not from the Infinity Cache an isolated
// loop keeps them in, and fewer, fatter tiles re-read less).  The 128x384 forms (eight waves, four waves, ring with loader
// waves) and the XCD-packed placement table of round 4 measured level or behind (profiles/r04_tn_l2_counters.txt) and
// live on only as tools/diag/variants/gemm_tn_r04_forms.hip.
static int tn_tile_rule(const svit_tn_problem& p, int mode) {
  // mode 1: 128 x 192 tiles where they are fully used (K a multiple of 192) and measured faster with the
  // round-3 LDS-DMA body (tools/bench_kernels.py tngroup, profiles/r03_tn_tile_modes.txt): the
  // M = 3656 groups of blocks 14-15 (-5 / -11 %) and the M = 50696 groups of blocks 2-3 (-16 / -22 %);
  // not the M = 13064 groups of blocks 4-13 (+10 %: the doubled fp32 tile a workgroup flushes with
  // atomics outweighs the smaller operand traffic) nor the M = 201224 group of block 0 (+11 %)
  const bool whole = p.K % TnBigD::TK == 0 && p.N >= 128;
  return mode == 1 ? (whole && (p.M <= 4096 || (p.M >= 32768 && p.M < 131072))) : mode == 3 ? whole : (mode == 2);
}

// Every problem is cut into chunks of `steps` steps (64 reduction rows on 128 x 96 tiles, 32 on
// 128 x 192: the same 12 MFMAs per wave), so all workgroups run about equally long.  Same
// fitted model as svit_gemm_tn: 0.85 us per step with 512 resident workgroups, plus the atomic
// flush of one fp32 tile per workgroup at ~0.75 TB/s.  Reads g.p, g.big, g.tiles; ordered: nothing is cut.
static long tn_chunk_steps(const TnGroup& g, int ordered, double step_us, double atomic_tbs) {
  constexpr long slots = 512;      // resident 4-wave workgroups the planner counts on
  long st[SVIT_TN_GROUP_MAX], max_steps = 1;
  for (int i = 0; i < g.count; ++i) {
    st[i] = tn_ceil(g.p[i].M, tn_dims(g.big[i]).bm);
    if (st[i] > max_steps) max_steps = st[i];
  }
  if (ordered) return max_steps;
  double best = 1e30;
  long best_steps = max_steps;
  for (long steps = 2; steps <= max_steps; steps += (steps < 32 ? 1 : steps / 16)) {
    long blocks = 0;
    double flush = 0.0;
    for (int i = 0; i < g.count; ++i) {
      const TnTileDims t = tn_dims(g.big[i]);
      const long nb = (long)g.tiles[i] * ((st[i] + steps - 1) / steps);
      blocks += nb;
      flush += (double)nb * ((double)t.tn * t.tk * 4.0);
    }
    const double time = (double)((blocks + slots - 1) / slots) * steps * step_us + flush / (atomic_tbs * 1e6);
    if (time < best) { best = time; best_steps = steps; }
  }
  return best_steps;
}

// The ONE planner of the grouped forms: fills g for problems [0, n) (n <= SVIT_TN_GROUP_MAX) and returns the grid size.
static int tn_plan(const svit_tn_problem* probs, int n, int ordered, TnGroup& g) {
  const int mode = svit_knob(SVIT_K_TN_TILE);
  g.count = n;
  for (int i = 0; i < n; ++i) {
    g.p[i] = probs[i];
    g.big[i] = tn_tile_rule(probs[i], mode);
    const TnTileDims t = tn_dims(g.big[i]);
    g.tiles_n[i] = tn_ceil(probs[i].N, t.tn);
    g.tiles[i] = g.tiles_n[i] * tn_ceil(probs[i].K, t.tk);
  }
  const long steps = tn_chunk_steps(g, ordered, svit_knob(SVIT_K_TN_STEP_US_X100) * 0.01,
                                    svit_knob(SVIT_K_TN_ATOMIC_TBS_X100) * 0.01);
  int total = 0;
  for (int i = 0; i < n; ++i) {      // the fill: rows per split, (problem, split)-major block ranges
    g.rows_per_split[i] = (int)steps * tn_dims(g.big[i]).bm;
    g.first_block[i] = total;
    total += g.tiles[i] * tn_ceil(g.p[i].M, g.rows_per_split[i]);
  }
  for (int i = n; i <= SVIT_TN_GROUP_MAX; ++i) g.first_block[i] = total;
  return total;
}

// slab regions of a planned group -> floats of workspace (every offset a multiple of 4 floats)
static int64_t tn_slab_layout(const TnGroup& g, TnSlabs& sl) {
  long long off = 0;
  int red = 0;
  for (int i = 0; i < g.count; ++i) {
    const int tk = tn_dims(g.big[i]).tk, k32 = (g.p[i].K + 31) / 32 * 32;
    sl.w[i] = k32 < tk ? k32 : tk;
    sl.tile_off[i] = off;
    off += (long long)(g.first_block[i + 1] - g.first_block[i]) * (128 * sl.w[i]);
  }
  for (int i = 0; i < g.count; ++i) {
    sl.bias_off[i] = off;
    const int splits = (g.first_block[i + 1] - g.first_block[i]) / g.tiles[i];
    if (g.p[i].dbias) off += (long long)splits * g.tiles_n[i] * 128;
    const long long rg_n = (g.p[i].N + 3) / 4, thr = rg_n * g.p[i].K + (g.p[i].dbias ? rg_n : 0);
    sl.red_first[i] = red;
    red += (int)((thr + TN_RED_THREADS - 1) / TN_RED_THREADS);
  }
  for (int i = g.count; i < SVIT_TN_GROUP_MAX; ++i) sl.tile_off[i] = sl.bias_off[i] = 0, sl.w[i] = 0;
  for (int i = g.count; i <= SVIT_TN_GROUP_MAX; ++i) sl.red_first[i] = red;
  return off;
}

// The ONE walk over a problem list: checked, cut into launch groups of SVIT_TN_GROUP_MAX, each planned once (with its
// slab layout where wanted).  Every launch form and both queries go through it.
struct TnChunk {
  TnGroup g;
  TnSlabs sl;                // (slabs only)
  int grid;
  int64_t slab_floats;       // (slabs only, else 0)
};
static int tn_chunks(const svit_tn_problem* probs, int count, int ordered, bool slabs, std::vector<TnChunk>& chunks) {
  const int rc = tn_check_all(probs, count);
  if (rc) return rc;
  chunks.resize((count + SVIT_TN_GROUP_MAX - 1) / SVIT_TN_GROUP_MAX);
  for (size_t c = 0; c < chunks.size(); ++c) {
    const int base = (int)c * SVIT_TN_GROUP_MAX;
    chunks[c].grid = tn_plan(probs + base, std::min(count - base, SVIT_TN_GROUP_MAX), ordered, chunks[c].g);
    chunks[c].slab_floats = slabs ? tn_slab_layout(chunks[c].g, chunks[c].sl) : 0;
  }
  return SVIT_OK;
}
static int64_t tn_slab_need(const std::vector<TnChunk>& chunks) {      // every chunk reuses the workspace from offset 0
  int64_t need = 0;
  for (const TnChunk& c : chunks) need = std::max(need, c.slab_floats);
  return need;
}

// ordered != 0: no problem is cut along its reduction rows, so every element of every dW
// receives exactly ONE atomic add -- the weight gradients are bit-reproducible (a debugging /
// regression-diff mode: few workgroups, several times slower than the split form).
extern "C" int svit_gemm_tn_grouped_ex(const svit_tn_problem* probs, int count, int ordered, void* stream) {
  std::vector<TnChunk> chunks;
  const int rc = tn_chunks(probs, count, ordered, false, chunks);
  if (rc) return rc;
  for (const TnChunk& c : chunks) {
    hipLaunchKernelGGL(gemm_tn_grouped_kernel, dim3(c.grid), dim3(256), 0, (hipStream_t)stream, c.g);
    SVIT_LAUNCH_CHECK();
  }
  return SVIT_OK;
}
extern "C" int svit_gemm_tn_grouped(const svit_tn_problem* probs, int count, void* stream) {
  return svit_gemm_tn_grouped_ex(probs, count, 0, stream);
}

extern "C" int64_t svit_gemm_tn_grouped_workspace(const svit_tn_problem* probs, int count) {
  std::vector<TnChunk> chunks;
  const int rc = tn_chunks(probs, count, 0, true, chunks);
  return rc ? rc : tn_slab_need(chunks);
}

extern "C" int svit_gemm_tn_grouped_slab(const svit_tn_problem* probs, int count, float* workspace,
                                         int64_t workspace_floats, void* stream) {
  std::vector<TnChunk> chunks;
  const int rc = tn_chunks(probs, count, 0, true, chunks);
  if (rc) return rc;
  if (!workspace || workspace_floats < tn_slab_need(chunks)) return SVIT_ERR_ARG;
  if ((uintptr_t)workspace & 15) return SVIT_ERR_ALIGN;
  // the chunk's reduce is behind its GEMM and in front of the next chunk's GEMM on the one stream
  for (const TnChunk& c : chunks) {
    hipLaunchKernelGGL(gemm_tn_grouped_slab_kernel, dim3(c.grid), dim3(256), 0, (hipStream_t)stream, c.g, c.sl, workspace);
    SVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tn_slab_reduce_kernel, dim3(c.sl.red_first[SVIT_TN_GROUP_MAX]), dim3(TN_RED_THREADS), 0,
                       (hipStream_t)stream, c.g, c.sl, (const float*)workspace);
    SVIT_LAUNCH_CHECK();
  }
  return SVIT_OK;
}

// svit_gemm_tn_grouped_slab for the LEADING `launch_count` problems of a list that is checked and planned whole: the
// rest only takes part in the plan (its pointers are never followed).  A backward that stops above frozen blocks hands
// over the problems the full backward would have had in the same launch, and the leading ones get the full backward's
// row splits -- the planner cuts every problem of a launch by one step count found over all of them -- hence its
// weight gradients, bit for bit.  Logical workgroup ids are problem-major: the leading problems own the ids below
// first_block[lead], the reduce blocks below red_first[lead], and the XCD remap is a bijection for any grid size.
extern "C" int svit_gemm_tn_grouped_slab_lead(const svit_tn_problem* probs, int count, int launch_count,
                                              float* workspace, int64_t workspace_floats, void* stream) {
  if (launch_count < 1 || launch_count > count) return SVIT_ERR_ARG;
  std::vector<TnChunk> chunks;
  const int rc = tn_chunks(probs, count, 0, true, chunks);
  if (rc) return rc;
  if (!workspace || workspace_floats < tn_slab_need(chunks)) return SVIT_ERR_ARG;
  if ((uintptr_t)workspace & 15) return SVIT_ERR_ALIGN;
  for (size_t i = 0; i < chunks.size(); ++i) {
    const TnChunk& c = chunks[i];
    const int lead = std::min(launch_count - (int)i * SVIT_TN_GROUP_MAX, c.g.count);
    if (lead <= 0) break;
    hipLaunchKernelGGL(gemm_tn_grouped_slab_kernel, dim3(c.g.first_block[lead]), dim3(256), 0, (hipStream_t)stream, c.g,
                       c.sl, workspace);
    SVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tn_slab_reduce_kernel, dim3(c.sl.red_first[lead]), dim3(TN_RED_THREADS), 0, (hipStream_t)stream,
                       c.g, c.sl, (const float*)workspace);
    SVIT_LAUNCH_CHECK();
  }
  return SVIT_OK;
}

// What a call would launch (include/svit_hip.h has the layout): the check, planners and walk above, no HIP call.
extern "C" int svit_debug_gemm_tn_plan(const svit_tn_problem* probs, int count, int form, int arg, int64_t* out,
                                       int n_out) {
  if (form < 0 || form > 3 || !out || (form == 3 && count != 1)) return SVIT_ERR_ARG;
  std::vector<TnChunk> chunks;
  const int rc = form == 3 ? tn_check_all(probs, count) : tn_chunks(probs, count, form == 1, form == 2, chunks);
  if (rc) return rc;
  const int groups = form == 3 ? 1 : (int)chunks.size(), n = 2 + 3 * groups + 10 * count;
  if (n_out < n) return SVIT_ERR_ARG;
  int64_t* o = out;
  *o++ = groups;
  *o++ = tn_slab_need(chunks);
  if (form == 3) {
    const TnSingle s = tn_single_plan(probs[0].M, probs[0].N, probs[0].K, arg);
    const int64_t v[13] = {1, (int64_t)s.tiles_n * s.tiles_k * s.splits, 0,
                           0, s.tiles_n, s.tiles_k, s.rows_per_split, s.splits, 0, 0, 0, 0, 0};
    o = std::copy(v, v + 13, o);
  }
  for (const TnChunk& c : chunks) {
    const TnGroup& g = c.g;
    const bool slab = form == 2;
    const int64_t head[3] = {g.count, c.grid, slab ? c.sl.red_first[SVIT_TN_GROUP_MAX] : 0};
    o = std::copy(head, head + 3, o);
    for (int i = 0; i < g.count; ++i) {
      const int64_t v[10] = {g.big[i], g.tiles_n[i], g.tiles[i] / g.tiles_n[i], g.rows_per_split[i],
                             (g.first_block[i + 1] - g.first_block[i]) / g.tiles[i], g.first_block[i],
                             slab ? c.sl.w[i] : 0, slab ? c.sl.tile_off[i] : 0, slab ? c.sl.bias_off[i] : 0,
                             slab ? c.sl.red_first[i] : 0};
      o = std::copy(v, v + 10, o);
    }
  }
  return (int)(o - out);
}

extern "C" int svit_colsum_bf16(const void* A, int lda, float* out, int M, int N, void* stream) {
  if (!A || !out || M <= 0 || N <= 0 || (N & 1) || (lda & 1)) return SVIT_ERR_ARG;
  const int col_groups = (N + 127) / 128;
  int row_chunks = 2048 / col_groups;
  if (row_chunks < 1) row_chunks = 1;
  int rows_per_block = (M + row_chunks - 1) / row_chunks;
  if (rows_per_block < 64) rows_per_block = 64;
  row_chunks = (M + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL(colsum_kernel, dim3(col_groups, row_chunks), dim3(64, 4), 0,
                     (hipStream_t)stream, (const bf16_t*)A, lda, out, M, N, rows_per_block);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
