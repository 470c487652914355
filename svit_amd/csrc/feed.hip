// The batch feeder's device half (svit_amd/feeder.py): one uploaded SLOT -> the captured step's static buffers -- gfx950.
//
// The host packs a batch's videos TIGHTLY into a pinned slot (each video its own T x h_v x w_v x 3 bytes, no padding rows,
// no zero fill; the small tables behind them) and uploads it with one copy on a copy stream.  `svit_feed_unpack` is the one
// launch that takes the uploaded slot apart: every video into the top-left corner of its frames of the padded buffer
// u8 [V,T,Hs,Ws,3] the step was captured over (`fill` everywhere else, so every byte of the buffer is written once), and up
// to eight small segments (records, extents, RandAugment table, labels) to where the step reads them.  It replaces the
// device-to-device copy of the padded buffer and the handful of small copies a replay made before.
//
// Shape of the frames part: memory-bound.  One lane owns one ALIGNED 16-byte chunk of the destination and stores it with
// one 16-byte store.  The bytes of a chunk come from RUNS: a run is a stretch of one video row inside the chunk (a chunk
// spans several rows when Ws*3 < 16, and video as well as padding at a row's end).  A run's source bytes start at an
// arbitrary byte address (33- and 57-byte rows, 54-byte videos), so they are assembled from ALIGNED source dwords with a
// byte funnel: five consecutive dwords cover any 16 source bytes, dword j of the chunk is the funnel of words j and j + 1.
// A source dword is loaded only when it holds a byte of the run's own row -- a row of a video that lies inside the slot --
// so no load leaves [slot, slot + slot_bytes) whatever the tables hold (slot 16-byte aligned, slot_bytes a multiple of 16).
// swap_rb: byte c of a pixel comes from byte 2 - c, i.e. from the funnels two bytes ahead, in place and two bytes back.
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int FEED_THREADS = 256;
constexpr int64_t FEED_MAX_BLOCKS = 16384;

__device__ __forceinline__ int feed_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the bytes i of a dword with lo <= i < hi
__device__ __forceinline__ uint32_t feed_byte_mask(int lo, int hi) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > 4 ? 4 : hi;
  if (hi <= lo) return 0u;
  return (0xffffffffu >> (8 * (4 - hi))) & (0xffffffffu << (8 * lo));
}
// the bytes i of a dword with i % 3 == q
__device__ __forceinline__ uint32_t feed_channel_mask(int q) {
  return q == 0 ? 0xff0000ffu : (q == 1 ? 0x0000ff00u : 0x00ff0000u);
}
// bytes sh .. sh+3 of the little-endian pair (lo, hi), sh in 0..3
__device__ __forceinline__ uint32_t feed_funnel(uint32_t lo, uint32_t hi, int sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}
// aligned dword `wi` of the slot if it holds a byte of the row [wlo, whi] (dword indices), else 0
__device__ __forceinline__ uint32_t feed_word(const uint32_t* __restrict__ slotw, int64_t wi, int64_t wlo, int64_t whi) {
  return (wi >= wlo && wi <= whi) ? slotw[wi] : 0u;
}

__device__ __forceinline__ void feed_segment(const svit_feed_args& a, int s) {
  const svit_feed_seg sg = a.seg[s];
  const uint32_t* __restrict__ src = (const uint32_t*)(a.slot + sg.src_off);     // (src_off % 16 == 0)
  uint32_t* __restrict__ dst = (uint32_t*)sg.dst;                                 // (4-byte aligned)
  const int64_t full = sg.bytes >> 2;
  for (int64_t i = threadIdx.x; i < full; i += FEED_THREADS) dst[i] = src[i];
  const int tail = (int)(sg.bytes & 3);
  if (threadIdx.x == 0 && tail) {
    const uint32_t w = src[full];      // inside the slot: src_off + bytes <= slot_bytes, and slot_bytes % 16 == 0
    uint8_t* d8 = (uint8_t*)sg.dst + full * 4;
    for (int b = 0; b < tail; ++b) d8[b] = (uint8_t)(w >> (8 * b));
  }
}

template <bool SWAP>
__global__ __launch_bounds__(FEED_THREADS) void feed_unpack_kernel(const svit_feed_args a, int64_t total, int64_t n_chunks,
                                                                   unsigned frame_blocks) {
  if (blockIdx.x >= frame_blocks) {
    feed_segment(a, (int)(blockIdx.x - frame_blocks));
    return;
  }
  const uint32_t* __restrict__ slotw = (const uint32_t*)a.slot;
  const int T = a.T, Hs = a.Hs, Ws = a.Ws;
  const uint32_t pitch = (uint32_t)Ws * 3u;
  const uint32_t vol = (uint32_t)T * (uint32_t)Hs * pitch;           // bytes per video of the buffer (host: below 2^31)
  const uint32_t fill4 = (uint32_t)a.fill * 0x01010101u;
  const int64_t stride = (int64_t)frame_blocks * FEED_THREADS;
  for (int64_t ch = (int64_t)blockIdx.x * FEED_THREADS + threadIdx.x; ch < n_chunks; ch += stride) {
    const int64_t d0 = ch * 16;
    const int nb = total - d0 < 16 ? (int)(total - d0) : 16;         // (only the buffer's last chunk may be short)
    uint32_t out[4] = {fill4, fill4, fill4, fill4};
    int64_t v;
    uint32_t rem;
    if (total <= 0xffffffffLL) {                                     // (uniform: a 32-bit division is a third of a 64-bit one)
      const uint32_t q = (uint32_t)d0 / vol;
      v = q;
      rem = (uint32_t)d0 - q * vol;
    } else {
      v = d0 / vol;
      rem = (uint32_t)(d0 - v * (int64_t)vol);
    }
    int k = 0;                                                       // bytes of the chunk done
    while (k < nb) {
      if (rem >= vol) {                                              // (a row's end was the video's end)
        rem -= vol;
        ++v;
      }
      const uint32_t r = rem / pitch;
      const int xb = (int)(rem - r * pitch), t = (int)(r / (uint32_t)Hs), y = (int)(r - (uint32_t)t * (uint32_t)Hs);
      int h = Hs, w = Ws;
      if (a.extents) {
        h = feed_clampi(a.extents[2 * v], 1, Hs);
        w = feed_clampi(a.extents[2 * v + 1], 1, Ws);
      }
      const int wb = w * 3;
      const int64_t n_v = (int64_t)T * h * wb;
      const int64_t off = a.offsets ? a.offsets[v] : v * (int64_t)vol;
      const bool present = off >= 0 && off <= a.slot_bytes - n_v;
      if (!present || y >= h || xb >= wb) {                          // fill to the end of this buffer row
        const int skip = (int)pitch - xb;
        k += skip;
        rem += (uint32_t)skip;
        continue;
      }
      const int n = wb - xb < nb - k ? wb - xb : nb - k;             // the run: n bytes of row (t, y) from byte xb
      const int64_t rs = off + ((int64_t)t * h + y) * wb;            // the row's first byte in the slot
      const int64_t wlo = rs >> 2, whi = (rs + wb - 1) >> 2;         // the aligned dwords that hold bytes of the row
      const int64_t a0 = rs + xb - k;                                // the source byte under byte 0 of the chunk
      if (!SWAP) {
        const int64_t w0 = a0 >> 2;
        const int sh = (int)(a0 & 3);
        uint32_t W[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) W[m] = feed_word(slotw, w0 + m, wlo, whi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t mask = feed_byte_mask(k - 4 * j, k + n - 4 * j);
          out[j] = (out[j] & ~mask) | (feed_funnel(W[j], W[j + 1], sh) & mask);
        }
      } else {
        const int64_t b0 = a0 - 2, w0 = b0 >> 2;
        const int base = (int)(b0 & 3);
        const int p = ((xb - k) % 3 + 3) % 3;                        // byte m of the chunk is channel (m + p) % 3
        uint32_t W[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) W[m] = feed_word(slotw, w0 + m, wlo, whi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t s[3];                                             // the source 2 bytes back, in place, 2 bytes ahead
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const int b = base + 2 * q;
            const bool up = b >= 4;
            s[q] = feed_funnel(up ? W[j + 1] : W[j], up ? W[j + 2] : W[j + 1], b & 3);
          }
          const int rr = (j + p) % 3;                                // byte i of this dword is channel (rr + i) % 3
          const uint32_t val = (s[2] & feed_channel_mask((3 - rr) % 3)) | (s[1] & feed_channel_mask((4 - rr) % 3)) |
                               (s[0] & feed_channel_mask((5 - rr) % 3));
          const uint32_t mask = feed_byte_mask(k - 4 * j, k + n - 4 * j);
          out[j] = (out[j] & ~mask) | (val & mask);
        }
      }
      k += n;
      rem += (uint32_t)n;
    }
    if (nb == 16) {
      *(uint4*)(a.frames + d0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
          if (4 * j + i < nb) a.frames[d0 + 4 * j + i] = (uint8_t)(out[j] >> (8 * i));
    }
  }
}
}  // namespace

extern "C" int svit_feed_unpack(const svit_feed_args* a, void* stream) {
  if (!a || !a->slot || !a->frames) return SVIT_ERR_ARG;
  if ((uintptr_t)a->slot % 16 || (uintptr_t)a->frames % 16 || a->slot_bytes % 16) return SVIT_ERR_ALIGN;
  if ((uintptr_t)a->offsets % 8 || (uintptr_t)a->extents % 4) return SVIT_ERR_ALIGN;
  if (a->V < 1 || a->T < 1 || a->Hs < 1 || a->Ws < 1 || a->slot_bytes < 16) return SVIT_ERR_SHAPE;
  if ((int64_t)a->T * a->Hs * a->Ws * 3 > 0x7fffffffLL) return SVIT_ERR_SHAPE;
  if (a->fill < 0 || a->fill > 255 || a->n_seg < 0 || a->n_seg > 8) return SVIT_ERR_ARG;
  for (int s = 0; s < a->n_seg; ++s) {
    const svit_feed_seg& sg = a->seg[s];
    if (!sg.dst || sg.bytes < 0 || sg.src_off < 0 || sg.src_off > a->slot_bytes - sg.bytes) return SVIT_ERR_ARG;
    if (sg.src_off % 16 || (uintptr_t)sg.dst % 4) return SVIT_ERR_ALIGN;
  }
  const int64_t total = (int64_t)a->V * a->T * a->Hs * a->Ws * 3;
  const int64_t n_chunks = (total + 15) / 16;
  int64_t blocks = (n_chunks + FEED_THREADS - 1) / FEED_THREADS;
  if (blocks > FEED_MAX_BLOCKS) blocks = FEED_MAX_BLOCKS;
  const dim3 grid((unsigned)(blocks + a->n_seg)), block(FEED_THREADS);
  if (a->swap_rb)
    hipLaunchKernelGGL(feed_unpack_kernel<true>, grid, block, 0, (hipStream_t)stream, *a, total, n_chunks, (unsigned)blocks);
  else
    hipLaunchKernelGGL(feed_unpack_kernel<false>, grid, block, 0, (hipStream_t)stream, *a, total, n_chunks, (unsigned)blocks);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
