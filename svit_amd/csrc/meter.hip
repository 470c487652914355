// Meters on the device -- gfx950: the multi-view test ensemble and, at the end of the file, the
// per-iteration row of the train / val meters (meter_push_kernel).
//
// The reference copies every batch of clip probabilities to the host and folds them into
// per-video sums one clip at a time in Python (slowfast/utils/meters.py:303-336, after
// tools/test_net.py:147-160), i.e. one device->host sync per iteration.  Here the per-video
// accumulators live in HBM and one launch folds a whole batch; a second launch at the end counts
// the top-k hits (slowfast/utils/metrics.py:9-50).  A few hundred floats per launch: neither HBM-
// nor MFMA-bound, the point is that the eval loop never waits for the host.
//
// Bit-exactness: fp32 addition is not associative, so the kernel keeps the reference's ORDER --
// the first clip of a video inside the batch (its "leader" workgroup) folds all of that video's
// clips of the batch in batch order; no atomics on the scores.
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
constexpr int NT = 256;

__global__ __launch_bounds__(NT) void ensemble_update_kernel(
    const float* __restrict__ preds, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ clip_ids, int N, int C, int num_clips, int num_videos, int mode,
    int repeat, float* __restrict__ video_preds, int64_t* __restrict__ video_labels,
    int64_t* __restrict__ clip_count, int* __restrict__ err) {
  const int n = blockIdx.x;
  const int64_t id = clip_ids[n];
  const int64_t vid = id / num_clips;
  if (id < 0 || vid >= num_videos) {
    if (threadIdx.x == 0) atomicAdd(err + 0, 1);     // clip id outside the table
    return;
  }
  for (int m = 0; m < n; ++m)                          // uniform over the block
    if (clip_ids[m] >= 0 && clip_ids[m] / num_clips == vid) return;   // not the leader
  // labels / counts: one lane, sequential like the reference's loop
  if (threadIdx.x == 0) {
    int64_t cur = video_labels[vid], cnt = 0;
    for (int m = n; m < N; ++m) {
      if (clip_ids[m] < 0 || clip_ids[m] / num_clips != vid) continue;
      if (cur > 0 && cur != labels[m]) atomicAdd(err + 1, 1);         // meters.py:318-322 assert
      cur = labels[m];
      ++cnt;
    }
    video_labels[vid] = cur;
    clip_count[vid] += cnt * repeat;
  }
  for (int c = threadIdx.x; c < C; c += NT) {
    float acc = video_preds[(size_t)vid * C + c];
    // `repeat`: the dataset lists every view NUM_ENSEMBLE_VIEWS times (identical frames in test
    // mode); the unique views are folded cyclically `repeat` times = the reference's order
    for (int rep = 0; rep < repeat; ++rep)
      for (int m = n; m < N; ++m) {
        if (clip_ids[m] < 0 || clip_ids[m] / num_clips != vid) continue;
        const float p = preds[(size_t)m * C + c];
        acc = mode == 0 ? acc + p : fmaxf(acc, p);
      }
    video_preds[(size_t)vid * C + c] = acc;
  }
}

__global__ __launch_bounds__(NT) void topk_correct_kernel(
    const float* __restrict__ video_preds, const int64_t* __restrict__ video_labels, int V, int C,
    const int* __restrict__ ks, int nk, int* __restrict__ counts, int* __restrict__ err) {
  __shared__ int red[NT / 64];
  const int v = blockIdx.x;
  const int64_t label = video_labels[v];
  if (label < 0 || label >= C) {
    if (threadIdx.x == 0) atomicAdd(err + 2, 1);
    return;
  }
  const float s = video_preds[(size_t)v * C + label];
  int above = 0;     // classes ranked before the label: larger score, or equal and lower index
  for (int c = threadIdx.x; c < C; c += NT) {
    const float p = video_preds[(size_t)v * C + c];
    above += (p > s) || (p == s && c < (int)label);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = above;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int rank = red[0] + red[1] + red[2] + red[3];
    for (int i = 0; i < nk; ++i)
      if (rank < ks[i]) atomicAdd(counts + i, 1);      // integer atomics: order-independent
  }
}

// One iteration of the train / val meters (slowfast/utils/meters.py:454-709) recorded on the device: the reference reads
// every loss with .item() in every iteration (tools/train_net.py:153-167, 325-335); here a row of an fp32 ring takes the
// numbers and the host reads the ring once per cfg.LOG_PERIOD.  ONE workgroup: a wave per logits row, the lanes walk the
// classes -- a batch of logits is tens of KB, and a single workgroup is what lets the launch advance its own row counter
// without a last-block ticket.  No float arithmetic at all: scalar bits are copied as uint32 (NaN payloads and -0.0
// survive -ffast-math), the counts are integers converted once.
struct MeterScalars {
  const float* p[SVIT_METER_MAX_SCALARS];
};

__global__ __launch_bounds__(NT) void meter_push_kernel(
    float* __restrict__ ring, int W, int K, int64_t* __restrict__ state, MeterScalars sc, int ns,
    const float* __restrict__ logits, const int64_t* __restrict__ labels, int N, int C, int k0, int k1) {
  __shared__ int red[3][NT / 64];
  int64_t r = state[0] % W;
  if (r < 0) r += W;                                   // a row inside the ring whatever the counter holds
  uint32_t* __restrict__ row = reinterpret_cast<uint32_t*>(ring + (size_t)r * K);
  if ((int)threadIdx.x < ns) row[threadIdx.x] = *reinterpret_cast<const uint32_t*>(sc.p[threadIdx.x]);
  int hit0 = 0, hit1 = 0, bad = 0;                     // wave-uniform
  if (logits) {
    const int lane = threadIdx.x & 63;
    for (int n = threadIdx.x >> 6; n < N; n += NT / 64) {
      const int64_t label = labels[n];
      if (label < 0 || label >= C) {                   // reads nothing, counts as wrong
        ++bad;
        continue;
      }
      const float* __restrict__ x = logits + (size_t)n * C;
      const float s = x[label];
      int above = 0;     // classes ranked before the label: larger score, or equal and lower index
      for (int c = lane; c < C; c += 64) {
        const float p = x[c];
        above += (p > s) || (p == s && c < (int)label);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
      hit0 += above < k0;
      hit1 += above < k1;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = hit0;
    red[1][threadIdx.x >> 6] = hit1;
    red[2][threadIdx.x >> 6] = bad;
  }
  __syncthreads();                                     // (every thread has read state[0] by now)
  if (threadIdx.x == 0) {
    int t[3];
    for (int i = 0; i < 3; ++i) t[i] = red[i][0] + red[i][1] + red[i][2] + red[i][3];
    if (logits) {
      ring[(size_t)r * K + ns] = (float)t[0];          // exact below 2^24
      ring[(size_t)r * K + ns + 1] = (float)t[1];
      state[1] += t[2];
    }
    state[0] += 1;
  }
}
}  // namespace

extern "C" int svit_ensemble_update(const float* preds, const int64_t* labels,
                                    const int64_t* clip_ids, int N, int C, int num_clips,
                                    int num_videos, int mode, int repeat, float* video_preds,
                                    int64_t* video_labels, int64_t* clip_count, int* err,
                                    void* stream) {
  if (!preds || !labels || !clip_ids || !video_preds || !video_labels || !clip_count || !err)
    return SVIT_ERR_ARG;
  if (N <= 0 || N > 65535 || C <= 0 || num_clips <= 0 || num_videos <= 0 || repeat <= 0 ||
      (mode != 0 && mode != 1))
    return SVIT_ERR_SHAPE;
  hipLaunchKernelGGL(ensemble_update_kernel, dim3(N), dim3(NT), 0, (hipStream_t)stream, preds,
                     labels, clip_ids, N, C, num_clips, num_videos, mode, repeat, video_preds,
                     video_labels, clip_count, err);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_topk_correct(const float* video_preds, const int64_t* video_labels, int V,
                                 int C, const int* ks, int nk, int* counts, int* err,
                                 void* stream) {
  if (!video_preds || !video_labels || !ks || !counts || !err) return SVIT_ERR_ARG;
  if (V <= 0 || C <= 0 || nk <= 0 || nk > 8) return SVIT_ERR_SHAPE;
  hipLaunchKernelGGL(topk_correct_kernel, dim3(V), dim3(NT), 0, (hipStream_t)stream, video_preds,
                     video_labels, V, C, ks, nk, counts, err);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}

extern "C" int svit_meter_push(float* ring, int W, int K, int64_t* state, const float* const* scalars,
                               int n_scalars, const float* logits, const int64_t* labels, int N, int C,
                               int k0, int k1, void* stream) {
  if (!ring || !state || n_scalars < 0 || (n_scalars > 0 && !scalars) || (logits && !labels)) return SVIT_ERR_ARG;
  if (n_scalars > SVIT_METER_MAX_SCALARS || W <= 0) return SVIT_ERR_SHAPE;
  if (K != n_scalars + (logits ? 2 : 0) || K <= 0) return SVIT_ERR_SHAPE;
  if (logits && (N <= 0 || C <= 0 || k0 < 1 || k0 > C || k1 < 1 || k1 > C)) return SVIT_ERR_SHAPE;
  MeterScalars sc = {};
  for (int i = 0; i < n_scalars; ++i) {
    if (!scalars[i]) return SVIT_ERR_ARG;
    sc.p[i] = scalars[i];
  }
  hipLaunchKernelGGL(meter_push_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, ring, W, K, state, sc,
                     n_scalars, logits, labels, N, C, k0, k1);
  SVIT_LAUNCH_CHECK();
  return SVIT_OK;
}
