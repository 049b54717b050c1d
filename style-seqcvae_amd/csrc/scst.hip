// Self-critical sequence training (SCST): what lies between the sampled decode, the per-caption reward and the train step.
// ssc_scst_prepare turns the sampled captions into the `caps` of a train step and the rewards into the per-row upstream gradients
// of ssc_train_bwd, on the device and in stream order (no read-back, capturable).
//
// Two kernels.  Pack: one wave per row finds the row's first end_index with a ballot over 64 columns at a time and writes the
// row's caption, 0-padded to L columns, and its length.  Advantage: one workgroup per image, one thread per sample; the rewards
// are weighted sums of the six score columns in fp64, the leave-one-out sum of an image is formed once, by one thread, in sample
// order.  One more workgroup forms the four statistics from the same fp64 terms: thread t walks the images t, t + 128, ... in
// order, the threads' sums are added in thread order.  No atomics at all; every output is a function of the inputs alone, so two
// calls are bit-identical.
#include "ssc_common.h"

namespace {

constexpr int SCST_MAX_N = 128;      // samples per image, as ssc_eval_score
constexpr int SCST_THREADS = 128;    // advantage kernel: one thread per sample
constexpr int PACK_THREADS = 256;    // pack kernel: four rows per workgroup
constexpr int PACK_ROWS = PACK_THREADS / SSC_WAVE;

struct ScstArgs {
  int P, N, steps, L, end_index, baseline;
  const int64_t* predictions; const double* scores; const double* base_scores;
  double w[6]; double loss_scale, kld_scale;
  int64_t* caps; int* lengths; float* reward; float* advantage; float* gl; float* gk; double* stats;
};

__global__ __launch_bounds__(PACK_THREADS) void scst_pack_kernel(ScstArgs a) {
  const int lane = threadIdx.x & (SSC_WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * PACK_ROWS + (threadIdx.x >> 6);
  if (g >= (int64_t)a.P * a.N) return;   // (wave-uniform)
  const int64_t* src = a.predictions + (size_t)g * a.steps;
  int len = a.steps;   // a row with no end_index keeps all its tokens
  for (int base = 0; base < a.steps; base += SSC_WAVE) {
    const int c = base + lane;
    const bool is_end = c < a.steps && src[c] == (int64_t)a.end_index;
    const unsigned long long m = __ballot(is_end);
    if (m) { len = base + __builtin_ctzll(m); break; }
  }
  int64_t* dst = a.caps + (size_t)g * a.L;
  for (int c = lane; c < a.L; c += SSC_WAVE) dst[c] = c < len ? src[c] : 0;   // (len <= steps: src is read below steps only)
  if (lane == 0) a.lengths[g] = len;
}

// r = sum_k w_k score_k, in column order
__device__ __forceinline__ double scst_reward(const double* s, const double* w) {
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) r += w[k] * s[k];
  return r;
}

// the sum of an image's rewards, in sample order
__device__ __forceinline__ double scst_image_sum(const double* s, int N, const double* w) {
  double S = 0.0;
  for (int i = 0; i < N; ++i) S += scst_reward(s + (size_t)i * 6, w);
  return S;
}

// the baseline of a sample of reward r: S = the image's sum (leave-one-out), bg = the image's given reward
__device__ __forceinline__ double scst_baseline(int kind, double r, double S, double bg, int N) {
  if (kind == 1) return (S - r) / (double)(N - 1);
  return kind == 2 ? bg : 0.0;
}

__global__ __launch_bounds__(SCST_THREADS) void scst_advantage_kernel(ScstArgs a) {
  __shared__ double sh[4][SCST_THREADS];
  const int N = a.N, tid = threadIdx.x;
  if ((int)blockIdx.x < a.P) {   // one image
    const int p = blockIdx.x;
    const double* s = a.scores + (size_t)p * N * 6;
    if (tid == 0) {
      sh[0][0] = a.baseline == 1 ? scst_image_sum(s, N, a.w) : 0.0;
      sh[1][0] = a.baseline == 2 ? scst_reward(a.base_scores + (size_t)p * 6, a.w) : 0.0;
    }
    __syncthreads();
    if (tid < N) {
      const size_t g = (size_t)p * N + tid;
      const double r = scst_reward(s + (size_t)tid * 6, a.w);
      const double adv = r - scst_baseline(a.baseline, r, sh[0][0], sh[1][0], N);
      a.reward[g] = (float)r;
      a.advantage[g] = (float)adv;
      a.gl[g] = (float)(a.loss_scale * adv);
      a.gk[g] = (float)a.kld_scale;
    }
    return;
  }
  // the statistics: mean reward, mean baseline, mean |advantage|, share of rows with no end_index (length == steps)
  double sr = 0.0, sb = 0.0, sa = 0.0, sn = 0.0;
  for (int p = tid; p < a.P; p += SCST_THREADS) {
    const double* s = a.scores + (size_t)p * N * 6;
    const double S = a.baseline == 1 ? scst_image_sum(s, N, a.w) : 0.0;
    const double bg = a.baseline == 2 ? scst_reward(a.base_scores + (size_t)p * 6, a.w) : 0.0;
    for (int i = 0; i < N; ++i) {
      const double r = scst_reward(s + (size_t)i * 6, a.w);
      const double b = scst_baseline(a.baseline, r, S, bg, N);
      sr += r;
      sb += b;
      sa += fabs(r - b);
      sn += a.lengths[(size_t)p * N + i] == a.steps ? 1.0 : 0.0;
    }
  }
  sh[0][tid] = sr; sh[1][tid] = sb; sh[2][tid] = sa; sh[3][tid] = sn;
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int j = 0; j < SCST_THREADS; ++j) t += sh[tid][j];
    a.stats[tid] = t / ((double)a.P * (double)N);
  }
}

}  // namespace

extern "C" int ssc_scst_prepare(const ssc_scst_desc* d, void* stream) {
  if (!d) return SSC_EINVAL;
  if (d->P < 1 || d->N < 1 || d->N > SCST_MAX_N || d->steps < 1 || d->L < d->steps || d->end_index < 0) return SSC_EINVAL;
  if ((int64_t)d->P * d->N > 0x7fffffffLL / 2) return SSC_EINVAL;
  if (d->baseline < 0 || d->baseline > 2 || (d->baseline == 1 && d->N == 1) || (d->baseline == 2 && !d->base_scores)) return SSC_EINVAL;
  if (!d->predictions || !d->scores || !d->caps || !d->lengths || !d->reward || !d->advantage || !d->gl || !d->gk || !d->stats)
    return SSC_EINVAL;
  ScstArgs a{};
  a.P = d->P; a.N = d->N; a.steps = d->steps; a.L = d->L; a.end_index = d->end_index; a.baseline = d->baseline;
  a.predictions = d->predictions; a.scores = d->scores; a.base_scores = d->base_scores;
  for (int k = 0; k < 6; ++k) a.w[k] = d->reward_weights[k];
  a.loss_scale = d->loss_scale; a.kld_scale = d->kld_scale;
  a.caps = d->caps; a.lengths = d->lengths; a.reward = d->reward; a.advantage = d->advantage; a.gl = d->gl; a.gk = d->gk;
  a.stats = d->stats;
  hipStream_t st = (hipStream_t)stream;
  const int G = d->P * d->N;
  SSC_LAUNCH(scst_pack_kernel, dim3(ssc_cdiv(G, PACK_ROWS)), dim3(PACK_THREADS), 0, st, a);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(scst_advantage_kernel, dim3(d->P + 1), dim3(SCST_THREADS), 0, st, a);   // (reads the lengths the pack kernel wrote)
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
