// Scheduled sampling of the cross-entropy train step (Bengio et al. 2015; include/ssc.h: ssc_sched_sampling): the kernel that
// decides, per row of one time step, whether the attention LSTM is fed the ground-truth word or a word the model draws from its own
// logits of the previous step, and gathers the embedding row of the word that is fed - one launch per step inside the time loop of
// ssc_train_fwd_opts (sequence.hip).
//
// One workgroup per row.  The decision is one Philox4x32-10 block of counter (0, step, row, 1): its last word keeps the stream
// apart from the word draws' (last word 0).  A row that fires draws with sample_draw_row (sample_draw.h) - the code of
// ssc_sample_rows, so the token is that call's token for the same logits, sampler, step, row and seed; a row that does not fire
// never touches its logits.  No atomics on global memory, no scratch, no read-back: stream-ordered and graph-capturable.
#include <math.h>

#include "sample_draw.h"

namespace {

struct MixArgs {
  const float* logits; size_t ld; int V;
  int kind, top_k; float top_p, temperature, prob;
  uint32_t seed_lo, seed_hi;
  int step;
  const int64_t* truth; const float* w_prev; const float* w_cur;
  const float* table; int ldt, E;
  int64_t* tok_out; float* fed_out; float* emb_out; int ldo;
};

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void sched_mix_rows_kernel(MixArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  const int r = blockIdx.x;
  int64_t tok = a.truth[r];
  // workgroup-uniform: the row has a target at this step and its previous step's logits row is one the head projects
  bool fire = a.w_prev[r] != 0.f && a.w_cur[r] != 0.f;
  if (fire) {
    uint32_t ctr[4] = {0u, (uint32_t)a.step, (uint32_t)r, 1u};
    philox4x32_10(ctr, a.seed_lo, a.seed_hi);
    fire = sample_uniform(ctr[0]) < a.prob;
  }
  if (fire) {
    const SampleDraw dr = sample_draw_row<STAGED>(a.logits + (size_t)r * a.ld, srow, a.V, a.kind, a.top_k, a.top_p, a.temperature,
                                                  a.seed_lo, a.seed_hi, a.step, (uint32_t)r, false, sh);
    // (a row without one comparable logit - all NaN - has no draw: it keeps the ground-truth word, and no id leaves [0, V))
    if (dr.tok >= 0) tok = dr.tok;
    else fire = false;
  }
  if (threadIdx.x == 0) {
    a.tok_out[r] = tok;
    a.fed_out[r] = fire ? 1.f : 0.f;
  }
  // the embedding row of the fed word (id 0: the table's pad row, as ssc_embed_gather)
  const float* src = a.table + (size_t)tok * a.ldt;
  float* dst = a.emb_out + (size_t)r * a.ldo;
  if (ssc_aligned16_dev(src) && ssc_aligned16_dev(dst)) {
    const int n4 = a.E >> 2;
    for (int j = threadIdx.x; j < n4; j += SAMPLE_THREADS)
      reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
    for (int e = 4 * n4 + threadIdx.x; e < a.E; e += SAMPLE_THREADS) dst[e] = src[e];
  } else {
    for (int e = threadIdx.x; e < a.E; e += SAMPLE_THREADS) dst[e] = src[e];
  }
}

}  // namespace

extern "C" int ssc_sched_mix_rows(const float* logits, int ld, int rows, int V, const int64_t* truth, const float* w_prev,
                                  const float* w_cur, const float* table, int ldt, int E, int step, const ssc_sched_sampling* ss,
                                  int64_t* tok_out, float* fed_out, float* emb_out, int ldo, void* stream) {
  if (!logits || !truth || !w_prev || !w_cur || !table || !ss || !tok_out || !fed_out || !emb_out) return SSC_EINVAL;
  if (rows < 0 || V <= 0 || ld < V || E <= 0 || ldt < E || ldo < E || step < 1) return SSC_EINVAL;
  if (!(ss->prob >= 0.f && ss->prob <= 1.f) || !sampler_ok(&ss->sampler, V)) return SSC_EINVAL;   // NaN included
  if (rows == 0) return SSC_OK;
  MixArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V;
  a.kind = ss->sampler.kind; a.top_k = ss->sampler.top_k; a.top_p = ss->sampler.top_p; a.temperature = ss->sampler.temperature;
  a.prob = ss->prob;
  a.seed_lo = (uint32_t)(ss->sampler.seed & 0xffffffffu); a.seed_hi = (uint32_t)(ss->sampler.seed >> 32);
  a.step = step;
  a.truth = truth; a.w_prev = w_prev; a.w_cur = w_cur;
  a.table = table; a.ldt = ldt; a.E = E;
  a.tok_out = tok_out; a.fed_out = fed_out; a.emb_out = emb_out; a.ldo = ldo;
  return sample_row_launch(sched_mix_rows_kernel<true>, sched_mix_rows_kernel<false>, V, rows, (hipStream_t)stream, a);
}
