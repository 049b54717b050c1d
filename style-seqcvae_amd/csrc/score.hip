// Scoring given captions under the model: the forced counterpart of the word samplers.  ssc_score_rows returns, per row of raw
// logits, the log-probability (and optionally the rank) of a GIVEN token; ssc_decode_score is the teacher-forced decode of a whole
// scoring call - nimg images x C captions x N latent samples - in one library call: the step loop of ssc_decode_sample with the
// given tokens fed in place of chosen ones and ssc_score_rows in place of the draw.
//
// One workgroup per row.  The row is read from HBM ONCE: every thread keeps a running (maximum, sum of exp(x - maximum)) pair over
// its share of the row - 16-byte loads where the row is 16-byte aligned and V % 4 == 0, scalar loads otherwise - and counts the
// entries that rank ahead of the target, whose logit is read first.  The pairs are combined in a fixed order (wave butterflies,
// then the waves in index order): no float atomics, the same bits on every run.  The step log-prob is formed as
// (x_target - max) - log(sum): the first difference is exact, so logits of magnitude 1e4 lose nothing to the subtraction.
// ssc_decode_score's host loop is built from the shared driver of decode_loop.h ("the one-call decodes' host driver").
//
// ssc_posterior_rows scores the POSTERIOR branch of a train forward: per caption row the log-density ratio log p(z) - log q(z | x) at
// the sampled z and the training KL, split by latent dimension and by step.
#include <math.h>

#include "decode_loop.h"
#include "latent_common.h"
#include "ssc_radix.h"

namespace {

constexpr int SCORE_THREADS = 256;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;

struct ScoreArgs {
  const float* logits; size_t ld; int V;
  const int64_t* target; const int64_t* last_target; int end_index;
  float* row_lp; float* lp_out; int* rank_out;
  int lp_stride, rank_stride;   // lp_out / rank_out of row r at r * stride (the driver writes column t of its (G, L) outputs)
};

// (m, s) <- the pair of the union: s sums exp(x - m)
__device__ __forceinline__ void score_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) { m = M; s = 0.f; return; }
  s = s * expf(m - M) + os * expf(om - M);
  m = M;
}

__global__ __launch_bounds__(SCORE_THREADS) void score_rows_kernel(ScoreArgs a) {
  __shared__ float sh_m[SCORE_WAVES], sh_s[SCORE_WAVES];
  __shared__ int sh_c[SCORE_WAVES];
  const int r = blockIdx.x;
  const int V = a.V;
  const int64_t tgt = a.target[r];
  const size_t o = (size_t)r * a.lp_stride, ro = (size_t)r * a.rank_stride;
  // workgroup-uniform: an ended row (its logits are not read), or an id that must not index the row
  const bool ended = tgt < 0 || (a.last_target && a.last_target[r] == a.end_index);
  if (ended || tgt >= V) {
    if (threadIdx.x == 0) {
      const float lp = ended ? 0.f : -INFINITY;
      a.lp_out[o] = lp;
      if (a.rank_out) a.rank_out[ro] = -1;
      if (!ended && a.row_lp) a.row_lp[r] += lp;
    }
    return;
  }
  const float* g = a.logits + (size_t)r * a.ld;
  const RowView<false> row{g, nullptr, V, ssc_aligned16_dev(g) && (V & 3) == 0};
  const int t = (int)tgt;
  const float xt = g[t];
  const int nj = (V + 3) >> 2;
  float m = -INFINITY, s = 0.f;
  int ahead = 0;
#pragma unroll 2
  for (int j = threadIdx.x; j < nj; j += SCORE_THREADS) {
    float x[4];
    row.get4(j, x);   // (entries >= V read as -inf)
    const float m4 = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
#pragma unroll
    for (int c = 0; c < 4; ++c) ahead += (x[c] > xt || (x[c] == xt && 4 * j + c < t)) ? 1 : 0;
    if (m4 == -INFINITY) continue;
    if (m4 > m) { s *= expf(m - m4); m = m4; }
    s += (expf(x[0] - m) + expf(x[1] - m)) + (expf(x[2] - m) + expf(x[3] - m));
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const float om = __shfl_xor(m, w, 64), os = __shfl_xor(s, w, 64);
    score_merge(m, s, om, os);
    ahead += __shfl_xor(ahead, w, 64);
  }
  if ((threadIdx.x & 63) == 0) { sh_m[threadIdx.x >> 6] = m; sh_s[threadIdx.x >> 6] = s; sh_c[threadIdx.x >> 6] = ahead; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SCORE_WAVES; ++w) {
      score_merge(m, s, sh_m[w], sh_s[w]);
      ahead += sh_c[w];
    }
    const float lp = (xt - m) - logf(s);
    a.lp_out[o] = lp;
    if (a.rank_out) a.rank_out[ro] = ahead;
    if (a.row_lp) a.row_lp[r] += lp;
  }
}

int score_launch(const ScoreArgs& a, int rows, hipStream_t st) {
  SSC_LAUNCH(score_rows_kernel, dim3(rows), dim3(SCORE_THREADS), 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// targets (nimg, C, L) -> time-major rows g = (image, caption, sample): tgt (L, G) as given up to the caption's end - its first END,
// negative id or id >= V - and -1 after it (an absent slot: -1 throughout), fed (L, G): the token fed at step t - END at step 0,
// target t - 1 after, every id that cannot index the embedding replaced by END.  n_tokens (nimg, C): scored tokens.
__global__ void score_prepare_kernel(const int64_t* __restrict__ targets, int NC, int N, int L, int V, int end_index,
                                     int64_t* __restrict__ tgt, int64_t* __restrict__ fed, float* __restrict__ lp,
                                     int* __restrict__ n_tokens) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int G = NC * N;
  if (g >= G) return;
  const int ic = g / N;
  const int64_t* src = targets + (size_t)ic * L;
  const bool absent = src[0] < 0;
  int count = 0;
  bool open = !absent;
  fed[g] = end_index;
  for (int t = 0; t < L; ++t) {
    const int64_t x = open ? src[t] : -1;   // (nothing after a caption's end is scored or fed)
    tgt[(size_t)t * G + g] = x;
    if (t + 1 < L) fed[(size_t)(t + 1) * G + g] = (x < 0 || x >= V) ? end_index : x;
    if (open) {
      if (x >= 0) ++count;
      if (x < 0 || x >= V || x == end_index) open = false;
    }
  }
  lp[g] = 0.f;
  if (g % N == 0) n_tokens[ic] = count;
}

struct ScoreLayout {
  SscStepStates states;   // (G, H) rows
  size_t tgt;        // (L, G) int64
  size_t fed;        // (L, G) int64
  size_t parent0;    // (G) int64 zeros: every row is its own parent (the beam-1 search's parent list)
  size_t lp;         // (G) running caption log-probs
  size_t steplp;     // (G) the last step's log-probs (when the caller takes no token_lp)
  size_t alpha;      // (G, R)
  size_t logits;     // (G, V)
  size_t stepws, stepws_bytes;
  size_t total;
};

ScoreLayout score_layout(const ssc_model_cfg* cfg, const ssc_score_desc* d) {
  ScoreLayout l;
  const size_t G = (size_t)d->nimg * d->n_captions * d->n_samples;
  size_t o = 0;
  l.states.reserve(o, G, cfg->H);
  l.tgt = ssc_ws_take(o, (size_t)d->max_len * G * 8);
  l.fed = ssc_ws_take(o, (size_t)d->max_len * G * 8);
  l.parent0 = ssc_ws_take(o, G * 8);
  l.lp = ssc_ws_take(o, G * 4);
  l.steplp = ssc_ws_take(o, G * 4);
  l.alpha = ssc_ws_take(o, G * (size_t)d->R * 4);
  l.logits = ssc_ws_take(o, G * (size_t)cfg->V * 4);
  l.stepws_bytes = ssc_decode_step_workspace_bytes(cfg, (int)G, d->R);
  l.stepws = ssc_ws_take(o, l.stepws_bytes);
  l.total = o;
  return l;
}

bool score_dims_ok(const ssc_model_cfg* cfg, const ssc_score_desc* d) {
  if (!ssc_decode_dims_ok(cfg, d, d ? d->max_len : 0) || d->n_captions <= 0) return false;
  return (long)d->nimg * d->n_captions * d->n_samples <= (1L << 24);
}

bool score_desc_ok(const ssc_model_cfg* cfg, const ssc_score_desc* d) {
  return score_dims_ok(cfg, d) && ssc_decode_inputs_ok(cfg, d, d->max_len) && d->targets && d->log_probs && d->n_tokens;
}

// ---- posterior rows (include/ssc.h: ssc_posterior_rows) ------------------------------------------------------------------------------
// One wave per caption row b, lanes over the latent dimensions j = lane + 64 k (k < NJ), the steps in sequence.  Each lane keeps the
// KL of its NJ dimensions summed over t (kl_dim) and one running sum of its log-ratio terms; the row scalars are ONE butterfly of
// those at the end (the step outputs, where asked for, a butterfly per step): a fixed order, no atomics.  A step with w == 0 is
// skipped before any of its rows is read.
constexpr int POST_MAX_NJ = 8;

template <int NJ>
__global__ __launch_bounds__(64) void posterior_rows_kernel(const ssc_posterior_rows_desc d) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Z = d.Z, B = d.B;
  const float pv = d.prior_var, lpv = logf(pv);
  const bool steps = d.step_kl || d.step_ratio;   // (wave-uniform)
  float kd[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) kd[k] = 0.f;
  float racc = 0.f;
  for (int t = 0; t < d.T; ++t) {
    const size_t r = (size_t)t * B + b;
    const float w = d.w[r];
    if (w == 0.f) {   // (wave-uniform)
      if (lane == 0) {
        if (d.step_kl) d.step_kl[r] = 0.f;
        if (d.step_ratio) d.step_ratio[r] = 0.f;
      }
      continue;
    }
    const float* pm_t = d.pm ? d.pm + (size_t)t * B * d.ldpm : nullptr;   // (this step's (B, ldpm) block)
    float sk = 0.f, sr = 0.f;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      const int j = lane + 64 * k;
      if (j < Z) {
        const float m = d.mu[r * d.ldz + j], l = d.lv[r * d.ldz + j], zz = d.z[r * d.ldz + j];
        const float e = d.eps[r * d.ldeps + j];
        const float pm = latent_prior_mean(pm_t, d.ldpm, d.sent, d.pm_scale, b, j);
        const float dz = zz - pm;
        const float rt = 0.5f * (e * e + l - lpv - dz * dz / pv);
        const float kt = latent_kl_elem(d.kld_mode, m, l, expf(l), pm, lpv, pv);   // (the training KL: the forward's function)
        kd[k] += w * kt;
        racc += w * rt;
        sk += kt;
        sr += rt;
      }
    }
    if (steps) {
      sk = ssc_wave_sum(sk);
      sr = ssc_wave_sum(sr);
      if (lane == 0) {
        if (d.step_kl) d.step_kl[r] = w * sk;
        if (d.step_ratio) d.step_ratio[r] = w * sr;
      }
    }
  }
  float kacc = 0.f;
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const int j = lane + 64 * k;
    if (d.kl_dim && j < Z) d.kl_dim[(size_t)b * d.ld + j] = kd[k];
    kacc += kd[k];
  }
  kacc = ssc_wave_sum(kacc);
  racc = ssc_wave_sum(racc);
  if (lane == 0) {
    d.kl[b] = kacc;
    d.log_ratio[b] = racc;
  }
}

}  // namespace

extern "C" int ssc_posterior_rows(const ssc_posterior_rows_desc* d, void* stream) {
  if (!d || !d->mu || !d->lv || !d->z || !d->eps || !d->w || !d->log_ratio || !d->kl) return SSC_EINVAL;
  if (d->T <= 0 || d->B <= 0 || d->Z <= 0 || d->Z > 64 * POST_MAX_NJ || d->ldz < d->Z || d->ldeps < d->Z) return SSC_EINVAL;
  if (!(d->prior_var > 0.f) || d->kld_mode < 0 || d->kld_mode > 2) return SSC_EINVAL;   // (NaN included)
  if ((d->kld_mode == 2 && !d->pm) || (d->pm && d->ldpm < d->Z) || (d->kl_dim && d->ld < d->Z)) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nj = ssc_cdiv(d->Z, 64);
  if (nj <= 1) SSC_LAUNCH(posterior_rows_kernel<1>, dim3(d->B), dim3(64), 0, st, *d);
  else if (nj == 2) SSC_LAUNCH(posterior_rows_kernel<2>, dim3(d->B), dim3(64), 0, st, *d);
  else if (nj <= 4) SSC_LAUNCH(posterior_rows_kernel<4>, dim3(d->B), dim3(64), 0, st, *d);
  else SSC_LAUNCH(posterior_rows_kernel<POST_MAX_NJ>, dim3(d->B), dim3(64), 0, st, *d);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_score_rows(const float* logits, int ld, int rows, int V, const int64_t* target, const int64_t* last_target,
                              int end_index, float* row_lp, float* lp_out, int* rank_out, void* stream) {
  if (!logits || !target || !lp_out || rows < 0 || V <= 0 || ld < V || end_index < 0 || end_index >= V) return SSC_EINVAL;
  if (rows == 0) return SSC_OK;
  ScoreArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V; a.target = target; a.last_target = last_target; a.end_index = end_index;
  a.row_lp = row_lp; a.lp_out = lp_out; a.rank_out = rank_out; a.lp_stride = a.rank_stride = 1;
  return score_launch(a, rows, (hipStream_t)stream);
}

// ssc_common.h: ssc_score_rows with lp_out of row r at r * lp_stride - column t of a driver's (rows, L) output (ssc_decode_prime)
int ssc_score_rows_at(const float* logits, int ld, int rows, int V, const int64_t* target, const int64_t* last_target, int end_index,
                      float* row_lp, float* lp_out, int lp_stride, hipStream_t st) {
  ScoreArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V; a.target = target; a.last_target = last_target; a.end_index = end_index;
  a.row_lp = row_lp; a.lp_out = lp_out; a.lp_stride = lp_stride; a.rank_stride = 1;
  return score_launch(a, rows, st);
}

extern "C" size_t ssc_decode_score_workspace_bytes(const ssc_model_cfg* cfg, const ssc_score_desc* d) {
  if (!score_dims_ok(cfg, d)) return 0;
  return score_layout(cfg, d).total;
}

extern "C" int ssc_decode_score(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_score_desc* d, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return ssc_decode_score_guided(cfg, p, d, nullptr, workspace, workspace_bytes, stream);
}

// guide (or null): step t's z block from slab t of the call's latent guide, one entry per row g = (image, caption, sample)
extern "C" int ssc_decode_score_guided(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_score_desc* d,
                                       const ssc_latent_guide* guide, void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);   // the numerics mode of this cfg, for every product the call issues
  if (!p || !workspace || !score_desc_ok(cfg, d) || (guide && !ssc_latent_guide_ok(cfg, guide))) return SSC_EINVAL;
  const ScoreLayout l = score_layout(cfg, d);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* W = (char*)workspace;
  const int rpi = d->n_captions * d->n_samples, G = d->nimg * rpi, V = cfg->V, Z = cfg->Z, L = d->max_len;
  const SscStepStates& states = l.states;
  int64_t* tgt = (int64_t*)(W + l.tgt);
  int64_t* fed = (int64_t*)(W + l.fed);
  int64_t* parent0 = (int64_t*)(W + l.parent0);
  float* lp = (float*)(W + l.lp);
  float* logits = (float*)(W + l.logits);

  SSC_LAUNCH(score_prepare_kernel, dim3(ssc_cdiv(G, 256)), dim3(256), 0, st, d->targets, d->nimg * d->n_captions, d->n_samples, L, V,
             d->end_index, tgt, fed, lp, d->n_tokens);
  SSC_CHECK_LAUNCH();
  if (hipMemsetAsync(parent0, 0, (size_t)G * 8, st) != hipSuccess) return SSC_EHIP;
  SSC_TRY(states.zero(W, 1, G, st));

  // the steps take the form the beam-1 drivers give them (ssc_decode_sample): same tables, same parent list
  const bool want_table = ssc_att_table_wanted(d->R, G, rpi);
  SscAttTable table;
  ssc_decode_step_desc sd{};
  sd.R = d->R; sd.feats = d->feats; sd.imgbuf = d->imgbuf; sd.alpha = (float*)(W + l.alpha); sd.log_probs = logits; sd.raw_logits = 1;
  sd.obj_atts = d->obj_atts;
  sd.G = G; sd.rows_per_image = rpi; sd.sentiment = d->sentiment;
  ScoreArgs a{};
  a.logits = logits; a.ld = (size_t)V; a.V = V; a.end_index = d->end_index; a.row_lp = lp;
  a.lp_stride = d->token_lp ? L : 1; a.rank_stride = L;
  int cur = 1;
  for (int t = 0; t < L; ++t) {
    sd.tokens = fed + (size_t)t * G;
    sd.eps = t == 0 ? d->eps0 : d->eps + (size_t)(t - 1) * G * Z;
    states.bind(W, cur, &sd);
    sd.att_table = table.next(want_table);
    sd.alpha = ssc_decode_alpha_at(d->attn, (float*)(W + l.alpha), t, G, d->R);
    ssc_forced_step_rows(&sd, t, parent0, lp, d->end_index);   // ended and absent rows (fed token END) are not stepped
    const SscStepGuide sg{guide, t, 1};
    SSC_TRY(ssc_decode_step_guided(cfg, p, &sd, &sg, W + l.stepws, l.stepws_bytes, st));
    a.target = tgt + (size_t)t * G;
    a.last_target = t == 0 ? nullptr : fed + (size_t)t * G;
    a.lp_out = d->token_lp ? d->token_lp + t : (float*)(W + l.steplp);
    a.rank_out = d->token_rank ? d->token_rank + t : nullptr;
    SSC_TRY(score_launch(a, G, st));
    cur = 1 - cur;
  }
  // the trace's ancestry is the identity wherever a target is scored: tgt holds -1 after a caption's end, for an absent slot and
  // from a negative id on
  if (d->attn) SSC_TRY(ssc_attn_anc(tgt, nullptr, nullptr, nullptr, L, G, 1, d->end_index, d->attn->anc, st));
  if (hipMemcpyAsync(d->log_probs, lp, (size_t)G * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  return SSC_OK;
}
