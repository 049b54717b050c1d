// Word-level sampling decoders: multinomial, top-k and top-p (nucleus) draws of one word per row, as a stand-alone row sampler
// (ssc_sample_rows) and as the whole sampled decode of a diverse-decode call in one library call (ssc_decode_sample).
// Reference: MultinomialSampler / TopKSampler / TopPSampler.sample_nodes (var_updown/var_updown/modules/beam_search.py:103-293)
// at per_node_beam_size 1, driven like the one-state beam search of ssc_decode_search with beam 1.
//
// One workgroup per row.  The row's raw logits are read from HBM once: for V <= SAMPLE_LDS_MAX_V into LDS, after which every pass
// (maximum, log-sum-exp, the radix selection of the cut, the draw) runs on LDS; longer rows take the same passes over global memory.
// The cut of top-k / top-p is a radix select (8-bit digits, most significant first) on an order-preserving key of the value, with
// per-bucket histograms of the count (top-k) or of the tempered probability mass in 2^-40 fixed point (top-p): integer LDS atomics
// only, so every histogram - and therefore the kept set - is independent of the order the lanes arrive in.  Ties at the cut are
// resolved by a second radix select on the index (lower index first).  The draw is Gumbel-max over the kept set with
// counter-based Philox4x32-10 noise: bit-reproducible for a given seed, no float atomics, no order-dependent reduction.
// The draw of one row (sample_draw_row) lives in sample_draw.h: the scheduled-sampling mix kernel of the train step calls the same code.
// The edits of the raw logits in front of the draw - the logit rules (logit_rules.hip) and the truncation (truncation.hip) - are launches
// of their own between a step's decode step and its draw (ssc_decode_sample_opts); the draw itself does not know of them.  Mirostat
// (mirostat.hip) adds a cut in front of and an update behind the draw, with a value per row carried between the steps
// (ssc_decode_sample_mirostat).  Arithmetic sampling (arith.hip) replaces the draw's launch by its own, with a code per row carried
// between the steps (ssc_decode_sample_arith).
// ssc_decode_sample's host loop is built from the shared driver of decode_loop.h ("the one-call decodes' host driver").
#include <math.h>

#include "decode_loop.h"
#include "sample_draw.h"

namespace {

struct SampleArgs {
  const float* logits; size_t ld; int V;
  int kind, top_k; float top_p, temperature;
  uint32_t seed_lo, seed_hi;
  const int64_t* row_ids; int step;
  const int64_t* last_pred; float* row_lp; int end_index;
  int64_t* pred_out; float* lp_out; float* probs_out;
  int* ctl; int max_steps; int* host_flag;
};

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  const int r = blockIdx.x;
  const int V = a.V;
  const bool stopped = a.ctl && a.ctl[0] <= a.step;   // (written by an EARLIER launch of this stream: the search has ended)
  const bool ended = stopped || (a.last_pred && a.last_pred[r] == a.end_index);   // workgroup-uniform
  int64_t tok = a.end_index;
  float lp = 0.f;
  if (!ended) {
    const float* g = a.logits + (size_t)r * a.ld;
    // the draw itself is shared with the scheduled-sampling mix kernel of the train step (sample_draw.h)
    const uint32_t b = (uint32_t)(a.row_ids ? a.row_ids[r] : r);
    const SampleDraw dr = sample_draw_row<STAGED>(g, srow, V, a.kind, a.top_k, a.top_p, a.temperature, a.seed_lo, a.seed_hi, a.step, b,
                                                  a.probs_out != nullptr, sh);
    const RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
    const float T = a.temperature, mx = dr.mx;
    const uint32_t cut_key = dr.cut_key;
    const int cut_idx = dr.cut_idx;
    float zk = dr.zk;
    tok = dr.tok;
    lp = dr.lp;
    if (a.probs_out) {   // the filtered, renormalised distribution in vocabulary order (tests, diagnostics)
      zk = block_sum(zk, sh);
      float* po = a.probs_out + (size_t)r * V;
      for (int v = threadIdx.x; v < V; v += SAMPLE_THREADS) {
        const float x = row.at(v);
        const uint32_t key = sample_key(x);
        const bool kept = key > cut_key || (key == cut_key && v <= cut_idx);
        po[v] = kept ? expf((x - mx) / T) / zk : 0.f;
      }
    }
  } else if (a.probs_out) {
    float* po = a.probs_out + (size_t)r * V;
    for (int v = threadIdx.x; v < V; v += SAMPLE_THREADS) po[v] = v == a.end_index ? 1.f : 0.f;
  }
  if (threadIdx.x == 0) {
    a.pred_out[r] = tok;
    a.lp_out[r] = lp;
    if (a.row_lp) a.row_lp[r] += lp;
  }
  // early stop: sample_step_done of sample_draw.h, shared with the arithmetic draw (arith.hip)
  if (a.ctl && threadIdx.x == 0) sample_step_done(a.ctl, a.max_steps, a.host_flag, a.step, stopped, tok != a.end_index);
}

int sample_launch(SampleArgs a, int rows, hipStream_t st) {
  return sample_row_launch(sample_rows_kernel<true>, sample_rows_kernel<false>, a.V, rows, st, a);
}

SampleArgs sample_args(const ssc_sampler_desc* s, const float* logits, size_t ld, int V) {
  SampleArgs a{};
  a.logits = logits; a.ld = ld; a.V = V;
  a.kind = s->kind; a.top_k = s->top_k; a.top_p = s->top_p; a.temperature = s->temperature;
  a.seed_lo = (uint32_t)(s->seed & 0xffffffffu); a.seed_hi = (uint32_t)(s->seed >> 32);
  return a;
}

// preds (max_steps, B) -> out (B, max_steps); columns >= ctl[0] (steps the host never queued) hold end_index
__global__ void sample_collect_kernel(const int64_t* __restrict__ preds, const int* __restrict__ ctl, int max_steps, int B,
                                      int end_index, int64_t* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int steps = ctl ? min(max(ctl[0], 1), max_steps) : max_steps;
  for (int t = 0; t < max_steps; ++t) out[(size_t)b * max_steps + t] = t < steps ? preds[(size_t)t * B + b] : end_index;
}

struct SampleLayout {
  SscStepStates states;   // (B, H) rows
  size_t tokens0;    // (B) int64 start tokens
  size_t parent0;    // (B) int64 zeros: every row is its own parent (the beam-1 search's parent list)
  size_t preds;      // (max_steps, B) int64
  size_t lp;         // (B) running caption log-probs
  size_t steplp;     // (B) the last step's log-probs
  size_t alpha;      // (B, R)
  size_t logits;     // (B, V)
  size_t stepws, stepws_bytes;
  size_t total;
};

SampleLayout sample_layout(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  SampleLayout l;
  const size_t B = (size_t)d->nimg * d->n_samples;
  size_t o = 0;
  l.states.reserve(o, B, cfg->H);
  l.tokens0 = ssc_ws_take(o, B * 8);
  l.parent0 = ssc_ws_take(o, B * 8);
  l.preds = ssc_ws_take(o, (size_t)d->max_steps * B * 8);
  l.lp = ssc_ws_take(o, B * 4);
  l.steplp = ssc_ws_take(o, B * 4);
  l.alpha = ssc_ws_take(o, B * (size_t)d->R * 4);
  l.logits = ssc_ws_take(o, B * (size_t)cfg->V * 4);
  l.stepws_bytes = ssc_decode_step_workspace_bytes(cfg, (int)B, d->R);
  l.stepws = ssc_ws_take(o, l.stepws_bytes);
  l.total = o;
  return l;
}

bool sample_desc_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!ssc_decode_dims_ok(cfg, d, d ? d->max_steps : 0)) return false;
  if (d->S != 1 || d->beam != 1 || d->fsm || d->tables || d->mach) return false;   // word sampling: one row per batch entry, no machine
  const long B = (long)d->nimg * d->n_samples;
  if (B > (1L << 24)) return false;
  return ssc_decode_inputs_ok(cfg, d, d->max_steps) && d->predictions && d->log_probs && d->ctl && ssc_decode_start_ok(d->start);
}

}  // namespace

// include/ssc_debug.h, ssc_debug_decode_view: where ssc_decode_sample keeps its chosen words (max_steps, B)
size_t ssc_sample_words_offset(const ssc_model_cfg* cfg, const ssc_search_desc* d) { return sample_layout(cfg, d).preds; }

extern "C" int ssc_sample_rows(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const int64_t* row_ids,
                               int step, const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out,
                               float* probs_out, void* stream) {
  if (!logits || !pred_out || !lp_out || rows < 0 || ld < V || step < 0 || !sampler_ok(s, V)) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  if (rows == 0) return SSC_OK;
  SampleArgs a = sample_args(s, logits, (size_t)ld, V);
  a.row_ids = row_ids; a.step = step; a.last_pred = last_pred; a.row_lp = row_lp; a.end_index = end_index;
  a.pred_out = pred_out; a.lp_out = lp_out; a.probs_out = probs_out;
  return sample_launch(a, rows, (hipStream_t)stream);
}

namespace {

// The amateur stream of a contrastive call (ssc_contrast, include/ssc.h), behind the expert's blocks: what an ensemble member has of
// its own - two generations of states, alpha scratch, a logits block and a step workspace.  An amateur is stepped iff alpha != 0.
struct AmateurLayout {
  SscStepStates states;
  size_t alpha, logits, stepws, stepws_bytes;
};
inline bool contrast_steps_amateur(const ssc_contrast* c) { return c && c->alpha != 0.f; }
size_t contrast_layout(const ssc_model_cfg* cfg, const ssc_search_desc* d, const SampleLayout& l, AmateurLayout* am) {
  const size_t B = (size_t)d->nimg * d->n_samples;
  size_t o = l.total;
  am->states.reserve(o, B, cfg->H);
  am->alpha = ssc_ws_take(o, B * (size_t)d->R * 4);
  am->logits = ssc_ws_take(o, B * (size_t)cfg->V * 4);
  am->stepws_bytes = l.stepws_bytes;
  am->stepws = ssc_ws_take(o, am->stepws_bytes);
  return o;
}

// the fields of a caller's ssc_sample_opts that lie inside its `bytes` (include/ssc.h: the `bytes` rule), the others null; opts null:
// every field null.  false: a size this library refuses.  Every field behind `bytes` is one pointer, so a whole number of pointers
// holds whole fields.
static_assert(sizeof(ssc_sample_opts) == 5 * sizeof(void*), "ssc_sample_opts: the size and four pointers (a later option: one more)");
bool sample_opts_read(const ssc_sample_opts* opts, ssc_sample_opts* o) {
  *o = ssc_sample_opts{};
  if (!opts) return true;
  const size_t n = opts->bytes;
  if (n < sizeof(size_t) || n % sizeof(void*) != 0 || n > sizeof(ssc_sample_opts)) return false;
  memcpy(o, opts, n);
  return true;
}

}  // namespace

extern "C" size_t ssc_decode_sample_opts_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d,
                                                         const ssc_sample_opts* opts) {
  ssc_sample_opts o;
  if (!sample_opts_read(opts, &o) || !ssc_decode_dims_ok(cfg, d, d ? d->max_steps : 0)) return 0;
  const SampleLayout l = sample_layout(cfg, d);
  if (!contrast_steps_amateur(o.contrast)) return l.total;
  AmateurLayout am;
  return contrast_layout(cfg, d, l, &am);
}

// Mirostat's (include/ssc.h, ssc_mirostat) share of the workspace: the cut's norm, 2 B floats, behind everything else
inline size_t mirostat_norm_bytes(const ssc_search_desc* d) { return ((size_t)d->nimg * d->n_samples * 2 * 4 + 255) & ~(size_t)255; }

extern "C" size_t ssc_decode_sample_mirostat_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d,
                                                             const ssc_sample_opts* opts, const ssc_mirostat* m) {
  const size_t base = ssc_decode_sample_opts_workspace_bytes(cfg, d, opts);
  if (base == 0 || !m || m->tau == 0.f) return base;
  return ((base + 255) & ~(size_t)255) + mirostat_norm_bytes(d);
}

extern "C" size_t ssc_decode_sample_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  return ssc_decode_sample_opts_workspace_bytes(cfg, d, nullptr);
}

extern "C" int ssc_decode_sample(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return ssc_decode_sample_opts(cfg, p, d, s, nullptr, workspace, workspace_bytes, stream);
}

// The sampled decode under its options (include/ssc.h, ssc_sample_opts).  Per step: the expert's decode step (its z block from slab t
// of the guide), the amateur's decode step, the contrast, the logit rules, the truncation, the draw; step t's statistics go to slab t
// of contrast->kept / ->divergence and trunc->entropy / ->kept.  Under an active Mirostat (m, may be null) the cut follows the
// truncation with slab t of m->mu and the update follows the draw, slab t -> slab t + 1.  Under an active arithmetic descriptor (ar,
// may be null) the draw of step t is ssc_arith_rows with slab t of ar->code, writing slab t + 1.
namespace {
int sample_decode(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                  const ssc_sample_opts* opts, const ssc_mirostat* m, const ssc_arith* ar, void* workspace, size_t workspace_bytes,
                  void* stream) {
  ssc_sample_opts o;
  if (!sample_opts_read(opts, &o)) return SSC_EINVAL;
  const ssc_latent_guide* guide = o.guide;
  const ssc_logit_rules* rules = o.rules;
  const ssc_truncation* trunc = o.trunc;
  const ssc_contrast* contrast = o.contrast;
  SscGemmModeScope mode_scope(cfg);   // the numerics mode of this cfg, for every product the call issues
  if (!p || !workspace || !sample_desc_ok(cfg, d) || !sampler_ok(s, cfg->V)) return SSC_EINVAL;
  if (guide && !ssc_latent_guide_ok(cfg, guide)) return SSC_EINVAL;
  if (!ssc_decode_start_ok(d->start, !guide)) return SSC_EINVAL;   // (no start state under a guide)
  bool contrasted = false;
  if (contrast) {
    const int rc = ssc_contrast_check(contrast->alpha, contrast->beta, contrast->kept, contrast->divergence, &contrasted);
    if (rc == SSC_EINVAL) return rc;
    if ((contrast->feats != nullptr) != (contrast->imgbuf != nullptr) || (contrast->params && !contrast->imgbuf)) return SSC_EINVAL;
    if (contrast->guide_mode != 0 && contrast->guide_mode != 1) return SSC_EINVAL;
    if (contrast_steps_amateur(contrast)) {   // (an amateur that is not stepped reads no start state)
      if ((contrast->start != nullptr) != (d->start != nullptr)) return SSC_EINVAL;
      const ssc_start_state* cs = contrast->start;
      if (cs && !(cs->h1 && cs->c1 && cs->hd && cs->cd)) return SSC_EINVAL;   // (its tokens are not read: the expert's are fed)
    }
    SSC_TRY(rc);
  }
  const bool amateur = contrasted && contrast_steps_amateur(contrast);
  bool ruled = false;
  if (rules) {
    SSC_TRY(ssc_logit_rules_check(rules, cfg->V, d->end_index, &ruled));
    if (ruled && (d->max_steps > SSC_RULES_MAX_LEN || (long)cfg->V <= (long)d->max_steps + rules->n_suppress)) return SSC_EINVAL;
  }
  bool cut = false;
  if (trunc) SSC_TRY(ssc_truncation_check(trunc, s->temperature, &cut));
  bool miro = false;
  SSC_TRY(ssc_mirostat_check(m, s->temperature, &miro));
  bool arith = false;
  SSC_TRY(ssc_arith_check(ar, &arith));
  const SampleLayout l = sample_layout(cfg, d);
  AmateurLayout am{};
  size_t total = amateur ? contrast_layout(cfg, d, l, &am) : l.total;
  size_t norm_at = 0;
  if (miro) {   // (the cut's norm behind everything else: no existing offset moves)
    norm_at = (total + 255) & ~(size_t)255;
    total = norm_at + mirostat_norm_bytes(d);
  }
  if (workspace_bytes < total) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* W = (char*)workspace;
  const int B = d->nimg * d->n_samples, V = cfg->V, Z = cfg->Z;
  const SscStepStates& states = l.states;
  int64_t* tokens0 = (int64_t*)(W + l.tokens0);
  int64_t* parent0 = (int64_t*)(W + l.parent0);
  int64_t* preds = (int64_t*)(W + l.preds);
  float* lp = (float*)(W + l.lp);
  float* steplp = (float*)(W + l.steplp);
  float* logits = (float*)(W + l.logits);
  int* ctl = d->ctl;

  // where the call starts: zero states and @@BOUNDARY@@, or the caller's start state
  SSC_TRY(ssc_decode_start(ctl, d->max_steps, tokens0, B, d->end_index, d->start ? d->start->tokens : nullptr, V, st));
  if (hipMemsetAsync(parent0, 0, (size_t)B * 8, st) != hipSuccess) return SSC_EHIP;
  if (hipMemsetAsync(lp, 0, (size_t)B * 4, st) != hipSuccess) return SSC_EHIP;
  SSC_TRY(ssc_decode_start_states(d->start, states, W, 1, B, st));
  if (amateur) SSC_TRY(ssc_decode_start_states(contrast->start, am.states, W, 1, B, st));
  float* norm = miro ? (float*)(W + norm_at) : nullptr;
  if (miro) SSC_TRY(ssc_mirostat_fill(m->mu, B, m->mu0, st));   // (slab 0; under d->start too: the control starts at the continuation)
  if (arith && ar->mode == 1) SSC_TRY(ssc_arith_codes_launch(s->seed, d->nimg, d->n_samples, ar->code, st));   // (slab 0, likewise)

  // the steps take the form the beam-1 search gives them (ssc_decode_search with S = beam = 1): same tables, same parent list
  const bool want_table = ssc_att_table_wanted(d->R, B, d->n_samples);
  SscAttTable table;
  ssc_decode_step_desc sd{};
  sd.R = d->R; sd.feats = d->feats; sd.imgbuf = d->imgbuf; sd.alpha = (float*)(W + l.alpha); sd.log_probs = logits; sd.raw_logits = 1;
  sd.obj_atts = d->obj_atts;
  sd.G = B; sd.rows_per_image = d->n_samples; sd.tokens = tokens0; sd.sentiment = d->sentiment; sd.eps = d->eps0;
  states.bind(W, 1, &sd);
  sd.att_table = table.next(want_table);
  sd.alpha = ssc_decode_alpha_at(d->attn, (float*)(W + l.alpha), 0, B, d->R);
  SscStepGuide sg{guide, 0, 1};
  SSC_TRY(ssc_decode_step_guided(cfg, p, &sd, &sg, W + l.stepws, l.stepws_bytes, st));
  // the amateur's step: the expert's descriptor - the same fed tokens, parent list and skipped rows - over its own context, noise,
  // states and blocks; its attention weights stay in its scratch (the trace records the expert)
  const ssc_params* pa = amateur && contrast->params ? contrast->params : p;
  SscAttTable table_a;
  SscStepGuide sga{amateur && contrast->guide_mode == 0 ? guide : nullptr, 0, 1};
  const float* eps_a = amateur && contrast->eps ? contrast->eps : d->eps;
  auto amateur_step = [&](int gen) {
    ssc_decode_step_desc sa = sd;
    if (contrast->imgbuf) { sa.feats = contrast->feats; sa.imgbuf = contrast->imgbuf; }
    if (contrast->sentiment) sa.sentiment = contrast->sentiment;
    if (contrast->obj_atts) sa.obj_atts = contrast->obj_atts;
    sa.eps = sga.t == 0 ? (contrast->eps0 ? contrast->eps0 : d->eps0) : eps_a + (size_t)(sga.t - 1) * B * Z;
    sa.alpha = (float*)(W + am.alpha); sa.log_probs = (float*)(W + am.logits);
    am.states.bind(W, gen, &sa);
    sa.att_table = table_a.next(want_table);
    return ssc_decode_step_guided(cfg, pa, &sa, &sga, W + am.stepws, am.stepws_bytes, st);
  };
  if (amateur) SSC_TRY(amateur_step(1));
  SampleArgs a = sample_args(s, logits, (size_t)V, V);
  a.end_index = d->end_index; a.row_lp = lp; a.lp_out = steplp;
  a.ctl = d->early_stop ? ctl : nullptr; a.max_steps = d->max_steps; a.host_flag = d->early_stop ? d->host_flag : nullptr;
  // the tail of step t, behind its decode steps: the edits of the expert's logits in place - the contrast against the amateur's, the
  // logit rules, the truncation, their statistics going to slab t - and the draw; last: the previous step's words (null at step 0)
  auto edit_and_draw = [&](int t, const int64_t* last) -> int {
    if (contrasted)
      SSC_TRY(ssc_contrast_launch(logits, V, amateur ? (const float*)(W + am.logits) : nullptr, V, B, V, contrast->alpha, contrast->beta,
                                  contrast->kept ? contrast->kept + (size_t)t * B : nullptr,
                                  contrast->divergence ? contrast->divergence + (size_t)t * B : nullptr, last, d->end_index, st));
    if (ruled) SSC_TRY(ssc_logit_rules_launch(logits, V, B, V, rules, preds, B, t, d->end_index, st));
    if (cut)
      SSC_TRY(ssc_truncation_launch(logits, V, B, V, trunc, s->temperature, trunc->entropy ? trunc->entropy + (size_t)t * B : nullptr,
                                    trunc->kept ? trunc->kept + (size_t)t * B : nullptr, last, d->end_index, st));
    a.step = t; a.last_pred = last; a.pred_out = preds + (size_t)t * B;
    // the draw: the sampler's own, or the arithmetic one along the rows' codes, slab t -> slab t + 1
    auto draw = [&]() -> int {
      if (!arith) return sample_launch(a, B, st);
      uint64_t* code = ar->code + (size_t)t * B;
      return ssc_arith_rows_launch(logits, V, B, V, s, code, last, lp, d->end_index, a.pred_out, steplp, code + B, nullptr, t, a.ctl,
                                   a.max_steps, a.host_flag, st);
    };
    if (!miro) return draw();
    float* mu = m->mu + (size_t)t * B;
    SSC_TRY(ssc_mirostat_rows_launch(logits, V, B, V, s->temperature, mu, last, d->end_index, m->kept ? m->kept + (size_t)t * B : nullptr,
                                     norm, st));
    SSC_TRY(draw());
    return ssc_mirostat_update_launch(logits, V, B, V, s->temperature, m->tau, m->eta, norm, a.pred_out, last, d->end_index, mu, mu + B,
                                      m->surprise ? m->surprise + (size_t)t * B : nullptr, st);
  };
  SSC_TRY(edit_and_draw(0, nullptr));
  const SscStepPacer pacer(d->early_stop, d->host_flag_host, st);   // (the sampler's last workgroup of a step notes it for the host)
  int cur = 0;
  sd.parent = parent0; sd.group = 1;
  for (int t = 1; t < d->max_steps; ++t) {
    if (pacer.stop_before(t)) break;
    const int64_t* last = preds + (size_t)(t - 1) * B;
    sd.tokens = last; sd.eps = d->eps + (size_t)(t - 1) * B * Z;
    states.bind(W, cur, &sd);
    sd.att_table = table.next(want_table);
    sd.alpha = ssc_decode_alpha_at(d->attn, (float*)(W + l.alpha), t, B, d->R);
    sd.row_lp = d->skip_dead ? lp : nullptr; sd.end_index = d->end_index;   // ended rows are not stepped
    sg.t = t;
    SSC_TRY(ssc_decode_step_guided(cfg, p, &sd, &sg, W + l.stepws, l.stepws_bytes, st));
    sga.t = t;
    if (amateur) SSC_TRY(amateur_step(cur));
    SSC_TRY(edit_and_draw(t, last));
    cur = 1 - cur;
  }
  SSC_LAUNCH(sample_collect_kernel, dim3(ssc_cdiv(B, 64)), dim3(64), 0, st, preds, d->early_stop ? ctl : nullptr, d->max_steps, B,
             d->end_index, d->predictions);
  SSC_CHECK_LAUNCH();
  if (d->attn)   // the trace's ancestry is the identity: row b, until the row has ended or the call has stopped
    SSC_TRY(ssc_attn_anc(preds, nullptr, d->early_stop ? ctl : nullptr, nullptr, d->max_steps, B, 1, d->end_index, d->attn->anc, st));
  if (hipMemcpyAsync(d->log_probs, lp, (size_t)B * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  return SSC_OK;
}
}  // namespace

extern "C" int ssc_decode_sample_opts(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                      const ssc_sampler_desc* s, const ssc_sample_opts* opts, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return sample_decode(cfg, p, d, s, opts, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ssc_decode_sample_mirostat(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                          const ssc_sampler_desc* s, const ssc_sample_opts* opts, const ssc_mirostat* m, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return sample_decode(cfg, p, d, s, opts, m, nullptr, workspace, workspace_bytes, stream);
}

// the arithmetic draw needs no workspace of its own: its codes live in the caller's block
extern "C" size_t ssc_decode_sample_arith_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d,
                                                          const ssc_sample_opts* opts, const ssc_mirostat* m, const ssc_arith* a) {
  (void)a;
  return ssc_decode_sample_mirostat_workspace_bytes(cfg, d, opts, m);
}

extern "C" int ssc_decode_sample_arith(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                       const ssc_sampler_desc* s, const ssc_sample_opts* opts, const ssc_mirostat* m, const ssc_arith* a,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return sample_decode(cfg, p, d, s, opts, m, a, workspace, workspace_bytes, stream);
}
