// The whole constrained beam search of one diverse-decode call as ONE sequence-level entry point (ssc_decode_search):
// first step, state enlargement, then per step  decode step -> selection -> back-pointers  with the early-stop bookkeeping on the
// device - launched from here like ssc_train_fwd launches the training time loop: no Python and no framework glue between the
// steps (round 3's driver issued ~100 copy / fill / elementwise launches per call from torch around the ~25 library launches of a
// step).  The step states, the table decision, the early-stop pacing and the descriptor checks are the shared host driver of
// decode_loop.h ("the one-call decodes' host driver").
// Reference: ConstrainedBeamSearch.search (updown-baseline/updown/modules/cbs.py:59-277) driving
// UpDownCaptioner._decode_step in eval mode (var_updown/var_updown/models/updown_captioner.py:371-455), as the reference's
// inference loop does per image and latent sample (var_updown/scripts/inference.py:117-189).
#include <math.h>

#include <algorithm>

#include "decode_loop.h"

namespace {

// The selection a search runs: beam search (the machine's top-k), the stochastic beam search (Gumbel-top-k, sbs.hip) or the
// sampled-node beam search (a word sampler's draws per beam, sampled_beam.hip) or the diverse beam search (groups of beams with a
// Hamming penalty, diverse_beam.hip) or the beam search under the decode rules (n-gram blocking, minimum length, suppressed tokens,
// length penalty: rules_beam.hip).
// SEARCH_ENSEMBLE: the beam search over several members (ssc_decode_search_ensemble): the layout of SEARCH_BEAM, never the records head.
enum SearchKind { SEARCH_BEAM, SEARCH_GUMBEL, SEARCH_SAMPLED, SEARCH_DIVERSE, SEARCH_RULES, SEARCH_ENSEMBLE };

// The vocabulary head of the later steps leaves per-tile records instead of logits (ssc_decode_step_desc.topk_part) when the machine
// is the trivial one, at most two candidates per row are wanted and the head is one aligned 3xBF16 / 2xFP16 product.  Beam search
// only: any token can win a Gumbel draw or a sampler's draw, a penalised row needs more than its two best tokens, and a ban of
// the decode rules can remove both records of a tile, so those selections read the raw logits.
bool search_uses_parts(const ssc_model_cfg* cfg, const ssc_search_desc* d, SearchKind kind) {
  const long G = (long)d->nimg * d->n_samples * d->S * d->beam;
  return kind == SEARCH_BEAM && d->S == 1 && !d->fsm && !d->tables && d->per_node <= 2 && !cfg->tied && cfg->gemm_mode != 2 &&
         cfg->H % 4 == 0 && G >= 512 && ssc_decode_parts_enabled();
}

struct SearchLayout {
  SscStepStates states;   // (G, H) rows; 2xFP16 numerics: with the fp16 pieces of h1, hd, (G, Hk) words
  size_t tokens0;      // (B) int64 start tokens
  size_t sent_rows;    // (G) float
  size_t preds;        // (max_steps, B, SB) int64
  size_t backs;        // (max_steps-1, B, SB) int64
  size_t parent0;      // (B, SB) int64 zeros: every beam of the first expanded step descends from the one start row
  size_t lp[2];        // (B, S, beam) float
  size_t gs[2];        // gumbel: (B, beam) float, the beams' G (empty for beam search)
  size_t rhist[2], rlen[2], rscore[2];   // rules: (G, max_steps) int32 histories, (G) int32 lengths, (G) float scores (empty otherwise)
  size_t sval, sidx;   // B*S*SB*per_node (gumbel: twice as many values - the candidates' G and log-probs; diverse: the rows' lists,
                       // `list` entries per row instead of per_node)
  size_t alpha;        // (G, R)
  size_t logits;       // (G, V); (B, V) when the later steps leave records
  size_t parts;        // (G, ceil(V / 128), 6) records
  size_t stepws;       // ssc_decode_step workspace
  size_t stepws_bytes;
  size_t total;
};

SearchLayout search_layout(const ssc_model_cfg* cfg, const ssc_search_desc* d, SearchKind kind, int list = 0) {
  SearchLayout l;
  const size_t per_row = kind == SEARCH_DIVERSE ? (size_t)std::max(list, d->beam) : (size_t)d->per_node;
  const bool gumbel = kind == SEARCH_GUMBEL;
  const size_t B = (size_t)d->nimg * d->n_samples, SB = (size_t)d->S * d->beam, G = B * SB;
  size_t o = 0;
  const size_t prow = cfg->gemm_mode == 3 && !cfg->tied && G >= 512 ? (size_t)ssc_decode_planes_ld(cfg) : 0;
  l.states.reserve(o, G, cfg->H, prow);
  l.tokens0 = ssc_ws_take(o, B * 8);
  l.sent_rows = ssc_ws_take(o, G * 4);
  l.preds = ssc_ws_take(o, (size_t)d->max_steps * G * 8);
  l.backs = ssc_ws_take(o, (size_t)std::max(d->max_steps - 1, 1) * G * 8);
  l.parent0 = ssc_ws_take(o, G * 8);
  for (int g = 0; g < 2; ++g) l.lp[g] = ssc_ws_take(o, G * 4);
  for (int g = 0; g < 2; ++g) l.gs[g] = ssc_ws_take(o, gumbel ? G * 4 : 0);
  const bool rules = kind == SEARCH_RULES;
  for (int g = 0; g < 2; ++g) {
    l.rhist[g] = ssc_ws_take(o, rules ? G * (size_t)d->max_steps * 4 : 0);
    l.rlen[g] = ssc_ws_take(o, rules ? G * 4 : 0);
    l.rscore[g] = ssc_ws_take(o, rules ? G * 4 : 0);
  }
  l.sval = ssc_ws_take(o, B * d->S * SB * per_row * 4 * (gumbel ? 2 : 1));
  l.sidx = ssc_ws_take(o, B * d->S * SB * per_row * 8);
  l.alpha = ssc_ws_take(o, G * (size_t)d->R * 4);
  const bool parts = search_uses_parts(cfg, d, kind);
  l.logits = ssc_ws_take(o, (parts ? B : G) * (size_t)cfg->V * 4);
  l.parts = ssc_ws_take(o, parts ? G * (size_t)ssc_cdiv(cfg->V, 128) * 6 * 4 : 0);
  l.stepws_bytes = ssc_decode_step_workspace_bytes(cfg, (int)G, d->R);
  l.stepws = ssc_ws_take(o, l.stepws_bytes);
  l.total = o;
  return l;
}

// the extents a search's workspace size depends on
bool search_dims_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  return ssc_decode_dims_ok(cfg, d, d ? d->max_steps : 0) && d->S > 0 && d->beam > 0 && d->per_node > 0;
}

bool desc_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!search_dims_ok(cfg, d) || d->S > 32) return false;
  const long G = (long)d->nimg * d->n_samples * d->S * d->beam;
  if (G <= 0 || G > (1L << 24)) return false;
  if (!ssc_decode_inputs_ok(cfg, d, d->max_steps) || !d->predictions || !d->log_probs || !d->ctl) return false;
  if (d->S > 1 && !d->fsm) return false;
  if (!ssc_decode_start_ok(d->start)) return false;
  if (d->skip_dead && !d->tables && (d->S != 1 || d->fsm)) return false;   // (the one-state machine has no fill-only rows: skip_dead then only leaves ENDED beams out of the steps)
  return true;
}

__global__ void fill_i64_kernel(int64_t* __restrict__ p, size_t n, int64_t v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// a start state's tokens: the caller's, an id that cannot index the embedding replaced by END
__global__ void start_tokens_kernel(const int64_t* __restrict__ src, int n, int V, int end_index, int64_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int64_t x = src[i];
    dst[i] = x >= 0 && x < V ? x : (int64_t)end_index;
  }
}
__global__ void ctl_init_kernel(int* __restrict__ ctl, int n, int max_steps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ctl[i] = i == 0 ? max_steps : 0;
}
// dst row g <- src row g / rep   (cbs.py:10-17: the start row's state for every (state, beam) of its batch entry)
__global__ void expand_rows_kernel(const float* __restrict__ src, int Wd, int rep, size_t rows, float* __restrict__ dst) {
  const size_t row = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (row < rows && x < Wd) dst[row * Wd + x] = src[(row / rep) * Wd + x];
}

}  // namespace

int ssc_decode_start(int* ctl, int max_steps, int64_t* tokens0, int B, int end_index, const int64_t* start_tokens, int V,
                     hipStream_t st) {
  const int nctl = 2 + 2 * max_steps;
  SSC_LAUNCH(ctl_init_kernel, dim3(ssc_cdiv(nctl, 256)), dim3(256), 0, st, ctl, nctl, max_steps);
  SSC_CHECK_LAUNCH();
  if (start_tokens) {
    SSC_LAUNCH(start_tokens_kernel, dim3(ssc_cdiv(B, 256)), dim3(256), 0, st, start_tokens, B, V, end_index, tokens0);
    SSC_CHECK_LAUNCH();
    return SSC_OK;
  }
  SSC_LAUNCH(fill_i64_kernel, dim3(ssc_cdiv(B, 256)), dim3(256), 0, st, tokens0, (size_t)B, (int64_t)end_index);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" size_t ssc_decode_search_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!search_dims_ok(cfg, d)) return 0;
  return search_layout(cfg, d, SEARCH_BEAM).total;
}

namespace {

// The selections the search loop below runs: beam search (the machine's top-k, ssc_beam_*_fsm / ssc_beam_step_parts), the
// stochastic beam search (Gumbel-top-k, sbs.hip), the sampled-node beam search (sampled_beam.hip) and the diverse beam search
// (diverse_beam.hip) and the beam search under the decode rules (rules_beam.hip).  first() selects step 0;
// step(a) a later step, reading the running state of generation a and writing generation 1 - a.
struct BeamSelect {
  bool use_parts;
  const float* parts;
  int first(ssc_beam_desc* bd, hipStream_t st) const { return ssc_beam_first_fsm(bd, st); }
  int step(ssc_beam_desc* bd, int, hipStream_t st) const {
    return use_parts ? ssc_beam_step_parts(bd, parts, st) : ssc_beam_step_fsm(bd, st);
  }
};
struct GumbelSelect {
  const ssc_gumbel_desc* s;
  float* g[2];
  int first(ssc_beam_desc* bd, hipStream_t st) const { return ssc_beam_first_gumbel(bd, s, g[0], st); }
  int step(ssc_beam_desc* bd, int a, hipStream_t st) const { return ssc_beam_step_gumbel(bd, s, g[a], g[1 - a], st); }
};
struct SampledSelect {   // step 0 is the word samplers' sample_beams: the plain top-k of the trivial machine
  const ssc_sampler_desc* s;
  int with_replacement;
  int first(ssc_beam_desc* bd, hipStream_t st) const { return ssc_beam_first_fsm(bd, st); }
  int step(ssc_beam_desc* bd, int, hipStream_t st) const { return ssc_beam_step_sampled(bd, s, with_replacement, st); }
};

struct DiverseSelect {
  const ssc_diverse_desc* s;
  int first(ssc_beam_desc* bd, hipStream_t st) const { return ssc_beam_first_diverse(bd, s, st); }
  int step(ssc_beam_desc* bd, int, hipStream_t st) const { return ssc_beam_step_diverse(bd, s, st); }
};

struct RulesSelect {   // generation a of the histories, lengths and scores goes with generation a of the log-probs
  const ssc_rules_desc* r;
  int* hist[2]; int* len[2]; float* score[2];
  int ld_hist;
  int first(ssc_beam_desc* bd, hipStream_t st) const {
    const ssc_rules_state s{nullptr, nullptr, hist[0], len[0], score[0], ld_hist};
    return ssc_beam_first_rules(bd, r, &s, st);
  }
  int step(ssc_beam_desc* bd, int a, hipStream_t st) const {
    const ssc_rules_state s{hist[a], len[a], hist[1 - a], len[1 - a], score[1 - a], ld_hist};
    return ssc_beam_step_rules(bd, r, &s, st);
  }
};

// What a search steps: one member per parameter set, each with its image buffer, its two generations of states, its logits
// block, its step workspace and its attended-feature-table decision.  The plain searches run a list of one over the blocks of
// their SearchLayout (search_self); ssc_decode_search_ensemble runs up to SSC_ENSEMBLE_MAX.
struct SearchMember {
  const ssc_params* p;
  const void* imgbuf;
  SscStepStates states;
  size_t logits, stepws;   // offsets into the workspace
  SscAttTable table;
};
SearchMember search_self(const ssc_params* p, const ssc_search_desc* d, const SearchLayout& l) {
  return SearchMember{p, d->imgbuf, l.states, l.logits, l.stepws, SscAttTable{}};
}
// Several members: where their logits are combined (ssc_ensemble_combine_rows) for the selection, which then reads log-probs.
struct SearchCombine {
  float logw[SSC_ENSEMBLE_MAX];
  int mode;
  size_t out;   // (G, V) block of the workspace
};

// final_gen: the generation of the running per-beam state (lp, and a selection's own) that holds the search's last step
// mem / M: the members (a list of one issues the launches of a single-model search); comb: null for a single-model search, whose
// selection normalises the one member's raw logits itself
// guide: the call's latent guide (ssc_decode_search_guided) or null - step t's z block then comes from its slab t, one entry per
// batch entry: one row in the first step, S * beam rows in the later ones
template <class Select>
int search_run(const ssc_model_cfg* cfg, SearchMember* mem, int M, const SearchCombine* comb, const ssc_search_desc* d,
               const SearchLayout& l, char* W, const Select& sel, bool use_parts, hipStream_t st, int* final_gen = nullptr,
               const ssc_latent_guide* guide = nullptr) {
  const int B = d->nimg * d->n_samples, S = d->S, beam = d->beam, SB = S * beam, G = B * SB, H = cfg->H, V = cfg->V, Z = cfg->Z;
  int64_t* tokens0 = (int64_t*)(W + l.tokens0);
  float* sent_rows = (float*)(W + l.sent_rows);
  int64_t* preds = (int64_t*)(W + l.preds);
  int64_t* backs = (int64_t*)(W + l.backs);
  int64_t* parent0 = (int64_t*)(W + l.parent0);
  float* lp[2] = {(float*)(W + l.lp[0]), (float*)(W + l.lp[1])};
  float* alpha = (float*)(W + l.alpha);
  const size_t plane = (size_t)G;
  // the scores the selection reads: the one member's raw logits, or the members' combined log-probs
  const float* scores = comb ? (const float*)(W + comb->out) : (const float*)(W + mem[0].logits);
  const float* mlogits[SSC_ENSEMBLE_MAX];
  for (int m = 0; m < M; ++m) mlogits[m] = (const float*)(W + mem[m].logits);
  ssc_ensemble_rows_desc ed{M, mlogits, V, comb ? comb->logw : nullptr, comb ? comb->mode : 0};

  // where the call starts: zero states and @@BOUNDARY@@, or the caller's start state (never with several members)
  SSC_TRY(ssc_decode_start(d->ctl, d->max_steps, tokens0, B, d->end_index, d->start ? d->start->tokens : nullptr, V, st));
  if (hipMemsetAsync(parent0, 0, (size_t)G * 8, st) != hipSuccess) return SSC_EHIP;
  for (int m = 0; m < M; ++m) SSC_TRY(ssc_decode_start_states(d->start, mem[m].states, W, 1, B, st));

  // which form the steps take is decided once per extent: the first step's B rows and the later steps' G rows each ask
  ssc_decode_step_desc sd{};
  sd.R = d->R; sd.feats = d->feats; sd.alpha = alpha; sd.raw_logits = 1;
  sd.obj_atts = d->obj_atts;
  // ---- first step: one row per batch entry (cbs.py:127) ------------------------------------------------------------------
  sd.G = B; sd.rows_per_image = d->n_samples; sd.tokens = tokens0; sd.sentiment = d->sentiment; sd.eps = d->eps0;
  sd.alpha = ssc_decode_alpha_at(d->attn, alpha, 0, G, d->R);   // (a trace's slab 0: the B rows of this step are its head)
  for (int m = 0; m < M; ++m) {
    sd.imgbuf = mem[m].imgbuf; sd.log_probs = (float*)(W + mem[m].logits);
    mem[m].states.bind(W, 1, &sd);
    sd.att_table = mem[m].table.next(ssc_att_table_wanted(d->R, B, d->n_samples));
    const SscStepGuide sg{guide, 0, 1};
    SSC_TRY(ssc_decode_step_guided(cfg, mem[m].p, &sd, &sg, W + mem[m].stepws, l.stepws_bytes, st));
  }
  if (comb) SSC_TRY(ssc_ensemble_combine_rows(&ed, B, V, nullptr, nullptr, d->end_index, (float*)(W + comb->out), V, st));
  ssc_beam_desc bd{};
  bd.scores = scores; bd.ld = V; bd.raw_logits = comb ? 0 : 1;
  bd.fsm = d->fsm; bd.tables = d->tables; bd.dims = d->dims; bd.mach = d->mach;
  if (!d->tables) { bd.dims.M = d->mach ? 0 : B; bd.dims.S = S; bd.dims.V = V; bd.dims.E = 0; bd.dims.P = 1; }
  if (bd.dims.S != S || bd.dims.V != V) return SSC_EINVAL;
  bd.B = B; bd.beam = beam; bd.per_node = d->per_node; bd.end_index = d->end_index;
  bd.pred = preds; bd.lp_out = lp[0];
  bd.ctl = d->early_stop ? d->ctl : nullptr; bd.max_steps = d->max_steps; bd.host_flag = d->early_stop ? d->host_flag : nullptr;
  bd.scratch_val = (float*)(W + l.sval); bd.scratch_idx = (int64_t*)(W + l.sidx);
  SSC_TRY(sel.first(&bd, st));
  // ---- enlarge the states to (B, S, beam) rows (cbs.py:152-155) --------------------------------------------------------------
  if (d->max_steps > 1) {
    for (int m = 0; m < M; ++m)
      for (int k = 0; k < 4; ++k) {
        SSC_LAUNCH(expand_rows_kernel, dim3(ssc_cdiv(H, 256), G), dim3(256), 0, st, mem[m].states.state(W, 0, k), H, SB, (size_t)G,
                   mem[m].states.state(W, 1, k));
        SSC_CHECK_LAUNCH();
      }
    if (d->sentiment) {
      SSC_LAUNCH(expand_rows_kernel, dim3(1, G), dim3(64), 0, st, d->sentiment, 1, SB, (size_t)G, sent_rows);
      SSC_CHECK_LAUNCH();
    }
  }
  int cur = 1, a = 0;
  const int rpi = d->n_samples * SB;
  const bool tmode = ssc_att_table_wanted(d->R, G, rpi);
  const bool ung = SB > 1 && ssc_decode_ungathered_ok(cfg, d->nimg, G, SB, tmode) != 0;
  bool ungathered = false;
  sd.G = G; sd.rows_per_image = rpi; sd.sentiment = d->sentiment ? sent_rows : nullptr; sd.group = SB;
  bd.skip_dead = d->skip_dead && d->tables ? 1 : 0;
  const SscStepPacer pacer(d->early_stop, d->host_flag_host, st);
  for (int t = 1; t < d->max_steps; ++t) {
    if (pacer.stop_before(t)) break;   // cbs.py:167
    const int64_t* last = preds + (size_t)(t - 1) * plane;
    sd.tokens = last; sd.eps = d->eps + (size_t)(t - 1) * G * Z;
    sd.parent = t == 1 ? parent0 : backs + (size_t)(t - 2) * plane;
    sd.alpha = ssc_decode_alpha_at(d->attn, alpha, t, G, d->R);
    sd.ungathered = ungathered ? 1 : 0;
    sd.row_lp = d->skip_dead ? lp[a] : nullptr; sd.end_index = d->end_index;
    for (int m = 0; m < M; ++m) {
      sd.imgbuf = mem[m].imgbuf; sd.log_probs = (float*)(W + mem[m].logits);
      mem[m].states.bind(W, cur, &sd);
      mem[m].states.bind_planes(W, cur, ungathered, &sd);
      sd.att_table = mem[m].table.next(tmode);
      if (use_parts) { sd.log_probs = nullptr; sd.topk_part = (float*)(W + l.parts); }
      const SscStepGuide sg{guide, t, SB};
      SSC_TRY(ssc_decode_step_guided(cfg, mem[m].p, &sd, &sg, W + mem[m].stepws, l.stepws_bytes, st));
    }
    if (comb)   // the rows the steps have left unspecified (row_lp) are not read and not written
      SSC_TRY(ssc_ensemble_combine_rows(&ed, G, V, d->skip_dead ? last : nullptr, d->skip_dead ? lp[a] : nullptr, d->end_index,
                                        (float*)(W + comb->out), V, st));
    bd.last_pred = last; bd.last_lp = lp[a]; bd.pred = preds + (size_t)t * plane; bd.lp_out = lp[1 - a];
    bd.backptr = backs + (size_t)(t - 1) * plane; bd.step_index = t;
    SSC_TRY(sel.step(&bd, a, st));
    a = 1 - a;
    if (ung) {   // the next step reads these outputs through the back-pointers (ssc_decode_step_desc.ungathered)
      cur = 1 - cur;
      ungathered = true;
    } else {     // cbs.py:236-250: re-order the states by back-pointer (into the generation the step has just consumed)
      for (int m = 0; m < M; ++m)
        for (int k = 0; k < 4; ++k)
          SSC_TRY(ssc_gather_rows(mem[m].states.state(W, 1 - cur, k), H, bd.backptr, B, SB, H, mem[m].states.state(W, cur, k), st));
    }
  }
  if (d->early_stop) {
    SSC_TRY(ssc_beam_backtrace_ctl(preds, backs, d->ctl, d->max_steps, B, SB, d->end_index, d->predictions, st));
  } else {
    SSC_TRY(ssc_beam_backtrace(preds, backs, d->max_steps, B, SB, d->predictions, st));
  }
  // the trace's ancestry: the chain the back-trace has just walked.  Row g of step t is beam g after step t - 1's selection in the
  // gathered and the un-gathered form alike (a step's outputs are in row order either way)
  if (d->attn)
    SSC_TRY(ssc_attn_anc(preds, backs, d->early_stop ? d->ctl : nullptr, lp[a], d->max_steps, B, SB, d->end_index, d->attn->anc, st));
  if (hipMemcpyAsync(d->log_probs, lp[a], (size_t)G * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  if (final_gen) *final_gen = a;
  return SSC_OK;
}

}  // namespace

extern "C" int ssc_decode_search(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return ssc_decode_search_guided(cfg, p, d, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ssc_decode_search_guided(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                        const ssc_latent_guide* guide, void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);   // the numerics mode of this cfg, for every product the call issues
  if (!p || !workspace || !desc_ok(cfg, d) || (guide && !ssc_latent_guide_ok(cfg, guide))) return SSC_EINVAL;
  if (!ssc_decode_start_ok(d->start, !guide)) return SSC_EINVAL;   // (no start state under a guide)
  const SearchLayout l = search_layout(cfg, d, SEARCH_BEAM);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  char* W = (char*)workspace;
  const bool use_parts = search_uses_parts(cfg, d, SEARCH_BEAM);
  SearchMember self = search_self(p, d, l);
  return search_run(cfg, &self, 1, nullptr, d, l, W, BeamSelect{use_parts, (const float*)(W + l.parts)}, use_parts,
                    (hipStream_t)stream, nullptr, guide);
}

// ---- the beam search over several members (include/ssc.h: ssc_ensemble_desc) ------------------------------------------------------
// Workspace: the SearchLayout of a beam search without the records head - member 0 steps in its states, logits and step-workspace
// blocks, everything else in it (tokens, sentiment rows, words, back-pointers, parent lists, running log-probs, selection
// scratch, alpha) is shared -, then per further member its states (two generations, with the fp16 pieces where the layout has
// them), its (G, V) logits and its step workspace, then the (G, V) combined log-probs the selection reads.
namespace {

struct EnsembleLayout {
  SearchLayout base;
  SscStepStates states[SSC_ENSEMBLE_MAX];   // [0] = base.states
  size_t logits[SSC_ENSEMBLE_MAX], stepws[SSC_ENSEMBLE_MAX];
  size_t combined;
  size_t total;
};

EnsembleLayout ensemble_layout(const ssc_model_cfg* cfg, const ssc_search_desc* d, int M) {
  EnsembleLayout l;
  l.base = search_layout(cfg, d, SEARCH_ENSEMBLE);
  const size_t G = (size_t)d->nimg * d->n_samples * d->S * d->beam;
  const size_t prow = l.base.states.has_planes() ? (size_t)ssc_decode_planes_ld(cfg) : 0;
  size_t o = l.base.total;
  l.states[0] = l.base.states; l.logits[0] = l.base.logits; l.stepws[0] = l.base.stepws;
  for (int m = 1; m < M; ++m) {
    l.states[m].reserve(o, G, cfg->H, prow);
    l.logits[m] = ssc_ws_take(o, G * (size_t)cfg->V * 4);
    l.stepws[m] = ssc_ws_take(o, l.base.stepws_bytes);
  }
  l.combined = ssc_ws_take(o, G * (size_t)cfg->V * 4);
  l.total = o;
  return l;
}

bool ensemble_members_ok(const ssc_ensemble_desc* e) {
  return e && e->M >= 1 && e->M <= SSC_ENSEMBLE_MAX && (e->mode == 0 || e->mode == 1);
}

}  // namespace

extern "C" size_t ssc_decode_search_ensemble_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d,
                                                             const ssc_ensemble_desc* e) {
  if (!search_dims_ok(cfg, d) || !ensemble_members_ok(e)) return 0;
  return ensemble_layout(cfg, d, e->M).total;
}

extern "C" int ssc_decode_search_ensemble(const ssc_model_cfg* cfg, const ssc_ensemble_desc* e, const ssc_search_desc* d,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);
  if (!workspace || !ensemble_members_ok(e) || !e->params || !e->imgbufs || !desc_ok(cfg, d) || d->attn) return SSC_EINVAL;
  if (!ssc_decode_start_ok(d->start, false)) return SSC_EINVAL;   // (no start state of an ensemble)
  SearchCombine comb{};
  double wsum = 0.0;
  for (int m = 0; m < e->M; ++m) {
    if (!e->params[m] || !e->imgbufs[m]) return SSC_EINVAL;
    const float w = e->weights ? e->weights[m] : 1.f;
    if (!(w > 0.f) || !isfinite(w)) return SSC_EINVAL;
    wsum += (double)w;
  }
  if (d->imgbuf != e->imgbufs[0] || !isfinite(wsum)) return SSC_EINVAL;
  for (int m = 0; m < e->M; ++m) comb.logw[m] = (float)log((double)(e->weights ? e->weights[m] : 1.f) / wsum);
  comb.mode = e->mode;
  const EnsembleLayout l = ensemble_layout(cfg, d, e->M);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  comb.out = l.combined;
  SearchMember mem[SSC_ENSEMBLE_MAX];
  for (int m = 0; m < e->M; ++m) mem[m] = SearchMember{e->params[m], e->imgbufs[m], l.states[m], l.logits[m], l.stepws[m], SscAttTable{}};
  return search_run(cfg, mem, e->M, &comb, d, l.base, (char*)workspace, BeamSelect{false, nullptr}, false, (hipStream_t)stream);
}

// the stochastic beam search: S = 1, no machine, the limits of ssc_beam_step_gumbel (k <= 32, per_node <= k, k <= V)
static bool sbs_search_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_gumbel_desc* s) {
  if (!desc_ok(cfg, d) || !s) return false;
  if (d->S != 1 || d->fsm || d->tables || d->mach) return false;
  if (d->beam > 32 || d->beam > cfg->V || d->per_node > d->beam) return false;
  return s->temperature > 0.f && isfinite(s->temperature);
}

extern "C" size_t ssc_decode_stochastic_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!search_dims_ok(cfg, d)) return 0;
  return search_layout(cfg, d, SEARCH_GUMBEL).total;
}

extern "C" int ssc_decode_stochastic_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                          const ssc_gumbel_desc* s, void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);
  if (!p || !workspace || !sbs_search_ok(cfg, d, s)) return SSC_EINVAL;
  const SearchLayout l = search_layout(cfg, d, SEARCH_GUMBEL);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  char* W = (char*)workspace;
  SearchMember self = search_self(p, d, l);
  return search_run(cfg, &self, 1, nullptr, d, l, W, GumbelSelect{s, {(float*)(W + l.gs[0]), (float*)(W + l.gs[1])}}, false,
                    (hipStream_t)stream);
}

// the sampled-node beam search: S = 1, no machine, the limits of ssc_beam_step_sampled
static bool snb_search_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_sampler_desc* s) {
  if (!desc_ok(cfg, d) || !s) return false;
  if (d->S != 1 || d->fsm || d->tables || d->mach) return false;
  return ssc_sampled_beam_ok(d->nimg * d->n_samples, d->beam, d->per_node, cfg->V, s);
}

extern "C" size_t ssc_decode_sampled_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!search_dims_ok(cfg, d)) return 0;
  return search_layout(cfg, d, SEARCH_SAMPLED).total;
}

extern "C" int ssc_decode_sampled_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                       const ssc_sampler_desc* s, int with_replacement, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  SscGemmModeScope mode_scope(cfg);
  if (!p || !workspace || !snb_search_ok(cfg, d, s)) return SSC_EINVAL;
  const SearchLayout l = search_layout(cfg, d, SEARCH_SAMPLED);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  SearchMember self = search_self(p, d, l);
  return search_run(cfg, &self, 1, nullptr, d, l, (char*)workspace, SampledSelect{s, with_replacement}, false, (hipStream_t)stream);
}

// the diverse beam search: S = 1, no machine, the limits of ssc_beam_step_diverse
static bool dbs_search_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_diverse_desc* s) {
  if (!desc_ok(cfg, d) || !s) return false;
  if (d->S != 1 || d->fsm || d->tables || d->mach) return false;
  return ssc_diverse_beam_ok(d->nimg * d->n_samples, d->beam, d->per_node, cfg->V, s);
}

extern "C" size_t ssc_decode_diverse_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d,
                                                          const ssc_diverse_desc* s) {
  if (!search_dims_ok(cfg, d) || !s || s->groups < 1 || d->beam % s->groups != 0) return 0;
  return search_layout(cfg, d, SEARCH_DIVERSE, ssc_diverse_beam_list(d->beam, s->groups, d->per_node, cfg->V)).total;
}

extern "C" int ssc_decode_diverse_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d,
                                       const ssc_diverse_desc* s, void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);
  if (!p || !workspace || !dbs_search_ok(cfg, d, s)) return SSC_EINVAL;
  const SearchLayout l = search_layout(cfg, d, SEARCH_DIVERSE, ssc_diverse_beam_list(d->beam, s->groups, d->per_node, cfg->V));
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  SearchMember self = search_self(p, d, l);
  return search_run(cfg, &self, 1, nullptr, d, l, (char*)workspace, DiverseSelect{s}, false, (hipStream_t)stream);
}

// the beam search under the decode rules: S = 1, no machine, the limits of ssc_beam_step_rules (every step index below 64)
static bool rules_search_ok(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_rules_desc* r) {
  if (!desc_ok(cfg, d) || !r) return false;
  if (d->S != 1 || d->fsm || d->tables || d->mach || d->max_steps > SSC_RULES_MAX_LEN) return false;
  return ssc_rules_beam_ok(d->nimg * d->n_samples, d->beam, d->per_node, cfg->V, d->end_index, r);
}

extern "C" size_t ssc_decode_rules_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d) {
  if (!search_dims_ok(cfg, d)) return 0;
  return search_layout(cfg, d, SEARCH_RULES).total;
}

extern "C" int ssc_decode_rules_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_rules_desc* r,
                                     float* scores, int* lengths, void* workspace, size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);
  if (!p || !workspace || !scores || !lengths || !rules_search_ok(cfg, d, r)) return SSC_EINVAL;
  const SearchLayout l = search_layout(cfg, d, SEARCH_RULES);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  char* W = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  RulesSelect sel{r, {(int*)(W + l.rhist[0]), (int*)(W + l.rhist[1])}, {(int*)(W + l.rlen[0]), (int*)(W + l.rlen[1])},
                  {(float*)(W + l.rscore[0]), (float*)(W + l.rscore[1])}, d->max_steps};
  int a = 0;
  SearchMember self = search_self(p, d, l);
  SSC_TRY(search_run(cfg, &self, 1, nullptr, d, l, W, sel, false, st, &a));
  const size_t G = (size_t)d->nimg * d->n_samples * d->beam;
  if (hipMemcpyAsync(scores, sel.score[a], G * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  if (hipMemcpyAsync(lengths, sel.len[a], G * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  return SSC_OK;
}

// include/ssc_debug.h: where the call that has just run in `workspace` keeps its chosen words and back-pointers.  Both lie in front of
// every block whose size depends on the selection, so one layout serves the five searches.
size_t ssc_sample_words_offset(const ssc_model_cfg* cfg, const ssc_search_desc* d);   // (sample.hip)
extern "C" void* ssc_debug_decode_view(const void* cfg_, const void* desc, void* workspace, int driver, int which) {
  const ssc_model_cfg* cfg = (const ssc_model_cfg*)cfg_;
  const ssc_search_desc* d = (const ssc_search_desc*)desc;
  if (!workspace || !ssc_decode_dims_ok(cfg, d, d ? d->max_steps : 0)) return nullptr;
  char* W = (char*)workspace;
  if (driver == 1) return which == 0 ? W + ssc_sample_words_offset(cfg, d) : nullptr;
  if (driver != 0 || !search_dims_ok(cfg, d)) return nullptr;
  const SearchLayout l = search_layout(cfg, d, SEARCH_BEAM);
  return which == 0 ? W + l.preds : which == 1 ? W + l.backs : nullptr;
}
