// Beam search under the decode rules (ssc_rules_desc, include/ssc.h): blocking of repeated n-grams, a minimum caption length, a list
// of tokens that are never emitted, and a length penalty in the ranking.  Deterministic beam search with the trivial machine; every
// beam carries its true summed log-prob, its token history, its length and its score (the sum over the penalty of its length).
// ssc_beam_first_rules / ssc_beam_step_rules are the stand-alone steps, ssc_decode_rules_beam (search.hip) runs them inside the
// one-call search loop.  The rules live where the selection lives: the host never sees a step of a one-call search, and blocking
// needs every beam's history at every step.
//   (A) rows kernel, one workgroup of 256 per live row: beam_list_rows_kernel of beam_common.h with the rules.  One wave forms the
//       row's ban list in LDS first (beam_ban_list: at most 63 + 8 + 1 tokens), then the log-sum-exp every search shares (bit-equal
//       to ssc_log_softmax) and per_node rounds of a block argmax in which a banned token never becomes a thread's candidate.  The
//       scores are never written and nothing is renormalised.
//   (B) merge kernel, one wave per batch entry: the keys of the k * per_node candidates in LDS, k rounds of a wave argmax (ties:
//       lower candidate index), then the lanes copy the parents' history rows into the other generation and append the tokens.
//       Early stop: the protocol of ssc_beam_desc.ctl (beam_early_stop_tail).
// No float atomics: two calls on the same inputs are bit-identical.  A slot that finds no finite candidate emits end_index at -inf
// with the identity back-pointer, never index -1.
#include <math.h>

#include "beam_common.h"
#include "ssc_common.h"

namespace {

struct RulesMergeArgs {
  const float* lval; const int64_t* ltok;
  int k, n;
  const int64_t* last_pred; const float* last_lp;   // NULL at step 0: one row per entry, phi = 0
  const int* hist; const int* len; int ld_hist;     // NULL at step 0
  int64_t* pred; float* lp_out; int64_t* backptr;
  int* hist_out; int* len_out; float* score_out;
  int end_index;
  int* ctl; int step_index, max_steps; int* host_flag;
  float penalty[SSC_RULES_MAX_LEN];
};

__global__ __launch_bounds__(64) void rules_merge_kernel(RulesMergeArgs a) {
  __shared__ float ckey[BEAM_LIST_MAX * BEAM_LIST_MAX], csum[BEAM_LIST_MAX * BEAM_LIST_MAX];   // the candidates: key, true sum,
  __shared__ int ctk[BEAM_LIST_MAX * BEAM_LIST_MAX];                                           // token
  __shared__ float tab[SSC_RULES_MAX_LEN];
  __shared__ int opar[BEAM_LIST_MAX], otok[BEAM_LIST_MAX];   // the selected slots' parents and tokens, for the histories
  const int b = blockIdx.x, lane = threadIdx.x;
  const int k = a.k, t = a.step_index;
  const bool first = a.last_pred == nullptr;
  const bool stopped = a.ctl && !first && a.ctl[0] <= a.step_index;   // (written by an EARLIER launch of this stream)
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < SSC_RULES_MAX_LEN; ++q) tab[q] = a.penalty[q];
  }
  __syncthreads();
  int live = 0;
  if (stopped) {
    // the search had ended before this step: END from the same beam; the sum, the length and the score stay as they were
    if (lane < k) {
      const size_t o = (size_t)b * k + lane;
      const int L = min(max(a.len[o], 1), SSC_RULES_MAX_LEN);
      a.pred[o] = a.end_index;
      a.lp_out[o] = a.last_lp[o];
      a.backptr[o] = lane;
      a.len_out[o] = a.len[o];
      a.score_out[o] = a.last_lp[o] / tab[L - 1];
      opar[lane] = lane;
      otok[lane] = a.end_index;
    }
  } else {
    const int rows = first ? 1 : k;
    const int nr = first ? k : a.n;   // candidates per row
    const int C = rows * nr;
    for (int c = lane; c < C; c += 64) {
      const int j = c / nr, slot = c - j * nr;
      const size_t r = first ? (size_t)b : (size_t)b * k + j;
      float key = -INFINITY, s = -INFINITY;
      int tok = a.end_index;
      if (!first && a.last_pred[r] == a.end_index) {   // END after END: one candidate at phi exactly, ranked by the score it had
        if (slot == 0) {
          const int L = min(max(a.len[r], 1), SSC_RULES_MAX_LEN);
          s = a.last_lp[r];
          key = s / tab[L - 1];
        }
      } else {
        const int v = (int)a.ltok[r * nr + slot];
        if (v >= 0) {
          const float lp = a.lval[r * nr + slot];
          s = first ? lp : a.last_lp[r] + lp;
          key = s / tab[t];
          tok = v;
        }
      }
      ckey[c] = key; csum[c] = s; ctk[c] = tok;
    }
    __syncthreads();
    // the k best candidates by key, descending (ties: lower candidate index)
    Cand prev{INFINITY, -1};
    for (int i = 0; i < k; ++i) {
      const Cand best = beam_next_key(ckey, C, prev);
      const int c = best.i;
      if (c >= 0) prev = best;
      if (lane == 0) {
        const size_t o = (size_t)b * k + i;
        const int j = c >= 0 ? c / nr : i;
        const int tok = c >= 0 ? ctk[c] : a.end_index;
        const bool ended = c >= 0 && !first && a.last_pred[(size_t)b * k + j] == a.end_index;
        a.pred[o] = tok;
        a.lp_out[o] = c >= 0 ? csum[c] : -INFINITY;
        if (a.backptr) a.backptr[o] = j;
        a.len_out[o] = ended ? a.len[(size_t)b * k + j] : t + 1;
        a.score_out[o] = c >= 0 ? ckey[c] : -INFINITY;
        opar[i] = j;
        otok[i] = tok;
        live += tok != a.end_index;
      }
    }
  }
  __syncthreads();
  // the histories: the parent's first t tokens, then the new one (t <= 63: one pass of the wave per slot)
  for (int i = 0; i < k; ++i) {
    int* dst = a.hist_out + ((size_t)b * k + i) * a.ld_hist;
    if (!first && lane < t) dst[lane] = a.hist[((size_t)b * k + opar[i]) * a.ld_hist + lane];
    if (lane == 0) dst[t] = otok[i];
  }
  if (a.ctl && lane == 0) {   // early stop: the protocol of ssc_beam_desc.ctl
    beam_early_stop_tail(a.ctl, a.host_flag, a.step_index, a.max_steps, live, stopped);
  }
}

// the limits of both entries (include/ssc.h): trivial machine, the rules, the state's outputs, scratch for the lists
bool rules_desc_ok(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, int per_node) {
  if (!d || !r || !s || !d->scores || !d->pred || !d->lp_out || !d->scratch_val || !d->scratch_idx) return false;
  if (!s->hist_out || !s->len_out || !s->score_out) return false;
  if (d->fsm || d->tables || d->mach || d->dims.S != 1 || d->ld < d->dims.V) return false;
  return ssc_rules_beam_ok(d->B, d->beam, per_node, d->dims.V, d->end_index, r);
}

void rules_fill(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, int m, BeamListRowArgs* a, RulesMergeArgs* g) {
  a->scores = d->scores; a->ld = (size_t)d->ld; a->V = d->dims.V; a->m = m; a->end_index = d->end_index;
  a->ngram = r->no_repeat_ngram; a->min_length = r->min_length; a->n_suppress = r->n_suppress;
  for (int q = 0; q < SSC_RULES_MAX_SUPPRESS; ++q) a->suppress[q] = q < r->n_suppress ? r->suppress[q] : -1;
  a->lval = d->scratch_val; a->ltok = d->scratch_idx;
  g->lval = d->scratch_val; g->ltok = d->scratch_idx; g->k = d->beam; g->n = m;
  g->pred = d->pred; g->lp_out = d->lp_out; g->end_index = d->end_index;
  g->hist_out = s->hist_out; g->len_out = s->len_out; g->score_out = s->score_out; g->ld_hist = s->ld_hist;
  g->ctl = d->ctl; g->max_steps = d->max_steps; g->host_flag = d->host_flag;
  for (int q = 0; q < SSC_RULES_MAX_LEN; ++q) g->penalty[q] = r->length_penalty[q];
}

}  // namespace

// trivial machine aside (checked by the callers): 1 <= k, n <= 32, k, n <= V, B * k <= 2^24, end_index in [0, V), and the rules'
// own ranges (include/ssc.h: ssc_rules_desc)
bool ssc_rules_beam_ok(int B, int k, int n, int V, int end_index, const ssc_rules_desc* r) {
  if (!r || !beam_list_dims_ok(B, k, n, V)) return false;
  if (end_index < 0 || end_index >= V) return false;
  if (r->no_repeat_ngram < 0 || r->no_repeat_ngram > SSC_RULES_MAX_LEN || r->min_length < 0) return false;
  if (r->n_suppress < 0 || r->n_suppress > SSC_RULES_MAX_SUPPRESS) return false;
  for (int q = 0; q < r->n_suppress; ++q)
    if (r->suppress[q] < 0 || r->suppress[q] >= V || r->suppress[q] == end_index) return false;
  for (int q = 0; q < SSC_RULES_MAX_LEN; ++q)
    if (!(r->length_penalty[q] > 0.f) || !isfinite(r->length_penalty[q])) return false;
  return true;
}

extern "C" int ssc_beam_first_rules(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, void* stream) {
  if (!rules_desc_ok(d, r, s, 1) || s->ld_hist < 1) return SSC_EINVAL;
  if (d->ctl && d->max_steps <= 0) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // step 0: one row per entry with an empty history; its k best unbanned tokens
  BeamListRowArgs a{};
  RulesMergeArgs g{};
  rules_fill(d, r, s, d->beam, &a, &g);
  SSC_TRY(beam_list_rows_launch<true>(a, d->raw_logits != 0, d->B, st));
  g.step_index = 0;
  SSC_LAUNCH(rules_merge_kernel, dim3(d->B), dim3(64), 0, st, g);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_beam_step_rules(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, void* stream) {
  if (!rules_desc_ok(d, r, s, d ? d->per_node : 0) || !d->last_pred || !d->last_lp || !d->backptr) return SSC_EINVAL;
  if (!s->hist || !s->len || s->hist == s->hist_out || s->len == s->len_out) return SSC_EINVAL;
  if (d->step_index < 1 || d->step_index > SSC_RULES_MAX_LEN - 1 || s->ld_hist < d->step_index + 1) return SSC_EINVAL;
  if (d->ctl && (d->max_steps <= 0 || d->step_index >= d->max_steps)) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  BeamListRowArgs a{};
  RulesMergeArgs g{};
  rules_fill(d, r, s, d->per_node, &a, &g);
  a.last_pred = d->last_pred; a.hist = s->hist; a.ld_hist = s->ld_hist; a.ctl = d->ctl; a.step = d->step_index;
  SSC_TRY(beam_list_rows_launch<true>(a, d->raw_logits != 0, d->B * d->beam, st));
  g.last_pred = d->last_pred; g.last_lp = d->last_lp; g.hist = s->hist; g.len = s->len; g.backptr = d->backptr;
  g.step_index = d->step_index;
  SSC_LAUNCH(rules_merge_kernel, dim3(d->B), dim3(64), 0, st, g);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
