// Diverse beam search (Vijayakumar et al., "Diverse Beam Search", AAAI 2018; the "Div-BS" baseline of the diverse-captioning
// papers): the k beams of a batch entry are Gr groups of k' = k / Gr consecutive beams; the groups of an entry are searched in
// order, and a token that beams of EARLIER groups have selected at this same step c times is ranked lambda * c lower (Hamming
// diversity).  The penalty steers the choice of a step only: every beam carries its true summed log-prob.  include/ssc.h has the
// definition (ssc_diverse_desc); ssc_beam_first_diverse / ssc_beam_step_diverse are the stand-alone steps,
// ssc_decode_diverse_beam (search.hip) runs them inside the one-call search loop.
//
// The groups of an entry depend on each other inside a step, the pass over a row's V logits must not: a penalty only lowers values,
// and the beams of the other groups select at most P = k - k' distinct tokens.  So the n best tokens of a row under the penalised
// score r lie among its m = n + P best tokens under lp (value descending, token ascending): of those m at most P are penalised, at
// least n unpenalised ones remain, and each of them ranks before every token outside the list both before and after the penalty.
//   (A) rows kernel, one workgroup per live row, independent of groups: beam_list_rows_kernel of beam_common.h without the rules -
//       the log-sum-exp every search shares (bit-identical to ssc_beam_step_fsm) and the row's top m by lp, left in scratch as
//       (lp, token).  Ended rows are not read.
//   (B) merge kernel, one wave per batch entry, the groups in order over those short lists: lane e holds entry e of a row
//       (m <= 63), subtracts lambda * count (the counts of <= 32 distinct tokens live in LDS), ranks the entries by counting and
//       leaves the n best as candidates; k' rounds of a wave argmax over the group's k' * n candidates; the chosen tokens join
//       the counts.  Early stop: the protocol of ssc_beam_desc.ctl (beam_early_stop_tail).
// No atomics in the choice: two calls on the same inputs are bit-identical.  A slot that finds no finite candidate emits end_index
// at -inf with the identity back-pointer, never index -1.
#include <math.h>

#include <algorithm>

#include "beam_common.h"
#include "ssc_common.h"

namespace {

struct DbsMergeArgs {
  const float* lval; const int64_t* ltok; int m;
  int k, groups, n; float strength;
  const int64_t* last_pred; const float* last_lp;   // NULL at step 0: one row per entry, phi = 0
  int64_t* pred; float* lp_out; int64_t* backptr;
  int end_index;
  int* ctl; int step_index, max_steps; int* host_flag;
};

__global__ __launch_bounds__(64) void dbs_merge_kernel(DbsMergeArgs a) {
  // k <= 32 (the counts, this one wave), n <= 32: m = n + k - k' <= 63 lanes
  __shared__ float ca[BEAM_LIST_MAX * BEAM_LIST_MAX], cs[BEAM_LIST_MAX * BEAM_LIST_MAX];   // a group's candidates: augmented sum, true sum,
  __shared__ int ctk[BEAM_LIST_MAX * BEAM_LIST_MAX];                                        // token
  __shared__ int ptok[BEAM_LIST_MAX], pcnt[BEAM_LIST_MAX];   // the tokens selected at this step so far, and by how many beams
  const int b = blockIdx.x, lane = threadIdx.x;
  const int k = a.k, Gr = a.groups, kp = k / Gr, m = a.m;
  const bool first = a.last_pred == nullptr;
  const bool stopped = a.ctl && !first && a.ctl[0] <= a.step_index;   // (written by an EARLIER launch of this stream)
  int live = 0;
  if (stopped) {
    // the search had ended before this step: END at +0 from the same beam, so that nothing moves
    if (lane < k) {
      const size_t o = (size_t)b * k + lane;
      a.pred[o] = a.end_index;
      a.lp_out[o] = a.last_lp[o];
      a.backptr[o] = lane;
    }
  } else {
    const int rows = first ? 1 : kp;      // rows of a group; step 0: every group selects from the entry's one row
    const int nr = first ? kp : a.n;      // candidates per row
    const int C = rows * nr;
    int np = 0;                           // distinct tokens counted so far (wave-uniform)
    for (int g = 0; g < Gr; ++g) {
      for (int c = lane; c < C; c += 64) { ca[c] = -INFINITY; cs[c] = -INFINITY; ctk[c] = a.end_index; }
      __syncthreads();
      unsigned endmask = 0u;              // rows of this group whose beam had ended (wave-uniform)
      for (int j = 0; j < rows; ++j) {
        const size_t r = first ? (size_t)b : (size_t)b * k + g * kp + j;
        const float phi = first ? 0.f : a.last_lp[r];
        if (!first && a.last_pred[r] == a.end_index) {   // END after END: one candidate at phi exactly, no penalty, nothing counted
          endmask |= 1u << j;
          if (lane == 0) { ca[j * nr] = phi; cs[j * nr] = phi; }
          continue;
        }
        int tok = -1;
        float lp = -INFINITY, rv = -INFINITY;
        if (lane < m) {
          tok = (int)a.ltok[r * m + lane];
          lp = a.lval[r * m + lane];
        }
        if (tok >= 0) {
          int c = 0;
          for (int q = 0; q < np; ++q)
            if (ptok[q] == tok) c = pcnt[q];
          rv = lp - (a.strength * (float)c);
        }
        // the entry's place among the row's m under the penalised score (value descending, token ascending)
        int rank = 0;
        for (int e = 0; e < m; ++e) {
          const float ov = __shfl(rv, e, 64);
          const int ot = __shfl(tok, e, 64);
          rank += ot >= 0 && (ov > rv || (ov == rv && ot < tok));
        }
        if (tok >= 0 && rank < nr) {
          const int c = j * nr + rank;
          ca[c] = first ? rv : phi + rv;
          cs[c] = first ? lp : phi + lp;
          ctk[c] = tok;
        }
      }
      __syncthreads();
      // the group's k' best candidates by augmented sum, descending (ties: lower candidate index)
      Cand prev{INFINITY, -1};
      for (int i = 0; i < kp; ++i) {
        const Cand best = beam_next_key(ca, C, prev);
        const int c = best.i;
        const int tok = c >= 0 ? ctk[c] : a.end_index;
        if (c >= 0) prev = best;
        if (lane == 0) {
          const size_t o = (size_t)b * k + g * kp + i;
          a.pred[o] = tok;
          a.lp_out[o] = c >= 0 ? cs[c] : -INFINITY;
          if (a.backptr) a.backptr[o] = g * kp + (c >= 0 ? c / nr : i);
          live += tok != a.end_index;
        }
        // the token joins the counts of the later groups (not the forced END of an ended beam, not an empty slot)
        if (g + 1 < Gr && c >= 0 && !((endmask >> (c / nr)) & 1u)) {
          int at = -1;
          for (int q = 0; q < np; ++q)
            if (ptok[q] == tok) at = q;
          __syncthreads();
          if (lane == 0) {
            if (at >= 0) ++pcnt[at];
            else { ptok[np] = tok; pcnt[np] = 1; }   // (np < k <= 32: at most one new token per selected beam)
          }
          np += at < 0;
          __syncthreads();
        }
      }
      __syncthreads();
    }
  }
  if (a.ctl && lane == 0) {   // early stop: the protocol of ssc_beam_desc.ctl
    beam_early_stop_tail(a.ctl, a.host_flag, a.step_index, a.max_steps, live, stopped);
  }
}

// the limits of both entries (include/ssc.h): trivial machine, the group split, scratch for the lists
bool dbs_desc_ok(const ssc_beam_desc* d, const ssc_diverse_desc* s, int per_node) {
  if (!d || !s || !d->scores || !d->pred || !d->lp_out || !d->scratch_val || !d->scratch_idx) return false;
  if (d->fsm || d->tables || d->mach || d->dims.S != 1 || d->ld < d->dims.V) return false;
  if (!ssc_diverse_beam_ok(d->B, d->beam, per_node, d->dims.V, s)) return false;
  return d->end_index >= 0 && d->end_index < d->dims.V;
}

}  // namespace

// trivial machine aside (checked by the callers): 1 <= k, n <= 32, k, n <= V, k % groups == 0, B * k <= 2^24, 0 <= strength finite
bool ssc_diverse_beam_ok(int B, int k, int n, int V, const ssc_diverse_desc* s) {
  if (!s || !beam_list_dims_ok(B, k, n, V)) return false;
  if (s->groups < 1 || k % s->groups != 0) return false;
  return s->strength >= 0.f && isfinite(s->strength);
}

// entries of a row's list at a later step: n + (k - k'), the whole row when that is more
int ssc_diverse_beam_list(int k, int groups, int n, int V) { return std::min(n + k - k / groups, V); }

extern "C" int ssc_beam_first_diverse(const ssc_beam_desc* d, const ssc_diverse_desc* s, void* stream) {
  if (!dbs_desc_ok(d, s, 1)) return SSC_EINVAL;
  if (d->ctl && d->max_steps <= 0) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, k = d->beam;
  // step 0: one row per entry; its k best tokens hold every group's k' best under the penalty (m = k' + (k - k'))
  BeamListRowArgs a{};
  a.scores = d->scores; a.ld = (size_t)d->ld; a.V = d->dims.V; a.m = k; a.end_index = d->end_index;
  a.lval = d->scratch_val; a.ltok = d->scratch_idx;
  SSC_TRY(beam_list_rows_launch<false>(a, d->raw_logits != 0, B, st));
  DbsMergeArgs g{};
  g.lval = d->scratch_val; g.ltok = d->scratch_idx; g.m = k; g.k = k; g.groups = s->groups; g.n = k / s->groups;
  g.strength = s->strength; g.pred = d->pred; g.lp_out = d->lp_out; g.end_index = d->end_index;
  g.ctl = d->ctl; g.step_index = 0; g.max_steps = d->max_steps; g.host_flag = d->host_flag;
  SSC_LAUNCH(dbs_merge_kernel, dim3(B), dim3(64), 0, st, g);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_beam_step_diverse(const ssc_beam_desc* d, const ssc_diverse_desc* s, void* stream) {
  if (!dbs_desc_ok(d, s, d ? d->per_node : 0) || !d->last_pred || !d->last_lp || !d->backptr) return SSC_EINVAL;
  if (d->step_index <= 0 || (d->ctl && (d->max_steps <= 0 || d->step_index >= d->max_steps))) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, k = d->beam, n = d->per_node;
  const int m = ssc_diverse_beam_list(k, s->groups, n, d->dims.V);
  BeamListRowArgs a{};
  a.scores = d->scores; a.ld = (size_t)d->ld; a.V = d->dims.V; a.m = m; a.last_pred = d->last_pred; a.end_index = d->end_index;
  a.ctl = d->ctl; a.step = d->step_index;
  a.lval = d->scratch_val; a.ltok = d->scratch_idx;
  SSC_TRY(beam_list_rows_launch<false>(a, d->raw_logits != 0, B * k, st));
  DbsMergeArgs g{};
  g.lval = d->scratch_val; g.ltok = d->scratch_idx; g.m = m; g.k = k; g.groups = s->groups; g.n = n; g.strength = s->strength;
  g.last_pred = d->last_pred; g.last_lp = d->last_lp; g.pred = d->pred; g.lp_out = d->lp_out; g.backptr = d->backptr;
  g.end_index = d->end_index; g.ctl = d->ctl; g.step_index = d->step_index; g.max_steps = d->max_steps; g.host_flag = d->host_flag;
  SSC_LAUNCH(dbs_merge_kernel, dim3(B), dim3(64), 0, st, g);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
