// The row-selection core of the deterministic beam searches (decode.hip, fsm.hip, diverse_beam.hip, rules_beam.hip; ensemble.hip
// takes its log-sum-exp from here).  Selection order everywhere: value descending, index ascending ("k-pass selection": pass k finds
// the best candidate strictly after the previous pick in that order).
#pragma once
#include "ssc_common.h"

namespace {

struct Cand {
  float v;
  int i;
};
__device__ __forceinline__ bool better(float v, int i, const Cand& o) {  // (v,i) ranks before o
  return (v > o.v) || (v == o.v && i < o.i);
}
__device__ __forceinline__ bool after(float v, int i, const Cand& prev) {  // (v,i) ranks strictly after the previous pick
  return (prev.i < 0) || (v < prev.v) || (v == prev.v && i > prev.i);
}
__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand t;
    t.v = __shfl_xor(c.v, o, 64);
    t.i = __shfl_xor(c.i, o, 64);
    if (t.i >= 0 && (c.i < 0 || better(t.v, t.i, c))) c = t;
  }
  return c;
}
__device__ __forceinline__ Cand block_best(Cand c, Cand* sh) {
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  c = wave_best(c);
  __syncthreads();
  if (lane == 0) sh[wv] = c;
  __syncthreads();
  Cand r = sh[0];
  for (int k = 1; k < nw; ++k)
    if (sh[k].i >= 0 && (r.i < 0 || better(sh[k].v, sh[k].i, r))) r = sh[k];
  return r;
}

// One-barrier forms for kernels that run several reductions in a row: consecutive reductions alternate between two LDS slots
// (`par` = 0, 1, 0, ...), so the write of reduction n + 1 cannot overtake a slow wave's read of reduction n - 1's slot (there is a
// barrier of reduction n in between), and the leading barrier of the two-barrier forms is not needed.  Same arithmetic and order.
__device__ __forceinline__ Cand block_best1(Cand c, Cand (*sh)[4], int par) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  c = wave_best(c);
  if (lane == 0) sh[par][wv] = c;
  __syncthreads();
  Cand r = sh[par][0];
  for (int k = 1; k < nw; ++k)
    if (sh[par][k].i >= 0 && (r.i < 0 || better(sh[par][k].v, sh[par][k].i, r))) r = sh[par][k];
  return r;
}
__device__ __forceinline__ float dec_block_reduce1(float v, float (*sh)[4], int par, bool is_max) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = is_max ? ssc_wave_max(v) : ssc_wave_sum(v);
  if (lane == 0) sh[par][wv] = v;
  __syncthreads();
  float r = sh[par][0];
  for (int i = 1; i < nw; ++i) r = is_max ? fmaxf(r, sh[par][i]) : r + sh[par][i];
  return r;
}

// ---- pieces of the selections that take a whole row per workgroup of 256 -----------------------------------------------------------

constexpr int BEAM_ROW_NV = 40;   // V <= 256 * 40: the row in registers, thread t holds tokens t, t + 256, ...

// The two-barrier float reduction as beam_row_lse takes it: ssc_block_reduce of ssc_common.h, the function log_softmax_kernel itself
// calls.  shr: 16 floats of LDS.
__device__ __forceinline__ auto beam_reduce2(float* shr) {
  return [shr](float v, bool is_max) { return ssc_block_reduce(v, shr, is_max); };
}

// A row's log-sum-exp with the arithmetic and the thread ownership of log_softmax_kernel (thread t owns tokens t, t + 256, ...):
// row - lse is bit-equal to ssc_log_softmax.  REG: the row is loaded into x and x - lse is left there (NORM false: x as loaded, no
// reduction runs) - one memory round trip per row, all loads of a thread in flight at once, no LDS row; otherwise x is not touched and
// the caller subtracts the returned lse from what it reads.  red(v, is_max): the caller's block reduction, called twice when NORM
// (beam_reduce2, or dec_block_reduce1 with the caller's alternating slot); whichever it is, the waves are summed in index order.
template <bool NORM, bool REG, class Red>
__device__ __forceinline__ float beam_row_lse(const float* __restrict__ row, int V, float (&x)[REG ? BEAM_ROW_NV : 1], Red red) {
  const int t = threadIdx.x;
  float lse = 0.f;
  if (REG) {
#pragma unroll
    for (int u = 0; u < BEAM_ROW_NV; ++u) x[u] = row[min(t + u * 256, V - 1)];
    if (NORM) {
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u)
        if (t + u * 256 < V) mx = fmaxf(mx, x[u]);
      mx = red(mx, true);
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u)
        if (t + u * 256 < V) sum += expf(x[u] - mx);
      sum = red(sum, false);
      lse = mx + logf(sum);
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u) x[u] -= lse;
    }
  } else if (NORM) {   // thread t owns v = t, t + 256, ...: the order of log_softmax_kernel
    float mx = -INFINITY;
    for (int v = t; v < V; v += 256) mx = fmaxf(mx, row[v]);
    mx = red(mx, true);
    float sum = 0.f;
    for (int v = t; v < V; v += 256) sum += expf(row[v] - mx);
    sum = red(sum, false);
    lse = mx + logf(sum);
  }
  return lse;
}

// Thread t's best token strictly after `prev` in the (value descending, token ascending) order, among the tokens it owns.  REG: x
// as beam_row_lse (or the kernel's own fill of an ended row) left it; otherwise the row is read again.  keep(u, v) admits token
// v = t + 256 u; it comes last in the condition, so it is evaluated only for a value that would replace the thread's current best,
// which is rare (a ban list is a loop over LDS).  REG: "ranks after prev and before the current best" is formed as one value with
// `&`, not as a chain of `&&`: the range test and a keep that is a per-thread bit (the compiled machine's exceptions) then fold into
// ONE lane mask per u, formed once before the rounds, as the hand-written scan of beam_row_fsm_kernel had it.  With the chain the
// two masks stayed apart, twice the spilled SGPR pairs, and that kernel went from 92 / 99 to 115 / 117 VGPRs, a wave of occupancy
// less without NORM.
template <bool NORM, bool REG, class Keep>
__device__ __forceinline__ Cand beam_own_best(const float (&x)[REG ? BEAM_ROW_NV : 1], const float* __restrict__ row, float lse, int V,
                                              const Cand& prev, Keep keep) {
  const int t = threadIdx.x;
  Cand best{-INFINITY, -1};
  if (REG) {
#pragma unroll
    for (int u = 0; u < BEAM_ROW_NV; ++u) {
      const int v = t + u * 256;
      const float y = x[u];
      const bool cand = after(y, v, prev) & (best.i < 0 || better(y, v, best));
      if (v < V && cand && keep(u, v)) best = Cand{y, v};
    }
  } else {
    for (int v = t, u = 0; v < V; v += 256, ++u) {
      const float y = NORM ? row[v] - lse : row[v];
      if (after(y, v, prev) && (best.i < 0 || better(y, v, best)) && keep(u, v)) best = Cand{y, v};
    }
  }
  return best;
}

// ---- the rows kernel of the searches that merge short per-row lists (diverse_beam.hip, rules_beam.hip) -----------------------------

struct BeamListRowArgs {
  const float* scores; size_t ld; int V, m;   // m: entries of a row's list
  const int64_t* last_pred;                   // (rows) or NULL (step 0: every row is live)
  int end_index;
  const int* ctl; int step;
  float* lval; int64_t* ltok;   // (rows, m): the row's m best admitted (lp, token), descending
  // RULES only:
  const int* hist; int ld_hist;               // (rows, ld_hist): tokens 0 .. step - 1 of every row; not read at step 0
  int ngram, min_length, n_suppress;
  int suppress[SSC_RULES_MAX_SUPPRESS];
};

constexpr int BEAM_MAX_BAN = SSC_RULES_MAX_LEN + SSC_RULES_MAX_SUPPRESS + 1;   // n-gram bans (one per history position), suppress list, END

__device__ __forceinline__ bool beam_banned(const int* ban, int nb, int v) {
  for (int q = 0; q < nb; ++q)
    if (ban[q] == v) return true;
  return false;
}

// Row r's ban list under the decode rules (ssc_rules_desc), formed by wave 0 of a workgroup of 256 in LDS (hs: SSC_RULES_MAX_LEN ints,
// ban: BEAM_MAX_BAN): lane i compares the (n-1)-gram at history position i with the history's last n - 1 tokens and bans the token that
// followed it; then the suppress list; then END below the minimum length.  Ends with a barrier; *nban is the list's length.
__device__ __forceinline__ void beam_ban_list(const BeamListRowArgs& a, int r, int* hs, int* ban, int* nban) {
  const int t = threadIdx.x;
  const int T = a.last_pred ? min(a.step, SSC_RULES_MAX_LEN - 1) : 0;   // tokens of history
  const bool grams = a.ngram >= 1 && T >= a.ngram;   // (workgroup-uniform; fewer than n tokens of history: no n-gram to repeat)
  if (grams) {
    if (t < SSC_RULES_MAX_LEN) hs[t] = t < T ? a.hist[(size_t)r * a.ld_hist + t] : -1;
    __syncthreads();
  }
  if (t < 64) {
    const int n = a.ngram;
    int nb = 0;
    if (grams) {
      // the n-gram that starts at position t ends inside the history; its first n - 1 tokens against the history's last n - 1
      bool hit = t + n <= T;
      if (hit) {
        for (int q = 0; q < n - 1; ++q) hit = hit && hs[t + q] == hs[T - (n - 1) + q];
      }
      const int tok = hit ? hs[t + n - 1] : -1;
      hit = hit && tok != a.end_index && tok >= 0;   // (END is never banned by this rule)
      const unsigned long long mask = __ballot(hit);
      if (hit) ban[__popcll(mask & ((1ull << t) - 1ull))] = tok;
      nb = __popcll(mask);
    }
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < SSC_RULES_MAX_SUPPRESS; ++q)
        if (q < a.n_suppress) ban[nb + q] = a.suppress[q];
      nb += a.n_suppress;
      if (a.step < a.min_length) ban[nb++] = a.end_index;
      *nban = nb;
    }
  }
  __syncthreads();
}

// One workgroup per live row, independent of the row's entry: the log-sum-exp (beam_row_lse: bit-equal to ssc_log_softmax) and the
// row's m best tokens by lp, left as (lp, token).  Every thread keeps its best token; a round is one block argmax, after which only
// the winner's thread looks at its tokens again.  RULES: a token on the row's ban list never becomes a thread's candidate; the
// scores are never written and nothing is renormalised.  Without RULES the history, the ban list and their LDS compile away.
template <bool NORM, bool REG, bool RULES>
__global__ __launch_bounds__(256) void beam_list_rows_kernel(BeamListRowArgs a) {
  __shared__ Cand sh2[2][4];
  __shared__ float shr[16];
  __shared__ int hs[SSC_RULES_MAX_LEN];
  __shared__ int ban[BEAM_MAX_BAN];
  __shared__ int nban;
  const int r = blockIdx.x, t = threadIdx.x;
  const int V = a.V, m = a.m;
  const bool stopped = a.ctl && a.last_pred && a.ctl[0] <= a.step;   // (written by an EARLIER launch of this stream)
  if (stopped || (a.last_pred && a.last_pred[r] == a.end_index)) return;   // workgroup-uniform: an ended beam never looks at its row
  int nb = 0;
  if (RULES) {
    beam_ban_list(a, r, hs, ban, &nban);
    nb = nban;
  }
  auto keep = [&](int, int v) { return !RULES || !beam_banned(ban, nb, v); };
  const float* row = a.scores + (size_t)r * a.ld;
  float x[REG ? BEAM_ROW_NV : 1];
  const float lse = beam_row_lse<NORM, REG>(row, V, x, beam_reduce2(shr));
  float* lval = a.lval + (size_t)r * m;
  int64_t* ltok = a.ltok + (size_t)r * m;
  Cand mine = beam_own_best<NORM, REG>(x, row, lse, V, Cand{INFINITY, -1}, keep);
  int par = 0;
  for (int i = 0; i < m; ++i) {
    const Cand w = block_best1(mine, sh2, par); par ^= 1;
    // (w.i < 0: NaN scores only, or fewer than m unbanned tokens - the merge leaves such an entry out)
    if (t == 0) { lval[i] = w.i >= 0 ? w.v : -INFINITY; ltok[i] = w.i; }
    if (w.i >= 0 && (w.i & 255) == t) mine = beam_own_best<NORM, REG>(x, row, lse, V, w, keep);   // the owner of token w.i: its best after w
  }
}

template <bool RULES>
int beam_list_rows_launch(const BeamListRowArgs& a, bool norm, int rows, hipStream_t st) {
  const bool reg = a.V <= 256 * BEAM_ROW_NV;
  auto* kernel = reg ? (norm ? beam_list_rows_kernel<true, true, RULES> : beam_list_rows_kernel<false, true, RULES>)
                     : (norm ? beam_list_rows_kernel<true, false, RULES> : beam_list_rows_kernel<false, false, RULES>);
  SSC_LAUNCH(kernel, dim3(rows), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// ---- pieces of the two list merges (one wave per batch entry) ----------------------------------------------------------------------

constexpr int BEAM_LIST_MAX = 32;   // k, n <= 32: the merge's one wave, its LDS candidates, the counts of the diverse search

// the range checks the list searches share: 1 <= k, n <= 32, k, n <= V, B * k <= 2^24
inline bool beam_list_dims_ok(int B, int k, int n, int V) {
  if (B <= 0 || V <= 0 || k < 1 || k > BEAM_LIST_MAX || n < 1 || n > BEAM_LIST_MAX || k > V || n > V) return false;
  return (long)B * k <= (1L << 24);
}

// One round of a merge's selection: the best finite key strictly after `prev` among the C candidate keys in LDS, descending, ties to
// the lower candidate index (NaN and -inf are never taken); .i < 0: none is left.  The same in every lane of the wave.
__device__ __forceinline__ Cand beam_next_key(const float* key, int C, const Cand& prev) {
  Cand best{-INFINITY, -1};
  for (int c = threadIdx.x; c < C; c += 64) {
    const float x = key[c];
    if (x > -INFINITY && after(x, c, prev) && (best.i < 0 || better(x, c, best))) best = Cand{x, c};
  }
  return wave_best(best);
}

// The early-stop tail of a merge kernel that runs one workgroup per batch entry (the protocol of ssc_beam_desc.ctl): one thread of
// every workgroup calls it with the number of beams of its entry that have not ended.  The last workgroup of the step to get here
// stops the search when there are none, and notes the step's completion in the progress word (the one-call searches queue step t
// only once step t - 2 has got here: their run-ahead bound).
__device__ __forceinline__ void beam_early_stop_tail(int* ctl, int* host_flag, int step_index, int max_steps, int live, bool stopped) {
  int* cnt = ctl + 2 + step_index;
  int* ticket = ctl + 2 + max_steps + step_index;
  if (live) atomicAdd(cnt, live);
  __threadfence();
  const int done = atomicAdd(ticket, 1);
  if (done == (int)gridDim.x - 1) {   // the last workgroup of this step
    if (!stopped) {
      __threadfence();
      if (atomicAdd(cnt, 0) == 0) {
        atomicMin(ctl, step_index + 1);
        if (host_flag) __hip_atomic_store(host_flag, step_index + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (host_flag) __hip_atomic_store(host_flag + 1, step_index, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace
