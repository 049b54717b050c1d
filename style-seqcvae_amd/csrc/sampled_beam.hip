// Sampled-node beam search: the reference's BeamSearch driven by a word sampler (MultinomialSampler / TopKSampler / TopPSampler,
// var_updown/var_updown/modules/beam_search.py:103-293, :592-768).  Every live beam samples per_node candidate tokens from its
// filtered distribution (with or without replacement); the beam * per_node candidates of a batch entry are merged deterministically.
// ssc_beam_step_sampled is the stand-alone step; ssc_decode_sampled_beam (search.hip) runs it inside the one-call search loop,
// after ssc_beam_first_fsm for step 0 (the word samplers keep Sampler.sample_beams, a plain top-k).
//
// Row kernel, one workgroup per row (b, j).  The row's raw logits are read from HBM once: for V <= SAMPLE_LDS_MAX_V into LDS, longer
// rows take the same passes over global memory.  Passes: the maximum; the log-sum-exp (and, for top-p, the tempered normaliser); the
// top-k / top-p cut by the radix select of ssc_radix.h (for top-p without replacement, when that cut keeps fewer than n tokens, also
// the top-n cut: the reference always keeps the first per_node tokens of the sorted distribution there); then the draw over the
// kept set, score s_v = logit_v / T + g_v:
//   without replacement - the n largest scores (Gumbel-top-n, the distribution of torch.multinomial(replacement=False)): every
//     thread keeps its best (s, v), then n rounds of a block argmax; after a round only the winner's thread rescans its tokens
//     (from the scores it left in LDS, or by recomputing the noise in the global-memory form);
//   with replacement - n independent Gumbel-max draws, draw d over noise word d: one pass and one block argmax per draw.
// Noise word 0 is ssc_sample_rows' (and sbs.hip's) noise, and the score is computed as ssc_sample_rows computes it, so at
// beam = per_node = 1 a step draws ssc_sample_rows' token with its log-prob, bit for bit.
//
// Merge, one wave per batch entry: the top k of the entry's k * n candidates by summed log-prob, descending (ties: lower candidate
// index); back-pointer = candidate / n.  Early stop: the protocol of ssc_beam_desc.ctl.  A slot that finds no finite candidate emits
// end_index at -inf with the identity back-pointer, never index -1.
#include <math.h>

#include "ssc_common.h"
#include "ssc_philox.h"
#include "ssc_radix.h"

namespace {

constexpr int SNB_MAX_BEAM = 32;   // k <= 32 (the merge's one wave), n <= 32 (the survivor slots)

struct SnbCand { float v; int i; };
// the (value descending, index ascending) order
__device__ __forceinline__ bool snb_after(float x, int i, const SnbCand& p) { return p.i < 0 || x < p.v || (x == p.v && i > p.i); }
__device__ __forceinline__ void snb_take(SnbCand& best, float x, int i) {
  if (i >= 0 && (best.i < 0 || x > best.v || (x == best.v && i < best.i))) best = SnbCand{x, i};
}
__device__ __forceinline__ SnbCand snb_wave_best(SnbCand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(c.v, o, 64);
    const int oi = __shfl_xor(c.i, o, 64);
    snb_take(c, ov, oi);
  }
  return c;
}
__device__ __forceinline__ SnbCand snb_block_best(SnbCand c, SampleShared& sh) {
  c = snb_wave_best(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh.bestv[threadIdx.x >> 6] = c.v; sh.besti[threadIdx.x >> 6] = c.i; }
  __syncthreads();
  SnbCand r{sh.bestv[0], sh.besti[0]};
  for (int w = 1; w < SAMPLE_WAVES; ++w) snb_take(r, sh.bestv[w], sh.besti[w]);
  return r;
}

struct SnbRowArgs {
  const float* logits; size_t ld; int V; int n;
  int kind, top_k; float top_p, temperature;
  int replace;                  // 1: n independent draws (with replacement)
  uint32_t seed_lo, seed_hi; int step;
  const int64_t* last_pred;     // (rows)
  const float* phi;             // (rows) running log-probs
  int end_index;
  const int* ctl;
  float* clp; int64_t* ctok;    // (rows, n) candidates: summed log-prob, token
};

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void snb_rows_kernel(SnbRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  __shared__ int selv[SNB_MAX_BEAM];
  __shared__ int nsel;
  const int r = blockIdx.x;
  const int V = a.V, n = a.n;
  const bool stopped = a.ctl && a.ctl[0] <= a.step;   // (written by an EARLIER launch of this stream: the search has ended)
  const bool ended = stopped || a.last_pred[r] == a.end_index;   // workgroup-uniform
  const float phi = a.phi[r];
  float* clp = a.clp + (size_t)r * n;
  int64_t* ctok = a.ctok + (size_t)r * n;
  if (ended) {   // one-hot at end_index (log_probs_after_end, beam_search.py:656-688): no read, no noise
    for (int i = threadIdx.x; i < n; i += SAMPLE_THREADS) {
      clp[i] = i == 0 || a.replace ? phi : -INFINITY;   // (with replacement every draw is the end token)
      ctok[i] = a.end_index;
    }
    return;
  }
  const float* g = a.logits + (size_t)r * a.ld;
  RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
  const int nj = (V + 3) >> 2;
  // ---- stage the row (once from HBM) and its maximum (as sample_rows_kernel) -----------------------------------------------
  const float mx = row_stage_max(row, srow, sh);
  const float T = a.temperature;
  const bool topp = a.kind == 2 && a.top_p < 1.f;
  // ---- untempered log-sum-exp (the step log-prob) and the tempered normaliser (top-p masses) ---------------------------------
  float s = 0.f, st = 0.f;
  for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
    float x[4];
    row.get4(j, x);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s += expf(x[c] - mx);
      if (topp) st += expf((x[c] - mx) / T);
    }
  }
  s = block_sum(s, sh);
  const float lse = mx + logf(s);
  float invz = 0.f;
  if (topp) invz = 1.f / block_sum(st, sh);
  // ---- the cut; top-p without replacement also keeps the first n tokens (beam_search.py:269-270) -----------------------------
  uint32_t ck, fk = 0xffffffffu;   // (fk / fi: the forced cut, by default keeping nothing)
  int ci, fi = -1;
  sample_cut(row, a.kind, a.top_k, a.top_p, mx, T, invz, sh, ck, ci);
  if (topp && !a.replace && n > 1) {
    // the forced keep only matters when the top-p cut keeps fewer than n tokens: count them first (one pass, no histograms)
    int kept = 0;
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4];
      row.get4(j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int v = 4 * j + c;
        const uint32_t key = sample_key(x[c]);
        kept += v < V && (key > ck || (key == ck && v <= ci));
      }
    }
    if (block_sum((float)kept, sh) < (float)n) sample_cut(row, 1, n, 1.f, mx, T, invz, sh, fk, fi);   // (counts < 2^24: exact)
  }
  // score of the four tokens of block j under noise word d: logit / T + Gumbel(u), NaN outside the kept set (never taken)
  auto score4 = [&](int j, const float x[4], int d, float y[4]) {
    uint32_t ctr[4] = {(uint32_t)j, (uint32_t)a.step, (uint32_t)r, (uint32_t)d};
    philox4x32_10(ctr, a.seed_lo, a.seed_hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = 4 * j + c;
      const uint32_t key = sample_key(x[c]);
      const bool kept = v < V && (key > ck || (key == ck && v <= ci) || key > fk || (key == fk && v <= fi));
      y[c] = kept ? x[c] / T + sample_gumbel(ctr[c]) : __builtin_nanf("");
    }
  };
  if (threadIdx.x == 0) nsel = 0;
  if (a.replace) {
    // ---- n independent Gumbel-max draws over the kept set -------------------------------------------------------------------
    for (int d = 0; d < n; ++d) {
      SnbCand mine{-INFINITY, -1};
      for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
        float x[4], y[4];
        row.get4(j, x);
        score4(j, x, d, y);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (!(y[c] != y[c])) snb_take(mine, y[c], 4 * j + c);
      }
      const SnbCand w = snb_block_best(mine, sh);
      if (threadIdx.x == 0) { selv[d] = w.i; nsel = d + 1; }
    }
  } else {
    // ---- Gumbel-top-n: every thread's best (s, v); in the LDS form the score replaces the logit ------------------------------
    SnbCand mine{-INFINITY, -1};
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4], y[4];
      row.get4(j, x);
      score4(j, x, 0, y);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int v = 4 * j + c;
        if (v < V) {
          if (STAGED) srow[v] = y[c];   // (the thread's own entries: no other thread reads them before the barrier below)
          if (!(y[c] != y[c])) snb_take(mine, y[c], v);
        }
      }
    }
    // n rounds of the block argmax; only the winner's thread looks at its tokens again
    for (int i = 0; i < n; ++i) {
      const SnbCand w = snb_block_best(mine, sh);
      if (w.i < 0) break;   // (workgroup-uniform: fewer than n kept tokens)
      if (threadIdx.x == 0) { selv[i] = w.i; nsel = i + 1; }
      if (((w.i >> 2) & (SAMPLE_THREADS - 1)) == (int)threadIdx.x) {   // owner of token w.i: its best after w
        mine = SnbCand{-INFINITY, -1};
        for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
          float y[4];
          if (STAGED) {
#pragma unroll
            for (int c = 0; c < 4; ++c) y[c] = 4 * j + c < V ? srow[4 * j + c] : __builtin_nanf("");
          } else {
            float x[4];
            row.get4(j, x);
            score4(j, x, 0, y);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int v = 4 * j + c;
            if (v < V && !(y[c] != y[c]) && snb_after(y[c], v, w)) snb_take(mine, y[c], v);
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- the candidates: token and summed UNTEMPERED log-prob phi + lp[token], lp read back from the row in global memory --------
  const int ns = nsel;
  for (int i = threadIdx.x; i < n; i += SAMPLE_THREADS) {
    const int v = i < ns ? selv[i] : -1;
    clp[i] = v >= 0 ? phi + (g[v] - lse) : -INFINITY;
    ctok[i] = v >= 0 ? v : a.end_index;
  }
}

// per batch entry b: the top k of the k * n candidates by summed log-prob, descending (sample_beams = torch.topk)
__global__ __launch_bounds__(64) void snb_merge_kernel(const float* __restrict__ clp, const int64_t* __restrict__ ctok, int n, int k,
                                                       const float* __restrict__ last_lp, int64_t* __restrict__ pred,
                                                       float* __restrict__ lp_out, int64_t* __restrict__ backptr, int end_index,
                                                       int* __restrict__ ctl, int step_index, int max_steps, int* __restrict__ host_flag) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool stopped = ctl && ctl[0] <= step_index;   // (written by an EARLIER launch of this stream)
  int live = 0;
  if (stopped) {
    // the search had ended before this step: END at +0 from the same beam, so that nothing moves
    if (lane < k) {
      const size_t o = (size_t)b * k + lane;
      pred[o] = end_index;
      lp_out[o] = last_lp[o];
      backptr[o] = lane;
    }
  } else {
    const int C = k * n;
    const float* l = clp + (size_t)b * C;
    SnbCand prev{INFINITY, -1};
    for (int i = 0; i < k; ++i) {
      SnbCand best{-INFINITY, -1};
      for (int c = lane; c < C; c += 64) {
        const float x = l[c];
        if (x > -INFINITY && snb_after(x, c, prev)) snb_take(best, x, c);   // (finite log-probs only: NaN and -inf are never taken)
      }
      best = snb_wave_best(best);
      if (best.i >= 0) prev = best;
      if (lane == 0) {
        const size_t o = (size_t)b * k + i;
        const int c = best.i;
        const int64_t tok = c >= 0 ? ctok[(size_t)b * C + c] : (int64_t)end_index;
        pred[o] = tok;
        lp_out[o] = c >= 0 ? best.v : -INFINITY;
        backptr[o] = c >= 0 ? c / n : i;
        live += tok != end_index;
      }
    }
  }
  if (ctl && lane == 0) {
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
      // progress word: ssc_decode_sampled_beam queues step t only once step t - 2 has got here (its run-ahead bound)
      if (host_flag) __hip_atomic_store(host_flag + 1, step_index, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

// trivial machine aside (checked by the callers): 1 <= k, n <= 32, k, n <= V, B * k <= 2^24, T > 0 finite, a known kind, top-k with
// n <= top_k <= V, 0 <= top_p <= 1
bool ssc_sampled_beam_ok(int B, int k, int n, int V, const ssc_sampler_desc* s) {
  if (!s || B <= 0 || V <= 0 || k < 1 || k > SNB_MAX_BEAM || n < 1 || n > SNB_MAX_BEAM || k > V || n > V) return false;
  if ((long)B * k > (1L << 24)) return false;
  if (!(s->temperature > 0.f) || !isfinite(s->temperature)) return false;
  if (s->kind == 0) return true;
  if (s->kind == 1) return s->top_k >= n && s->top_k <= V;
  if (s->kind == 2) return s->top_p >= 0.f && s->top_p <= 1.f;
  return false;
}

extern "C" int ssc_beam_step_sampled(const ssc_beam_desc* d, const ssc_sampler_desc* s, int with_replacement, void* stream) {
  if (!d || !d->scores || !d->pred || !d->lp_out || !d->backptr || !d->last_pred || !d->last_lp || !d->scratch_val ||
      !d->scratch_idx)
    return SSC_EINVAL;
  if (d->fsm || d->tables || d->mach || d->dims.S != 1 || d->ld < d->dims.V) return SSC_EINVAL;
  if (!ssc_sampled_beam_ok(d->B, d->beam, d->per_node, d->dims.V, s)) return SSC_EINVAL;
  if (d->end_index < 0 || d->end_index >= d->dims.V) return SSC_EINVAL;
  if (d->step_index <= 0 || (d->ctl && (d->max_steps <= 0 || d->step_index >= d->max_steps))) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, k = d->beam, n = d->per_node;
  SnbRowArgs a{};
  a.logits = d->scores; a.ld = (size_t)d->ld; a.V = d->dims.V; a.n = n;
  a.kind = s->kind; a.top_k = s->top_k; a.top_p = s->top_p; a.temperature = s->temperature;
  a.replace = with_replacement ? 1 : 0;
  a.seed_lo = (uint32_t)(s->seed & 0xffffffffu); a.seed_hi = (uint32_t)(s->seed >> 32); a.step = d->step_index;
  a.last_pred = d->last_pred; a.phi = d->last_lp; a.end_index = d->end_index; a.ctl = d->ctl;
  a.clp = d->scratch_val; a.ctok = d->scratch_idx;
  SSC_TRY(sample_row_launch(snb_rows_kernel<true>, snb_rows_kernel<false>, a.V, B * k, st, a));
  SSC_LAUNCH(snb_merge_kernel, dim3(B), dim3(64), 0, st, d->scratch_val, d->scratch_idx, n, k, d->last_lp, d->pred, d->lp_out,
             d->backptr, d->end_index, d->ctl, d->step_index, d->max_steps, d->host_flag);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
