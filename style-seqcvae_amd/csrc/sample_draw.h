// The word draw of one row of raw logits, shared by the word samplers (sample.hip: sample_rows_kernel) and the scheduled-sampling
// mix kernel of the train step (sched_sampling.hip): the row staged with its maximum (row_stage_max of ssc_radix.h), its
// log-sum-exp, the top-k / top-p cut, and the Gumbel-max draw over the kept set with Philox4x32-10 noise of counter
// (v / 4, step, row, 0).  One definition: a kernel that calls sample_draw_row draws ssc_sample_rows' token for the same row, sampler,
// step, row id and seed.  Also the limits of ssc_sampler_desc every entry point that takes one checks before a launch (sampler_ok);
// the launch of the two kernel forms is ssc_radix.h's sample_row_launch.
#pragma once
#include <math.h>

#include "ssc_philox.h"
#include "ssc_radix.h"

namespace {

inline bool sampler_ok(const ssc_sampler_desc* s, int V) {
  if (!s || V <= 0) return false;
  if (!(s->temperature > 0.f) || !isfinite(s->temperature)) return false;
  if (s->kind == 0) return true;
  if (s->kind == 1) return s->top_k >= 1 && s->top_k <= V;
  if (s->kind == 2) return s->top_p >= 0.f && s->top_p <= 1.f;
  return false;
}

// The early stop of a sampled decode's draw kernels (the protocol of ssc_beam_desc.ctl, with the step as the column index), called
// by ONE thread per workgroup behind the row's writes: count the rows that have not ended (`live`); the last workgroup of the step
// notes an all-ended step in ctl[0] / host_flag[0] and its own completion in host_flag[1].  stopped: ctl[0] <= step at entry.
__device__ __forceinline__ void sample_step_done(int* ctl, int max_steps, int* host_flag, int step, bool stopped, bool live) {
  int* cnt = ctl + 2 + step;
  int* ticket = ctl + 2 + max_steps + step;
  if (live) atomicAdd(cnt, 1);
  __threadfence();
  const int done = atomicAdd(ticket, 1);
  if (done == (int)gridDim.x - 1) {
    if (!stopped) {
      __threadfence();
      if (atomicAdd(cnt, 0) == 0) {
        atomicMin(ctl, step + 1);
        if (host_flag) __hip_atomic_store(host_flag, step + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (host_flag) __hip_atomic_store(host_flag + 1, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct SampleDraw {
  int tok;            // the drawn token (-1: no entry of the row is comparable - every logit NaN)
  float lp;           // its untempered log-probability
  float mx, zk;       // the row's maximum; with want_zk the thread's share of the kept set's tempered mass (block_sum it)
  uint32_t cut_key;   // kept <=> key > cut_key, or key == cut_key and v <= cut_idx
  int cut_idx;
};

// Every thread of the workgroup (SAMPLE_THREADS) calls it for the same row; tok, lp, mx and the cut come back the same on all.
// g: the row in global memory, read once when STAGED (into srow, (V + 3) & ~3 floats of LDS), else once per pass.
template <bool STAGED>
__device__ __forceinline__ SampleDraw sample_draw_row(const float* g, float* srow, int V, int kind, int top_k, float top_p, float T,
                                                      uint32_t seed_lo, uint32_t seed_hi, int step, uint32_t b, bool want_zk,
                                                      SampleShared& sh) {
  SampleDraw out;
  RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
  const int nj = (V + 3) >> 2;
  // ---- stage the row (once from HBM) and its maximum ---------------------------------------------------------------------
  const float mx = row_stage_max(row, srow, sh);
  const bool topp = kind == 2 && top_p < 1.f;
  // ---- untempered log-sum-exp (the step log-prob) and the tempered normaliser (top-p masses) -------------------------------
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
  // ---- the cut: kept <=> key > cut_key, or key == cut_key and v <= cut_idx ------------------------------------------------
  // (the same code as sample_cut in ssc_radix.h, kept inline here because the samplers' ISA is held fixed: change both together)
  uint32_t cut_key = 0;
  int cut_idx = 0x7fffffff;   // (defaults: every entry kept)
  const bool topk = kind == 1 && top_k < V;
  if (topk || topp) {
    unsigned long long thr;
    bool found;
    if (topk) {
      thr = (unsigned long long)top_k;
      radix_descent<STAGED, false>(row, [&](int, float x, uint32_t& key, unsigned long long& w) {
        key = sample_key(x); w = 1; return true; }, thr, sh);
    } else {
      thr = (unsigned long long)llrint((double)top_p * SAMPLE_MASS_ONE);
      radix_descent<STAGED, true>(row, [&](int, float x, uint32_t& key, unsigned long long& w) {
        key = sample_key(x);
        w = (unsigned long long)llrintf(expf((x - mx) / T) * invz * 1099511627776.0f);
        return true; }, thr, sh);
    }
    found = sh.sel_found != 0;
    if (found) {
      cut_key = sh.sel_key;
      const unsigned long long ahead = sh.sel_ahead, wt = sh.sel_w;
      const uint32_t ct = sh.sel_cnt;
      // entries tied at the cut share one weight; the n-th of them (lowest index first) is the cut
      unsigned long long n;
      if (topk) n = thr - ahead;
      else {
        const unsigned long long each = wt / ct;
        n = (each == 0 || thr <= ahead) ? 1 : (thr - ahead + each - 1) / each;
      }
      n = n < 1 ? 1 : (n > ct ? ct : n);
      __syncthreads();
      if (n < ct) {
        const uint32_t ck = cut_key;
        radix_descent<STAGED, false>(row, [&](int v, float x, uint32_t& key, unsigned long long& w) {
          key = ~(uint32_t)v; w = 1; return sample_key(x) == ck; }, n, sh);
        cut_idx = (int)~sh.sel_key;
      }
      __syncthreads();
    }
  }
  // ---- Gumbel-max over the kept set: argmax_v logit_v / T + g_v, ties to the lower index --------------------------------------
  float best = -INFINITY, zk = 0.f;
  int besti = -1;
  for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
    float x[4];
    row.get4(j, x);
    uint32_t ctr[4] = {(uint32_t)j, (uint32_t)step, b, 0u};
    philox4x32_10(ctr, seed_lo, seed_hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = 4 * j + c;
      const uint32_t key = sample_key(x[c]);
      const bool kept = v < V && (key > cut_key || (key == cut_key && v <= cut_idx));
      if (kept) {
        const float sc = x[c] / T + sample_gumbel(ctr[c]);
        if (besti < 0 || sc > best) { best = sc; besti = v; }   // (v ascending within the thread: > keeps the lower index)
        if (want_zk) zk += expf((x[c] - mx) / T);
      }
    }
  }
  // block argmax, ties to the lower index
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (oi >= 0 && (besti < 0 || ov > best || (ov == best && oi < besti))) { best = ov; besti = oi; }
  }
  __syncthreads();
  if (lane == 0) { sh.bestv[threadIdx.x >> 6] = best; sh.besti[threadIdx.x >> 6] = besti; }
  __syncthreads();
  best = sh.bestv[0]; besti = sh.besti[0];
  for (int w = 1; w < SAMPLE_WAVES; ++w) {
    const float ov = sh.bestv[w];
    const int oi = sh.besti[w];
    if (oi >= 0 && (besti < 0 || ov > best || (ov == best && oi < besti))) { best = ov; besti = oi; }
  }
  out.tok = besti;
  out.lp = besti >= 0 ? row.at(besti) - lse : 0.f;
  out.mx = mx; out.zk = zk; out.cut_key = cut_key; out.cut_idx = cut_idx;
  return out;
}

}  // namespace
