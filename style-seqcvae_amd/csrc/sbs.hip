// Stochastic beam search (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them: The Gumbel-Top-k Trick for Sampling
// Sequences Without Replacement", ICML 2019): the selection of one step as a row kernel and a per-entry merge.  ssc_beam_first_gumbel
// / ssc_beam_step_gumbel are the stand-alone steps; ssc_decode_stochastic_beam (search.hip) runs them inside the one-call search loop.
// Reference: GumbelSampler driving BeamSearch._search (var_updown/var_updown/modules/beam_search.py:294-432, :592-768).
//
// Row kernel, one workgroup per row (b, j).  The row's raw logits are read from HBM once: for V <= SBS_LDS_MAX_V into LDS, longer
// rows take the same passes over global memory.  Passes: the maximum; the log-sum-exp (and, at T != 1, the tempered one); the
// Gumbel pass g_v = (phi + lpT_v) + Gumbel(u_v) with one Philox block per 4 tokens, each thread keeping its best (g, v); then n
// rounds of a block argmax that pick the survivors in (g descending, v ascending) order - after a round only the thread that owned
// the winner rescans its own tokens (from the g it left in LDS, or by recomputing the noise in the global-memory form).
//
// Monotonicity.  gumbel_with_max maps g_v to G_v = Tp - softplus(w_v), w_v = Tp - g_v + log1p(-exp(g_v - Z)), Z = max_v g_v.
// For fixed (Tp, Z) both terms of w_v are strictly decreasing in g_v (-g_v, and log1p(-exp(g_v - Z)) since exp(g_v - Z) rises
// towards 1), and softplus is strictly increasing, so G_v is strictly increasing in g_v.  The top n by G are therefore the top n by
// g, and only the n survivors need the transform: the other V - n tokens cost their noise, one compare and the running maximum.
// (Where the reference's fp32 transform rounds two distinct g to one G, this order is the exact one.)
//
// Merge, one wave per batch entry: top-k of the entry's K * n candidates by G (ties: lower candidate index), then a stable sort of
// those k by summed log-prob, descending.  Early stop: the protocol of ssc_beam_desc.ctl, as beam_merge_kernel (fsm.hip) follows
// it.  A slot that finds no candidate with a finite G emits end_index at -inf with the identity back-pointer, never index -1.
#include <math.h>

#include "ssc_common.h"
#include "ssc_philox.h"

namespace {

constexpr int SBS_THREADS = 256;
constexpr int SBS_WAVES = SBS_THREADS / 64;
constexpr int SBS_LDS_MAX_V = 32768;   // 128 KiB row in LDS of the 160 KiB per CU
constexpr int SBS_MAX_BEAM = 32;       // k <= 32 (the merge's LDS slots and its one wave), 1 <= n <= k

struct SbsCand { float v; int i; };
// the (value descending, index ascending) order
__device__ __forceinline__ bool sbs_better(float x, int i, const SbsCand& c) { return x > c.v || (x == c.v && i < c.i); }
__device__ __forceinline__ bool sbs_after(float x, int i, const SbsCand& p) { return p.i < 0 || x < p.v || (x == p.v && i > p.i); }
__device__ __forceinline__ void sbs_take(SbsCand& best, float x, int i) {
  if (i >= 0 && (best.i < 0 || sbs_better(x, i, best))) best = SbsCand{x, i};
}
__device__ __forceinline__ SbsCand sbs_wave_best(SbsCand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(c.v, o, 64);
    const int oi = __shfl_xor(c.i, o, 64);
    sbs_take(c, ov, oi);
  }
  return c;
}

struct SbsRowArgs {
  const float* logits; size_t ld; int V; int n;
  float temperature;            // 1: untempered (step 0)
  uint32_t seed_lo, seed_hi; int step;
  const int64_t* last_pred;     // (rows) or NULL (step 0)
  const float* phi;             // (rows) running log-probs, or NULL: 0
  const float* gprev;           // (rows) running G, or NULL: target 0
  int end_index;
  const int* ctl;
  float* cg; float* clp; int64_t* ctok;   // (rows, n) candidates: G, summed log-prob, token
};

struct SbsShared {
  float red[SBS_WAVES];
  float bestv[SBS_WAVES];
  int besti[SBS_WAVES];
  float selg[SBS_MAX_BEAM];
  int selv[SBS_MAX_BEAM];
  int nsel;
};

__device__ __forceinline__ float sbs_block_max(float v, SbsShared& sh) {
  v = ssc_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh.red[0];
  for (int w = 1; w < SBS_WAVES; ++w) r = fmaxf(r, sh.red[w]);
  return r;
}
__device__ __forceinline__ float sbs_block_sum(float v, SbsShared& sh) {
  v = ssc_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh.red[0];
  for (int w = 1; w < SBS_WAVES; ++w) r += sh.red[w];
  return r;
}
__device__ __forceinline__ SbsCand sbs_block_best(SbsCand c, SbsShared& sh) {
  c = sbs_wave_best(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh.bestv[threadIdx.x >> 6] = c.v; sh.besti[threadIdx.x >> 6] = c.i; }
  __syncthreads();
  SbsCand r{sh.bestv[0], sh.besti[0]};
  for (int w = 1; w < SBS_WAVES; ++w) sbs_take(r, sh.bestv[w], sh.besti[w]);
  return r;
}

// four consecutive row entries (entries >= V read as -inf)
__device__ __forceinline__ void sbs_get4(const float* p, bool vec, int V, int j, float x[4]) {
  const int v = 4 * j;
  if (vec && v + 3 < V) {
    const float4 q = *reinterpret_cast<const float4*>(p + v);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c] = v + c < V ? p[v + c] : -INFINITY;
}

template <bool STAGED>
__global__ __launch_bounds__(SBS_THREADS) void sbs_rows_kernel(SbsRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SbsShared sh;
  const int r = blockIdx.x;
  const int V = a.V, n = a.n;
  const bool stopped = a.ctl && a.ctl[0] <= a.step;   // (written by an EARLIER launch of this stream: the search has ended)
  const bool ended = stopped || (a.last_pred && a.last_pred[r] == a.end_index);   // workgroup-uniform
  const float phi = a.phi ? a.phi[r] : 0.f;
  const float Tp = a.gprev ? a.gprev[r] : 0.f;
  float* cg = a.cg + (size_t)r * n;
  float* clp = a.clp + (size_t)r * n;
  int64_t* ctok = a.ctok + (size_t)r * n;
  if (ended) {   // one-hot at end_index (beam_search.py:656-688): G stays Tp exactly, the log-prob phi + 0; no read, no noise
    for (int i = threadIdx.x; i < n; i += SBS_THREADS) {
      cg[i] = i == 0 ? Tp : -INFINITY;
      clp[i] = i == 0 ? phi : -INFINITY;
      ctok[i] = a.end_index;
    }
    return;
  }
  const float* g = a.logits + (size_t)r * a.ld;
  const bool gvec = ssc_aligned16_dev(g) && (V & 3) == 0;
  const float* rowp = STAGED ? srow : g;
  const bool rvec = STAGED ? true : gvec;
  const int nj = (V + 3) >> 2;
  // ---- stage the row (once from HBM) and its maximum -----------------------------------------------------------------------
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < nj; j += SBS_THREADS) {
    float x[4];
    sbs_get4(g, gvec, V, j, x);
    if (STAGED) {
      if (4 * j + 3 < V) {
        *reinterpret_cast<float4*>(srow + 4 * j) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
        for (int c = 0; c < 4; ++c)
          if (4 * j + c < V) srow[4 * j + c] = x[c];
      }
    }
    mx = fmaxf(fmaxf(mx, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
  }
  mx = sbs_block_max(mx, sh);   // (its barriers also publish srow)
  // ---- log-sum-exp of the row (lp = x - lse) and, at T != 1, of the tempered log-probs (lpT = (x - lse) / T - lseT) ---------
  float s = 0.f;
  for (int j = threadIdx.x; j < nj; j += SBS_THREADS) {
    float x[4];
    sbs_get4(rowp, rvec, V, j, x);
#pragma unroll
    for (int c = 0; c < 4; ++c) s += expf(x[c] - mx);
  }
  const float lse = mx + logf(sbs_block_sum(s, sh));
  const float T = a.temperature;
  const bool tempered = T != 1.f;
  float lseT = 0.f;
  if (tempered) {
    const float mT = (mx - lse) / T;
    float st = 0.f;
    for (int j = threadIdx.x; j < nj; j += SBS_THREADS) {
      float x[4];
      sbs_get4(rowp, rvec, V, j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) st += expf((x[c] - lse) / T - mT);
    }
    lseT = mT + logf(sbs_block_sum(st, sh));
  }
  // g of the four tokens of block j: (phi + lpT_v) + Gumbel(u_v), the reference's gumbel(phi_S + _log_probs) (beam_search.py:410-416)
  auto g4 = [&](int j, const float x[4], float y[4]) {
    uint32_t ctr[4] = {(uint32_t)j, (uint32_t)a.step, (uint32_t)r, 0u};
    philox4x32_10(ctr, a.seed_lo, a.seed_hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float lp = x[c] - lse;
      const float lpT = tempered ? lp / T - lseT : lp;
      y[c] = sample_gumbel(ctr[c]) + (phi + lpT);
    }
  };
  // ---- the Gumbel pass: every thread's best (g, v); in the LDS form g replaces the logit ------------------------------------
  SbsCand mine{-INFINITY, -1};
  for (int j = threadIdx.x; j < nj; j += SBS_THREADS) {
    float x[4], y[4];
    sbs_get4(rowp, rvec, V, j, x);
    g4(j, x, y);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = 4 * j + c;
      if (v < V) {
        if (STAGED) srow[v] = y[c];   // (the thread's own entries: no other thread reads them before the barrier below)
        if (!(y[c] != y[c])) sbs_take(mine, y[c], v);   // (v ascending within the thread: ties keep the lower index)
      }
    }
  }
  // ---- n rounds of the block argmax; only the winner's thread looks at its tokens again ----------------------------------------
  if (threadIdx.x == 0) sh.nsel = 0;
  for (int i = 0; i < n; ++i) {
    const SbsCand w = sbs_block_best(mine, sh);
    if (w.i < 0) break;   // (workgroup-uniform: no token left with a comparable g - a row of NaN)
    if (threadIdx.x == 0) { sh.selg[i] = w.v; sh.selv[i] = w.i; sh.nsel = i + 1; }
    if (((w.i >> 2) & (SBS_THREADS - 1)) == (int)threadIdx.x) {   // owner of token w.i: its best after w
      mine = SbsCand{-INFINITY, -1};
      for (int j = threadIdx.x; j < nj; j += SBS_THREADS) {
        float y[4];
        if (STAGED) {
#pragma unroll
          for (int c = 0; c < 4; ++c) y[c] = 4 * j + c < V ? srow[4 * j + c] : -INFINITY;
        } else {
          float x[4];
          sbs_get4(g, gvec, V, j, x);
          g4(j, x, y);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int v = 4 * j + c;
          if (v < V && !(y[c] != y[c]) && sbs_after(y[c], v, w)) sbs_take(mine, y[c], v);
        }
      }
    }
  }
  __syncthreads();
  // ---- gumbel_with_max for the survivors only (beam_search.py:418-432), Z = the first survivor's g ------------------------------
  const int ns = sh.nsel;
  for (int i = threadIdx.x; i < n; i += SBS_THREADS) {
    if (i < ns) {
      const float Z = sh.selg[0], gv = sh.selg[i];
      const int v = sh.selv[i];
      const float w = Tp - gv + log1pf(-expf(gv - Z));
      cg[i] = Tp - fmaxf(w, 0.f) - log1pf(expf(-fabsf(w)));
      clp[i] = phi + (g[v] - lse);   // the UNTEMPERED log-prob of the token (:360), read back from the row in global memory
      ctok[i] = v;
    } else {
      cg[i] = -INFINITY;
      clp[i] = -INFINITY;
      ctok[i] = a.end_index;
    }
  }
}

// per batch entry b: top-k of the K * n candidates by G, then a stable sort by summed log-prob (sample_beams, beam_search.py:366-403)
__global__ __launch_bounds__(64) void sbs_merge_kernel(const float* __restrict__ cg, const float* __restrict__ clp,
                                                       const int64_t* __restrict__ ctok, int K, int n, int k,
                                                       const float* __restrict__ last_lp, const float* __restrict__ g_last,
                                                       int64_t* __restrict__ pred, float* __restrict__ lp_out,
                                                       float* __restrict__ g_out, int64_t* __restrict__ backptr, int end_index,
                                                       int* __restrict__ ctl, int step_index, int max_steps,
                                                       int* __restrict__ host_flag) {
  __shared__ float sg[SBS_MAX_BEAM], sl[SBS_MAX_BEAM];
  __shared__ int sc[SBS_MAX_BEAM];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool stopped = ctl && ctl[0] <= step_index;   // (written by an EARLIER launch of this stream)
  bool live = false;
  if (stopped) {
    // the search had ended before this step: END at +0 from the same beam, so that nothing moves
    if (lane < k) {
      const size_t o = (size_t)b * k + lane;
      pred[o] = end_index;
      lp_out[o] = last_lp ? last_lp[o] : 0.f;
      g_out[o] = g_last ? g_last[o] : 0.f;
      if (backptr) backptr[o] = lane;
    }
  } else {
    const int C = K * n;
    const float* g = cg + (size_t)b * C;
    SbsCand prev{INFINITY, -1};
    for (int i = 0; i < k; ++i) {
      SbsCand best{-INFINITY, -1};
      for (int c = lane; c < C; c += 64) {
        const float x = g[c];
        if (x > -INFINITY && sbs_after(x, c, prev)) sbs_take(best, x, c);   // (finite G only: NaN and -inf are never taken)
      }
      best = sbs_wave_best(best);
      if (lane == 0) { sg[i] = best.v; sc[i] = best.i; }
      if (best.i >= 0) prev = best;
    }
    __syncthreads();
    // the k selected, stably by summed log-prob descending: slot i goes to its rank (NaN ranks as -inf)
    float l = -INFINITY;
    int c = -1;
    if (lane < k) {
      c = sc[lane];
      if (c >= 0) l = clp[(size_t)b * C + c];
      if (l != l) l = -INFINITY;
      sl[lane] = l;
    }
    __syncthreads();
    if (lane < k) {
      int rank = 0;
      for (int j = 0; j < k; ++j) rank += sl[j] > l || (sl[j] == l && j < lane);
      const size_t o = (size_t)b * k + rank;
      const int64_t tok = c >= 0 ? ctok[(size_t)b * C + c] : (int64_t)end_index;
      pred[o] = tok;
      lp_out[o] = l;
      g_out[o] = c >= 0 ? sg[lane] : -INFINITY;
      if (backptr) backptr[o] = c >= 0 ? c / n : rank;
      live = tok != end_index;
    }
  }
  const int not_ended = __popcll(__ballot(live));
  if (ctl && lane == 0) {
    int* cnt = ctl + 2 + step_index;
    int* ticket = ctl + 2 + max_steps + step_index;
    if (not_ended) atomicAdd(cnt, not_ended);
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
      // progress word: ssc_decode_stochastic_beam queues step t only once step t - 2 has got here (its run-ahead bound)
      if (host_flag) __hip_atomic_store(host_flag + 1, step_index, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

int sbs_rows_launch(const SbsRowArgs& a, int rows, hipStream_t st) {
  if (a.V <= SBS_LDS_MAX_V) {
    const size_t lds = (size_t)((a.V + 3) & ~3) * 4;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)sbs_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return SSC_EHIP;
    SSC_LAUNCH(sbs_rows_kernel<true>, dim3(rows), dim3(SBS_THREADS), lds, st, a);
  } else {
    SSC_LAUNCH(sbs_rows_kernel<false>, dim3(rows), dim3(SBS_THREADS), 0, st, a);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// the limits of both entries (include/ssc.h): trivial machine, 1 <= n <= k <= min(32, V), T > 0 finite, scratch for the candidates
bool sbs_desc_ok(const ssc_beam_desc* d, const ssc_gumbel_desc* s, int per_node) {
  if (!d || !s || !d->scores || !d->pred || !d->lp_out || !d->scratch_val || !d->scratch_idx) return false;
  if (d->fsm || d->tables || d->mach || d->dims.S != 1) return false;
  const int V = d->dims.V, k = d->beam;
  if (d->B <= 0 || V <= 0 || d->ld < V || k < 1 || k > SBS_MAX_BEAM || k > V || per_node < 1 || per_node > k || per_node > V) return false;
  if ((long)d->B * k > (1L << 24)) return false;
  if (d->end_index < 0 || d->end_index >= V) return false;
  if (!(s->temperature > 0.f) || !isfinite(s->temperature)) return false;
  return true;
}

SbsRowArgs sbs_args(const ssc_beam_desc* d, const ssc_gumbel_desc* s, int n, float T, int step) {
  SbsRowArgs a{};
  a.logits = d->scores; a.ld = (size_t)d->ld; a.V = d->dims.V; a.n = n; a.temperature = T;
  a.seed_lo = (uint32_t)(s->seed & 0xffffffffu); a.seed_hi = (uint32_t)(s->seed >> 32); a.step = step;
  a.end_index = d->end_index; a.ctl = d->ctl;
  a.cg = d->scratch_val; a.ctok = d->scratch_idx;
  return a;
}

}  // namespace

extern "C" int ssc_beam_first_gumbel(const ssc_beam_desc* d, const ssc_gumbel_desc* s, float* g_out, void* stream) {
  if (!sbs_desc_ok(d, s, d ? d->beam : 0) || !g_out) return SSC_EINVAL;
  if (d->ctl && d->max_steps <= 0) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, k = d->beam;
  // step 0 (init_state + sample_beams): one row per entry, untempered, target 0, the top k of the row are the k candidates
  SbsRowArgs a = sbs_args(d, s, k, 1.f, 0);
  a.clp = d->scratch_val + (size_t)B * k;
  a.ctl = nullptr;
  SSC_TRY(sbs_rows_launch(a, B, st));
  SSC_LAUNCH(sbs_merge_kernel, dim3(B), dim3(64), 0, st, d->scratch_val, a.clp, d->scratch_idx, 1, k, k, nullptr, nullptr, d->pred,
             d->lp_out, g_out, nullptr, d->end_index, d->ctl, 0, d->max_steps, d->host_flag);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_beam_step_gumbel(const ssc_beam_desc* d, const ssc_gumbel_desc* s, const float* g_last, float* g_out,
                                    void* stream) {
  if (!sbs_desc_ok(d, s, d ? d->per_node : 0) || !g_last || !g_out || !d->last_pred || !d->last_lp || !d->backptr) return SSC_EINVAL;
  if (d->step_index <= 0 || (d->ctl && (d->max_steps <= 0 || d->step_index >= d->max_steps))) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, k = d->beam, n = d->per_node, rows = B * k;
  SbsRowArgs a = sbs_args(d, s, n, s->temperature, d->step_index);
  a.clp = d->scratch_val + (size_t)rows * n;
  a.last_pred = d->last_pred; a.phi = d->last_lp; a.gprev = g_last;
  SSC_TRY(sbs_rows_launch(a, rows, st));
  SSC_LAUNCH(sbs_merge_kernel, dim3(B), dim3(64), 0, st, d->scratch_val, a.clp, d->scratch_idx, k, n, k, d->last_lp, g_last, d->pred,
             d->lp_out, g_out, d->backptr, d->end_index, d->ctl, d->step_index, d->max_steps, d->host_flag);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
