// The vocabulary cross-entropy of the train step (include/ssc.h: ssc_ce_fwd / ssc_ce_bwd and their _smooth, _distill and _unlike
// forms): one workgroup of 256 per row (t, b) of the (T*B, V) logits block, then one lane per caption for the per-caption sums.
//   plain       row = lse - x[y]: a two-pass scan (maximum, then the sum of exponentials), element by element.
//   smoothed    row(eps) = lse - (1-eps) x[y] - (eps/V) sum_v x[v] = (lse - x[y]) - (eps/V) sum_v (x[v] - x[y]): the unsmoothed NLL of
//               the row and one extra sum, taken relative to the target logit so that no large lse - mean(x) difference is ever
//               formed; ONE scan of the row (running maximum, rescaled sum of exponentials, sum_v (x[v] - x[y])).
//   distilled   the student's row x against the teacher's scores row s at temperature tau, mixed with the smoothed hard loss:
//               q = softmax(s / tau), p_tau = softmax(x / tau), kd_row = tau^2 KL(q || p_tau), row = (1 - alpha) row(eps) + alpha kd_row.
//               The forward walks the two rows twice:
//                 1. the two maxima Mx, Ms and sum_v (x[v] - x[y]): the one read of both rows from HBM (2 * V * 4 bytes);
//                 2. sum exp(x - Mx), sum exp((x - Mx) / tau), sum exp((s - Ms) / tau) and the q-weighted sum
//                    sum_v exp((s[v] - Ms) / tau) * ((s[v] - Ms) - (x[v] - Mx)) / tau: the workgroup has just streamed both rows, the
//                    pass hits L2.
//               kd_row = tau^2 (A / Ss - (log Ss - log Sxt)): every term is relative to its row's maximum, so a constant added to s
//               (raw logits or log-probs) never enters a sum and no two large quantities cancel; a teacher that is a bit copy of the
//               student gives exactly 0.  An entry whose exp((s - Ms) / tau) is 0 - s = -inf - is skipped: 0 * inf never appears; a
//               student entry at -inf under positive teacher mass gives +inf; a NaN in either row makes its sums NaN.
//   unlikelihood  beside the smoothed likelihood of its target, row (t, b) lowers the probability of the candidates
//               C(t,b) = the distinct targets y[s,b], s < t, w[s,b] != 0, minus y[t,b]:   ul_row = - sum_c log(max(1 - p[c], delta)).
//               Lane s owns context position s (T <= 256): lane s < t puts y[s,b] (-1 where w[s,b] = 0) into LDS (1 KB) and keeps it
//               when it differs from the row's target and no earlier position holds it - an O(t) look-back in LDS; forward and
//               backward build the same list.  Forward: the smoothed scan, then the surviving lanes gather their x[c] - at most t
//               loads of a row the workgroup has just streamed -, form om_c = -expm1f(x[c] - lse), -log(max(om_c, delta)) and
//               g_c = p[c] / om_c (0 when clamped); two block reductions give ul_row and G = sum_c g_c.  Backward: the candidate
//               lanes read x[c] and form alpha * g_c * coef BEFORE any lane overwrites the row; a barrier; the in-place stream
//               x <- (softmax(x) - keep [v == y] - eps/V - alpha G softmax(x)) * coef; a barrier; the candidate lanes add their patch
//               to x[c] (distinct ids: no two lanes write one element).
// Every backward is one in-place stream over the row: x <- (the row's gradient) * gl[b] * w[row] * n / (n + 1e-13).
// All but the plain pair move 16 bytes per lane where the host's ssc_row_split allows it (ldl % 4 == 0; with a teacher, its rows
// sharing the student's misalignment and ldt % 4 == 0), else element by element.  Columns V .. ld-1 are never touched.  No atomics,
// every sum in a fixed order: two calls agree bit for bit.
#include <math.h>

#include <initializer_list>

#include "ssc_common.h"

namespace {

// What the host hands every kernel but the plain pair (which keep the few scalars they always took): the call's arguments and what
// ce_form made of them.  Kernels read the fields of their own form only.
struct CeArgs {
  float* logits; int ldl;          // (the forward only reads it)
  const float* teacher; int ldt;   // distillation: the teacher's scores
  const int64_t* targets;
  const float *w, *nvalid, *gl;
  float *lse, *nllw, *nllw0;       // (the backward only reads lse)
  float *loss, *nll;
  int T, B, V, rows;               // rows = T * B
  int head, n4;                    // ssc_row_split of the row (pair)
  float eps, keep, eps_over_v;     // keep = 1 - eps
  // the term beside the smoothed hard loss, if any: its descriptor's `rows` (distillation: [lse(x/tau) | lse(s/tau) | w*kd_row],
  // unlikelihood: [G | w*ul_row], `rows` floats each), the [w*term] block among them and the descriptor's per-caption sums (or null)
  float *trows, *termw, *term;
  float alpha, tau, inv_tau, atau, delta;   // atau = alpha * tau (distillation); delta = min_one_minus (unlikelihood)
};

// ---- the pieces every form shares --------------------------------------------------------------------------------------------------

// the padded-target exit of a forward kernel: no loss, and the row (either matrix's) may not have been computed at all - a zero
// into every row block the kernel owns
template <class... P>
__device__ __forceinline__ void ce_pad_row(int row, P*... block) {
  if (threadIdx.x == 0) ((block[row] = 0.f), ...);
}

__device__ __forceinline__ void ce_online(float x, float r, float& m, float& s, float& d) {
  if (x > m) { s *= expf(m - x); m = x; }
  s += expf(x - m);
  d += x - r;
}

// One scan of the row p for this thread: running max m, the sum s of exp(x - m) rescaled when m moves, and the sum d of x - r.
// Elements [0, head) and [head + 4 * n4, V) go one by one, the n4 groups of four in between as 16-byte loads with one rescale per
// group (head = V, n4 = 0: the scalar path throughout).
__device__ __forceinline__ void ce_row_scan(const float* __restrict__ p, int V, int head, int n4, float r, float& m, float& s,
                                            float& d) {
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 x = p4[i];
    const float mx = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
    if (mx > m) { s *= expf(m - mx); m = mx; }
    s += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
    d += ((x.x - r) + (x.y - r)) + ((x.z - r) + (x.w - r));
  }
  const int tail = head + (n4 << 2), ns = head + (V - tail);
  for (int k = threadIdx.x; k < ns; k += 256) ce_online(p[ssc_row_split_col(k, head, tail)], r, m, s, d);
}

// f(x[v], s[v]) over the row pair, split as above
template <class F>
__device__ __forceinline__ void ce_pair_scan(const float* __restrict__ x, const float* __restrict__ s, int V, int head, int n4, F f) {
  const float4* x4 = reinterpret_cast<const float4*>(x + head);
  const float4* s4 = reinterpret_cast<const float4*>(s + head);
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 a = x4[i], b = s4[i];
    f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
  }
  const int tail = head + (n4 << 2), ns = head + (V - tail);
  for (int k = threadIdx.x; k < ns; k += 256) {
    const int v = ssc_row_split_col(k, head, tail);
    f(x[v], s[v]);
  }
}

// the backward's factor of row (t, b): the caption's loss gradient, the row's weight and the per-caption normalisation
__device__ __forceinline__ float ce_bwd_coef(const float* __restrict__ gl, const float* __restrict__ w,
                                             const float* __restrict__ nvalid, int row, int b) {
  const float n = nvalid[b];
  return gl[b] * w[row] * (n / (n + 1e-13f));
}

// a row whose factor is 0: zeros, and never a load - a padded target's rows may hold anything
__device__ __forceinline__ void ce_row_zero(float* p, int V, int head, int n4) {
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const int tail = head + (n4 << 2), ns = head + (V - tail);
  for (int i = threadIdx.x; i < n4; i += 256) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = threadIdx.x; k < ns; k += 256) p[ssc_row_split_col(k, head, tail)] = 0.f;
}

__device__ __forceinline__ float4 ce_load4(const float* p, int head, int i) { return reinterpret_cast<const float4*>(p + head)[i]; }

// in place over the split row: x[v] <- one(x[v], side[v]..., v), `side` the rows read beside it (none, or the teacher's).  No barrier.
template <class F, class... S>
__device__ __forceinline__ void ce_row_stream(float* x, int V, int head, int n4, F one, const S*... side) {
  float4* x4 = reinterpret_cast<float4*>(x + head);
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 a = x4[i];
    const int v = head + (i << 2);
    a.x = one(a.x, ce_load4(side, head, i).x..., v);
    a.y = one(a.y, ce_load4(side, head, i).y..., v + 1);
    a.z = one(a.z, ce_load4(side, head, i).z..., v + 2);
    a.w = one(a.w, ce_load4(side, head, i).w..., v + 3);
    x4[i] = a;
  }
  const int tail = head + (n4 << 2), ns = head + (V - tail);
  for (int k = threadIdx.x; k < ns; k += 256) {
    const int v = ssc_row_split_col(k, head, tail);
    x[v] = one(x[v], side[v]..., v);
  }
}

// the gradient of the smoothed hard loss at element v: sm = softmax(x)[v], tgt the row's target
__device__ __forceinline__ float ce_hard(float sm, int v, int tgt, float keep, float eps_over_v) {
  return sm - (v == tgt ? keep : 0.f) - eps_over_v;
}

// sum[j] = the sum over the T steps of caption b of the (T, B) block blk[j], j < N: eight loads of each block in flight, summed in
// step order; each(t, x) sees the first block's element of step t
template <int N, class F>
__device__ __forceinline__ void ce_caption_sums(const float* const* blk, int T, int B, int b, float* sum, F each) {
#pragma unroll
  for (int j = 0; j < N; ++j) sum[j] = 0.f;
  for (int t = 0; t < T; t += 8) {
    float x[N][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t i = (size_t)min(t + u, T - 1) * B + b;
#pragma unroll
      for (int j = 0; j < N; ++j) x[j][u] = blk[j][i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool live = t + u < T;   // (a select per sum: as an `if` around the N adds it compiled to a branch per step at N = 3)
#pragma unroll
      for (int j = 0; j < N; ++j) sum[j] = live ? sum[j] + x[j][u] : sum[j];
      if (live) each(t + u, x[0][u]);
    }
  }
}

// ---- per-caption sums --------------------------------------------------------------------------------------------------------------
struct CeLossArgs {
  const float* blk[3];   // [w*row(eps)], [w*row(0)], [w*term]: the first N are read
  float* out[3];         // loss (B), nll (B, optional), the term's sums (B, optional)
  float* copy0;          // N = 1 (eps = 0: the first two blocks are one): the [w*row(0)] block to write as a copy, or null
  const float* nvalid;
  int T, B;
};

// One lane per caption: out[j][b] from the first N blocks.  N = 1 also stands for the second: nll[b] = loss[b].
template <int N>
__global__ void ce_loss_kernel(const CeLossArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  float sum[N];
  ce_caption_sums<N>(a.blk, a.T, a.B, b, sum, [&](int t, float x) {
    if (N == 1 && a.copy0) a.copy0[(size_t)t * a.B + b] = x;
  });
  const float n = a.nvalid[b];
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (a.out[j]) a.out[j][b] = n * (sum[j] / (n + 1e-13f));
  if (N == 1 && a.out[1]) a.out[1][b] = n * (sum[0] / (n + 1e-13f));
}

// ---- plain -------------------------------------------------------------------------------------------------------------------------
__global__ void ce_fwd_kernel(const float* __restrict__ logits, int ldl, const int64_t* __restrict__ targets,
                              const float* __restrict__ w, int V, float* __restrict__ lse, float* __restrict__ nllw) {
  __shared__ float sh[16];
  int row = blockIdx.x;
  if (w[row] == 0.f) {
    ce_pad_row(row, lse, nllw);
    return;
  }
  const float* p = logits + (size_t)row * ldl;
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, p[v]);
  mx = ssc_block_reduce(mx, sh, true);
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) s += expf(p[v] - mx);
  s = ssc_block_reduce(s, sh, false);
  if (threadIdx.x == 0) {
    float l = mx + logf(s);
    lse[row] = l;
    nllw[row] = w[row] * (l - p[targets[row]]);
  }
}

// in place: x <- (softmax(x) - [v == y]) * coef, element by element
__global__ void ce_bwd_kernel(float* __restrict__ logits, int ldl, const int64_t* __restrict__ targets,
                              const float* __restrict__ w, const float* __restrict__ nvalid, const float* __restrict__ lse,
                              const float* __restrict__ gl, int B, int V) {
  int row = blockIdx.x;
  float coef = ce_bwd_coef(gl, w, nvalid, row, row % B);
  float* p = logits + (size_t)row * ldl;
  float l = lse[row];
  int tgt = (int)targets[row];
  if (coef == 0.f) {
    for (int v = threadIdx.x; v < V; v += blockDim.x) p[v] = 0.f;
    return;
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    float sm = expf(p[v] - l);
    p[v] = (sm - (v == tgt ? 1.f : 0.f)) * coef;
  }
}

// ---- smoothed ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_fwd_smooth_kernel(const CeArgs a) {
  __shared__ float sh[16];
  const int row = blockIdx.x;
  const float wr = a.w[row];
  if (wr == 0.f) {
    ce_pad_row(row, a.lse, a.nllw, a.nllw0);
    return;
  }
  const float* p = a.logits + (size_t)row * a.ldl;
  const float r = p[a.targets[row]];
  float m = -INFINITY, s = 0.f, d = 0.f;
  ce_row_scan(p, a.V, a.head, a.n4, r, m, s, d);
  const float M = ssc_block_reduce(m, sh, true);
  s = ssc_block_reduce(s * expf(m - M), sh, false);   // a thread without elements: m = -inf, s = 0 -> 0
  d = ssc_block_reduce(d, sh, false);
  if (threadIdx.x == 0) {
    const float l = M + logf(s);
    const float nll = l - r;
    a.lse[row] = l;
    a.nllw[row] = wr * (nll - a.eps_over_v * d);
    a.nllw0[row] = wr * nll;
  }
}

// in place: x <- (softmax(x) - keep [v == y] - eps/V) * coef
__global__ __launch_bounds__(256) void ce_bwd_smooth_kernel(const CeArgs a) {
  const int row = blockIdx.x;
  const float coef = ce_bwd_coef(a.gl, a.w, a.nvalid, row, row % a.B);
  float* p = a.logits + (size_t)row * a.ldl;
  if (coef == 0.f) return ce_row_zero(p, a.V, a.head, a.n4);
  const float l = a.lse[row];
  const int tgt = (int)a.targets[row];
  ce_row_stream(p, a.V, a.head, a.n4, [&](float xv, int v) -> float {
    return ce_hard(expf(xv - l), v, tgt, a.keep, a.eps_over_v) * coef;
  });
}

// ---- distilled ---------------------------------------------------------------------------------------------------------------------
// TAU1: tau == 1 - lse(x / tau) is lse(x), formed once
template <bool TAU1>
__global__ __launch_bounds__(256) void kd_fwd_kernel(const CeArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  const float wr = a.w[row];
  if (wr == 0.f) {
    ce_pad_row(row, a.lse, a.nllw, a.nllw0, a.trows, a.trows + a.rows, a.trows + 2 * a.rows);
    return;
  }
  const float* x = a.logits + (size_t)row * a.ldl;
  const float* s = a.teacher + (size_t)row * a.ldt;
  const float r = x[a.targets[row]];
  float mx = -INFINITY, ms = -INFINITY, d = 0.f;
  ce_pair_scan(x, s, a.V, a.head, a.n4, [&](float xv, float sv) {
    mx = fmaxf(mx, xv);
    ms = fmaxf(ms, sv);
    d += xv - r;
  });
  const float Mx = ssc_block_reduce(mx, sh, true), Ms = ssc_block_reduce(ms, sh, true);
  d = ssc_block_reduce(d, sh, false);
  const float it = a.inv_tau;
  float sx = 0.f, sxt = 0.f, ss = 0.f, acc = 0.f;
  ce_pair_scan(x, s, a.V, a.head, a.n4, [&](float xv, float sv) {
    const float dx = xv - Mx, ds = sv - Ms;
    sx += expf(dx);
    if (!TAU1) sxt += expf(dx * it);
    const float es = expf(TAU1 ? ds : ds * it);
    ss += es;
    if (es > 0.f) acc += es * (TAU1 ? ds - dx : (ds - dx) * it);   // q[v] = 0 contributes nothing (never 0 * inf)
  });
  sx = ssc_block_reduce(sx, sh, false);
  sxt = TAU1 ? sx : ssc_block_reduce(sxt, sh, false);
  ss = ssc_block_reduce(ss, sh, false);
  acc = ssc_block_reduce(acc, sh, false);
  if (threadIdx.x == 0) {
    const float l = Mx + logf(sx);
    const float lsxt = logf(sxt), lss = logf(ss);
    const float nll = l - r;
    const float kd = (a.tau * a.tau) * (acc / ss - (lss - lsxt));
    const float hard = nll - a.eps_over_v * d;
    a.lse[row] = l;
    a.nllw[row] = wr * (a.alpha == 1.f ? kd : (1.f - a.alpha) * hard + a.alpha * kd);
    a.nllw0[row] = wr * nll;
    a.trows[row] = TAU1 ? l : Mx * it + lsxt;
    a.trows[a.rows + row] = TAU1 ? Ms + lss : Ms * it + lss;
    a.trows[2 * a.rows + row] = wr * kd;
  }
}

// in place: x <- ((1 - alpha) (softmax(x) - keep [v == y] - eps/V) + alpha tau (p_tau - q)) * coef
template <bool TAU1>
__global__ __launch_bounds__(256) void kd_bwd_kernel(const CeArgs a) {
  const int row = blockIdx.x;
  const float coef = ce_bwd_coef(a.gl, a.w, a.nvalid, row, row % a.B);
  float* p = a.logits + (size_t)row * a.ldl;
  if (coef == 0.f) return ce_row_zero(p, a.V, a.head, a.n4);
  const float l = a.lse[row], lxt = a.trows[row], lst = a.trows[a.rows + row];
  const int tgt = (int)a.targets[row];
  const float hardw = 1.f - a.alpha, it = a.inv_tau;
  ce_row_stream(p, a.V, a.head, a.n4, [&](float xv, float sv, int v) -> float {
    const float sm = expf(xv - l);
    const float pt = TAU1 ? sm : expf(xv * it - lxt);
    const float q = expf((TAU1 ? sv : sv * it) - lst);
    return (hardw * ce_hard(sm, v, tgt, a.keep, a.eps_over_v) + a.atau * (pt - q)) * coef;
  }, a.teacher + (size_t)row * a.ldt);
}

// ---- unlikelihood ------------------------------------------------------------------------------------------------------------------
// The candidate of lane threadIdx.x for row (t, b) with target tgt, or -1: see above.  ids: 256 ints of LDS; holds a barrier, so
// every lane of the workgroup calls it.  An id outside [0, V) is no candidate (it could not be a target of a row with w != 0).
__device__ __forceinline__ int ul_candidate(const int64_t* __restrict__ targets, const float* __restrict__ w, int B, int V, int t,
                                            int b, int tgt, int* ids) {
  const int s = threadIdx.x;
  int id = -1;
  if (s < t) {
    const size_t i = (size_t)s * B + b;
    if (w[i] != 0.f) {
      const int64_t y = targets[i];
      if (y >= 0 && y < V) id = (int)y;
    }
  }
  ids[s] = id;
  __syncthreads();
  if (id < 0 || id == tgt) return -1;
  for (int k = 0; k < s; ++k)
    if (ids[k] == id) return -1;
  return id;
}

// om = 1 - p[c] and g = p[c] / om (0 where the clamp holds) of a candidate whose logit is xc, l the row's log-sum-exp
__device__ __forceinline__ void ul_terms(float xc, float l, float delta, float& om, float& g) {
  const float z = xc - l;
  om = -expm1f(z);
  g = om > delta ? expf(z) / om : 0.f;
}

__global__ __launch_bounds__(256) void ul_fwd_kernel(const CeArgs a) {
  __shared__ float sh[4];
  __shared__ int ids[256];
  const int row = blockIdx.x;
  const float wr = a.w[row];
  if (wr == 0.f) {   // (workgroup-uniform, ahead of the first barrier)
    ce_pad_row(row, a.lse, a.nllw, a.nllw0, a.trows, a.trows + a.rows);
    return;
  }
  const int t = row / a.B, b = row - t * a.B;
  const float* p = a.logits + (size_t)row * a.ldl;
  const int tgt = (int)a.targets[row];
  const int c = ul_candidate(a.targets, a.w, a.B, a.V, t, b, tgt, ids);
  const float r = p[tgt];
  float m = -INFINITY, s = 0.f, d = 0.f;
  ce_row_scan(p, a.V, a.head, a.n4, r, m, s, d);
  const float M = ssc_block_reduce(m, sh, true);
  s = ssc_block_reduce(s * expf(m - M), sh, false);   // a thread without elements: m = -inf, s = 0 -> 0
  d = ssc_block_reduce(d, sh, false);
  const float l = M + logf(s);
  float term = 0.f, g = 0.f;
  if (c >= 0) {
    float om;
    ul_terms(p[c], l, a.delta, om, g);
    term = -logf(fmaxf(om, a.delta));
  }
  const float ul = ssc_block_reduce(term, sh, false);
  const float G = ssc_block_reduce(g, sh, false);
  if (threadIdx.x == 0) {
    const float nll = l - r;
    a.lse[row] = l;
    a.nllw[row] = wr * ((nll - a.eps_over_v * d) + a.alpha * ul);
    a.nllw0[row] = wr * nll;
    a.trows[row] = G;
    a.trows[a.rows + row] = wr * ul;
  }
}

__global__ __launch_bounds__(256) void ul_bwd_kernel(const CeArgs a) {
  __shared__ int ids[256];
  const int row = blockIdx.x;
  const int t = row / a.B, b = row - t * a.B;
  const float coef = ce_bwd_coef(a.gl, a.w, a.nvalid, row, b);
  float* p = a.logits + (size_t)row * a.ldl;
  if (coef == 0.f) return ce_row_zero(p, a.V, a.head, a.n4);   // (workgroup-uniform, ahead of the first barrier)
  const float l = a.lse[row];
  const int tgt = (int)a.targets[row];
  const int c = ul_candidate(a.targets, a.w, a.B, a.V, t, b, tgt, ids);
  float patch = 0.f;
  if (c >= 0) {
    float om, g;
    ul_terms(p[c], l, a.delta, om, g);
    patch = a.alpha * g * coef;
  }
  const float aG = a.alpha * a.trows[row];
  __syncthreads();   // every candidate's logit is read: the row may be overwritten
  ce_row_stream(p, a.V, a.head, a.n4, [&](float xv, int v) -> float {
    const float sm = expf(xv - l);
    return (ce_hard(sm, v, tgt, a.keep, a.eps_over_v) - aG * sm) * coef;
  });
  __syncthreads();   // the dense term is stored: the candidates' own terms go on top
  if (c >= 0) p[c] += patch;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// the [first, first + (rows-1) * ld + V) float ranges of the two matrices may not meet
inline bool kd_overlap(const float* logits, int ldl, const float* teacher, int ldt, size_t rows, int V) {
  const uintptr_t a0 = (uintptr_t)logits, a1 = a0 + ((rows - 1) * (size_t)ldl + (size_t)V) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)teacher, b1 = b0 + ((rows - 1) * (size_t)ldt + (size_t)V) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

// The refusals every entry shares: the common pointers and sizes, the direction's own pointers (`also`) and eps - SSC_EINVAL -, then
// the 4-byte alignment of the logits - SSC_EALIGN; the plain pair, which has no vector path, never asked for it (align4 false).
int ce_check(const CeArgs& a, std::initializer_list<const void*> also, bool align4) {
  bool ok = a.logits && a.targets && a.w && a.nvalid && a.lse && a.T > 0 && a.B > 0 && a.V > 0 && a.ldl >= a.V && ssc_ce_eps_ok(a.eps);
  for (const void* p : also) ok = ok && p;
  if (!ok) return SSC_EINVAL;
  if (align4 && ((uintptr_t)a.logits & 3u) != 0) return SSC_EALIGN;
  return SSC_OK;
}

// The descriptors' refusals on checked arguments, then everything the kernels derive from the call: the smoothing constants, the
// term's fields (kd / ul: the descriptor that is on, or null) and the split of the row (pair).
int ce_form(CeArgs& a, const ssc_distill* kd, const ssc_unlikelihood* ul) {
  bool kd_on, ul_on;
  SSC_TRY(ssc_distill_check(kd, a.logits, a.ldl, (size_t)a.T * a.B, a.V, &kd_on));
  SSC_TRY(ssc_unlike_check(ul, a.T, &ul_on));
  if (kd_on && ul_on) return SSC_EINVAL;   // one term beside the hard loss: the two are not composed
  a.rows = a.T * a.B;
  a.keep = 1.f - a.eps;
  a.eps_over_v = (float)((double)a.eps / a.V);
  if (kd_on) {
    a.teacher = kd->teacher; a.ldt = kd->ldt;
    a.trows = kd->rows; a.termw = kd->rows + 2 * (size_t)a.rows; a.term = kd->kd;
    a.alpha = kd->alpha; a.tau = kd->temperature; a.inv_tau = 1.f / kd->temperature; a.atau = kd->alpha * kd->temperature;
  } else if (ul_on) {
    a.trows = ul->rows; a.termw = ul->rows + (size_t)a.rows; a.term = ul->ul;
    a.alpha = ul->alpha; a.delta = ul->min_one_minus;
  }
  ssc_row_split(a.logits, a.ldl, a.teacher, a.ldt, a.V, &a.head, &a.n4);
  return SSC_OK;
}

// the row kernel of the call's form - a.teacher: distilled; else a.trows: unlikelihood; else eps > 0: smoothed; else plain -, then
// the per-caption sums.  a.nllw0 / a.nll null (the plain entry): no [w*row(0)] block, no unsmoothed loss.
int ce_fwd_run(const CeArgs& a, hipStream_t st) {
  const dim3 grid(a.rows), wg(256);
  if (a.teacher) {
    if (a.tau == 1.f) SSC_LAUNCH(kd_fwd_kernel<true>, grid, wg, 0, st, a);
    else SSC_LAUNCH(kd_fwd_kernel<false>, grid, wg, 0, st, a);
  } else if (a.trows) {
    SSC_LAUNCH(ul_fwd_kernel, grid, wg, 0, st, a);
  } else if (a.eps != 0.f) {
    SSC_LAUNCH(ce_fwd_smooth_kernel, grid, wg, 0, st, a);
  } else {
    SSC_LAUNCH(ce_fwd_kernel, grid, wg, 0, st, a.logits, a.ldl, a.targets, a.w, a.V, a.lse, a.nllw);
  }
  SSC_CHECK_LAUNCH();
  CeLossArgs s{{a.nllw, a.nllw0, a.termw}, {a.loss, a.nll, a.term}, nullptr, a.nvalid, a.T, a.B};
  const dim3 lgrid(ssc_cdiv(a.B, 64)), lwg(64);
  if (a.termw) {
    SSC_LAUNCH(ce_loss_kernel<3>, lgrid, lwg, 0, st, s);
  } else if (a.eps != 0.f) {
    SSC_LAUNCH(ce_loss_kernel<2>, lgrid, lwg, 0, st, s);
  } else {   // the plain row kernel left no [w*row(0)] block: it is a copy of the [w*row(eps)] block
    s.copy0 = a.nllw0;
    SSC_LAUNCH(ce_loss_kernel<1>, lgrid, lwg, 0, st, s);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

int ce_bwd_run(const CeArgs& a, hipStream_t st) {
  const dim3 grid(a.rows), wg(256);
  if (a.teacher) {
    if (a.tau == 1.f) SSC_LAUNCH(kd_bwd_kernel<true>, grid, wg, 0, st, a);
    else SSC_LAUNCH(kd_bwd_kernel<false>, grid, wg, 0, st, a);
  } else if (a.trows) {
    SSC_LAUNCH(ul_bwd_kernel, grid, wg, 0, st, a);
  } else if (a.eps != 0.f) {
    SSC_LAUNCH(ce_bwd_smooth_kernel, grid, wg, 0, st, a);
  } else {
    SSC_LAUNCH(ce_bwd_kernel, grid, wg, 0, st, a.logits, a.ldl, a.targets, a.w, a.nvalid, a.lse, a.gl, a.B, a.V);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

CeArgs ce_args(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B, int V,
               float eps, const float* lse) {
  CeArgs a{};
  a.logits = const_cast<float*>(logits); a.ldl = ldl; a.targets = targets; a.w = w; a.nvalid = nvalid;
  a.T = T; a.B = B; a.V = V; a.eps = eps; a.lse = const_cast<float*>(lse);
  return a;
}

// a forward entry whose `lse` holds the three blocks [lse | w*row(eps) | w*row(0)] one behind the other
int ce_fwd_packed(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B, int V,
                  float eps, const ssc_distill* kd, const ssc_unlikelihood* ul, float* lse, float* loss, float* nll, void* stream) {
  if (!lse || T <= 0 || B <= 0) return SSC_EINVAL;
  const size_t rows = (size_t)T * B;
  return ssc_ce_fwd_blocks(logits, ldl, targets, w, nvalid, T, B, V, eps, kd, ul, lse, lse + rows, lse + 2 * rows, loss, nll,
                           (hipStream_t)stream);
}

}  // namespace

// SSC_OK with *on = whether the descriptor switches distillation on (kd != NULL and alpha > 0); the refusals of include/ssc.h.
// logits may be NULL (the train step checks the descriptor before its workspace exists): the overlap test is then the caller's.
int ssc_distill_check(const ssc_distill* kd, const float* logits, int ldl, size_t rows, int V, bool* on) {
  *on = false;
  if (!kd) return SSC_OK;
  if (!(kd->alpha >= 0.f && kd->alpha <= 1.f)) return SSC_EINVAL;                                     // NaN included
  if (!(kd->temperature > 0.f && kd->temperature <= 3.402823466e38f)) return SSC_EINVAL;              // NaN, inf included
  if (kd->alpha == 0.f) return SSC_OK;
  if (!kd->teacher || !kd->rows || kd->ldt < V) return SSC_EINVAL;
  if (((uintptr_t)kd->teacher & 3u) != 0 || ((uintptr_t)kd->rows & 3u) != 0 || ((uintptr_t)kd->kd & 3u) != 0) return SSC_EALIGN;
  if (logits && kd_overlap(logits, ldl, kd->teacher, kd->ldt, rows, V)) return SSC_EINVAL;
  *on = true;
  return SSC_OK;
}

// SSC_OK with *on = whether the descriptor switches the term on (ul != NULL and alpha > 0); the refusals of include/ssc.h.  T = 0:
// the number of steps is not known yet (the train step checks the descriptor before its layout exists).
int ssc_unlike_check(const ssc_unlikelihood* ul, int T, bool* on) {
  *on = false;
  if (!ul) return SSC_OK;
  if (!(ul->alpha >= 0.f && ul->alpha <= 3.402823466e38f)) return SSC_EINVAL;               // NaN, inf included
  if (!(ul->min_one_minus > 0.f && ul->min_one_minus < 1.f)) return SSC_EINVAL;             // NaN included
  if (ul->alpha == 0.f) return SSC_OK;
  if (!ul->rows || T > 256) return SSC_EINVAL;                                              // one lane per context position
  if (((uintptr_t)ul->rows & 3u) != 0 || ((uintptr_t)ul->ul & 3u) != 0) return SSC_EALIGN;
  *on = true;
  return SSC_OK;
}

int ssc_ce_fwd_blocks(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B, int V,
                      float eps, const ssc_distill* kd, const ssc_unlikelihood* ul, float* lse, float* nllw, float* nllw0, float* loss,
                      float* nll, hipStream_t st) {
  CeArgs a = ce_args(logits, ldl, targets, w, nvalid, T, B, V, eps, lse);
  a.nllw = nllw; a.nllw0 = nllw0; a.loss = loss; a.nll = nll;
  SSC_TRY(ce_check(a, {nllw, nllw0, loss}, true));
  SSC_TRY(ce_form(a, kd, ul));
  return ce_fwd_run(a, st);
}

int ssc_ce_bwd_terms(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
                     const float* gl, int T, int B, int V, float eps, const ssc_distill* kd, const ssc_unlikelihood* ul, hipStream_t st) {
  CeArgs a = ce_args(logits, ldl, targets, w, nvalid, T, B, V, eps, lse);
  a.gl = gl;
  SSC_TRY(ce_check(a, {gl}, true));
  SSC_TRY(ce_form(a, kd, ul));
  return ce_bwd_run(a, st);
}

// lse must hold 2*T*B floats: [lse | w*nll]
extern "C" int ssc_ce_fwd(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T,
                          int B, int V, float* lse, float* loss, void* stream) {
  CeArgs a = ce_args(logits, ldl, targets, w, nvalid, T, B, V, 0.f, lse);
  a.loss = loss;
  SSC_TRY(ce_check(a, {loss}, false));
  SSC_TRY(ce_form(a, nullptr, nullptr));
  a.nllw = lse + a.rows;
  return ce_fwd_run(a, (hipStream_t)stream);
}

extern "C" int ssc_ce_bwd(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                          const float* lse, const float* gl, int T, int B, int V, void* stream) {
  CeArgs a = ce_args(logits, ldl, targets, w, nvalid, T, B, V, 0.f, lse);
  a.gl = gl;
  SSC_TRY(ce_check(a, {gl}, false));
  SSC_TRY(ce_form(a, nullptr, nullptr));
  return ce_bwd_run(a, (hipStream_t)stream);
}

// lse must hold 3*T*B floats: [lse | w*row(eps) | w*row(0)], here and in the two entries below
extern "C" int ssc_ce_fwd_smooth(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                 int T, int B, int V, float eps, float* lse, float* loss, float* nll, void* stream) {
  return ce_fwd_packed(logits, ldl, targets, w, nvalid, T, B, V, eps, nullptr, nullptr, lse, loss, nll, stream);
}

extern "C" int ssc_ce_fwd_distill(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T,
                                  int B, int V, float eps, const ssc_distill* kd, float* lse, float* loss, float* nll, void* stream) {
  return ce_fwd_packed(logits, ldl, targets, w, nvalid, T, B, V, eps, kd, nullptr, lse, loss, nll, stream);
}

extern "C" int ssc_ce_fwd_unlike(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T,
                                 int B, int V, float eps, const ssc_unlikelihood* ul, float* lse, float* loss, float* nll,
                                 void* stream) {
  return ce_fwd_packed(logits, ldl, targets, w, nvalid, T, B, V, eps, nullptr, ul, lse, loss, nll, stream);
}

extern "C" int ssc_ce_bwd_smooth(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                 const float* lse, const float* gl, int T, int B, int V, float eps, void* stream) {
  return ssc_ce_bwd_terms(logits, ldl, targets, w, nvalid, lse, gl, T, B, V, eps, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int ssc_ce_bwd_distill(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                  const float* lse, const float* gl, int T, int B, int V, float eps, const ssc_distill* kd,
                                  void* stream) {
  return ssc_ce_bwd_terms(logits, ldl, targets, w, nvalid, lse, gl, T, B, V, eps, kd, nullptr, (hipStream_t)stream);
}

extern "C" int ssc_ce_bwd_unlike(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                 const float* lse, const float* gl, int T, int B, int V, float eps, const ssc_unlikelihood* ul,
                                 void* stream) {
  return ssc_ce_bwd_terms(logits, ldl, targets, w, nvalid, lse, gl, T, B, V, eps, nullptr, ul, (hipStream_t)stream);
}
