// Token-level unlikelihood training in the cross-entropy train step (include/ssc.h: ssc_unlikelihood, ssc_ce_fwd_unlike /
// ssc_ce_bwd_unlike): beside the label-smoothed likelihood of its target, row (t, b) lowers the probability of the candidates
//   C(t,b) = the distinct targets y[s,b], s < t, w[s,b] != 0, minus y[t,b]:   ul_row = - sum_c log(max(1 - p[c], delta)).
// One workgroup of 256 per row, in the manner of ce_fwd_smooth_kernel (pointwise.hip); lane s owns context position s (T <= 256).
//   candidates: lane s < t puts y[s,b] (-1 where w[s,b] = 0) into LDS (1 KB) and keeps it when it differs from the row's target and
//               no earlier position holds it - an O(t) look-back in LDS; forward and backward build the same list.
//   forward:    the single scan of ce_fwd_smooth_kernel (running maximum, rescaled sum of exponentials, sum_v (x[v] - x[y])), then
//               the surviving lanes gather their x[c] - at most t loads of a row the workgroup has just streamed -, form
//               om_c = -expm1f(x[c] - lse), -log(max(om_c, delta)) and g_c = p[c] / om_c (0 when clamped); two block reductions
//               give ul_row and G = sum_c g_c.
//   backward:   the candidate lanes read x[c] and form alpha * g_c * coef BEFORE any lane overwrites the row; a barrier; the in-place
//               stream x <- (softmax(x) - keep [v == y] - eps/V - alpha G softmax(x)) * coef; a barrier; the candidate lanes add
//               their patch to x[c] (distinct ids: no two lanes write one element).
// 16 bytes per lane when ldl % 4 == 0 (ssc_row_split), else element by element.  Columns V .. ld-1 are never touched.  No atomics,
// every sum in a fixed order: two calls agree bit for bit.
#include <math.h>

#include "ssc_common.h"

namespace {

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

struct UlFwdArgs {
  const float* logits; int ldl;
  const int64_t* targets;
  const float* w;
  int B, V, head, n4, rows;
  float eps_over_v, alpha, delta;
  float *lse, *nllw, *nllw0, *ulrows;   // ulrows: [G | w*ul_row], `rows` floats each
};

__global__ __launch_bounds__(256) void ul_fwd_kernel(const UlFwdArgs a) {
  __shared__ float sh[4];
  __shared__ int ids[256];
  const int row = blockIdx.x;
  const float wr = a.w[row];
  if (wr == 0.f) {  // padded target: no loss, and its logits row may not have been computed at all
    if (threadIdx.x == 0) {
      a.lse[row] = 0.f; a.nllw[row] = 0.f; a.nllw0[row] = 0.f;
      a.ulrows[row] = 0.f; a.ulrows[a.rows + row] = 0.f;
    }
    return;
  }
  const int t = row / a.B, b = row - t * a.B;
  const float* p = a.logits + (size_t)row * a.ldl;
  const int tgt = (int)a.targets[row];
  const int c = ul_candidate(a.targets, a.w, a.B, a.V, t, b, tgt, ids);
  const float r = p[tgt];
  // the scan of ce_fwd_smooth_kernel
  float m = -INFINITY, s = 0.f, d = 0.f;
  const int head = a.head, n4 = a.n4;
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 x = p4[i];
    const float mx = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
    if (mx > m) { s *= expf(m - mx); m = mx; }
    s += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
    d += ((x.x - r) + (x.y - r)) + ((x.z - r) + (x.w - r));
  }
  const int tail = head + (n4 << 2), ns = head + (a.V - tail);
  for (int k = threadIdx.x; k < ns; k += 256) {
    const float x = p[ssc_row_split_col(k, head, tail)];
    if (x > m) { s *= expf(m - x); m = x; }
    s += expf(x - m);
    d += x - r;
  }
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
    a.ulrows[row] = G;
    a.ulrows[a.rows + row] = wr * ul;
  }
}

struct UlBwdArgs {
  float* logits; int ldl;
  const int64_t* targets;
  const float *w, *nvalid, *lse, *ulrows, *gl;
  int B, V, head, n4;
  float keep, eps_over_v, alpha, delta;   // keep = 1 - eps
};

__global__ __launch_bounds__(256) void ul_bwd_kernel(const UlBwdArgs a) {
  __shared__ int ids[256];
  const int row = blockIdx.x;
  const int t = row / a.B, b = row - t * a.B;
  const float n = a.nvalid[b];
  const float coef = a.gl[b] * a.w[row] * (n / (n + 1e-13f));
  float* p = a.logits + (size_t)row * a.ldl;
  float4* p4 = reinterpret_cast<float4*>(p + a.head);
  const int head = a.head, n4 = a.n4, tail = head + (n4 << 2), ns = head + (a.V - tail);
  if (coef == 0.f) {  // never reads the row: a padded target's logits may hold anything
    for (int i = threadIdx.x; i < n4; i += 256) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = threadIdx.x; k < ns; k += 256) p[ssc_row_split_col(k, head, tail)] = 0.f;
    return;
  }
  const float l = a.lse[row];
  const int tgt = (int)a.targets[row];
  const int c = ul_candidate(a.targets, a.w, a.B, a.V, t, b, tgt, ids);
  float patch = 0.f;
  if (c >= 0) {
    float om, g;
    ul_terms(p[c], l, a.delta, om, g);
    patch = a.alpha * g * coef;
  }
  const float aG = a.alpha * a.ulrows[row];
  __syncthreads();   // every candidate's logit is read: the row may be overwritten
  auto one = [&](float xv, int v) -> float {
    const float sm = expf(xv - l);
    return ((sm - (v == tgt ? a.keep : 0.f) - a.eps_over_v) - aG * sm) * coef;
  };
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 x = p4[i];
    const int v = head + (i << 2);
    x.x = one(x.x, v);
    x.y = one(x.y, v + 1);
    x.z = one(x.z, v + 2);
    x.w = one(x.w, v + 3);
    p4[i] = x;
  }
  for (int k = threadIdx.x; k < ns; k += 256) {
    const int v = ssc_row_split_col(k, head, tail);
    p[v] = one(p[v], v);
  }
  __syncthreads();   // the dense term is stored: the candidates' own terms go on top
  if (c >= 0) p[c] += patch;
}

}  // namespace

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

// ssc_ce_fwd_unlike with the three blocks of `lse` given one by one (the train workspace keeps the third apart, see
// ssc_ce_fwd_smooth_blocks)
int ssc_ce_fwd_unlike_blocks(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
                             int V, float eps, const ssc_unlikelihood* ul, float* lse, float* nllw, float* nllw0, float* loss,
                             float* nll, hipStream_t st) {
  if (!logits || !targets || !w || !nvalid || !lse || !nllw || !nllw0 || !loss || T <= 0 || B <= 0 || V <= 0 || ldl < V ||
      !ssc_ce_eps_ok(eps))
    return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0) return SSC_EALIGN;
  bool on;
  SSC_TRY(ssc_unlike_check(ul, T, &on));
  if (!on) return ssc_ce_fwd_smooth_blocks(logits, ldl, targets, w, nvalid, T, B, V, eps, lse, nllw, nllw0, loss, nll, st);
  const int rows = T * B;
  UlFwdArgs a{};
  a.logits = logits; a.ldl = ldl; a.targets = targets; a.w = w;
  a.B = B; a.V = V; a.rows = rows;
  ssc_row_split(logits, ldl, nullptr, 0, V, &a.head, &a.n4);
  a.eps_over_v = (float)((double)eps / V); a.alpha = ul->alpha; a.delta = ul->min_one_minus;
  a.lse = lse; a.nllw = nllw; a.nllw0 = nllw0; a.ulrows = ul->rows;
  SSC_LAUNCH(ul_fwd_kernel, dim3(rows), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return ssc_ce_loss3(nllw, nllw0, ul->rows + (size_t)rows, nvalid, T, B, loss, nll, ul->ul, st);
}

// lse must hold 3*T*B floats: [lse | w*row | w*row(0)]
extern "C" int ssc_ce_fwd_unlike(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T,
                                 int B, int V, float eps, const ssc_unlikelihood* ul, float* lse, float* loss, float* nll,
                                 void* stream) {
  if (!lse || T <= 0 || B <= 0) return SSC_EINVAL;
  const size_t rows = (size_t)T * B;
  return ssc_ce_fwd_unlike_blocks(logits, ldl, targets, w, nvalid, T, B, V, eps, ul, lse, lse + rows, lse + 2 * rows, loss, nll,
                                  (hipStream_t)stream);
}

extern "C" int ssc_ce_bwd_unlike(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                 const float* lse, const float* gl, int T, int B, int V, float eps, const ssc_unlikelihood* ul,
                                 void* stream) {
  if (!logits || !targets || !w || !nvalid || !lse || !gl || T <= 0 || B <= 0 || V <= 0 || ldl < V || !ssc_ce_eps_ok(eps))
    return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0) return SSC_EALIGN;
  bool on;
  SSC_TRY(ssc_unlike_check(ul, T, &on));
  if (!on) return ssc_ce_bwd_smooth(logits, ldl, targets, w, nvalid, lse, gl, T, B, V, eps, stream);
  UlBwdArgs a{};
  a.logits = logits; a.ldl = ldl; a.targets = targets;
  a.w = w; a.nvalid = nvalid; a.lse = lse; a.ulrows = ul->rows; a.gl = gl;
  a.B = B; a.V = V;
  ssc_row_split(logits, ldl, nullptr, 0, V, &a.head, &a.n4);
  a.keep = 1.f - eps; a.eps_over_v = (float)((double)eps / V); a.alpha = ul->alpha; a.delta = ul->min_one_minus;
  SSC_LAUNCH(ul_bwd_kernel, dim3(T * B), dim3(256), 0, (hipStream_t)stream, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
