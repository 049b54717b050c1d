// Knowledge distillation in the cross-entropy train step (include/ssc.h: ssc_distill, ssc_ce_fwd_distill / ssc_ce_bwd_distill):
// the student's row x is trained against the teacher's scores row s at temperature tau, mixed with the label-smoothed hard loss,
//   q = softmax(s / tau), p_tau = softmax(x / tau), kd_row = tau^2 KL(q || p_tau), row = (1 - alpha) row(eps) + alpha kd_row.
// One workgroup of 256 per row, in the manner of ce_fwd_smooth_kernel (pointwise.hip).  The forward walks the two rows twice:
//   1. the two maxima Mx, Ms and sum_v (x[v] - x[y]): the one read of both rows from HBM (2 * V * 4 bytes, 80 KB at V 10000);
//   2. sum exp(x - Mx), sum exp((x - Mx) / tau), sum exp((s - Ms) / tau) and the q-weighted sum
//      sum_v exp((s[v] - Ms) / tau) * ((s[v] - Ms) - (x[v] - Mx)) / tau: the workgroup has just streamed both rows, the pass hits L2.
// kd_row = tau^2 (A / Ss - (log Ss - log Sxt)): every term is relative to its row's maximum, so a constant added to s (raw logits
// or log-probs) never enters a sum and no two large quantities cancel; a teacher that is a bit copy of the student gives exactly 0.
// An entry whose exp((s - Ms) / tau) is 0 - s = -inf - is skipped: 0 * inf never appears; a student entry at -inf under positive
// teacher mass gives +inf; a NaN in either row makes its sums NaN.
// The backward is one in-place stream over the student's row that reads the teacher's row beside it.
// Both move 16 bytes per lane when the two rows share one misalignment and both leading dimensions are multiples of 4 (the train
// step: two workspaces' logits blocks, or the combiner's output); else element by element.  Columns V .. ld-1 are never touched.
// No atomics, every sum in a fixed order: two calls agree bit for bit.
#include <math.h>

#include "ssc_common.h"

namespace {

// f(x[v], s[v]) over the row pair: elements [0, head) and [head + 4 * n4, V) one by one, the n4 groups of four in between as
// 16-byte loads (head = V, n4 = 0: the scalar path throughout)
template <class F>
__device__ __forceinline__ void kd_scan(const float* __restrict__ x, const float* __restrict__ s, int V, int head, int n4, F f) {
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

struct KdFwdArgs {
  const float* logits; int ldl;
  const float* teacher; int ldt;
  const int64_t* targets;
  const float* w;
  int V, head, n4, rows;
  float eps_over_v, alpha, tau, inv_tau;
  float *lse, *nllw, *nllw0, *kdrows;   // kdrows: [lse(x/tau) | lse(s/tau) | w*kd_row], `rows` floats each
};

// TAU1: tau == 1 - lse(x / tau) is lse(x), formed once
template <bool TAU1>
__global__ __launch_bounds__(256) void kd_fwd_kernel(const KdFwdArgs a) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  const float wr = a.w[row];
  if (wr == 0.f) {  // padded target: no loss, and neither matrix's row may have been computed at all
    if (threadIdx.x == 0) {
      a.lse[row] = 0.f; a.nllw[row] = 0.f; a.nllw0[row] = 0.f;
      a.kdrows[row] = 0.f; a.kdrows[a.rows + row] = 0.f; a.kdrows[2 * a.rows + row] = 0.f;
    }
    return;
  }
  const float* x = a.logits + (size_t)row * a.ldl;
  const float* s = a.teacher + (size_t)row * a.ldt;
  const float r = x[a.targets[row]];
  float mx = -INFINITY, ms = -INFINITY, d = 0.f;
  kd_scan(x, s, a.V, a.head, a.n4, [&](float xv, float sv) {
    mx = fmaxf(mx, xv);
    ms = fmaxf(ms, sv);
    d += xv - r;
  });
  const float Mx = ssc_block_reduce(mx, sh, true), Ms = ssc_block_reduce(ms, sh, true);
  d = ssc_block_reduce(d, sh, false);
  const float it = a.inv_tau;
  float sx = 0.f, sxt = 0.f, ss = 0.f, acc = 0.f;
  kd_scan(x, s, a.V, a.head, a.n4, [&](float xv, float sv) {
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
    a.kdrows[row] = TAU1 ? l : Mx * it + lsxt;
    a.kdrows[a.rows + row] = TAU1 ? Ms + lss : Ms * it + lss;
    a.kdrows[2 * a.rows + row] = wr * kd;
  }
}

// loss[b], nll[b] and kd[b] (optional) from the [w*row], [w*row(0)] and [w*kd_row] blocks: ce_loss_kernel's walk (one lane per
// caption, eight of its T loads in flight, summed in step order) over three blocks
__global__ void kd_loss_kernel(const float* __restrict__ nllw, const float* __restrict__ nllw0, const float* __restrict__ kdw,
                               const float* __restrict__ nvalid, int T, int B, float* __restrict__ loss, float* __restrict__ nll,
                               float* __restrict__ kd) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f, s0 = 0.f, sk = 0.f;
  for (int t = 0; t < T; t += 8) {
    float x[8], x0[8], xk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t i = (size_t)min(t + u, T - 1) * B + b;
      x[u] = nllw[i];
      x0[u] = nllw0[i];
      xk[u] = kdw[i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (t + u < T) {
        s += x[u];
        s0 += x0[u];
        sk += xk[u];
      }
    }
  }
  const float n = nvalid[b];
  loss[b] = n * (s / (n + 1e-13f));
  if (nll) nll[b] = n * (s0 / (n + 1e-13f));
  if (kd) kd[b] = n * (sk / (n + 1e-13f));
}

struct KdBwdArgs {
  float* logits; int ldl;
  const float* teacher; int ldt;
  const int64_t* targets;
  const float *w, *nvalid, *lse, *kdrows, *gl;
  int B, V, head, n4, rows;
  float keep, eps_over_v, alpha, inv_tau, atau;   // keep = 1 - eps, atau = alpha * tau
};

// in place: x <- ((1 - alpha) (softmax(x) - keep [v == y] - eps/V) + alpha tau (p_tau - q)) * coef
template <bool TAU1>
__global__ __launch_bounds__(256) void kd_bwd_kernel(const KdBwdArgs a) {
  const int row = blockIdx.x;
  const int b = row % a.B;
  const float n = a.nvalid[b];
  const float coef = a.gl[b] * a.w[row] * (n / (n + 1e-13f));
  float* p = a.logits + (size_t)row * a.ldl;
  float4* p4 = reinterpret_cast<float4*>(p + a.head);
  const int head = a.head, n4 = a.n4, tail = head + (n4 << 2), ns = head + (a.V - tail);
  if (coef == 0.f) {  // never reads either row: a padded target's rows may hold anything
    for (int i = threadIdx.x; i < n4; i += 256) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = threadIdx.x; k < ns; k += 256) p[ssc_row_split_col(k, head, tail)] = 0.f;
    return;
  }
  const float* s = a.teacher + (size_t)row * a.ldt;
  const float4* s4 = reinterpret_cast<const float4*>(s + head);
  const float l = a.lse[row], lxt = a.kdrows[row], lst = a.kdrows[a.rows + row];
  const int tgt = (int)a.targets[row];
  const float hardw = 1.f - a.alpha, it = a.inv_tau;
  auto one = [&](float xv, float sv, int v) -> float {
    const float sm = expf(xv - l);
    const float pt = TAU1 ? sm : expf(xv * it - lxt);
    const float q = expf((TAU1 ? sv : sv * it) - lst);
    const float hard = sm - (v == tgt ? a.keep : 0.f) - a.eps_over_v;
    return (hardw * hard + a.atau * (pt - q)) * coef;
  };
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 x = p4[i];
    const float4 t = s4[i];
    const int v = head + (i << 2);
    x.x = one(x.x, t.x, v);
    x.y = one(x.y, t.y, v + 1);
    x.z = one(x.z, t.z, v + 2);
    x.w = one(x.w, t.w, v + 3);
    p4[i] = x;
  }
  for (int k = threadIdx.x; k < ns; k += 256) {
    const int v = ssc_row_split_col(k, head, tail);
    p[v] = one(p[v], s[v], v);
  }
}

// the [first, first + (rows-1) * ld + V) float ranges of the two matrices may not meet
inline bool kd_overlap(const float* logits, int ldl, const float* teacher, int ldt, size_t rows, int V) {
  const uintptr_t a0 = (uintptr_t)logits, a1 = a0 + ((rows - 1) * (size_t)ldl + (size_t)V) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)teacher, b1 = b0 + ((rows - 1) * (size_t)ldt + (size_t)V) * sizeof(float);
  return a0 < b1 && b0 < a1;
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

// kd_loss_kernel over the blocks [w*row], [w*row(0)] and a third [w*term] (T*B floats each): loss (B), nll (B, optional) and the
// term's per-caption sums (B, optional) - the third block is distillation's w*kd_row or unlikelihood training's w*ul_row
int ssc_ce_loss3(const float* nllw, const float* nllw0, const float* termw, const float* nvalid, int T, int B, float* loss, float* nll,
                 float* term, hipStream_t st) {
  SSC_LAUNCH(kd_loss_kernel, dim3(ssc_cdiv(B, 64)), dim3(64), 0, st, nllw, nllw0, termw, nvalid, T, B, loss, nll, term);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// ssc_ce_fwd_distill with the three blocks of `lse` given one by one (the train workspace keeps the third apart, see
// ssc_ce_fwd_smooth_blocks)
int ssc_ce_fwd_distill_blocks(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
                              int V, float eps, const ssc_distill* kd, float* lse, float* nllw, float* nllw0, float* loss, float* nll,
                              hipStream_t st) {
  if (!logits || !targets || !w || !nvalid || !lse || !nllw || !nllw0 || !loss || T <= 0 || B <= 0 || V <= 0 || ldl < V ||
      !ssc_ce_eps_ok(eps))
    return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0) return SSC_EALIGN;
  bool on;
  SSC_TRY(ssc_distill_check(kd, logits, ldl, (size_t)T * B, V, &on));
  if (!on) return ssc_ce_fwd_smooth_blocks(logits, ldl, targets, w, nvalid, T, B, V, eps, lse, nllw, nllw0, loss, nll, st);
  const int rows = T * B;
  KdFwdArgs a{};
  a.logits = logits; a.ldl = ldl; a.teacher = kd->teacher; a.ldt = kd->ldt; a.targets = targets; a.w = w;
  a.V = V; a.rows = rows;
  ssc_row_split(logits, ldl, kd->teacher, kd->ldt, V, &a.head, &a.n4);
  a.eps_over_v = (float)((double)eps / V); a.alpha = kd->alpha; a.tau = kd->temperature; a.inv_tau = 1.f / kd->temperature;
  a.lse = lse; a.nllw = nllw; a.nllw0 = nllw0; a.kdrows = kd->rows;
  if (kd->temperature == 1.f) SSC_LAUNCH(kd_fwd_kernel<true>, dim3(rows), dim3(256), 0, st, a);
  else SSC_LAUNCH(kd_fwd_kernel<false>, dim3(rows), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return ssc_ce_loss3(nllw, nllw0, kd->rows + 2 * (size_t)rows, nvalid, T, B, loss, nll, kd->kd, st);
}

// lse must hold 3*T*B floats: [lse | w*row | w*row(0)]
extern "C" int ssc_ce_fwd_distill(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T,
                                  int B, int V, float eps, const ssc_distill* kd, float* lse, float* loss, float* nll, void* stream) {
  if (!lse || T <= 0 || B <= 0) return SSC_EINVAL;
  const size_t rows = (size_t)T * B;
  return ssc_ce_fwd_distill_blocks(logits, ldl, targets, w, nvalid, T, B, V, eps, kd, lse, lse + rows, lse + 2 * rows, loss, nll,
                                   (hipStream_t)stream);
}

extern "C" int ssc_ce_bwd_distill(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid,
                                  const float* lse, const float* gl, int T, int B, int V, float eps, const ssc_distill* kd,
                                  void* stream) {
  if (!logits || !targets || !w || !nvalid || !lse || !gl || T <= 0 || B <= 0 || V <= 0 || ldl < V || !ssc_ce_eps_ok(eps))
    return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0) return SSC_EALIGN;
  bool on;
  SSC_TRY(ssc_distill_check(kd, logits, ldl, (size_t)T * B, V, &on));
  if (!on) return ssc_ce_bwd_smooth(logits, ldl, targets, w, nvalid, lse, gl, T, B, V, eps, stream);
  KdBwdArgs a{};
  a.logits = logits; a.ldl = ldl; a.teacher = kd->teacher; a.ldt = kd->ldt; a.targets = targets;
  a.w = w; a.nvalid = nvalid; a.lse = lse; a.kdrows = kd->rows; a.gl = gl;
  a.B = B; a.V = V; a.rows = T * B;
  ssc_row_split(logits, ldl, kd->teacher, kd->ldt, V, &a.head, &a.n4);
  a.keep = 1.f - eps; a.eps_over_v = (float)((double)eps / V); a.alpha = kd->alpha; a.inv_tau = 1.f / kd->temperature;
  a.atau = kd->alpha * kd->temperature;
  if (kd->temperature == 1.f) SSC_LAUNCH(kd_bwd_kernel<true>, dim3(T * B), dim3(256), 0, (hipStream_t)stream, a);
  else SSC_LAUNCH(kd_bwd_kernel<false>, dim3(T * B), dim3(256), 0, (hipStream_t)stream, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
