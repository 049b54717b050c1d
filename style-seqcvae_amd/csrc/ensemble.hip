// Ensemble decoding: M (rows, V) matrices of raw logits -> one (rows, V) matrix of log-probs (ssc_ensemble_combine_rows,
// include/ssc.h), the step between the members' decode steps and the selection of ssc_decode_search_ensemble (search.hip).
// One workgroup of 256 per row, as log_softmax_kernel and the row selections:
//   1. per member its log-sum-exp with beam_row_lse (beam_common.h) - the arithmetic and the thread ownership of
//      log_softmax_kernel, so logits_m - lse_m is bit-equal to ssc_log_softmax.  This is the one read of the members' rows from
//      HBM (M * V * 4 bytes, 40 KB per member at V 10000); the second pass of the sum finds the row in L2.
//   2. the combine pass reads the M rows once more (L2 hits: the workgroup has just streamed them) with 16-byte loads, M
//      values per token in registers, and writes the row with 16-byte stores.
//   mode 1 normalises the weighted sum it has just written: beam_row_lse once more, over the out row (L2), and one more pass
//   that subtracts - the log-softmax of the sums, in the arithmetic of ssc_log_softmax whatever the rows' alignment.
// No row is staged in LDS (M rows of 40 KB would leave one workgroup per CU); LDS holds the reductions' 16 floats.  No atomics;
// every sum has a fixed order, so two calls agree bit for bit.
#include <math.h>

#include "beam_common.h"

namespace {

struct EnsArgs {
  const float* logits[SSC_ENSEMBLE_MAX];
  float logw[SSC_ENSEMBLE_MAX];
  float w[SSC_ENSEMBLE_MAX];   // exp(logw), mode 1
  int M, ld, V, ldo, end_index, vec;
  const int64_t* last_pred;
  const float* row_lp;
  float* out;
};

// one token: the members' logits x[m] (m < M) -> mode 0: the token's log-prob; mode 1: the weighted sum of the members' log-probs
template <int MODE>
__device__ __forceinline__ float ens_token(const float (&x)[SSC_ENSEMBLE_MAX], const EnsArgs& a, const float (&lse)[SSC_ENSEMBLE_MAX]) {
  if (MODE == 0) {
    float y[SSC_ENSEMBLE_MAX];
    float mx = -INFINITY, ysum = 0.f;
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m)
      if (m < a.M) {
        y[m] = (x[m] - lse[m]) + a.logw[m];
        mx = fmaxf(mx, y[m]);
        ysum += y[m];
      }
    // no member gives the token any mass: -inf; or every y is NaN (fmaxf drops them) - a NaN in a member's row makes its
    // log-sum-exp NaN, and the row comes out NaN as ssc_log_softmax's does
    if (mx == -INFINITY) return ysum;
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m)
      if (m < a.M) s += expf(y[m] - mx);
    return mx + logf(s);
  } else {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m)
      if (m < a.M) s += a.w[m] * (x[m] - lse[m]);
    return s;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void ens_combine_kernel(const EnsArgs a) {
  __shared__ float shr[16];
  const int g = blockIdx.x, t = threadIdx.x, V = a.V;
  // workgroup-uniform: a skipped row is neither read nor written
  if (a.last_pred && a.last_pred[g] == (int64_t)a.end_index) return;
  if (a.row_lp && a.row_lp[g] <= -1e19f) return;
  float none[1];
  float lse[SSC_ENSEMBLE_MAX];   // (beam_row_lse leaves the row's value with every thread)
#pragma unroll
  for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m)
    lse[m] = m < a.M ? beam_row_lse<true, false>(a.logits[m] + (size_t)g * a.ld, V, none, beam_reduce2(shr)) : 0.f;
  float* o = a.out + (size_t)g * a.ldo;
  const int n4 = a.vec ? V >> 2 : 0;
  for (int i = t; i < n4; i += 256) {
    float4 x4[SSC_ENSEMBLE_MAX];
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m)
      if (m < a.M) x4[m] = reinterpret_cast<const float4*>(a.logits[m] + (size_t)g * a.ld)[i];
    float x[SSC_ENSEMBLE_MAX];
    float4 r;
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m) x[m] = m < a.M ? x4[m].x : 0.f;
    r.x = ens_token<MODE>(x, a, lse);
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m) x[m] = m < a.M ? x4[m].y : 0.f;
    r.y = ens_token<MODE>(x, a, lse);
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m) x[m] = m < a.M ? x4[m].z : 0.f;
    r.z = ens_token<MODE>(x, a, lse);
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m) x[m] = m < a.M ? x4[m].w : 0.f;
    r.w = ens_token<MODE>(x, a, lse);
    reinterpret_cast<float4*>(o)[i] = r;
  }
  for (int v = (n4 << 2) + t; v < V; v += 256) {
    float x[SSC_ENSEMBLE_MAX];
#pragma unroll
    for (int m = 0; m < SSC_ENSEMBLE_MAX; ++m) x[m] = m < a.M ? a.logits[m][(size_t)g * a.ld + v] : 0.f;
    const float r = ens_token<MODE>(x, a, lse);
    o[v] = r;
  }
  if (MODE == 1) {   // out = s - logsumexp_v s: the log-softmax of the row just written, whatever the rows' alignment
    __syncthreads();   // (the workgroup's stores of s, before other threads of it read them)
    const float l = beam_row_lse<true, false>(o, V, none, beam_reduce2(shr));   // (its reductions' barriers: every read of s is done)
    for (int i = t; i < n4; i += 256) {
      float4 r = reinterpret_cast<const float4*>(o)[i];
      r.x -= l; r.y -= l; r.z -= l; r.w -= l;
      reinterpret_cast<float4*>(o)[i] = r;
    }
    for (int v = (n4 << 2) + t; v < V; v += 256) o[v] -= l;
  }
}

}  // namespace

extern "C" int ssc_ensemble_combine_rows(const ssc_ensemble_rows_desc* e, int rows, int V, const int64_t* last_pred,
                                         const float* row_lp, int end_index, float* out, int ldo, void* stream) {
  if (!e || !out || !e->logits || !e->logw || e->M < 1 || e->M > SSC_ENSEMBLE_MAX) return SSC_EINVAL;
  if (rows < 0 || V < 1 || e->ld < V || ldo < V || (e->mode != 0 && e->mode != 1)) return SSC_EINVAL;
  EnsArgs a{};
  bool vec = e->ld % 4 == 0 && ldo % 4 == 0 && ssc_aligned16(out);
  for (int m = 0; m < e->M; ++m) {
    if (!e->logits[m] || !isfinite(e->logw[m])) return SSC_EINVAL;
    a.logits[m] = e->logits[m];
    a.logw[m] = e->logw[m];
    a.w[m] = expf(e->logw[m]);
    vec = vec && ssc_aligned16(e->logits[m]);
  }
  if (rows == 0) return SSC_OK;
  a.M = e->M; a.ld = e->ld; a.V = V; a.ldo = ldo; a.end_index = end_index; a.vec = vec ? 1 : 0;
  a.last_pred = last_pred; a.row_lp = row_lp; a.out = out;
  hipStream_t st = (hipStream_t)stream;
  if (e->mode == 0) SSC_LAUNCH(ens_combine_kernel<0>, dim3(rows), dim3(256), 0, st, a);
  else SSC_LAUNCH(ens_combine_kernel<1>, dim3(rows), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
