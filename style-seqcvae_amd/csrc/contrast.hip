// Contrastive decoding for the word samplers (ssc_contrast_rows, include/ssc.h): the raw logits of an EXPERT row and of an AMATEUR
// row - the same words decoded from a degraded image, a neutral latent or a weaker checkpoint - become, in place over the expert's,
//   y[v] = lp_e[v] + alpha * (lp_e[v] - lp_a[v])   where beta == 0 or lp_e[v] >= log(beta) + max_u lp_e[u],   -inf elsewhere
// (Li et al. 2023), a row of raw logits for the logit rules, the truncation and the unchanged draw behind it.  ssc_contrast_rows is
// the stand-alone edit of one step; ssc_decode_sample_opts (sample.hip) issues it between each step's two decode steps and its
// logit rules.
// One workgroup of 256 per row, as log_softmax_kernel and ssc_ensemble_combine_rows.  The passes of a live row:
//   1. the expert's log-sum-exp by beam_row_lse (beam_common.h): the arithmetic and the thread ownership of log_softmax_kernel, so
//      x_e - lse_e is bit-equal to ssc_log_softmax; its first reduction also leaves the row's maximum, m = max x_e - lse_e.  This is
//      the one read of the row from HBM; the second pass of the sum and pass 3 find it in L2;
//   2. the same for the amateur's row (not with a NULL amateur);
//   3. the edit: thread t owns the entries 4j .. 4j + 3, j = t, t + 256, ... of both rows - one 16-byte load per row and one 16-byte
//      store where both rows are 16-byte aligned with V % 4 == 0, scalar accesses otherwise, per entry the same operations and per
//      thread the same entries in the same order either way.  One subtraction, one multiplication, one addition per entry (the
//      library is built with -ffp-contract=off: no fma); the thread's share of KL(p_e || p_a) = sum p_e (lp_e - lp_a) and of the
//      kept count are summed in that order, then over the workgroup in a fixed order (wave butterflies, the waves in index order).
// No row is staged in LDS: two rows of V = 10000 are 80 KB and leave one workgroup of four waves per CU, which measured slower than
// re-reading through L2 ("contrastive decoding"); LDS holds the reductions' words only, so there is no bound on V.
// No atomics: two calls on equal inputs are bit-identical.  A row whose last token is END is neither read nor written; columns
// V .. ld - 1 of either row are never touched; the amateur's row is never written; no index depends on a value, so NaN or +-inf in
// a row (the caller's error) stays inside it.
#include <math.h>

#include "beam_common.h"

namespace {

struct ContrastArgs {
  float* logits; size_t ld;          // the expert's rows, edited in place
  const float* amateur; size_t lda;  // the amateur's rows, or null
  int V;
  float alpha, logb;   // logb: log(beta) rounded to fp32 on the host
  int cut;             // beta != 0
  const int64_t* last_pred; int end_index;
  int* kept; float* divergence;
};

// block-wide integer sum in a fixed order; shi: 4 ints of LDS
__device__ __forceinline__ int contrast_sum_int(int v, int* shi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = v;
  __syncthreads();
  return shi[0] + shi[1] + shi[2] + shi[3];
}

// the entries 4j .. 4j + 3 of a row: one 16-byte load, or scalar loads of those below V (the others read nothing and are 0)
__device__ __forceinline__ void contrast_get4(const float* row, int j, int V, bool vec, float (&x)[4]) {
  if (vec) {
    const float4 q = reinterpret_cast<const float4*>(row)[j];
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = 4 * j + c < V ? row[4 * j + c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void contrast_rows_kernel(const ContrastArgs a) {
  __shared__ float shr[16];
  __shared__ int shi[4];
  const int r = blockIdx.x, t = threadIdx.x, V = a.V;
  if (a.last_pred && a.last_pred[r] == (int64_t)a.end_index) {   // workgroup-uniform: an ended row is neither read nor written
    if (t == 0) {
      if (a.kept) a.kept[r] = 0;
      if (a.divergence) a.divergence[r] = 0.f;
    }
    return;
  }
  float* ge = a.logits + (size_t)r * a.ld;
  const float* ga = a.amateur ? a.amateur + (size_t)r * a.lda : nullptr;
  const bool vec = (V & 3) == 0 && ssc_aligned16_dev(ge) && ssc_aligned16_dev(ga);   // (a null amateur counts as aligned)
  // ---- 1, 2. the two log-sum-exps; the expert's maximum comes out of its first reduction -------------------------------------------
  float none[1];
  float mx = 0.f;
  const float lse_e = beam_row_lse<true, false>(ge, V, none, [&](float v, bool is_max) {
    const float red = ssc_block_reduce(v, shr, is_max);
    if (is_max) mx = red;
    return red; });
  const float lse_a = ga ? beam_row_lse<true, false>(ga, V, none, beam_reduce2(shr)) : 0.f;
  // (the barriers of the last reduction: every thread's reads of the sum passes are done before any entry is overwritten)
  const float thr = a.logb + (mx - lse_e);   // lp_e >= log(beta) + m; a maximal entry has lp_e == m >= thr as log(beta) <= 0
  // ---- 3. the edit -----------------------------------------------------------------------------------------------------------------
  const int nj = (V + 3) >> 2;
  int nkept = 0;
  float kl = 0.f;
  for (int j = t; j < nj; j += 256) {
    float xe[4], xa[4] = {0.f, 0.f, 0.f, 0.f}, y[4];
    contrast_get4(ge, j, V, vec, xe);
    if (ga) contrast_get4(ga, j, V, vec, xa);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool in = 4 * j + c < V;
      const float le = xe[c] - lse_e;
      float yy = le;
      if (ga) {
        const float d = le - (xa[c] - lse_a);
        if (in) kl += expf(le) * d;
        if (a.alpha != 0.f) {
          const float s = a.alpha * d;
          yy = le + s;
        }
      }
      const bool keep = in && (!a.cut || le >= thr);
      y[c] = keep ? yy : -INFINITY;
      nkept += keep ? 1 : 0;
    }
    if (vec) {
      reinterpret_cast<float4*>(ge)[j] = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * j + c < V) ge[4 * j + c] = y[c];
    }
  }
  if (a.kept) {   // (kernel arguments: workgroup-uniform)
    nkept = contrast_sum_int(nkept, shi);
    if (t == 0) a.kept[r] = nkept;
  }
  if (a.divergence) {
    kl = ssc_block_reduce(kl, shr, false);
    if (t == 0) a.divergence[r] = ga ? kl : 0.f;
  }
}

}  // namespace

int ssc_contrast_check(float alpha, float beta, const int* kept, const float* divergence, bool* active) {
  *active = false;
  if (!(alpha >= 0.f) || !ssc_finite_f(alpha)) return SSC_EINVAL;   // (false for NaN)
  if (!(beta >= 0.f && beta < 1.f)) return SSC_EINVAL;
  if (((uintptr_t)kept & 3u) != 0 || ((uintptr_t)divergence & 3u) != 0) return SSC_EALIGN;
  *active = alpha != 0.f || beta != 0.f;
  return SSC_OK;
}

int ssc_contrast_launch(float* logits, int ld, const float* amateur, int lda, int rows, int V, float alpha, float beta, int* kept,
                        float* divergence, const int64_t* last_pred, int end_index, hipStream_t st) {
  ContrastArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.amateur = amateur; a.lda = (size_t)lda; a.V = V;
  a.alpha = alpha; a.cut = beta != 0.f ? 1 : 0; a.logb = a.cut ? (float)log((double)beta) : 0.f;
  a.last_pred = last_pred; a.end_index = end_index;
  a.kept = kept; a.divergence = divergence;
  SSC_LAUNCH(contrast_rows_kernel, dim3(rows), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_contrast_rows(float* logits, int ld, const float* amateur, int ld_amateur, int rows, int V, float alpha, float beta,
                                 const int64_t* last_pred, int end_index, int* kept, float* divergence, void* stream) {
  if (!logits || rows < 0 || V < 1 || ld < V || (amateur && ld_amateur < V)) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  bool active;
  const int rc = ssc_contrast_check(alpha, beta, kept, divergence, &active);
  if (rc == SSC_EINVAL) return rc;
  if (!amateur && alpha != 0.f) return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0 || ((uintptr_t)amateur & 3u) != 0 || ((uintptr_t)last_pred & 3u) != 0) return SSC_EALIGN;
  SSC_TRY(rc);
  if (!active || rows == 0) return SSC_OK;
  return ssc_contrast_launch(logits, ld, amateur, ld_amateur, rows, V, alpha, beta, kept, divergence, last_pred, end_index,
                             (hipStream_t)stream);
}
