// Entropy-adaptive truncation for the word samplers (ssc_truncation, include/ssc.h): locally typical, min-p, eta and epsilon cuts
// of a row of RAW logits in front of the unchanged draw, so that the sampler draws from - and reports the log-prob under - the cut
// distribution.  ssc_truncate_rows is the stand-alone edit of one step; ssc_decode_sample_opts (sample.hip) issues it between each
// step's logit rules and its draw.
// One workgroup of SAMPLE_THREADS per row, two forms as for the samplers: the row staged in LDS once for V <= SAMPLE_LDS_MAX_V, every
// pass over global memory above that.  The passes of a live row; 1, 2 and 4 are the row passes of ssc_radix.h, which the Mirostat
// cut (mirostat.hip) shares:
//   1. row_stage_max: the maximum mx (and, STAGED, the copy into LDS);
//   2. row_tempered_sums, with a_v = (x_v - mx) / T over the finite entries: Z = sum exp(a_v), S = sum a_v exp(a_v), kinds 3 and 4
//      also the lowest index at which x_v == mx; then log Z, H = log Z - S / Z;
//   3. the kernel's own: the threshold of kinds 2 to 4, or, kind 1, the radix select of ssc_radix.h on the key of
//      d_v = |(log Z - a_v) - H|, ASCENDING (the key is complemented), weighted by the 2^-40 fixed-point masses of top-p; ties at the
//      cut by a second select on the index (lower index first);
//   4. row_write_kept under the kind's predicate: a dropped entry becomes -inf, a kept one is stored back with the bits it had; the
//      kept entries are counted.
// Kinds 2 to 4 compare a_v with one threshold and need no select.  Every reduction runs in a fixed order (wave butterflies, then the
// waves in index order) and the histograms of the select are integer: two calls on equal inputs are bit-identical.  An entry of
// -inf (a ban of the logit rules) stays dropped, weighs nothing and never meets a product; a row without a finite entry is left
// as it is; a row whose last token is END is neither read nor written; columns V .. ld - 1 are never touched.  16-byte accesses
// where the row is 16-byte aligned with V % 4 == 0, scalar ones otherwise: per element the same operations either way.
#include <math.h>

#include "ssc_radix.h"

namespace {

struct TruncArgs {
  float* logits; size_t ld; int V;
  int kind; float value, temperature;
  const int64_t* last_pred; int end_index;
  float* entropy; int* kept;
};

// the typical order's key of a finite entry: descending key <=> ascending d = |s_v - H|, s_v = log Z - a_v (d >= 0: its bits order it)
__device__ __forceinline__ uint32_t typical_key(float x, float mx, float T, float logz, float H) {
  const float a = (x - mx) / T;
  const float d = fabsf((logz - a) - H);
  return ~sample_key(d);
}

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void truncate_rows_kernel(TruncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  const int r = blockIdx.x;
  const int V = a.V;
  const auto leave = [&] {   // the statistics of a row that is not edited
    if (threadIdx.x == 0) {
      if (a.entropy) a.entropy[r] = 0.f;
      if (a.kept) a.kept[r] = 0;
    }
  };
  if (a.last_pred && a.last_pred[r] == a.end_index) return leave();   // workgroup-uniform: an ended row is neither read nor written
  float* g = a.logits + (size_t)r * a.ld;
  const RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
  const float T = a.temperature;
  // ---- 1. stage the row (once from HBM) and its maximum --------------------------------------------------------------------
  const float mx = row_stage_max(row, srow, sh);
  if (!(mx > -INFINITY)) return leave();   // no finite entry (workgroup-uniform): the row is left as it is
  // ---- 2. the tempered normaliser and the entropy over the finite entries; kinds 3 and 4: the lowest-index maximum -------------
  const RowSums sums = row_tempered_sums<STAGED, true>(row, mx, T, a.kind >= 3, sh);
  const float z = sums.z, logz = logf(z), H = logz - sums.s1 / z;
  const int first = sums.first;
  // ---- 3. the cut ------------------------------------------------------------------------------------------------------------
  // kinds 2 to 4: kept <=> a_v >= thr_a (or v == first); kind 1: kept <=> key > cut_key, or key == cut_key and v <= cut_idx
  float thr_a = -INFINITY;
  uint32_t cut_key = 0;
  int cut_idx = 0x7fffffff;   // (defaults: every finite entry kept)
  if (a.kind == 2) {
    thr_a = logf(a.value);
  } else if (a.kind == 3) {
    const float le = logf(a.value);
    thr_a = fminf(le, 0.5f * le - H) + logz;   // log q_v = a_v - log Z >= log eta
  } else if (a.kind == 4) {
    thr_a = logf(a.value) + logz;
  } else if (a.value < 1.f) {   // (tau = 1 keeps every finite entry, as top-p does at p = 1)
    const float invz = 1.f / z;
    const unsigned long long thr = (unsigned long long)llrint((double)a.value * SAMPLE_MASS_ONE);
    radix_descent<STAGED, true>(row, [&](int, float x, uint32_t& key, unsigned long long& w) {
      if (!(x > -INFINITY)) return false;
      key = typical_key(x, mx, T, logz, H);
      w = (unsigned long long)llrintf(expf((x - mx) / T) * invz * 1099511627776.0f);
      return true; }, thr, sh);
    if (sh.sel_found != 0) {   // (not found: the fixed-point masses stay below tau - every finite entry is kept)
      cut_key = sh.sel_key;
      const unsigned long long ahead = sh.sel_ahead, wt = sh.sel_w;
      const uint32_t ct = sh.sel_cnt;
      // entries tied at the cut are taken to share one weight (sample_cut's rule); the n-th of them, lowest index first, is the cut
      const unsigned long long each = wt / ct;
      unsigned long long n = (each == 0 || thr <= ahead) ? 1 : (thr - ahead + each - 1) / each;
      n = n < 1 ? 1 : (n > ct ? ct : n);
      __syncthreads();
      if (n < ct) {
        const uint32_t ck = cut_key;
        radix_descent<STAGED, false>(row, [&](int v, float x, uint32_t& key, unsigned long long& w) {
          key = ~(uint32_t)v; w = 1; return x > -INFINITY && typical_key(x, mx, T, logz, H) == ck; }, n, sh);
        cut_idx = (int)~sh.sel_key;
      }
      __syncthreads();
    }
  }
  // ---- 4. the write pass -------------------------------------------------------------------------------------------------------
  const int kind = a.kind;
  int nkept = row_write_kept(row, g, [&](int v, float x) -> bool {
    if (kind == 1) {
      const uint32_t key = typical_key(x, mx, T, logz, H);
      return key > cut_key || (key == cut_key && v <= cut_idx);
    }
    return ((x - mx) / T >= thr_a) | (v == first);   // (first stays 0x7fffffff for kind 2)
  });
  if (a.kept) {   // (a kernel argument: workgroup-uniform)
    nkept = block_sum_int(nkept, sh);
    if (threadIdx.x == 0) a.kept[r] = nkept;
  }
  if (a.entropy && threadIdx.x == 0) a.entropy[r] = H;
}

}  // namespace

int ssc_truncation_check(const ssc_truncation* tr, float temperature, bool* active) {
  *active = false;
  if (!tr || tr->kind < 0 || tr->kind > 4) return SSC_EINVAL;
  if (!(temperature > 0.f) || !ssc_finite_f(temperature)) return SSC_EINVAL;
  if (tr->kind == 1 || tr->kind == 2) {
    if (!(tr->value > 0.f && tr->value <= 1.f)) return SSC_EINVAL;   // (false for NaN)
  } else if (tr->kind != 0) {
    if (!(tr->value > 0.f && tr->value < 1.f)) return SSC_EINVAL;
  }
  if (((uintptr_t)tr->entropy & 3u) != 0 || ((uintptr_t)tr->kept & 3u) != 0) return SSC_EALIGN;
  *active = tr->kind != 0;
  return SSC_OK;
}

int ssc_truncation_launch(float* logits, int ld, int rows, int V, const ssc_truncation* tr, float temperature, float* entropy, int* kept,
                          const int64_t* last_pred, int end_index, hipStream_t st) {
  TruncArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V;
  a.kind = tr->kind; a.value = tr->value; a.temperature = temperature;
  a.last_pred = last_pred; a.end_index = end_index;
  a.entropy = entropy; a.kept = kept;
  return sample_row_launch(truncate_rows_kernel<true>, truncate_rows_kernel<false>, V, rows, st, a);
}

extern "C" int ssc_truncate_rows(float* logits, int ld, int rows, int V, const ssc_truncation* tr, float temperature,
                                 const int64_t* last_pred, int end_index, void* stream) {
  if (!logits || !tr || rows < 0 || V < 1 || ld < V) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  bool active;
  const int rc = ssc_truncation_check(tr, temperature, &active);
  if (rc == SSC_EINVAL) return rc;
  if (((uintptr_t)logits & 3u) != 0 || ((uintptr_t)last_pred & 3u) != 0) return SSC_EALIGN;
  SSC_TRY(rc);
  if (!active || rows == 0) return SSC_OK;
  return ssc_truncation_launch(logits, ld, rows, V, tr, temperature, tr->entropy, tr->kept, last_pred, end_index, (hipStream_t)stream);
}
