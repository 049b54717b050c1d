// Mirostat 2.0 for the word samplers (ssc_mirostat, include/ssc.h; Basu et al., ICLR 2021, algorithm 2): a surprise target tau held by
// feedback.  The one edit of the sampled decode that carries a value per row from step to step: the running threshold mu.
//   ssc_mirostat_rows    the CUT of one step: of a row of RAW logits, behind the contrast, the logit rules and the truncation, every
//                        entry whose surprise -log q_v under the tempered distribution exceeds the row's mu becomes -inf (the
//                        lowest-index maximum always stays), in front of the unchanged draw;
//   ssc_mirostat_update  the UPDATE behind the draw: mu' = mu - eta (s - tau), s the drawn word's surprise under the tempered
//                        distribution BEFORE the cut - the authors' reference implementation's choice, not the renormalised one.
// ssc_decode_sample_mirostat (sample.hip) issues the two around each step's draw; the draw itself does not know of them.
// The cut is the truncation's kinds 2 to 4 (truncation.hip) with a threshold per row, built from the same row passes of ssc_radix.h:
// one workgroup of SAMPLE_THREADS per row, the row staged in LDS once for V <= SAMPLE_LDS_MAX_V, every pass over global memory above
// that.  The passes of a live row:
//   1. row_stage_max: the maximum mx (and, STAGED, the copy into LDS);
//   2. row_tempered_sums, with a_v = (x_v - mx) / T over the finite entries: Z = sum exp(a_v) (no entropy sum), and the lowest index
//      at which x_v == mx; then log Z;
//   3. row_write_kept: kept <=> a_v >= log Z - mu or v == first; a dropped entry becomes -inf, a kept one is stored back with the bits
//      it had; the kept entries are counted.  mx and log Z go to `norm` for the update, which then reads ONE word of the row.
// What is the kernel's own: the threshold, the `norm` store, and which statistics a row that is not edited zeroes (`kept` alone).
// Every reduction runs in a fixed order (wave butterflies, then the waves in index order), no atomics: two calls on equal inputs are
// bit-identical.  An entry of -inf stays dropped and weighs nothing; a row without a finite entry is left as it is; a row whose last
// token is END is neither read nor written; columns V .. ld - 1 are never touched.  16-byte accesses where the row is 16-byte aligned
// with V % 4 == 0, scalar ones otherwise: per element the same operations either way.
#include <math.h>

#include "ssc_radix.h"

namespace {

struct MirostatArgs {
  float* logits; size_t ld; int V; int rows;
  float temperature;
  const float* mu;
  const int64_t* last_pred; int end_index;
  int* kept; float* norm;
};

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void mirostat_rows_kernel(MirostatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  const int r = blockIdx.x;
  const int V = a.V;
  if (a.last_pred && a.last_pred[r] == a.end_index) {   // workgroup-uniform: an ended row is neither read nor written
    if (threadIdx.x == 0 && a.kept) a.kept[r] = 0;
    return;
  }
  float* g = a.logits + (size_t)r * a.ld;
  const RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
  const float T = a.temperature;
  // ---- 1. stage the row (once from HBM) and its maximum --------------------------------------------------------------------
  const float mx = row_stage_max(row, srow, sh);
  if (!(mx > -INFINITY)) {  // no finite entry (workgroup-uniform): the row is left as it is, and so is its norm
    if (threadIdx.x == 0 && a.kept) a.kept[r] = 0;
    return;
  }
  // ---- 2. the tempered normaliser over the finite entries and the lowest-index maximum ---------------------------------------
  const RowSums sums = row_tempered_sums<STAGED, false>(row, mx, T, true, sh);
  const float logz = logf(sums.z);
  const int first = sums.first;
  // ---- 3. the cut: surprise log Z - a_v <= mu, or the top word ----------------------------------------------------------------
  const float thr = logz - a.mu[r];
  int nkept = row_write_kept(row, g, [&](int v, float x) { return ((x - mx) / T >= thr) | (v == first); });
  if (a.kept) {   // (a kernel argument: workgroup-uniform)
    nkept = block_sum_int(nkept, sh);
    if (threadIdx.x == 0) a.kept[r] = nkept;
  }
  if (threadIdx.x == 0) {
    a.norm[r] = mx;
    a.norm[(size_t)a.rows + r] = logz;
  }
}

struct MirostatUpdateArgs {
  const float* logits; size_t ld; int V; int rows;
  float temperature, tau, eta;
  const float* norm;
  const int64_t* pred; const int64_t* last_pred; int end_index;
  const float* mu_in; float* mu_out; float* surprise;
};

// one thread per row: the drawn word's surprise from the cut's mx and log Z and ONE word of the edited row (a drawn word is a kept
// word: it still holds its bits)
__global__ __launch_bounds__(256) void mirostat_update_kernel(MirostatUpdateArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.rows) return;
  const float mu = a.mu_in[r];
  float s = 0.f, mu2 = mu;
  if (!(a.last_pred && a.last_pred[r] == a.end_index)) {
    const int64_t w = a.pred[r];
    if (w >= 0 && w < (int64_t)a.V) {   // (a token outside the row: the row passes through)
      const float xw = a.logits[(size_t)r * a.ld + (size_t)w];
      if (xw > -INFINITY) {   // (false for a row without a finite entry, whose norm the cut left alone: it is not read)
        const float mx = a.norm[r], logz = a.norm[(size_t)a.rows + r];
        const float aw = (xw - mx) / a.temperature;
        s = logz - aw;
        const float e = s - a.tau;
        const float step = a.eta * e;
        mu2 = mu - step;
      }
    }
  }
  a.mu_out[r] = mu2;
  if (a.surprise) a.surprise[r] = s;
}

__global__ __launch_bounds__(256) void mirostat_fill_kernel(float* __restrict__ mu, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mu[i] = v;
}

}  // namespace

int ssc_mirostat_check(const ssc_mirostat* m, float temperature, bool* active) {
  *active = false;
  if (!m) return SSC_OK;
  if (!(m->tau >= 0.f) || !ssc_finite_f(m->tau)) return SSC_EINVAL;   // (false for NaN)
  if (m->tau == 0.f) return SSC_OK;                                // off: nothing else is read
  if (!(m->eta >= 0.f) || !ssc_finite_f(m->eta) || !ssc_finite_f(m->mu0)) return SSC_EINVAL;
  if (!(temperature > 0.f) || !ssc_finite_f(temperature)) return SSC_EINVAL;
  if (!m->mu) return SSC_EINVAL;
  if (((uintptr_t)m->mu & 3u) != 0 || ((uintptr_t)m->surprise & 3u) != 0 || ((uintptr_t)m->kept & 3u) != 0) return SSC_EALIGN;
  *active = true;
  return SSC_OK;
}

int ssc_mirostat_fill(float* mu, int n, float mu0, hipStream_t st) {
  if (n <= 0) return SSC_OK;
  SSC_LAUNCH(mirostat_fill_kernel, dim3(ssc_cdiv(n, 256)), dim3(256), 0, st, mu, n, mu0);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

int ssc_mirostat_rows_launch(float* logits, int ld, int rows, int V, float temperature, const float* mu, const int64_t* last_pred,
                             int end_index, int* kept, float* norm, hipStream_t st) {
  MirostatArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V; a.rows = rows;
  a.temperature = temperature; a.mu = mu;
  a.last_pred = last_pred; a.end_index = end_index;
  a.kept = kept; a.norm = norm;
  return sample_row_launch(mirostat_rows_kernel<true>, mirostat_rows_kernel<false>, V, rows, st, a);
}

int ssc_mirostat_update_launch(const float* logits, int ld, int rows, int V, float temperature, float tau, float eta, const float* norm,
                               const int64_t* pred, const int64_t* last_pred, int end_index, const float* mu_in, float* mu_out,
                               float* surprise, hipStream_t st) {
  MirostatUpdateArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V; a.rows = rows;
  a.temperature = temperature; a.tau = tau; a.eta = eta;
  a.norm = norm; a.pred = pred; a.last_pred = last_pred; a.end_index = end_index;
  a.mu_in = mu_in; a.mu_out = mu_out; a.surprise = surprise;
  SSC_LAUNCH(mirostat_update_kernel, dim3(ssc_cdiv(rows, 256)), dim3(256), 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_mirostat_rows(float* logits, int ld, int rows, int V, float temperature, const float* mu_in, const int64_t* last_pred,
                                 int end_index, int* kept, float* norm, void* stream) {
  if (!logits || !mu_in || !norm || rows < 0 || V < 1 || ld < V) return SSC_EINVAL;
  if (!(temperature > 0.f) || !ssc_finite_f(temperature)) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0 || ((uintptr_t)mu_in & 3u) != 0 || ((uintptr_t)last_pred & 3u) != 0 || ((uintptr_t)kept & 3u) != 0 ||
      ((uintptr_t)norm & 3u) != 0)
    return SSC_EALIGN;
  if (rows == 0) return SSC_OK;
  return ssc_mirostat_rows_launch(logits, ld, rows, V, temperature, mu_in, last_pred, end_index, kept, norm, (hipStream_t)stream);
}

extern "C" int ssc_mirostat_update(const float* logits, int ld, int rows, int V, float temperature, float tau, float eta,
                                   const float* norm, const int64_t* pred, const int64_t* last_pred, int end_index, const float* mu_in,
                                   float* mu_out, float* surprise, void* stream) {
  if (!logits || !norm || !pred || !mu_in || !mu_out || rows < 0 || V < 1 || ld < V) return SSC_EINVAL;
  if (!(temperature > 0.f) || !ssc_finite_f(temperature)) return SSC_EINVAL;
  if (!(tau >= 0.f) || !ssc_finite_f(tau) || !(eta >= 0.f) || !ssc_finite_f(eta)) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0 || ((uintptr_t)norm & 3u) != 0 || ((uintptr_t)pred & 3u) != 0 || ((uintptr_t)last_pred & 3u) != 0 ||
      ((uintptr_t)mu_in & 3u) != 0 || ((uintptr_t)mu_out & 3u) != 0 || ((uintptr_t)surprise & 3u) != 0)
    return SSC_EALIGN;
  if (rows == 0) return SSC_OK;
  return ssc_mirostat_update_launch(logits, ld, rows, V, temperature, tau, eta, norm, pred, last_pred, end_index, mu_in, mu_out, surprise,
                                    (hipStream_t)stream);
}
