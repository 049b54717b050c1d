// Logit rules for the word samplers (ssc_logit_rules, include/ssc.h): a word bias, repetition / presence / frequency penalties and
// bans (blocked n-grams, a minimum length, suppressed tokens), applied to the RAW logits of a row in front of the draw, so that the
// sampler draws from - and reports the log-prob under - the edited distribution.  ssc_logit_rules_rows is the stand-alone edit of
// one step; ssc_decode_sample_opts (sample.hip) issues it between each step's decode step and its draw.
// Two forms, chosen on the host:
//   (A) with a bias, one workgroup of 256 per row streams the row once, x += bias: 16 bytes per lane where both rows share one
//       misalignment and both leading dimensions are multiples of 4 (scalar head / float4 bulk / scalar tail, as cross_entropy.hip's
//       ce_pair_scan), scalar accesses throughout otherwise.  One fp32 add per element either way.  A workgroup barrier, then the sparse
//       edits by the first wave.
//   (B) without a bias no thread walks the row: one wave per row, LOGIT_RULES_ROWS rows per workgroup, at most t + n_suppress + 1
//       elements touched per row.
// The sparse edits: the row's history (at most 64 ids) goes into LDS.  Lane j owns position j.  Penalties: the lane counts its
// token's occurrences itself and edits x[c] only where position j is the FIRST occurrence of c - distinct lanes write distinct
// addresses.  A barrier.  Bans: lane q < n_suppress stores -inf at suppress[q], the last lane at END below the minimum length, lane
// j at the token that followed an earlier occurrence of the history's last n - 1 tokens; lanes that meet at one address store the
// same value.  No atomics: two calls on equal inputs are bit-identical.  A row whose last token is END is neither read nor written.
#include <math.h>

#include "ssc_common.h"

namespace {

constexpr int LOGIT_RULES_ROWS = 4;   // form (B): rows (waves) per workgroup

struct LogitRulesArgs {
  float* logits; size_t ld; int rows, V;
  const int64_t* hist; size_t ld_hist; int t;
  int end_index;
  int ngram, min_length, n_suppress;
  int suppress[SSC_RULES_MAX_SUPPRESS];
  float theta, presence, frequency;
  int pen;   // any penalty on
  const float* bias; size_t ld_bias; int n_bias;
  const int* bias_row;
  int head, n4;   // how form (A) walks a row pair (logit_rules_split)
};

// whether row r takes part at all: inside the launch and not ended
__device__ __forceinline__ bool logit_rules_live(const LogitRulesArgs& a, long r) {
  if (r >= a.rows) return false;
  return !(a.t >= 1 && a.hist[(size_t)(a.t - 1) * a.ld_hist + (size_t)r] == (int64_t)a.end_index);
}

// The sparse edits of one row by the lanes j = 0 .. 63 of one wave (active = this thread is one of them and the row is live).
// Called by every thread of the workgroup: it holds two workgroup barriers.
__device__ __forceinline__ void logit_rules_sparse(const LogitRulesArgs& a, float* __restrict__ x, long r, int64_t* hs, int j,
                                                   bool active) {
  const int t = a.t, V = a.V;
  if (active) hs[j] = j < t ? a.hist[(size_t)j * a.ld_hist + (size_t)r] : (int64_t)-1;
  __syncthreads();   // the history is in LDS; in form (A) also: the bias pass of this row is complete
  if (active && a.pen && j < t) {
    const int64_t c = hs[j];
    if (c >= 0 && c < V) {   // (an id outside the vocabulary is skipped: never indexed with)
      int n = 0;
      bool first = true;
      for (int i = 0; i < t; ++i) {
        const bool eq = hs[i] == c;
        n += eq ? 1 : 0;
        first = first && !(eq && i < j);
      }
      if (first) {
        float v = x[c];
        v = v > 0.f ? v / a.theta : v * a.theta;
        const float f = a.frequency * (float)n;
        const float s = a.presence + f;
        x[c] = v - s;
      }
    }
  }
  __syncthreads();   // penalties before bans: a ban is the last word on its token
  if (!active) return;
  int sup = -1;
#pragma unroll
  for (int q = 0; q < SSC_RULES_MAX_SUPPRESS; ++q)
    if (q == j && q < a.n_suppress) sup = a.suppress[q];
  if (sup >= 0 && sup < V) x[sup] = -INFINITY;
  if (j == SSC_WAVE - 1 && t < a.min_length) x[a.end_index] = -INFINITY;
  const int n = a.ngram;
  if (n >= 1 && j + n <= t) {   // the n-gram that starts at position j ends inside the history
    bool hit = true;
    for (int q = 0; q < n - 1; ++q) hit = hit && hs[j + q] == hs[t - (n - 1) + q];
    const int64_t tok = hs[j + n - 1];
    if (hit && tok != (int64_t)a.end_index && tok >= 0 && tok < V) x[tok] = -INFINITY;   // (END is never banned by this rule)
  }
}

// form (A): one workgroup per row
__global__ __launch_bounds__(256) void logit_rules_bias_kernel(const LogitRulesArgs a) {
  __shared__ int64_t hs[SSC_RULES_MAX_LEN];
  const long r = blockIdx.x;
  const bool live = logit_rules_live(a, r);   // workgroup-uniform
  float* x = a.logits + (size_t)r * a.ld;
  if (live) {
    const int br = a.bias_row ? a.bias_row[r] : 0;
    if (br >= 0 && br < a.n_bias) {   // (a value outside the matrix: no bias for this row, never indexed)
      const float* __restrict__ b = a.bias + (size_t)br * a.ld_bias;
      const int head = a.head, n4 = a.n4, V = a.V;
      float4* x4 = reinterpret_cast<float4*>(x + head);
      const float4* b4 = reinterpret_cast<const float4*>(b + head);
#pragma unroll 2
      for (int i = threadIdx.x; i < n4; i += 256) {
        float4 u = x4[i];
        const float4 w = b4[i];
        u.x = u.x + w.x; u.y = u.y + w.y; u.z = u.z + w.z; u.w = u.w + w.w;
        x4[i] = u;
      }
      const int tail = head + (n4 << 2), ns = head + (V - tail);
      for (int k = threadIdx.x; k < ns; k += 256) {
        const int v = k < head ? k : tail + (k - head);
        x[v] = x[v] + b[v];
      }
    }
  }
  logit_rules_sparse(a, x, r, hs, (int)threadIdx.x, live && threadIdx.x < SSC_WAVE);
}

// form (B): one wave per row
__global__ __launch_bounds__(SSC_WAVE * LOGIT_RULES_ROWS) void logit_rules_sparse_kernel(const LogitRulesArgs a) {
  __shared__ int64_t hs[LOGIT_RULES_ROWS][SSC_RULES_MAX_LEN];
  const int wv = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * LOGIT_RULES_ROWS + wv;   // wave-uniform
  const bool live = logit_rules_live(a, r);
  logit_rules_sparse(a, a.logits + (size_t)(live ? r : 0) * a.ld, r, hs[wv], (int)(threadIdx.x & 63), live);
}

// 16-byte accesses only where both rows of every pair share one misalignment (every bias row then does: ld_bias % 4 == 0)
inline void logit_rules_split(const float* logits, int ld, const float* bias, int ld_bias, int V, int* head, int* n4) {
  *head = V;
  *n4 = 0;
  if ((ld & 3) != 0 || (ld_bias & 3) != 0) return;
  if (((uintptr_t)logits & 15u) != ((uintptr_t)bias & 15u)) return;
  const int h = (int)(((16u - (unsigned)((uintptr_t)logits & 15u)) & 15u) >> 2);
  if (h >= V) return;
  *head = h;
  *n4 = (V - h) >> 2;
}

}  // namespace

int ssc_logit_rules_check(const ssc_logit_rules* r, int V, int end_index, bool* active) {
  *active = false;
  if (!r || V < 1 || end_index < 0 || end_index >= V) return SSC_EINVAL;
  if (r->no_repeat_ngram < 0 || r->no_repeat_ngram > SSC_RULES_MAX_LEN || r->min_length < 0) return SSC_EINVAL;
  if (r->n_suppress < 0 || r->n_suppress > SSC_RULES_MAX_SUPPRESS) return SSC_EINVAL;
  for (int q = 0; q < r->n_suppress; ++q)
    if (r->suppress[q] < 0 || r->suppress[q] >= V || r->suppress[q] == end_index) return SSC_EINVAL;
  if (!(r->repetition_penalty > 0.f) || !ssc_finite_f(r->repetition_penalty)) return SSC_EINVAL;
  if (!ssc_finite_f(r->presence_penalty) || !ssc_finite_f(r->frequency_penalty)) return SSC_EINVAL;
  if (r->bias && (r->ld_bias < V || r->n_bias < 1)) return SSC_EINVAL;
  if (((uintptr_t)r->bias & 3u) != 0 || (r->bias && ((uintptr_t)r->bias_row & 3u) != 0)) return SSC_EALIGN;
  *active = r->no_repeat_ngram >= 1 || r->min_length > 0 || r->n_suppress > 0 || r->repetition_penalty != 1.f ||
            r->presence_penalty != 0.f || r->frequency_penalty != 0.f || r->bias != nullptr;
  return SSC_OK;
}

int ssc_logit_rules_launch(float* logits, int ld, int rows, int V, const ssc_logit_rules* r, const int64_t* hist, int ld_hist, int t,
                           int end_index, hipStream_t st) {
  LogitRulesArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.rows = rows; a.V = V;
  a.hist = hist; a.ld_hist = (size_t)ld_hist; a.t = t; a.end_index = end_index;
  a.ngram = r->no_repeat_ngram; a.min_length = r->min_length; a.n_suppress = r->n_suppress;
  for (int q = 0; q < SSC_RULES_MAX_SUPPRESS; ++q) a.suppress[q] = q < r->n_suppress ? r->suppress[q] : -1;
  a.theta = r->repetition_penalty; a.presence = r->presence_penalty; a.frequency = r->frequency_penalty;
  a.pen = (a.theta != 1.f || a.presence != 0.f || a.frequency != 0.f) ? 1 : 0;
  if (r->bias) {
    a.bias = r->bias; a.ld_bias = (size_t)r->ld_bias; a.n_bias = r->n_bias; a.bias_row = r->bias_row;
    logit_rules_split(logits, ld, r->bias, r->ld_bias, V, &a.head, &a.n4);
    SSC_LAUNCH(logit_rules_bias_kernel, dim3(rows), dim3(256), 0, st, a);
  } else {
    SSC_LAUNCH(logit_rules_sparse_kernel, dim3(ssc_cdiv(rows, LOGIT_RULES_ROWS)), dim3(SSC_WAVE * LOGIT_RULES_ROWS), 0, st, a);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_logit_rules_rows(float* logits, int ld, int rows, int V, const ssc_logit_rules* r, const int64_t* hist,
                                    int ld_hist, int t, int end_index, void* stream) {
  if (!logits || !r || rows < 0 || V < 1 || ld < V || ld_hist < rows || t < 0 || t >= SSC_RULES_MAX_LEN) return SSC_EINVAL;
  if (t >= 1 && !hist) return SSC_EINVAL;
  bool active;
  const int rc = ssc_logit_rules_check(r, V, end_index, &active);
  if (rc == SSC_EINVAL) return rc;
  if ((long)V <= (long)t + r->n_suppress + 1) return SSC_EINVAL;
  if (((uintptr_t)logits & 3u) != 0 || ((uintptr_t)hist & 3u) != 0) return SSC_EALIGN;
  SSC_TRY(rc);
  if (!active || rows == 0) return SSC_OK;
  return ssc_logit_rules_launch(logits, ld, rows, V, r, hist, ld_hist, t, end_index, (hipStream_t)stream);
}
