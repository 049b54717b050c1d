// Internal helpers shared by the HIP translation units of libssc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ssc.h"

extern thread_local int ssc_tls_hip_error;

// Every kernel launch goes through SSC_LAUNCH: the thread's sticky HIP error is cleared first, so that SSC_CHECK_LAUNCH
// reports THIS launch and not an error some earlier, unrelated HIP call of the process left behind (seen: hipError 100
// from the host framework's device probing made the first launch of a process "fail").
#define SSC_LAUNCH(...)              \
  do {                               \
    (void)hipGetLastError();         \
    hipLaunchKernelGGL(__VA_ARGS__); \
  } while (0)

#define SSC_CHECK_LAUNCH()                         \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) {                       \
      ssc_tls_hip_error = (int)e__;                \
      return SSC_EHIP;                             \
    }                                              \
  } while (0)

#define SSC_TRY(expr)            \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ != SSC_OK) return rc__; \
  } while (0)

// Tuning / diagnostic defaults may be overridden from the environment ONLY in a process that opts in with SSC_DEBUG=1: a stray
// SSC_* variable must not change which kernels the product path runs.  Tools (tools/*.py) set SSC_DEBUG=1.
#include <stdlib.h>
#include <string.h>
static inline bool ssc_env_debug() { const char* d = getenv("SSC_DEBUG"); return d && d[0] == '1'; }
static inline int ssc_env_int(const char* name, int dflt) {
  if (!ssc_env_debug()) return dflt;
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

static inline bool ssc_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline int ssc_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t ssc_round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
static inline bool ssc_finite_f(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }   // false for NaN

#define SSC_WAVE 64
__device__ __forceinline__ bool ssc_aligned16_dev(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

__device__ __forceinline__ float ssc_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float ssc_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the sum or maximum of v over the workgroup (a multiple of 64 threads, sh: one float per wave), the same in every thread: wave
// butterflies, then the waves in index order.  Two barriers, so calls may follow one another on the same sh.
__device__ __forceinline__ float ssc_block_reduce(float v, float* sh, bool is_max) {
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = is_max ? ssc_wave_max(v) : ssc_wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < nw; ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

// How the cross-entropy kernels that stream a row (cross_entropy.hip: every form but the plain pair; distillation with a teacher's
// row b beside it) walk it: elements [0, head) and [head + 4 * n4, V) one by one, the n4 groups of four in between as 16-byte accesses.  With
// leading dimensions that are multiples of 4 every row shares the first row's misalignment; a second matrix must share it too.
// head = V, n4 = 0 is the scalar path throughout.
static inline void ssc_row_split(const float* a, int lda, const float* b, int ldb, int V, int* head, int* n4) {
  *head = V;
  *n4 = 0;
  if ((lda & 3) != 0) return;
  if (b && ((ldb & 3) != 0 || ((uintptr_t)a & 15u) != ((uintptr_t)b & 15u))) return;
  const int h = (int)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) >> 2);
  if (h >= V) return;
  *head = h;
  *n4 = (V - h) >> 2;
}
// the column of the k-th element of a split row's scalar part (k < head + V - tail, tail = head + 4 * n4)
__device__ __forceinline__ int ssc_row_split_col(int k, int head, int tail) { return k < head ? k : tail + (k - head); }
static inline bool ssc_ce_eps_ok(float eps) { return eps >= 0.f && eps < 1.f; }   // the label-smoothing weight; false for NaN

__device__ __forceinline__ float ssc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// tanh x = 1 - 2 / (1 + e^{2x}) on the hardware exp2 / rcp (v_exp_f32, v_rcp_f32: ~1 ulp each): absolute error < 3e-7 everywhere,
// exact limits (+-1) for large |x|.  Used where a kernel is bound by its tanh count (attention logits: G*R*A per step - 138 M
// at the decode shape, ~25 instructions each with the library tanhf); forward and backward of the attention use the SAME function.
__device__ __forceinline__ float ssc_tanh_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);   // e^{2x}
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
}

// 2xFP16 pieces (ssc_model_cfg.gemm_mode 3): hi = x truncated to fp16, lo = (x - hi) truncated to fp16 (x - hi is exact in fp32) -
// 21-22 significant bits of x; two v_cvt_pkrtz + two conversions back + two subtractions per pair.  |x| must stay below 65504.
// ONE definition for the product kernels' producers, ssc_split_f16 and the cells that leave their output already split.
typedef float ssc_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ssc_u32x2 __attribute__((ext_vector_type(2)));
typedef __fp16 ssc_h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void ssc_split4_f16(const ssc_f32x4& v, ssc_u32x2& hi, ssc_u32x2& lo) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const ssc_h16x2 h = __builtin_amdgcn_cvt_pkrtz(v[2 * j], v[2 * j + 1]);
    const float r0 = v[2 * j] - (float)h[0], r1 = v[2 * j + 1] - (float)h[1];
    const ssc_h16x2 l = __builtin_amdgcn_cvt_pkrtz(r0, r1);
    hi[j] = __builtin_bit_cast(unsigned, h);
    lo[j] = __builtin_bit_cast(unsigned, l);
  }
}
// one value: the two halfs as raw bits (the same conversions, element by element)
__device__ __forceinline__ void ssc_split1_f16(float x, unsigned short& hi, unsigned short& lo) {
  const ssc_h16x2 h = __builtin_amdgcn_cvt_pkrtz(x, 0.f);
  const ssc_h16x2 l = __builtin_amdgcn_cvt_pkrtz(x - (float)h[0], 0.f);
  hi = (unsigned short)(__builtin_bit_cast(unsigned, h) & 0xffffu);
  lo = (unsigned short)(__builtin_bit_cast(unsigned, l) & 0xffffu);
}
// plane layout (ssc_gemm_seg.A16): word offset of the hi half-pair of columns k, k + 1 (k even) inside a row; the lo pair is 16 words on
__device__ __forceinline__ int ssc_plane_word(int k) { return (k >> 5) * 32 + ((k & 31) >> 1); }

// internal cross-TU entry points (not part of the C ABI)
int ssc_gemm_slabs(const ssc_gemm_desc* d, int splits, float* slabs, hipStream_t st);  // partial slabs only
int ssc_attn_fwd_qslabs(const float* qslabs, int nslab, size_t slab_stride, float* q_out, int ldqo, const float* pv,
                        const float* wa, const float* mask, const float* feats, int G, int R, int A, int F,
                        int rows_per_image, float* logits, float* alpha, float* att, int ldatt, hipStream_t st,
                        const float* obj = nullptr, int D = 0, float* pool = nullptr, int ldpool = 0);
int ssc_gemm_slabs_auto(const ssc_gemm_desc* d, float* slabs, size_t cap_floats, int* nslab, hipStream_t st);
// n <= 3 independent minibatch products (M <= 64, same operand layout) in ONE launch, each left as split-K slabs in its
// own region; falls back to one launch per product when they do not qualify for the 64x256 wave-specialised kernel
int ssc_gemm_slabs_group(const ssc_gemm_desc* const* d, int n, float* const* regions, const size_t* caps, int* nslab,
                         hipStream_t st);
// C (+)= sum of split-K slabs (M x N, ld N) in index order (+ bias)
int ssc_reduce_slabs(const float* slabs, int nslab, size_t stride, int M, int N, float* C, int ldc, const float* bias,
                     int accumulate, hipStream_t st);

// beam-search stages shared by decode.hip and fsm.hip
int ssc_beam_first_dense(bool norm, const float* lp, int ldlp, const uint8_t* fsm, const int* mach, int B, int S, int V, int beam,
                         int64_t* pred, float* lp_out, hipStream_t st);
int ssc_beam_rows_dense(bool norm, const float* lp, int ldlp, const uint8_t* fsm, const int* mach, const int64_t* last_pred, int B,
                        int S, int V, int beam, int per_node, int end_index, float* scratch_val, int64_t* scratch_idx,
                        hipStream_t st);
int ssc_beam_merge(const float* sval, const int64_t* sidx, const float* last_lp, int B, int S, int beam, int per_node,
                   int64_t* pred, float* lp_out, int64_t* backptr, int end_index, int* ctl, int step_index, int max_steps,
                   int* host_flag, hipStream_t st);
// The cross-entropy of the train step (cross_entropy.hip).  The descriptors' refusals (include/ssc.h: ssc_distill, ssc_unlikelihood):
// *on = the descriptor is there and its alpha > 0; logits NULL leaves distillation's overlap test, T = 0 unlikelihood's limit on the
// steps to a later call.
int ssc_distill_check(const ssc_distill* kd, const float* logits, int ldl, size_t rows, int V, bool* on);
int ssc_unlike_check(const ssc_unlikelihood* ul, int T, bool* on);
// ssc_ce_fwd_smooth / _distill / _unlike (kd, ul: optional, at most one of them on) with the three blocks [lse], [w*row(eps)],
// [w*row(0)] given one by one: the train workspace keeps the third apart from the first two, whose place - and with it every other
// buffer's - is what it was before the third block existed.  ssc_ce_bwd_terms: the backward of that forward.
int ssc_ce_fwd_blocks(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B, int V,
                      float eps, const ssc_distill* kd, const ssc_unlikelihood* ul, float* lse, float* nllw, float* nllw0, float* loss,
                      float* nll, hipStream_t st);
int ssc_ce_bwd_terms(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
                     const float* gl, int T, int B, int V, float eps, const ssc_distill* kd, const ssc_unlikelihood* ul, hipStream_t st);
int ssc_decode_att_table_enabled();   // the "dec_att_table" switch (decode.hip)
// the start of a one-call decode with the early-stop protocol (search.hip): ctl[0] = max_steps, the counters behind it zero;
// tokens0 (B) = end_index, the token the first step feeds - or, with a start state (ssc_start_state), its tokens, an id outside
// [0, V) replaced by end_index (never used as an index)
int ssc_decode_start(int* ctl, int max_steps, int64_t* tokens0, int B, int end_index, const int64_t* start_tokens, int V,
                     hipStream_t st);

// ssc_score_rows (score.hip) with lp_out of row r at r * lp_stride: what a teacher-forced driver issues per step
int ssc_score_rows_at(const float* logits, int ld, int rows, int V, const int64_t* target, const int64_t* last_target, int end_index,
                      float* row_lp, float* lp_out, int lp_stride, hipStream_t st);

// numerics mode of the calling thread's current sequence-level call (ssc_model_cfg.gemm_mode: 0 = the process default set by
// ssc_set_gemm_mode, 1 = 3xBF16, 2 = exact-fp32 MFMA); -1 = none in force
extern thread_local int ssc_tls_gemm_mode;
extern thread_local int ssc_tls_gemm_f16;
struct SscGemmModeScope {
  int prev, prev16;
  explicit SscGemmModeScope(const ssc_model_cfg* c) : prev(ssc_tls_gemm_mode), prev16(ssc_tls_gemm_f16) {
    if (c && (c->gemm_mode == 1 || c->gemm_mode == 3)) ssc_tls_gemm_mode = 1;
    else if (c && c->gemm_mode == 2) ssc_tls_gemm_mode = 0;
    if (c && c->gemm_mode != 0) ssc_tls_gemm_f16 = c->gemm_mode == 3 ? 1 : 0;   // (0: the process default stays in force)
  }
  ~SscGemmModeScope() { ssc_tls_gemm_mode = prev; ssc_tls_gemm_f16 = prev16; }
};
int ssc_decode_parts_enabled();        // the "dec_parts" switch (decode.hip): vocabulary head records instead of logits
// the limits of the sampled-node beam search (sampled_beam.hip, include/ssc.h: ssc_beam_step_sampled) for B entries of k beams,
// n candidates per beam over V tokens
bool ssc_sampled_beam_ok(int B, int k, int n, int V, const ssc_sampler_desc* s);
// the limits of the diverse beam search (diverse_beam.hip, include/ssc.h: ssc_diverse_desc) for B entries of k beams, n candidates per
// beam over V tokens; the entries of a row's list at a later step (n + k - k / groups, at most V)
bool ssc_diverse_beam_ok(int B, int k, int n, int V, const ssc_diverse_desc* s);
int ssc_diverse_beam_list(int k, int groups, int n, int V);
bool ssc_rules_beam_ok(int B, int k, int n, int V, int end_index, const ssc_rules_desc* r);
// the `anc` of an attention trace (attn_trace.hip, include/ssc.h: ssc_attn_record) from a call's chosen words (max_steps, B * SB)
// time-major; backs (max_steps - 1, B * SB) or null: the identity; ctl or null: every step ran; lp (B * SB) or null: no dead beam
int ssc_attn_anc(const int64_t* words, const int64_t* backs, const int* ctl, const float* lp, int max_steps, int B, int SB,
                 int end_index, int* anc, hipStream_t st);
// Latent-guided decoding (latent_guide.hip, include/ssc.h: ssc_latent_guide).  What a one-call decode hands a step: the call's guide,
// the step index t (slab t of the guide) and the rows of one guide entry at this step.  ssc_decode_step_guided is ssc_decode_step
// with the step's z block drawn by ssc_latent_guide_rows; sg null, sg->guide null or t >= steps: the launches of ssc_decode_step.
struct SscStepGuide {
  const ssc_latent_guide* guide;
  int t, rows_per_entry;
};
// what the guided entry points check of a guide before any launch (NULL is refused: the caller passes it only where one is set)
bool ssc_latent_guide_ok(const ssc_model_cfg* cfg, const ssc_latent_guide* g);
int ssc_decode_step_guided(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_decode_step_desc* d, const SscStepGuide* sg,
                           void* workspace, size_t workspace_bytes, void* stream);
// Logit rules for the word samplers (logit_rules.hip, include/ssc.h: ssc_logit_rules).  ssc_logit_rules_check: the refusals that
// depend on the fields and V alone (SSC_OK with *active = whether any control is on or a bias is set); ssc_logit_rules_launch: the
// edit of one step from checked rules - what ssc_decode_sample_opts issues per step for its `rules`.
int ssc_logit_rules_check(const ssc_logit_rules* r, int V, int end_index, bool* active);
int ssc_logit_rules_launch(float* logits, int ld, int rows, int V, const ssc_logit_rules* r, const int64_t* hist, int ld_hist, int t,
                           int end_index, hipStream_t st);
// Truncation for the word samplers (truncation.hip, include/ssc.h: ssc_truncation).  ssc_truncation_check: the refusals that depend
// on the fields and the temperature alone (SSC_OK with *active = kind != 0); ssc_truncation_launch: the edit of one step from a
// checked descriptor, its statistics going to `entropy` / `kept` (rows, or null) - what ssc_decode_sample_opts issues per step for its
// `trunc`.
int ssc_truncation_check(const ssc_truncation* tr, float temperature, bool* active);
int ssc_truncation_launch(float* logits, int ld, int rows, int V, const ssc_truncation* tr, float temperature, float* entropy, int* kept,
                          const int64_t* last_pred, int end_index, hipStream_t st);
// Mirostat for the word samplers (mirostat.hip, include/ssc.h: ssc_mirostat).  ssc_mirostat_check: the refusals that depend on the
// fields and the temperature alone (SSC_OK with *active = m && tau != 0); ssc_mirostat_fill: n floats of mu set to mu0; the two
// launches: the cut in front of and the update behind one step's draw - what ssc_decode_sample_mirostat issues per step.
int ssc_mirostat_check(const ssc_mirostat* m, float temperature, bool* active);
int ssc_mirostat_fill(float* mu, int n, float mu0, hipStream_t st);
int ssc_mirostat_rows_launch(float* logits, int ld, int rows, int V, float temperature, const float* mu, const int64_t* last_pred,
                             int end_index, int* kept, float* norm, hipStream_t st);
int ssc_mirostat_update_launch(const float* logits, int ld, int rows, int V, float temperature, float tau, float eta, const float* norm,
                               const int64_t* pred, const int64_t* last_pred, int end_index, const float* mu_in, float* mu_out,
                               float* surprise, hipStream_t st);
// Arithmetic sampling for the word samplers (arith.hip, include/ssc.h: ssc_arith).  ssc_arith_check: the refusals that depend on the
// descriptor alone (SSC_OK with *active = a && mode != 0); ssc_arith_codes_launch: the lattice of a call; ssc_arith_rows_launch: the
// draw of one step from checked arguments, with the early-stop words of the decode (ctl null: none) - what ssc_decode_sample_arith
// issues per step in place of the sampler's draw.
int ssc_arith_check(const ssc_arith* a, bool* active);
int ssc_arith_codes_launch(uint64_t seed, int nimg, int n_samples, uint64_t* code_out, hipStream_t st);
int ssc_arith_rows_launch(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const uint64_t* code_in,
                          const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out, uint64_t* code_out,
                          int64_t* mass_out, int step, int* ctl, int max_steps, int* host_flag, hipStream_t st);
// Contrastive decoding for the word samplers (contrast.hip, include/ssc.h: ssc_contrast_rows, ssc_contrast).  ssc_contrast_check: the
// refusals that depend on the knobs and the statistics pointers alone (SSC_OK with *active = alpha != 0 || beta != 0);
// ssc_contrast_launch: the edit of one step from checked knobs - what ssc_decode_sample_opts issues per step for its `contrast`.
int ssc_contrast_check(float alpha, float beta, const int* kept, const float* divergence, bool* active);
int ssc_contrast_launch(float* logits, int ld, const float* amateur, int lda, int rows, int V, float alpha, float beta, int* kept,
                        float* divergence, const int64_t* last_pred, int end_index, hipStream_t st);
int ssc_attn_weights_rows(const float* q, int ldq, const float* pv, const float* wa, const float* mask, int G, int R, int A,
                          int rows_per_image, float* logits, float* alpha, const int* rows, const int* row_count, hipStream_t st);
