// Prompted decoding: start the one-call decodes from a forced prefix (include/ssc.h: ssc_start_state, ssc_decode_prime,
// ssc_prefix_join; DESIGN.md: "prompted decoding").  ssc_decode_prime is the teacher-forced loop of ssc_decode_score on the
// B = images x samples rows of a call that leaves STATES: after step t the rows whose prefix is t + 1 words long hand their four
// output states and their last word to the caller, who passes them to a search or a sampled decode as its start state.  The host
// loop is built from the shared driver of decode_loop.h, the per-word log-probs come from the score kernel (score.hip).
// Three small kernels live here: the preparation of the fed / target planes, the capture of one step's rows and the join of
// prefix and continuation.  None of them uses an atomic: the same bits on every run.
#include "decode_loop.h"

namespace {

constexpr int PREFIX_THREADS = 64;

// One workgroup per row b.  prefix (B, L) -> time-major planes tgt (L, B): the word scored at step t, -1 from the prefix's end on -
// its first id outside [0, V) or equal to end_index, which is never used as an index -, fed (L, B): the word fed at step t,
// END at step 0 and wherever the row has ended; lengths (B); lp (B) = 0.  A row without a prefix gets the start of an unprefixed
// call: zero states and END.
__global__ __launch_bounds__(PREFIX_THREADS) void prefix_prepare_kernel(const int64_t* __restrict__ prefix, int B, int L, int V, int H,
                                                                         int end_index, int64_t* __restrict__ tgt,
                                                                         int64_t* __restrict__ fed, float* __restrict__ lp,
                                                                         int* __restrict__ lengths, int64_t* __restrict__ tokens,
                                                                         float* __restrict__ h1, float* __restrict__ c1,
                                                                         float* __restrict__ hd, float* __restrict__ cd) {
  __shared__ int sh_len;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int64_t* src = prefix + (size_t)b * L;
    int len = 0;
    bool open = true;
    fed[b] = end_index;
    for (int t = 0; t < L; ++t) {
      const int64_t x = src[t];
      open = open && x >= 0 && x < V && x != end_index;
      tgt[(size_t)t * B + b] = open ? x : -1;
      if (t + 1 < L) fed[(size_t)(t + 1) * B + b] = open ? x : end_index;
      len += open ? 1 : 0;
    }
    lengths[b] = len;
    lp[b] = 0.f;
    if (len == 0) tokens[b] = end_index;
    sh_len = len;
  }
  __syncthreads();
  if (sh_len != 0) return;   // (workgroup-uniform)
  const size_t o = (size_t)b * H;
  for (int j = threadIdx.x; j < H; j += PREFIX_THREADS) {
    h1[o + j] = 0.f; c1[o + j] = 0.f; hd[o + j] = 0.f; cd[o + j] = 0.f;
  }
}

struct CaptureArgs {
  const float* src[4];   // the step's output states, (B, H)
  float* dst[4];         // the caller's blocks, (B, H)
  const int* lengths;
  const int64_t* tgt;    // this step's plane of targets (B)
  int64_t* tokens;
  int H, step;
};

// One workgroup per row: a row whose prefix ends with this step's word hands over its 4 x H floats and that word.  VEC: 16-byte
// moves (H % 4 == 0 and 16-byte aligned blocks: every row then starts on a 16-byte boundary); otherwise one float at a time.
template <bool VEC>
__global__ __launch_bounds__(PREFIX_THREADS) void prefix_capture_kernel(const CaptureArgs a) {
  const int b = blockIdx.x;
  if (a.lengths[b] != a.step + 1) return;   // (workgroup-uniform)
  const size_t o = (size_t)b * a.H;
  if (VEC) {
    const int n4 = a.H >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4* s = reinterpret_cast<const float4*>(a.src[k] + o);
      float4* d = reinterpret_cast<float4*>(a.dst[k] + o);
      for (int j = threadIdx.x; j < n4; j += PREFIX_THREADS) d[j] = s[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int j = threadIdx.x; j < a.H; j += PREFIX_THREADS) a.dst[k][o + j] = a.src[k][o + j];
  }
  if (threadIdx.x == 0) a.tokens[b] = a.tgt[b];
}

// One thread per returned caption (b, q).
__global__ void prefix_join_kernel(const int64_t* __restrict__ prefix, const int* __restrict__ lengths, int Lp,
                                   const int64_t* __restrict__ pred, const int* __restrict__ ctl, int steps,
                                   const float* __restrict__ lps, const float* __restrict__ prefix_lp, int B, int Q, int end_index,
                                   int64_t* __restrict__ out, float* __restrict__ total) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= B * Q) return;
  const int b = g / Q;
  const int len = min(max(lengths[b], 0), Lp);
  const int n = ctl ? min(max(ctl[0], 0), steps) : steps;
  const int W = Lp + steps;
  int64_t* o = out + (size_t)g * W;
  for (int j = 0; j < len; ++j) o[j] = prefix[(size_t)b * Lp + j];
  for (int t = 0; t < steps; ++t) o[len + t] = t < n ? pred[(size_t)g * steps + t] : (int64_t)end_index;
  for (int j = len + steps; j < W; ++j) o[j] = end_index;
  const float lp = lps[g];
  total[g] = lp <= -1e19f ? lp : prefix_lp[b] + lp;
}

struct PrimeLayout {
  SscStepStates states;   // (B, H) rows
  size_t tgt;        // (L, B) int64
  size_t fed;        // (L, B) int64
  size_t parent0;    // (B) int64 zeros: every row is its own parent (the beam-1 search's parent list)
  size_t lp;         // (B) running prefix log-probs
  size_t steplp;     // (B) the last step's log-probs (when the caller takes no token_lp)
  size_t alpha;      // (B, R)
  size_t logits;     // (B, V)
  size_t stepws, stepws_bytes;
  size_t total;
};

PrimeLayout prime_layout(const ssc_model_cfg* cfg, const ssc_prime_desc* d) {
  PrimeLayout l;
  const size_t B = (size_t)d->nimg * d->n_samples;
  size_t o = 0;
  l.states.reserve(o, B, cfg->H);
  l.tgt = ssc_ws_take(o, (size_t)d->max_len * B * 8);
  l.fed = ssc_ws_take(o, (size_t)d->max_len * B * 8);
  l.parent0 = ssc_ws_take(o, B * 8);
  l.lp = ssc_ws_take(o, B * 4);
  l.steplp = ssc_ws_take(o, B * 4);
  l.alpha = ssc_ws_take(o, B * (size_t)d->R * 4);
  l.logits = ssc_ws_take(o, B * (size_t)cfg->V * 4);
  l.stepws_bytes = ssc_decode_step_workspace_bytes(cfg, (int)B, d->R);
  l.stepws = ssc_ws_take(o, l.stepws_bytes);
  l.total = o;
  return l;
}

bool prime_dims_ok(const ssc_model_cfg* cfg, const ssc_prime_desc* d) {
  return ssc_decode_dims_ok(cfg, d, d ? d->max_len : 0) && (long)d->nimg * d->n_samples <= (1L << 24);
}

bool prime_desc_ok(const ssc_model_cfg* cfg, const ssc_prime_desc* d) {
  if (!prime_dims_ok(cfg, d) || !d->feats || !d->imgbuf || !d->prefix || !d->eps) return false;
  if (d->end_index < 0 || d->end_index >= cfg->V) return false;
  if (cfg->kld_mode == 2 ? !d->obj_atts : ((cfg->S || cfg->pm_scale != 0.f) && !d->sentiment)) return false;
  return d->h1 && d->c1 && d->hd && d->cd && d->tokens && d->lengths && d->log_probs;
}

}  // namespace

extern "C" size_t ssc_decode_prime_workspace_bytes(const ssc_model_cfg* cfg, const ssc_prime_desc* d) {
  if (!prime_dims_ok(cfg, d)) return 0;
  return prime_layout(cfg, d).total;
}

extern "C" int ssc_decode_prime(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_prime_desc* d, void* workspace,
                                size_t workspace_bytes, void* stream) {
  SscGemmModeScope mode_scope(cfg);   // the numerics mode of this cfg, for every product the call issues
  if (!p || !workspace || !prime_desc_ok(cfg, d)) return SSC_EINVAL;
  const PrimeLayout l = prime_layout(cfg, d);
  if (workspace_bytes < l.total) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* W = (char*)workspace;
  const int B = d->nimg * d->n_samples, V = cfg->V, Z = cfg->Z, H = cfg->H, L = d->max_len;
  const SscStepStates& states = l.states;
  int64_t* tgt = (int64_t*)(W + l.tgt);
  int64_t* fed = (int64_t*)(W + l.fed);
  int64_t* parent0 = (int64_t*)(W + l.parent0);
  float* lp = (float*)(W + l.lp);
  float* logits = (float*)(W + l.logits);

  SSC_LAUNCH(prefix_prepare_kernel, dim3(B), dim3(PREFIX_THREADS), 0, st, d->prefix, B, L, V, H, d->end_index, tgt, fed, lp,
             d->lengths, d->tokens, d->h1, d->c1, d->hd, d->cd);
  SSC_CHECK_LAUNCH();
  if (hipMemsetAsync(parent0, 0, (size_t)B * 8, st) != hipSuccess) return SSC_EHIP;
  SSC_TRY(states.zero(W, 1, B, st));

  // the steps take the form the beam-1 drivers give them (ssc_decode_score, ssc_decode_sample): same tables, same parent list
  const bool want_table = ssc_att_table_wanted(d->R, B, d->n_samples);
  SscAttTable table;
  ssc_decode_step_desc sd{};
  sd.R = d->R; sd.feats = d->feats; sd.imgbuf = d->imgbuf; sd.alpha = (float*)(W + l.alpha); sd.log_probs = logits; sd.raw_logits = 1;
  sd.obj_atts = d->obj_atts;
  sd.G = B; sd.rows_per_image = d->n_samples; sd.sentiment = d->sentiment;
  CaptureArgs ca{};
  ca.dst[0] = d->h1; ca.dst[1] = d->c1; ca.dst[2] = d->hd; ca.dst[3] = d->cd;
  ca.lengths = d->lengths; ca.tokens = d->tokens; ca.H = H;
  const bool vec = (H & 3) == 0 && ssc_aligned16(d->h1) && ssc_aligned16(d->c1) && ssc_aligned16(d->hd) && ssc_aligned16(d->cd);
  int cur = 1;
  for (int t = 0; t < L; ++t) {
    sd.tokens = fed + (size_t)t * B;
    sd.eps = d->eps + (size_t)t * B * Z;
    states.bind(W, cur, &sd);
    sd.att_table = table.next(want_table);
    ssc_forced_step_rows(&sd, t, parent0, lp, d->end_index);   // rows whose prefix has ended (fed token END) are not stepped
    SSC_TRY(ssc_decode_step_guided(cfg, p, &sd, nullptr, W + l.stepws, l.stepws_bytes, st));
    SSC_TRY(ssc_score_rows_at(logits, V, B, V, tgt + (size_t)t * B, t == 0 ? nullptr : fed + (size_t)t * B, d->end_index, lp,
                              d->token_lp ? d->token_lp + t : (float*)(W + l.steplp), d->token_lp ? L : 1, st));
    for (int k = 0; k < 4; ++k) ca.src[k] = states.state(W, 1 - cur, k);   // (the generation this step has written)
    ca.tgt = tgt + (size_t)t * B; ca.step = t;
    if (vec) SSC_LAUNCH(prefix_capture_kernel<true>, dim3(B), dim3(PREFIX_THREADS), 0, st, ca);
    else SSC_LAUNCH(prefix_capture_kernel<false>, dim3(B), dim3(PREFIX_THREADS), 0, st, ca);
    SSC_CHECK_LAUNCH();
    cur = 1 - cur;
  }
  if (hipMemcpyAsync(d->log_probs, lp, (size_t)B * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return SSC_EHIP;
  return SSC_OK;
}

extern "C" int ssc_prefix_join(const int64_t* prefix, const int* lengths, int Lp, const int64_t* predictions, const int* ctl, int steps,
                               const float* log_probs, const float* prefix_lp, int B, int Q, int end_index, int64_t* captions,
                               float* total, void* stream) {
  if (!prefix || !lengths || !predictions || !log_probs || !prefix_lp || !captions || !total) return SSC_EINVAL;
  if (B < 1 || Q < 1 || Lp < 1 || steps < 1 || end_index < 0 || (long)B * Q > (1L << 24)) return SSC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SSC_LAUNCH(prefix_join_kernel, dim3(ssc_cdiv(B * Q, 256)), dim3(256), 0, st, prefix, lengths, Lp, predictions, ctl, steps, log_probs,
             prefix_lp, B, Q, end_index, captions, total);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
