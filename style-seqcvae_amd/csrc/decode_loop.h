// The host driver the one-call decodes share (search.hip: ssc_decode_search and the three sampled / diverse searches on top of
// search_run; sample.hip: ssc_decode_sample; score.hip: ssc_decode_score) - DESIGN.md, "the one-call decodes' host driver".
// Host code only: the two generations of step states, the attended-feature-table decision, the early-stop step pacer and the
// checks every driver makes of its descriptor.  Each of these is decided HERE and nowhere else.
#pragma once
#include <thread>

#include "ssc_common.h"

// The workspace is laid out with a running cursor; every block starts 256-byte aligned.
inline size_t ssc_ws_take(size_t& cursor, size_t bytes) {
  const size_t at = cursor;
  cursor += ssc_round_up(bytes, 256);
  return at;
}

// Two generations of the step states h1, c1, hd, cd, each (rows, H) floats, and - 2xFP16 numerics of a large search only - of the
// fp16 pieces of h1 and hd (ssc_decode_step_desc.h1_planes ...), each (rows, plane_words) words.
struct SscStepStates {
  size_t st[2][4];
  size_t pl[2][2];
  size_t H;

  void reserve(size_t& cursor, size_t rows, size_t H_, size_t plane_words = 0) {
    H = H_;
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < 4; ++k) st[g][k] = ssc_ws_take(cursor, rows * H * 4);
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < 2; ++k) pl[g][k] = ssc_ws_take(cursor, rows * plane_words * 4);
  }
  bool has_planes() const { return pl[1][0] != pl[0][0]; }
  float* state(char* W, int gen, int k) const { return (float*)(W + st[gen][k]); }
  // zero start states (cbs.py: start_state None -> updown_cell.py:131-141)
  int zero(char* W, int gen, size_t rows, hipStream_t stream) const {
    for (int k = 0; k < 4; ++k)
      if (hipMemsetAsync(W + st[gen][k], 0, rows * H * 4, stream) != hipSuccess) return SSC_EHIP;
    return SSC_OK;
  }
  // a step reads generation `cur` and writes generation 1 - cur
  void bind(char* W, int cur, ssc_decode_step_desc* sd) const {
    sd->h1 = state(W, cur, 0); sd->c1 = state(W, cur, 1); sd->hd = state(W, cur, 2); sd->cd = state(W, cur, 3);
    sd->h1_out = state(W, 1 - cur, 0); sd->c1_out = state(W, 1 - cur, 1);
    sd->hd_out = state(W, 1 - cur, 2); sd->cd_out = state(W, 1 - cur, 3);
  }
  // the states' fp16 pieces travel with the un-gathered states (a re-ordered state is split again by its step)
  void bind_planes(char* W, int cur, bool ungathered, ssc_decode_step_desc* sd) const {
    if (!has_planes()) return;
    sd->h1_planes_out = W + pl[1 - cur][0]; sd->hd_planes_out = W + pl[1 - cur][1];
    sd->h1_planes = ungathered ? W + pl[cur][0] : nullptr; sd->hd_planes = ungathered ? W + pl[cur][1] : nullptr;
  }
};

// Where a call starts (ssc_search_desc.start, include/ssc.h: ssc_start_state).  What the drivers refuse before any launch: a NULL
// member, and a start state together with what it is not combined with - `alone` is false where the call has a latent guide or
// runs an ensemble.
inline bool ssc_decode_start_ok(const ssc_start_state* s, bool alone = true) {
  return !s || (alone && s->h1 && s->c1 && s->hd && s->cd && s->tokens);
}
// ... and the states the first step reads: generation `gen` zeroed (no start state: the launches of a call without the field) or
// the caller's four blocks copied into it.  The fed tokens are ssc_decode_start's.
inline int ssc_decode_start_states(const ssc_start_state* s, const SscStepStates& states, char* W, int gen, size_t rows,
                                   hipStream_t stream) {
  if (!s) return states.zero(W, gen, rows, stream);
  const float* src[4] = {s->h1, s->c1, s->hd, s->cd};
  for (int k = 0; k < 4; ++k)
    if (hipMemcpyAsync(states.state(W, gen, k), src[k], rows * states.H * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return SSC_EHIP;
  return SSC_OK;
}

// The attended-feature term of the gates from the per-image table (ssc_decode_step_desc.att_table): the decision
// DecodeEngine.step makes per call, here once per call and extent.
inline bool ssc_att_table_wanted(int R, int rows, int rows_per_image) {
  return R <= 128 && rows >= 512 && rows_per_image >= 16 && ssc_decode_att_table_enabled();
}
// ... and what a step is told: 2 = form the table first (the first step of a call that uses it), 1 = it is there, 0 = not used
struct SscAttTable {
  bool ready = false;
  int next(bool wanted) {
    if (!wanted) return 0;
    const int mode = ready ? 1 : 2;
    ready = true;
    return mode;
  }
};

// Early stop and the host's run-ahead.  The device notes the step after which every row had ended and turns later steps into
// no-ops (ssc_beam_desc.ctl); the host stops QUEUEING once it sees the flag the device wrote - a plain read of pinned memory.  The
// host queues a step in a fraction of the time the device needs for it, so a host that only polls the flag has long queued every
// step by the time the device writes it (measured: captions that all end at step 2 still cost all 20 steps).  The run-ahead is
// therefore bounded: step t is queued only once the step `ahead` steps before it has completed - the last workgroup of a step's
// selection (the merge kernel of a search, the sampler of a sampled decode) notes the step in the second pinned word
// (ssc_beam_desc.host_flag[1]) and the host reads it; no event, no synchronisation call (an event per step cost 1.7 % of a search
// that never stops).  The device always has that many steps of work queued, and at most that many surplus steps run.  Not under
// stream capture (a captured call queues every step).
struct SscStepPacer {
  static constexpr int RUN_AHEAD = 2;   // `ahead` above
  const volatile int* flag;   // the two pinned words, or null: no early stop, or nothing for the host to read
  hipStream_t stream;
  bool bounded = false;

  SscStepPacer(int early_stop, const int* host_flag_host, hipStream_t st)
      : flag(early_stop ? host_flag_host : nullptr), stream(st) {
    if (!flag) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    bounded = cs == hipStreamCaptureStatusNone;
  }
  // Call before queueing step t: has the device said stop?
  bool stop_before(int t) const {
    const int due = t - RUN_AHEAD;
    if (bounded && due > 0) {   // until the device has completed step `due` (or stopped, or the stream has drained: an error upstream)
      for (unsigned spin = 1; flag[1] < due && flag[0] == 0; ++spin) {
        if ((spin & 1023u) == 0 && hipStreamQuery(stream) != hipErrorNotReady) { (void)hipGetLastError(); break; }
        std::this_thread::yield();
      }
    }
    return flag && flag[0] != 0;
  }
};

// The rows a TEACHER-FORCED step leaves out (ssc_decode_score, ssc_decode_prime), decided here for both: at step 0 every row's fed
// token is END, so no row may be skipped by it; from step 1 on a row whose fed token is END - its caption or prefix has ended, or
// the slot is absent - is not stepped (ssc_decode_step_desc.row_lp), under the beam-1 parent list `parent0`.
inline void ssc_forced_step_rows(ssc_decode_step_desc* sd, int t, const int64_t* parent0, const float* lp, int end_index) {
  if (t == 0) return;
  sd->parent = parent0; sd->group = 1;
  sd->row_lp = lp; sd->end_index = end_index;
}

// The attention trace of a call (ssc_attn_record, D::attn): off, or both of the caller's buffers ...
template <class D>
bool ssc_decode_attn_ok(const D* d) {
  return !d->attn || (d->attn->hist && d->attn->anc);
}
// ... and where step t of `rows` rows writes its attention weights: its slab of the caller's history instead of the workspace
// block every step overwrites.  The step writes them either way: recording is no copy and no launch.
inline float* ssc_decode_alpha_at(const ssc_attn_record* attn, float* ws_alpha, int t, size_t rows, int R) {
  return attn ? attn->hist + (size_t)t * rows * R : ws_alpha;
}

// What every driver checks of its descriptor D (ssc_search_desc, ssc_score_desc); `steps` is its max_steps / max_len.
// ... the extents its workspace size depends on
template <class D>
bool ssc_decode_dims_ok(const ssc_model_cfg* cfg, const D* d, int steps) {
  return cfg && d && d->nimg > 0 && d->R > 0 && d->n_samples > 0 && steps > 0;
}
// ... and the inputs a step reads: features, image terms, noise, and what the prior of this configuration is formed from
template <class D>
bool ssc_decode_inputs_ok(const ssc_model_cfg* cfg, const D* d, int steps) {
  if (!d->feats || !d->imgbuf || !d->eps0 || (steps > 1 && !d->eps)) return false;
  if (d->end_index < 0 || d->end_index >= cfg->V || !ssc_decode_attn_ok(d)) return false;
  return !(cfg->kld_mode == 2 ? !d->obj_atts : ((cfg->S || cfg->pm_scale != 0.f) && !d->sentiment));
}
