// Attention traces of the one-call decodes (include/ssc.h: ssc_attn_record, ssc_attn_gather).  The decode steps write their
// attention weights straight into the caller's history (search.hip / sample.hip / score.hip hand step t the slab hist + t rows R);
// what lives here is the rest: the kernel that turns a call's chosen words and back-pointers into `anc` - which row of slab t word t
// of a returned caption read - and the gather that reads a trace back per selected caption.
//
// anc: one thread per returned caption, walking the chain the token back-trace walks (beam_backtrace_ctl_kernel, fsm.hip), with the
// step count from ctl[0].  The row decodes (sample, score) run the same kernel without back-pointers: the ancestry is the identity.
//
// gather: one wave per (caption, step) row, ATTN_ROWS rows per workgroup so that R = 36 fills a workgroup's four waves with four
// rows instead of leaving three idle; lanes over R, 16 bytes per lane where R, ld_maps and the pointers allow (loads and stores
// decided separately).  Each row is read from HBM once: the copy, the arg-max and the entropy term come from the same registers.
// Arg-max and entropy sum are wave butterflies in a fixed order - no atomics, no LDS, the same bits on every call.  Memory-bound:
// 2 R floats per row move, ~20 flops per element.
#include <math.h>

#include "ssc_common.h"

namespace {

constexpr int ATTN_ROWS = 4;   // rows (waves) per workgroup

// words (max_steps, B * SB) time-major: the chosen words (a scoring call: the targets, -1 from the caption's end on).
// backs (max_steps - 1, B * SB) or null: the identity.  ctl or null: every step ran.  lp (B * SB) or null: no beam is dead.
__global__ void attn_anc_kernel(const int64_t* __restrict__ words, const int64_t* __restrict__ backs, const int* __restrict__ ctl,
                                const float* __restrict__ lp, int max_steps, int B, int SB, int end_index, int* __restrict__ anc) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= B * SB) return;
  const int steps = ctl ? min(max(ctl[0], 1), max_steps) : max_steps;
  const int b = j / SB;
  const size_t plane = (size_t)B * SB, base = (size_t)b * SB;
  int* o = anc + (size_t)j * max_steps;
  for (int t = max_steps - 1; t >= steps; --t) o[t] = -1;
  const bool dead = lp && lp[j] <= -1e19f;
  int64_t idx = j % SB;
  for (int t = steps - 1; t >= 0; --t) {
    const int64_t w = words[(size_t)t * plane + base + idx];
    int a = b;   // (the first step has one row per batch entry)
    if (t > 0) {
      if (backs) idx = backs[(size_t)(t - 1) * plane + base + idx];
      // idx is now the beam's place after step t - 1's selection: the row step t gave it.  A row whose last word is END was not stepped.
      a = words[(size_t)(t - 1) * plane + base + idx] == end_index ? -1 : (int)(base + idx);
    }
    o[t] = (dead || w < 0) ? -1 : a;
  }
}

struct GatherArgs {
  const float* hist; int rows, R, steps;
  const int* anc; int n_caps;
  const int64_t* sel; long total;   // n_sel * steps
  float* maps; int ld_maps;
  int* top_region; float* top_weight; float* entropy;
};

// the better of two (value, index) candidates: the larger value, on a tie the lower index
__device__ __forceinline__ void attn_best(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// VEC_IN: 16-byte loads of the history (R % 4 == 0, 16-byte aligned base); VEC_OUT: 16-byte stores of the maps as well.  The order of
// the entropy sum depends on VEC_IN alone: what a call returns does not depend on which outputs it asks for.
template <bool VEC_IN, bool VEC_OUT>
__global__ __launch_bounds__(64 * ATTN_ROWS) void attn_gather_kernel(GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * ATTN_ROWS + (threadIdx.x >> 6);   // wave-uniform
  if (row >= a.total) return;
  const long i = row / a.steps;
  const int t = (int)(row - i * a.steps), R = a.R;
  const int64_t q = a.sel ? a.sel[i] : (int64_t)i;
  int src = -1;
  if (q >= 0 && q < a.n_caps) src = a.anc[(size_t)q * a.steps + t];
  const bool live = src >= 0 && src < a.rows;   // wave-uniform: a zero row never reads hist
  const float* h = a.hist + ((size_t)t * a.rows + (live ? src : 0)) * R;
  float* m = a.maps ? a.maps + (size_t)row * a.ld_maps : nullptr;
  float bv = -INFINITY, ent = 0.f;
  int bi = 0x7fffffff;
  if (VEC_IN) {
    for (int k = lane * 4; k < R; k += 256) {
      ssc_f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (live) x = *reinterpret_cast<const ssc_f32x4*>(h + k);
      if (m) {
        if (VEC_OUT) {
          *reinterpret_cast<ssc_f32x4*>(m + k) = x;
        } else {
          m[k] = x[0]; m[k + 1] = x[1]; m[k + 2] = x[2]; m[k + 3] = x[3];
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (x[c] > bv) { bv = x[c]; bi = k + c; }   // (ascending index: the first of equal values stays)
        if (x[c] > 0.f) ent -= x[c] * logf(x[c]);
      }
    }
  } else {
    for (int k = lane; k < R; k += 64) {
      const float x = live ? h[k] : 0.f;
      if (m) m[k] = x;
      if (x > bv) { bv = x; bi = k; }
      if (x > 0.f) ent -= x * logf(x);
    }
  }
  if (!a.top_region && !a.top_weight && !a.entropy) return;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const float ov = __shfl_xor(bv, w, 64);
    const int oi = __shfl_xor(bi, w, 64);
    attn_best(bv, bi, ov, oi);
    ent += __shfl_xor(ent, w, 64);
  }
  if (lane == 0) {
    const bool found = live && bi < R;   // (a row of NaNs has no arg-max: it reads as a zero row)
    if (a.top_region) a.top_region[row] = found ? bi : -1;
    if (a.top_weight) a.top_weight[row] = found ? bv : 0.f;
    if (a.entropy) a.entropy[row] = live ? ent : 0.f;
  }
}

}  // namespace

int ssc_attn_anc(const int64_t* words, const int64_t* backs, const int* ctl, const float* lp, int max_steps, int B, int SB,
                 int end_index, int* anc, hipStream_t st) {
  if (!words || !anc || max_steps <= 0 || B <= 0 || SB <= 0) return SSC_EINVAL;
  SSC_LAUNCH(attn_anc_kernel, dim3(ssc_cdiv(B * SB, 64)), dim3(64), 0, st, words, backs, ctl, lp, max_steps, B, SB, end_index, anc);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_attn_gather(const ssc_attn_gather_desc* d, void* stream) {
  if (!d || !d->hist || !d->anc) return SSC_EINVAL;
  if (!d->maps && !d->top_region && !d->top_weight && !d->entropy) return SSC_EINVAL;
  if (d->rows <= 0 || d->R <= 0 || d->steps <= 0 || d->n_caps <= 0 || d->n_sel <= 0) return SSC_EINVAL;
  if (d->maps && d->ld_maps < d->R) return SSC_EINVAL;
  if (!d->sel && d->n_sel != d->n_caps) return SSC_EINVAL;
  GatherArgs a;
  a.hist = d->hist; a.rows = d->rows; a.R = d->R; a.steps = d->steps;
  a.anc = d->anc; a.n_caps = d->n_caps;
  a.sel = d->sel; a.total = (long)d->n_sel * d->steps;
  a.maps = d->maps; a.ld_maps = d->ld_maps;
  a.top_region = d->top_region; a.top_weight = d->top_weight; a.entropy = d->entropy;
  const long nwg = (a.total + ATTN_ROWS - 1) / ATTN_ROWS;
  if (nwg > 0x7fffffffL) return SSC_EINVAL;
  const bool vec_in = (d->R & 3) == 0 && ssc_aligned16(d->hist);
  const bool vec_out = vec_in && (!d->maps || ((d->ld_maps & 3) == 0 && ssc_aligned16(d->maps)));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nwg), blk(64 * ATTN_ROWS);
  if (vec_out) SSC_LAUNCH((attn_gather_kernel<true, true>), grid, blk, 0, st, a);
  else if (vec_in) SSC_LAUNCH((attn_gather_kernel<true, false>), grid, blk, 0, st, a);
  else SSC_LAUNCH((attn_gather_kernel<false, false>), grid, blk, 0, st, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
