// Selection helpers shared by the beam-search kernels (decode.hip, fsm.hip, diverse_beam.hip, rules_beam.hip).  Selection order
// everywhere: value descending,
// index ascending ("k-pass selection": pass k finds the best candidate strictly after the previous pick in that order).
#pragma once
#include "ssc_common.h"

namespace {

struct Cand {
  float v;
  int i;
};
__device__ __forceinline__ bool better(float v, int i, const Cand& o) {  // (v,i) ranks before o
  return (v > o.v) || (v == o.v && i < o.i);
}
__device__ __forceinline__ bool after(float v, int i, const Cand& prev) {  // (v,i) ranks strictly after the previous pick
  return (prev.i < 0) || (v < prev.v) || (v == prev.v && i > prev.i);
}
__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand t;
    t.v = __shfl_xor(c.v, o, 64);
    t.i = __shfl_xor(c.i, o, 64);
    if (t.i >= 0 && (c.i < 0 || better(t.v, t.i, c))) c = t;
  }
  return c;
}
__device__ __forceinline__ Cand block_best(Cand c, Cand* sh) {
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  c = wave_best(c);
  __syncthreads();
  if (lane == 0) sh[wv] = c;
  __syncthreads();
  Cand r = sh[0];
  for (int k = 1; k < nw; ++k)
    if (sh[k].i >= 0 && (r.i < 0 || better(sh[k].v, sh[k].i, r))) r = sh[k];
  return r;
}

// One-barrier forms for kernels that run several reductions in a row: consecutive reductions alternate between two LDS slots
// (`par` = 0, 1, 0, ...), so the write of reduction n + 1 cannot overtake a slow wave's read of reduction n - 1's slot (there is a
// barrier of reduction n in between), and the leading barrier of the two-barrier forms is not needed.  Same arithmetic and order.
__device__ __forceinline__ Cand block_best1(Cand c, Cand (*sh)[4], int par) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  c = wave_best(c);
  if (lane == 0) sh[par][wv] = c;
  __syncthreads();
  Cand r = sh[par][0];
  for (int k = 1; k < nw; ++k)
    if (sh[par][k].i >= 0 && (r.i < 0 || better(sh[par][k].v, sh[par][k].i, r))) r = sh[par][k];
  return r;
}
__device__ __forceinline__ float dec_block_reduce1(float v, float (*sh)[4], int par, bool is_max) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = is_max ? ssc_wave_max(v) : ssc_wave_sum(v);
  if (lane == 0) sh[par][wv] = v;
  __syncthreads();
  float r = sh[par][0];
  for (int i = 1; i < nw; ++i) r = is_max ? fmaxf(r, sh[par][i]) : r + sh[par][i];
  return r;
}

// (the two-barrier float reduction is ssc_block_reduce of ssc_common.h: the function log_softmax_kernel itself calls)

// ---- pieces of the selections that take a whole row per workgroup of 256 (diverse_beam.hip, rules_beam.hip) ---------------------

constexpr int BEAM_ROW_NV = 40;   // V <= 256 * 40: the row in registers (decode.hip: beam_row_topk_reg_kernel)

// A row's log-sum-exp with the arithmetic and the thread ownership of log_softmax_kernel (thread t owns tokens t, t + 256, ...):
// row - lse is bit-equal to ssc_log_softmax.  REG: the row is loaded into x and x - lse is left there (NORM false: x as loaded);
// otherwise x is not touched and the caller subtracts the returned lse from what it reads.  shr: 16 floats of LDS.
template <bool NORM, bool REG>
__device__ __forceinline__ float beam_row_lse(const float* __restrict__ row, int V, float (&x)[REG ? BEAM_ROW_NV : 1], float* shr) {
  const int t = threadIdx.x;
  float lse = 0.f;
  if (REG) {
#pragma unroll
    for (int u = 0; u < BEAM_ROW_NV; ++u) x[u] = row[min(t + u * 256, V - 1)];
    if (NORM) {
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u)
        if (t + u * 256 < V) mx = fmaxf(mx, x[u]);
      mx = ssc_block_reduce(mx, shr, true);
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u)
        if (t + u * 256 < V) sum += expf(x[u] - mx);
      sum = ssc_block_reduce(sum, shr, false);
      lse = mx + logf(sum);
#pragma unroll
      for (int u = 0; u < BEAM_ROW_NV; ++u) x[u] -= lse;
    }
  } else if (NORM) {   // thread t owns v = t, t + 256, ...: the order of log_softmax_kernel
    float mx = -INFINITY;
    for (int v = t; v < V; v += 256) mx = fmaxf(mx, row[v]);
    mx = ssc_block_reduce(mx, shr, true);
    float sum = 0.f;
    for (int v = t; v < V; v += 256) sum += expf(row[v] - mx);
    sum = ssc_block_reduce(sum, shr, false);
    lse = mx + logf(sum);
  }
  return lse;
}

// The early-stop tail of a merge kernel that runs one workgroup per batch entry (the protocol of ssc_beam_desc.ctl): one thread of
// every workgroup calls it with the number of beams of its entry that have not ended.  The last workgroup of the step to get here
// stops the search when there are none, and notes the step's completion in the progress word (the one-call searches queue step t
// only once step t - 2 has got here: their run-ahead bound).
__device__ __forceinline__ void beam_early_stop_tail(int* ctl, int* host_flag, int step_index, int max_steps, int live, bool stopped) {
  int* cnt = ctl + 2 + step_index;
  int* ticket = ctl + 2 + max_steps + step_index;
  if (live) atomicAdd(cnt, live);
  __threadfence();
  const int done = atomicAdd(ticket, 1);
  if (done == (int)gridDim.x - 1) {   // the last workgroup of this step
    if (!stopped) {
      __threadfence();
      if (atomicAdd(cnt, 0) == 0) {
        atomicMin(ctl, step_index + 1);
        if (host_flag) __hip_atomic_store(host_flag, step_index + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (host_flag) __hip_atomic_store(host_flag + 1, step_index, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace
