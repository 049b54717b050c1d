// Arithmetic sampling for the word samplers (ssc_arith, include/ssc.h; Vilnis et al., ICML 2023, "Arithmetic Sampling: Parallel Diverse
// Decoding for Large Language Models"): every caption decodes along a code point in [0, 1) - a uint64 c, meaning c / 2^64 - by inverse
// CDF in vocabulary order, the code renormalised into the chosen word's interval after every step.  It replaces only the DRAW of the
// sampled decode; like Mirostat it carries one value per row from step to step.
//   ssc_arith_codes   the codes of a call: per image a randomly shifted lattice, row i N + j at u_i + floor(j 2^64 / N) (mod 2^64),
//                     u_i words 0 (low) and 1 (high) of Philox4x32-10 at counter (0, 0, i, SSC_ARITH_PHILOX_STREAM), key = the seed;
//   ssc_arith_rows    the draw of one step: of a row of RAW logits, behind every edit, the word whose interval of the kept set's
//                     integer masses holds the row's code, and the code inside that interval.
// ssc_decode_sample_arith (sample.hip) issues the draw in place of sample_rows_kernel's launch; nothing else of the step knows of it.
// One workgroup of SAMPLE_THREADS per row, the row staged in LDS once for V <= SAMPLE_LDS_MAX_V, every pass over global memory above
// that.  The passes of a live row:
//   1. row_stage_max: the maximum mx (and, STAGED, the copy into LDS);
//   2. the untempered log-sum-exp (the returned log-prob) and, for top-p, the tempered normaliser - the loop of sample_draw_row, so
//      that pass 3 is handed the bits the plain samplers hand it;
//   3. sample_cut: the top-k / top-p cut, the kept set of ssc_sample_rows;
//   4. the masses w_v = llrintf(expf((x_v - mx) / T) 2^40) of the kept entries, 0 for the others, summed to W in 64-bit integers, and
//      the fall-back word (the lowest-index kept maximum);  t = hi64(c W), lo = lo64(c W);
//   5. the walk in vocabulary order in tiles of SAMPLE_THREADS quads: a 64-bit inclusive wave scan of the quads' masses by __shfl_up,
//      the wave totals through LDS (two sets, so one barrier per tile), a running base across the tiles; the ONE lane whose quad
//      holds t publishes (v, cum(v), w_v); the masses go to mass_out on the way;
//   6. thread 0: c' = floor(((t - cum(v)) 2^64 + lo) / w_v) by a 64-step shift-subtract division - the remainder stays below
//      2 w_v <= 2^41, so 64-bit words suffice - and the writes; then the early-stop protocol of sample_rows_kernel (sample_step_done).
// Everything that decides a word is integer arithmetic on masses that are a pure function of (x_v, mx, T): no float atomics, no
// order-dependent float reduction - two calls on equal inputs are bit-identical, and a host that is handed the masses (mass_out) can
// restate token and code bit for bit (tests/arithref.py).  NaN and +inf are the caller's error: a mass that is not a positive number
// counts as 0, every trip count depends on V alone, every index is a loop index; if no lane claims t (W == 0) the fall-back word is
// emitted and the code passes through.
#include <math.h>

#include "sample_draw.h"

namespace {

// the last Philox counter word of the lattice shifts: "ARIT".  The other streams of the library use 0 (the word draws of
// sample_draw.h, sbs.hip), 1 (the scheduled-sampling coin of sched_sampling.hip) and the draw index 0 .. 31 (sampled_beam.hip).
constexpr uint32_t SSC_ARITH_PHILOX_STREAM = 0x41524954u;

struct ArithArgs {
  const float* logits; size_t ld; int V;
  int kind, top_k; float top_p, temperature;
  const unsigned long long* code_in; unsigned long long* code_out;
  const int64_t* last_pred; float* row_lp; int end_index;
  int64_t* pred_out; float* lp_out; long long* mass_out;
  int step; int* ctl; int max_steps; int* host_flag;
};

struct ArithHit { int v; unsigned long long cum, w; };

template <bool STAGED>
__global__ __launch_bounds__(SAMPLE_THREADS) void arith_rows_kernel(ArithArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ SampleShared sh;
  __shared__ unsigned long long wtot[2][SAMPLE_WAVES];
  __shared__ ArithHit hit;
  const int r = blockIdx.x;
  const int V = a.V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool stopped = a.ctl && a.ctl[0] <= a.step;   // (written by an EARLIER launch of this stream: the decode has ended)
  const bool ended = stopped || (a.last_pred && a.last_pred[r] == a.end_index);   // workgroup-uniform
  const unsigned long long code = a.code_in[r];
  unsigned long long code2 = code;
  int64_t tok = a.end_index;
  float lp = 0.f;
  long long* mo = a.mass_out ? a.mass_out + (size_t)r * V : nullptr;
  if (!ended) {
    const float* g = a.logits + (size_t)r * a.ld;
    const RowView<STAGED> row{g, srow, V, ssc_aligned16_dev(g) && (V & 3) == 0};
    const int nj = (V + 3) >> 2;
    const float T = a.temperature;
    // ---- 1. stage the row (once from HBM) and its maximum -------------------------------------------------------------------
    const float mx = row_stage_max(row, srow, sh);
    // ---- 2. untempered log-sum-exp and the tempered normaliser (top-p masses), as sample_draw_row forms them -------------------
    const bool topp = a.kind == 2 && a.top_p < 1.f;
    float s = 0.f, st = 0.f;
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4];
      row.get4(j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s += expf(x[c] - mx);
        if (topp) st += expf((x[c] - mx) / T);
      }
    }
    s = block_sum(s, sh);
    const float lse = mx + logf(s);
    float invz = 0.f;
    if (topp) invz = 1.f / block_sum(st, sh);
    // ---- 3. the cut: kept <=> key > cut_key, or key == cut_key and v <= cut_idx ------------------------------------------------
    uint32_t cut_key;
    int cut_idx;
    sample_cut(row, a.kind, a.top_k, a.top_p, mx, T, invz, sh, cut_key, cut_idx);
    // the masses of quad j (entries past V, cut entries, -inf and anything that is not a positive number: 0)
    auto mass4 = [&](int j, const float x[4], unsigned long long w[4]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int v = 4 * j + c;
        const uint32_t key = sample_key(x[c]);
        const bool kept = (v < V) & ((key > cut_key) | ((key == cut_key) & (v <= cut_idx)));
        const float e = expf((x[c] - mx) / T);
        w[c] = (kept & (e > 0.f)) ? (unsigned long long)llrintf(e * 1099511627776.0f) : 0ull;
      }
    };
    // ---- 4. W, and the fall-back word: the lowest-index kept maximum -----------------------------------------------------------
    unsigned long long part = 0;
    int fb = 0x7fffffff;
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4];
      unsigned long long w[4];
      row.get4(j, x);
      mass4(j, x, w);
      part += (w[0] + w[1]) + (w[2] + w[3]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int v = 4 * j + c;
        const uint32_t key = sample_key(x[c]);
        const bool kept = (v < V) & ((key > cut_key) | ((key == cut_key) & (v <= cut_idx)));
        if (kept & (x[c] == mx)) fb = min(fb, v);
      }
    }
    fb = block_min_int(fb, sh);
    part = wave_sum_u64(part);
    __syncthreads();
    if (lane == 0) sh.mass[wave] = part;
    if (threadIdx.x == 0) hit.v = -1;
    __syncthreads();
    unsigned long long W = 0;
    for (int k = 0; k < SAMPLE_WAVES; ++k) W += sh.mass[k];
    const unsigned long long t = __umul64hi(code, W), lo = code * W;
    // ---- 5. the walk in vocabulary order: which word's interval [cum(v), cum(v) + w_v) holds t -----------------------------------
    unsigned long long base = 0;
    int p = 0;
    for (int j0 = 0; j0 < nj; j0 += SAMPLE_THREADS, p ^= 1) {   // (workgroup-uniform trip count)
      const int j = j0 + (int)threadIdx.x;
      unsigned long long w[4] = {0ull, 0ull, 0ull, 0ull};
      if (j < nj) {
        float x[4];
        row.get4(j, x);
        mass4(j, x, w);
      }
      const unsigned long long q = (w[0] + w[1]) + (w[2] + w[3]);
      unsigned long long incl = q;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      if (lane == 63) wtot[p][wave] = incl;
      __syncthreads();   // (one per tile: the set written two tiles on is read by nobody behind the barrier in between)
      unsigned long long cum = base + (incl - q), tile = 0;
#pragma unroll
      for (int k = 0; k < SAMPLE_WAVES; ++k) {
        const unsigned long long u = wtot[p][k];
        if (k < wave) cum += u;
        tile += u;
      }
      base += tile;
      if (mo && j < nj) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * j + c < V) mo[4 * j + c] = (long long)w[c];
      }
      if (t >= cum && t - cum < q) {   // this quad's interval holds t: at most one lane of the workgroup
        bool done = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (!done && t - cum < w[c]) {
            hit.v = 4 * j + c; hit.cum = cum; hit.w = w[c];
            done = true;
          }
          if (!done) cum += w[c];
        }
      }
    }
    __syncthreads();
    // ---- 6. the word, its untempered log-prob and the code inside the word's interval ---------------------------------------
    int v = W != 0 ? hit.v : -1;
    if (v >= 0) {
      if (threadIdx.x == 0) {
        const unsigned long long wv = hit.w;
        unsigned long long rem = t - hit.cum, quo = 0;   // rem < wv <= 2^40
        for (int i = 63; i >= 0; --i) {
          rem = (rem << 1) | ((lo >> i) & 1ull);
          quo <<= 1;
          if (rem >= wv) { rem -= wv; quo |= 1ull; }
        }
        code2 = quo;
      }
    } else {
      v = fb == 0x7fffffff ? -1 : fb;   // (no word claims t - W == 0: the code passes through)
    }
    tok = v;
    lp = v >= 0 ? row.at(v) - lse : 0.f;
  } else if (mo) {
    for (int v = threadIdx.x; v < V; v += SAMPLE_THREADS) mo[v] = v == a.end_index ? (long long)SAMPLE_MASS_ONE : 0ll;
  }
  if (threadIdx.x == 0) {
    a.pred_out[r] = tok;
    a.lp_out[r] = lp;
    if (a.row_lp) a.row_lp[r] += lp;
    a.code_out[r] = code2;
  }
  if (a.ctl && threadIdx.x == 0) sample_step_done(a.ctl, a.max_steps, a.host_flag, a.step, stopped, tok != a.end_index);
}

// one thread per row: 2^64 = qN N + rN, so floor(j 2^64 / N) = j qN + floor(j rN / N) with j rN < N^2 <= 2^48
__global__ __launch_bounds__(256) void arith_codes_kernel(uint32_t seed_lo, uint32_t seed_hi, int nimg, int N,
                                                          unsigned long long* __restrict__ code) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (long)nimg * N) return;
  const uint32_t i = (uint32_t)(b / N), j = (uint32_t)(b % N);
  uint32_t ctr[4] = {0u, 0u, i, SSC_ARITH_PHILOX_STREAM};
  philox4x32_10(ctr, seed_lo, seed_hi);
  const unsigned long long u = ((unsigned long long)ctr[1] << 32) | ctr[0];
  unsigned long long qN = ~0ull / (unsigned long long)N, rN = ~0ull % (unsigned long long)N + 1ull;
  if (rN == (unsigned long long)N) { qN += 1ull; rN = 0ull; }   // (N == 1: qN wraps to 0, and j is 0)
  code[b] = u + (unsigned long long)j * qN + (unsigned long long)j * rN / (unsigned long long)N;
}

}  // namespace

int ssc_arith_check(const ssc_arith* a, bool* active) {
  *active = false;
  if (!a) return SSC_OK;
  if (a->mode < 0 || a->mode > 2) return SSC_EINVAL;
  if (a->mode == 0) return SSC_OK;   // off: nothing else is read
  if (!a->code) return SSC_EINVAL;
  if (((uintptr_t)a->code & 7u) != 0) return SSC_EALIGN;
  *active = true;
  return SSC_OK;
}

int ssc_arith_codes_launch(uint64_t seed, int nimg, int n_samples, uint64_t* code_out, hipStream_t st) {
  const long B = (long)nimg * n_samples;
  if (B <= 0) return SSC_OK;
  SSC_LAUNCH(arith_codes_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
             nimg, n_samples, (unsigned long long*)code_out);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

int ssc_arith_rows_launch(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const uint64_t* code_in,
                          const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out, uint64_t* code_out,
                          int64_t* mass_out, int step, int* ctl, int max_steps, int* host_flag, hipStream_t st) {
  ArithArgs a{};
  a.logits = logits; a.ld = (size_t)ld; a.V = V;
  a.kind = s->kind; a.top_k = s->top_k; a.top_p = s->top_p; a.temperature = s->temperature;
  a.code_in = (const unsigned long long*)code_in; a.code_out = (unsigned long long*)code_out;
  a.last_pred = last_pred; a.row_lp = row_lp; a.end_index = end_index;
  a.pred_out = pred_out; a.lp_out = lp_out; a.mass_out = (long long*)mass_out;
  a.step = step; a.ctl = ctl; a.max_steps = max_steps; a.host_flag = host_flag;
  return sample_row_launch(arith_rows_kernel<true>, arith_rows_kernel<false>, V, rows, st, a);
}

extern "C" int ssc_arith_codes(uint64_t seed, int nimg, int n_samples, uint64_t* code_out, void* stream) {
  if (!code_out || nimg < 0 || n_samples < 1 || n_samples > (1 << 24) || (long)nimg * n_samples > (1L << 31)) return SSC_EINVAL;
  if (((uintptr_t)code_out & 7u) != 0) return SSC_EALIGN;
  return ssc_arith_codes_launch(seed, nimg, n_samples, code_out, (hipStream_t)stream);
}

extern "C" int ssc_arith_rows(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const uint64_t* code_in,
                              const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out,
                              uint64_t* code_out, int64_t* mass_out, void* stream) {
  if (!logits || !code_in || !pred_out || !lp_out || !code_out || rows < 0 || V < 1 || ld < V || !sampler_ok(s, V)) return SSC_EINVAL;
  if (last_pred && (end_index < 0 || end_index >= V)) return SSC_EINVAL;
  if (((uintptr_t)code_in & 7u) != 0 || ((uintptr_t)code_out & 7u) != 0 || ((uintptr_t)mass_out & 7u) != 0) return SSC_EALIGN;
  if (rows == 0) return SSC_OK;
  return ssc_arith_rows_launch(logits, ld, rows, V, s, code_in, last_pred, row_lp, end_index, pred_out, lp_out, code_out, mass_out, 0,
                               nullptr, 0, nullptr, (hipStream_t)stream);
}
