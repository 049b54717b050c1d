// Row-pass helpers shared by the word samplers (sample.hip, sched_sampling.hip through sample_draw.h), the sampled-node beam search
// (sampled_beam.hip) and the cuts in front of the draw (truncation.hip, mirostat.hip): the order-preserving key of a logit, the row
// view (LDS-staged or global), block reductions in a fixed order, the row passes every one of these kernels is built from - stage
// the row and take its maximum (row_stage_max), the tempered sums (row_tempered_sums), the write pass of a cut (row_write_kept) -,
// the radix select with integer-only LDS histograms that finds the top-k / top-p cut (ties at the cut: lower index first), and the
// host side of the two kernel forms: the LDS row's size and the launch that chooses between them (sample_row_launch).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssc_common.h"

namespace {

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_LDS_MAX_V = 32768;             // 128 KiB row in LDS (+ ~3 KiB of histograms) of the 160 KiB per CU
constexpr double SAMPLE_MASS_ONE = 1099511627776.0;  // 2^40: fixed-point scale of the top-p masses

// order-preserving key: a > b (floats, no NaN) <=> key(a) > key(b)
__device__ __forceinline__ uint32_t sample_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct SampleShared {
  uint32_t cnt[256];
  unsigned long long mass[256];
  float red[SAMPLE_WAVES];
  float bestv[SAMPLE_WAVES];
  int besti[SAMPLE_WAVES];
  uint32_t sel_key;
  int sel_found;
  unsigned long long sel_ahead, sel_w;
  uint32_t sel_cnt;
};

// block-wide max / sum in a fixed order (wave butterflies, then the waves in index order): the same result on every run
__device__ __forceinline__ float block_max(float v, SampleShared& sh) {
  v = ssc_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh.red[0];
  for (int w = 1; w < SAMPLE_WAVES; ++w) r = fmaxf(r, sh.red[w]);
  return r;
}
__device__ __forceinline__ float block_sum(float v, SampleShared& sh) {
  v = ssc_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh.red[0];
  for (int w = 1; w < SAMPLE_WAVES; ++w) r += sh.red[w];
  return r;
}
// block-wide integer min / sum in the same fixed order (the samplers' besti words carry the waves' parts)
__device__ __forceinline__ int block_min_int(int v, SampleShared& sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.besti[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = sh.besti[0];
  for (int w = 1; w < SAMPLE_WAVES; ++w) r = min(r, sh.besti[w]);
  return r;
}
__device__ __forceinline__ int block_sum_int(int v, SampleShared& sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.besti[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = sh.besti[0];
  for (int w = 1; w < SAMPLE_WAVES; ++w) r += sh.besti[w];
  return r;
}

// the row, four consecutive entries at a time (entries >= V read as -inf)
template <bool STAGED>
struct RowView {
  const float* g;   // global row
  const float* s;   // LDS row (STAGED)
  int V;
  bool vec;         // global row 16-byte aligned with V % 4 == 0
  __device__ __forceinline__ void get4(int j, float x[4]) const {
    const int v = 4 * j;
    if (STAGED) {
      if (v + 3 < V) {
        const float4 q = *reinterpret_cast<const float4*>(s + v);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        return;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = v + c < V ? s[v + c] : -INFINITY;
    } else {
      if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(g + v);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        return;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = v + c < V ? g[v + c] : -INFINITY;
    }
  }
  __device__ __forceinline__ float at(int v) const { return STAGED ? s[v] : g[v]; }
};

// The first pass of a row kernel: the row's maximum, the same in every thread, and - STAGED - the row's one read from HBM into srow
// ((V + 3) & ~3 floats of LDS, row.s); the global form reads the row once per pass instead.
template <bool STAGED>
__device__ __forceinline__ float row_stage_max(const RowView<STAGED>& row, float* srow, SampleShared& sh) {
  const int V = row.V;
  const int nj = (V + 3) >> 2;
  float mx = -INFINITY;
  if (STAGED) {
    const RowView<false> gv{row.g, nullptr, V, row.vec};
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4];
      gv.get4(j, x);
      if (4 * j + 3 < V) {
        *reinterpret_cast<float4*>(srow + 4 * j) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
        for (int c = 0; c < 4; ++c)
          if (4 * j + c < V) srow[4 * j + c] = x[c];
      }
      mx = fmaxf(fmaxf(mx, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
    }
  } else {
    for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
      float x[4];
      row.get4(j, x);
      mx = fmaxf(fmaxf(mx, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
    }
  }
  return block_max(mx, sh);   // (its barriers also publish srow)
}

// The tempered sums of a live row with maximum mx, over its finite entries (-inf, and the columns past V, weigh nothing and are
// never multiplied), a_v = (x_v - mx) / T: z = sum exp(a_v); ENTROPY: s1 = sum a_v exp(a_v) (else 0); want_first (workgroup-uniform):
// the lowest index at which x_v == mx (else 0x7fffffff).  The same in every thread.
struct RowSums { float z, s1; int first; };
template <bool STAGED, bool ENTROPY>
__device__ __forceinline__ RowSums row_tempered_sums(const RowView<STAGED>& row, float mx, float T, bool want_first, SampleShared& sh) {
  const int nj = (row.V + 3) >> 2;
  RowSums o{0.f, 0.f, 0x7fffffff};
  for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
    float x[4];
    row.get4(j, x);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (x[c] > -INFINITY) {
        const float av = (x[c] - mx) / T;
        const float e = expf(av);
        o.z += e;
        if (ENTROPY) o.s1 += e * av;
        if (want_first && x[c] == mx) o.first = min(o.first, 4 * j + c);
      }
    }
  }
  o.z = block_sum(o.z, sh);
  if (ENTROPY) o.s1 = block_sum(o.s1, sh);
  if (want_first) o.first = block_min_int(o.first, sh);
  return o;
}

// The write pass of a cut over the row at g (the row of `row`, writable): keep(v, x) is asked for every v < V with a finite x; a
// dropped entry becomes -inf.  With row.vec a kept entry is stored back with the bits it had (16-byte stores), without it only the
// dropped entries are stored: per element the same result.  Returns the thread's count of kept entries (block_sum_int it).
// (A predicate that joins two comparisons joins them with |: behind this call a || compiles to a divergent branch per element,
// measured at 1 to 4 % of the cut kernels' time.)
template <bool STAGED, typename F>
__device__ __forceinline__ int row_write_kept(const RowView<STAGED>& row, float* g, F&& keep) {
  const int V = row.V;
  const int nj = (V + 3) >> 2;
  int nkept = 0;
  for (int j = threadIdx.x; j < nj; j += SAMPLE_THREADS) {
    float x[4];
    row.get4(j, x);
    bool drop[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = 4 * j + c;
      bool k = false;
      if (v < V && x[c] > -INFINITY) k = keep(v, x[c]);
      drop[c] = !k;
      nkept += k ? 1 : 0;
    }
    if (row.vec) {
      *reinterpret_cast<float4*>(g + 4 * j) = make_float4(drop[0] ? -INFINITY : x[0], drop[1] ? -INFINITY : x[1],
                                                          drop[2] ? -INFINITY : x[2], drop[3] ? -INFINITY : x[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * j + c < V && drop[c]) g[4 * j + c] = -INFINITY;
    }
  }
  return nkept;
}

// One radix-select descent.  Every row entry v offers (active, key, weight); the entries are ranked by key DESCENDING.  Finds the
// first entry, in that order, at which the running weight (inclusive) reaches `thr` - restricted to keys; the result is its key,
// the weight strictly ahead of its key, and the count / weight of the entries that share its key.  found = 0: the total weight
// stays below thr.  MASS = false: every active entry weighs 1.
template <bool STAGED, bool MASS, typename F>
__device__ void radix_descent(const RowView<STAGED>& row, F&& offer, unsigned long long thr, SampleShared& sh) {
  const int lane = threadIdx.x & 63;
  uint32_t prefix = 0;
  unsigned long long ahead = 0;
  const int nj = (row.V + 3) >> 2;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t hi_mask = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
    for (int b = threadIdx.x; b < 256; b += SAMPLE_THREADS) { sh.cnt[b] = 0; sh.mass[b] = 0; }
    __syncthreads();
    for (int j0 = 0; j0 < nj; j0 += SAMPLE_THREADS) {   // (wave-uniform trip count: the ballots below see whole waves)
      const int j = j0 + (int)threadIdx.x;
      float x[4];
      if (j < nj) row.get4(j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int v = 4 * j + c;
        bool act = false;
        uint32_t key = 0;
        unsigned long long w = 1;
        if (j < nj && v < row.V) act = offer(v, x[c], key, w);
        act = act && (key & hi_mask) == prefix;
        const uint32_t bucket = (key >> shift) & 255u;
        // the most frequent case - the lanes of a wave share their bucket (logits cluster in a few exponents) - as ONE atomic
        // pair per wave: the first active lane's bucket is aggregated, the other lanes add their own
        const unsigned long long am = __ballot(act);
        if (am) {
          const int leader = __ffsll((long long)am) - 1;
          const uint32_t lb = __shfl(bucket, leader, 64);
          const bool mine = act && bucket == lb;
          const unsigned long long mm = __ballot(mine);
          const unsigned long long ws = MASS ? wave_sum_u64(mine ? w : 0ull) : 0ull;
          if (lane == leader) {
            atomicAdd(&sh.cnt[lb], (uint32_t)__popcll(mm));
            if (MASS) atomicAdd(&sh.mass[lb], ws);
          }
          if (act && !mine) {
            atomicAdd(&sh.cnt[bucket], 1u);
            if (MASS) atomicAdd(&sh.mass[bucket], w);
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // wave 0: lane l holds buckets 255 - 4l ... 252 - 4l; exclusive scan of the weights, descending
      unsigned long long wb[4];
      uint32_t cb[4];
      unsigned long long tot = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int b = 255 - 4 * lane - c;
        cb[c] = sh.cnt[b];
        wb[c] = MASS ? sh.mass[b] : (unsigned long long)cb[c];
        tot += wb[c];
      }
      unsigned long long incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      unsigned long long a = ahead + (incl - tot);
      int hit = -1;
      unsigned long long hit_ahead = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (hit < 0 && cb[c] > 0 && a + wb[c] >= thr) { hit = c; hit_ahead = a; }
        a += wb[c];
      }
      const unsigned long long hm = __ballot(hit >= 0);
      const int first = hm ? __ffsll((long long)hm) - 1 : -1;
      if (lane == (first < 0 ? 0 : first)) {
        sh.sel_found = first >= 0;
        if (first >= 0) {
          const int b = 255 - 4 * lane - hit;
          sh.sel_key = prefix | ((uint32_t)b << shift);
          sh.sel_ahead = hit_ahead;
          sh.sel_w = wb[hit];
          sh.sel_cnt = cb[hit];
        }
      }
    }
    __syncthreads();
    if (!sh.sel_found) return;
    prefix = sh.sel_key;
    ahead = sh.sel_ahead;
    __syncthreads();   // (sh.sel_* and the histograms are rewritten by the next pass)
  }
  // here sh.sel_key is the whole key of the cut, sh.sel_ahead the weight ahead of it, sh.sel_cnt / sh.sel_w its entries
}

// The cut of a top-k (kind 1) / top-p (kind 2) row: kept <=> key > cut_key, or key == cut_key and v <= cut_idx.  mx is the
// row's maximum, invz the inverse of its tempered normaliser sum_v exp((x_v - mx) / T) (read for top-p only).  Every thread
// returns the same cut; kind 0, top_k >= V and top_p >= 1 keep every entry.  (sample_draw_row in sample_draw.h, the draw of
// sample_rows_kernel, keeps this code inline: called as a function it is laid out differently, and the samplers' ISA is held fixed.)
template <bool STAGED>
__device__ __forceinline__ void sample_cut(const RowView<STAGED>& row, int kind, int top_k, float top_p, float mx, float T,
                                           float invz, SampleShared& sh, uint32_t& cut_key, int& cut_idx) {
  const bool topp = kind == 2 && top_p < 1.f;
  cut_key = 0;
  cut_idx = 0x7fffffff;   // (defaults: every entry kept)
  const bool topk = kind == 1 && top_k < row.V;
  if (topk || topp) {
    unsigned long long thr;
    bool found;
    if (topk) {
      thr = (unsigned long long)top_k;
      radix_descent<STAGED, false>(row, [&](int, float x, uint32_t& key, unsigned long long& w) {
        key = sample_key(x); w = 1; return true; }, thr, sh);
    } else {
      thr = (unsigned long long)llrint((double)top_p * SAMPLE_MASS_ONE);
      radix_descent<STAGED, true>(row, [&](int, float x, uint32_t& key, unsigned long long& w) {
        key = sample_key(x);
        w = (unsigned long long)llrintf(expf((x - mx) / T) * invz * 1099511627776.0f);
        return true; }, thr, sh);
    }
    found = sh.sel_found != 0;
    if (found) {
      cut_key = sh.sel_key;
      const unsigned long long ahead = sh.sel_ahead, wt = sh.sel_w;
      const uint32_t ct = sh.sel_cnt;
      // entries tied at the cut share one weight; the n-th of them (lowest index first) is the cut
      unsigned long long n;
      if (topk) n = thr - ahead;
      else {
        const unsigned long long each = wt / ct;
        n = (each == 0 || thr <= ahead) ? 1 : (thr - ahead + each - 1) / each;
      }
      n = n < 1 ? 1 : (n > ct ? ct : n);
      __syncthreads();
      if (n < ct) {
        const uint32_t ck = cut_key;
        radix_descent<STAGED, false>(row, [&](int v, float x, uint32_t& key, unsigned long long& w) {
          key = ~(uint32_t)v; w = 1; return sample_key(x) == ck; }, n, sh);
        cut_idx = (int)~sh.sel_key;
      }
      __syncthreads();
    }
  }
}

// dynamic LDS of a kernel that stages its row (V <= SAMPLE_LDS_MAX_V), raised past the 64 KiB default where the row needs it
template <typename K>
inline int sample_row_lds(K kernel, int V, size_t* lds) {
  *lds = (size_t)((V + 3) & ~3) * 4;
  if (*lds > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds) != hipSuccess)
    return SSC_EHIP;
  return SSC_OK;
}

// the launch of a row kernel, one workgroup of SAMPLE_THREADS per row: its LDS form for V <= SAMPLE_LDS_MAX_V, its global form above
template <typename A>
inline int sample_row_launch(void (*lds_form)(A), void (*global_form)(A), int V, int rows, hipStream_t st, const A& a) {
  if (V <= SAMPLE_LDS_MAX_V) {
    size_t lds;
    SSC_TRY(sample_row_lds(lds_form, V, &lds));
    SSC_LAUNCH(lds_form, dim3(rows), dim3(SAMPLE_THREADS), lds, st, a);
  } else {
    SSC_LAUNCH(global_form, dim3(rows), dim3(SAMPLE_THREADS), 0, st, a);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

}  // namespace
