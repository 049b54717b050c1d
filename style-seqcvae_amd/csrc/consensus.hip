// Consensus re-ranking on the device (Devlin et al. 2015, Mao et al. 2015; the "best-1 after consensus re-ranking" column of
// AG-CVAE / Seq-CVAE / COS-CVAE): the k nearest bank images of every query image by cosine similarity, then every candidate caption's
// mean CIDEr-D against the pooled references of those images, and the candidates' order by that score.
//
//   l2n_rows      one workgroup per row: x / |x| in one pass (the row's first 4096 entries stay in registers), fixed reduction order
//   knn_merge     one workgroup per query: the k largest of a (Q x Mc) chunk of similarities by the radix select of ssc_radix.h
//                 (order-preserving keys, integer LDS histograms, ties at the cut to the lower index), gathered into LDS and merged
//                 with the running sorted list by rank: entry e goes to slot #{entries ahead of e} under the strict order
//                 (similarity descending, bank index ascending).  The rank depends on the entries alone, so neither the gathering
//                 order nor the chunking shows in the result.  The similarities come from ssc_gemm (NT).
//   ec_score      one wave per candidate: its n-grams, tf and df weights once (ev_candidate), then the references of the listed
//                 images in list order, each staged through LDS (ev_cider_ref); fp64, one accumulation order
//   ec_order      one workgroup per query: the candidates by score, stable descending; pick = the first
// No float atomics; bad ids / lengths / neighbour indices raise a device flag (SSC_EINVAL) and are never used as an index.
#include "caption_common.h"
#include "ssc_radix.h"

namespace {

constexpr int KNN_MAX_K = 128;
constexpr int KNN_MAX_CHUNK = 1 << 22;   // columns of one chunk (a global row view: no LDS staging)
constexpr int L2N_THREADS = 256;
constexpr int L2N_REG = 4;               // float4 per thread kept in registers: rows up to 4096 entries are read once

// -0 -> +0 (they compare equal but their keys differ); NaN -> -inf (ranked after every number)
__device__ __forceinline__ float knn_canon(float x) {
  if (x == 0.f) return 0.f;
  return x == x ? x : -INFINITY;
}

// ---- rows to unit norm --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(L2N_THREADS) void l2n_rows(const float* x, int F, int ld, float* out, int ldo, int vec) {
  __shared__ float red[L2N_THREADS / 64];
  const float* xr = x + (size_t)blockIdx.x * ld;
  float* orow = out + (size_t)blockIdx.x * ldo;
  const int tid = threadIdx.x;
  float4 keep[L2N_REG];
  float s = 0.f;
  const int nv = vec ? F >> 2 : 0;
#pragma unroll
  for (int i = 0; i < L2N_REG; ++i) {
    const int j = tid + i * L2N_THREADS;
    keep[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nv) keep[i] = *reinterpret_cast<const float4*>(xr + 4 * j);
    s += keep[i].x * keep[i].x;
    s += keep[i].y * keep[i].y;
    s += keep[i].z * keep[i].z;
    s += keep[i].w * keep[i].w;
  }
  for (int j = tid + L2N_REG * L2N_THREADS; j < nv; j += L2N_THREADS) {
    const float4 q = *reinterpret_cast<const float4*>(xr + 4 * j);
    s += q.x * q.x; s += q.y * q.y; s += q.z * q.z; s += q.w * q.w;
  }
  for (int c = 4 * nv + tid; c < F; c += L2N_THREADS) s += xr[c] * xr[c];
  s = ssc_wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  float tot = red[0];
#pragma unroll
  for (int w = 1; w < L2N_THREADS / 64; ++w) tot += red[w];
  const float inv = tot > 0.f ? 1.f / sqrtf(tot) : 0.f;
#pragma unroll
  for (int i = 0; i < L2N_REG; ++i) {
    const int j = tid + i * L2N_THREADS;
    if (j < nv) *reinterpret_cast<float4*>(orow + 4 * j) = make_float4(keep[i].x * inv, keep[i].y * inv, keep[i].z * inv, keep[i].w * inv);
  }
  for (int j = tid + L2N_REG * L2N_THREADS; j < nv; j += L2N_THREADS) {
    const float4 q = *reinterpret_cast<const float4*>(xr + 4 * j);
    *reinterpret_cast<float4*>(orow + 4 * j) = make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
  }
  for (int c = 4 * nv + tid; c < F; c += L2N_THREADS) orow[c] = xr[c] * inv;
}

// ---- streaming top-k ------------------------------------------------------------------------------------------------------------

// entry a goes ahead of entry b: filled slots first, then similarity descending, then bank index ascending (slot index among the
// empty ones: they all end up behind the filled ones, in any order)
__device__ __forceinline__ bool knn_ahead(float sa, int ia, int ea, float sb, int ib, int eb) {
  const bool fa = ia >= 0, fb = ib >= 0;
  if (fa != fb) return fa;
  if (!fa) return ea < eb;
  if (sa != sb) return sa > sb;
  if (ia != ib) return ia < ib;
  return ea < eb;   // (a bank row fed in twice)
}

__global__ __launch_bounds__(SAMPLE_THREADS) void knn_merge(const float* sims, int ld, int Mc, int bank_offset, int k,
                                                           const int* exclude, float* best_sim, int* best_idx) {
  __shared__ SampleShared sh;
  __shared__ float cs[2 * KNN_MAX_K];
  __shared__ int ci[2 * KNN_MAX_K];
  __shared__ int taken;
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* g = sims + (size_t)p * ld;
  RowView<false> row{g, nullptr, Mc, ssc_aligned16_dev(g) && (Mc & 3) == 0};
  int ex = -1;   // the chunk column this query skips
  if (exclude) {
    const long long e = (long long)exclude[p] - bank_offset;
    if (e >= 0 && e < Mc) ex = (int)e;
  }
  const int active = Mc - (ex >= 0 ? 1 : 0);
  // slots 0..k-1: the running list; k..2k-1: this chunk's selection (empty until gathered)
  for (int e = tid; e < 2 * KNN_MAX_K; e += SAMPLE_THREADS) {
    const bool run = e < k;
    ci[e] = run ? best_idx[(size_t)p * k + e] : -1;
    cs[e] = run ? knn_canon(best_sim[(size_t)p * k + e]) : -INFINITY;
  }
  if (tid == 0) taken = 0;
  uint32_t cut_key = 0;
  int cut_idx = 0x7fffffff;   // (defaults: every active column is selected)
  if (active > k) {
    radix_descent<false, false>(row, [&](int v, float x, uint32_t& key, unsigned long long& w) {
      key = sample_key(knn_canon(x)); w = 1; return v != ex; }, (unsigned long long)k, sh);
    // active > k: the k-th largest exists
    cut_key = sh.sel_key;
    const unsigned long long n = (unsigned long long)k - sh.sel_ahead;   // columns with the cut's key that are kept, lowest first
    const uint32_t ct = sh.sel_cnt;
    __syncthreads();
    if (n < ct) {
      const uint32_t ck = cut_key;
      radix_descent<false, false>(row, [&](int v, float x, uint32_t& key, unsigned long long& w) {
        key = ~(uint32_t)v; w = 1; return v != ex && sample_key(knn_canon(x)) == ck; }, n, sh);
      cut_idx = (int)~sh.sel_key;
    }
  }
  __syncthreads();
  const int nj = (Mc + 3) >> 2;
  for (int j = tid; j < nj; j += SAMPLE_THREADS) {
    float x[4];
    row.get4(j, x);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = 4 * j + c;
      if (v >= Mc || v == ex) continue;
      const float y = knn_canon(x[c]);
      const uint32_t key = sample_key(y);
      if (key > cut_key || (key == cut_key && v <= cut_idx)) {
        const int at = atomicAdd(&taken, 1);   // (integer, LDS: the slot order does not reach the result)
        if (at < k) { cs[k + at] = y; ci[k + at] = bank_offset + v; }
      }
    }
  }
  __syncthreads();
  // rank of every entry among the 2k; the first k are the new running list
  for (int e = tid; e < 2 * k; e += SAMPLE_THREADS) {
    const float s = cs[e];
    const int i = ci[e];
    int rank = 0;
    for (int o = 0; o < 2 * k; ++o) rank += o != e && knn_ahead(cs[o], ci[o], o, s, i, e);
    if (rank < k) {
      best_sim[(size_t)p * k + rank] = i >= 0 ? s : -INFINITY;
      best_idx[(size_t)p * k + rank] = i;
    }
  }
}

// ---- consensus scores -----------------------------------------------------------------------------------------------------------

struct EcArgs {
  const int64_t* pred; int N, steps, boundary, V, I, nref, W, k;
  const int* id_map; const int* neighbours; const int* ref_off;
  double* scores; int* pool_refs; int* pick; int* order; int* flag;
};

__global__ __launch_bounds__(64) void ec_score(EcArgs a, EvState st) {
  __shared__ int ot[EV_L], ct[EV_L];
  __shared__ unsigned long long sk[EV_NG];
  __shared__ double sw[EV_NG];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int p = row / a.N;
  EvCand c;
  ev_candidate(a.pred + (size_t)row * a.steps, a.steps, a.boundary, a.V, a.id_map, a.W, true, a.I, st, a.flag, ot, ct, c);
  const int* nb = a.neighbours + (size_t)p * a.k;
  double cid[4] = {0.0, 0.0, 0.0, 0.0};
  int pool = 0;
  for (int s = 0; s < a.k; ++s) {
    const int img = nb[s];
    if (img == -1) continue;
    if (img < 0 || img >= a.I) { if (lane == 0) a.flag[0] = 1; continue; }
    const int lo = a.ref_off[img], hi = a.ref_off[img + 1];
    if (lo < 0 || hi > a.nref || hi <= lo) { if (lane == 0) a.flag[0] = 1; continue; }
    for (int r = lo; r < hi; ++r) {
      const size_t b = 4 * (size_t)st.base[r];
      const int nr = min(st.nu[r], EV_NG), lr = min(st.len[r], EV_L);   // (<= 4 len and <= 64 as ev_ref_ngrams wrote them)
      __syncthreads();   // the previous reference's LDS reads are done
      for (int e = lane; e < nr; e += 64) { sk[e] = st.key[b + e]; sw[e] = st.w[b + e]; }
      __syncthreads();
      double v[4];
      int x[4];
      ev_cider_ref(c, sk, sw, nr, lr, st.norm + 4 * (size_t)r, v, x);
#pragma unroll
      for (int o = 0; o < 4; ++o) cid[o] += v[o];
    }
    pool += hi - lo;
  }
  if (lane == 0) {
    if (pool == 0) a.flag[0] = 1;   // a query without one valid neighbour
    a.scores[row] = pool > 0 ? (((cid[0] + cid[1]) + cid[2]) + cid[3]) / 4.0 / (double)pool * 10.0 : 0.0;
    if (row == p * a.N) a.pool_refs[p] = pool;
  }
}

__global__ __launch_bounds__(EV_MAX_N) void ec_order(EcArgs a) {
  __shared__ double sc[EV_MAX_N];
  const int p = blockIdx.x, n = threadIdx.x;
  if (n < a.N) sc[n] = a.scores[(size_t)p * a.N + n];
  __syncthreads();
  if (n >= a.N) return;
  // stable descending: rank = #{j : c_j > c_n, or c_j == c_n and j < n}
  const double c = sc[n];
  int rank = 0;
  for (int j = 0; j < a.N; ++j) rank += sc[j] > c || (sc[j] == c && j < n);
  a.order[(size_t)p * a.N + rank] = n;
  if (rank == 0) a.pick[p] = n;
}

bool ec_desc_ok(const ssc_eval_consensus_desc* d) {
  return d && d->P >= 1 && d->N >= 1 && d->N <= EV_MAX_N && d->steps >= 1 && d->V >= 1 && d->V <= 65535 && d->k >= 1 &&
         d->k <= KNN_MAX_K && (int64_t)d->P * d->N <= (1 << 24) && d->predictions && d->id_map && d->neighbours && d->scores &&
         d->pool_refs && d->pick && d->order;
}

}  // namespace

extern "C" int ssc_l2_normalize_rows(const float* x, int rows, int F, int ld, float* out, int ldo, void* stream) {
  if (!x || !out || rows < 1 || F < 1 || ld < F || ldo < F) return SSC_EINVAL;
  if ((((uintptr_t)x) & 3u) || (((uintptr_t)out) & 3u)) return SSC_EALIGN;
  const int vec = ssc_aligned16(x) && ssc_aligned16(out) && !(ld & 3) && !(ldo & 3);
  SSC_LAUNCH(l2n_rows, dim3(rows), dim3(L2N_THREADS), 0, (hipStream_t)stream, x, F, ld, out, ldo, vec);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_knn_merge(const float* sims, int ld, int Q, int Mc, int bank_offset, int k, const int* exclude, float* best_sim,
                             int* best_idx, void* stream) {
  if (!sims || !best_sim || !best_idx || Q < 1 || Mc < 1 || Mc > KNN_MAX_CHUNK || ld < Mc || k < 1 || k > KNN_MAX_K ||
      bank_offset < 0 || (int64_t)bank_offset + Mc > 0x7fffffff)
    return SSC_EINVAL;
  SSC_LAUNCH(knn_merge, dim3(Q), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, sims, ld, Mc, bank_offset, k, exclude, best_sim,
             best_idx);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" size_t ssc_eval_consensus_workspace_bytes(const ssc_eval_refs* r, const ssc_eval_consensus_desc* d) {
  if (!ev_refs_ok(r) || !ec_desc_ok(d)) return 0;
  return 256;
}

extern "C" int ssc_eval_consensus(const ssc_eval_refs* r, const ssc_eval_consensus_desc* d, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!ev_refs_ok(r) || !ec_desc_ok(d)) return SSC_EINVAL;
  if (r->state_bytes < ev_layout(r->I, r->nref, r->ntok).total || !workspace || workspace_bytes < 256) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const EvState s = ev_state(r);
  EcArgs a{d->predictions, d->N, d->steps, d->boundary_index, d->V, r->I, r->nref, r->W, d->k, d->id_map, d->neighbours,
           r->ref_offsets, d->scores, d->pool_refs, d->pick, d->order, (int*)workspace};
  if (hipMemsetAsync(workspace, 0, sizeof(int), st) != hipSuccess) return SSC_EHIP;
  SSC_LAUNCH(ec_score, dim3(d->P * d->N), dim3(64), 0, st, a, s);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(ec_order, dim3(d->P), dim3(EV_MAX_N), 0, st, a);
  SSC_CHECK_LAUNCH();
  return ev_read_flag(a.flag, st);
}
