// Pieces shared by the caption evaluation kernels (caption_eval.hip: scores against an image's own references, caption-set
// diversity) and the consensus re-ranking (consensus.hip: scores against the pooled references of a list of prepared images): the
// prepared-reference state ssc_eval_prepare_refs writes, the n-gram key helpers, a candidate's own n-grams with their CIDEr weights
// (ev_candidate) and its CiderScorer similarity to one reference staged in LDS (ev_cider_ref).
#pragma once
#include "ssc_common.h"

namespace {

constexpr int EV_L = 64;                  // tokens per caption (references and candidates)
constexpr int EV_NG = 4 * EV_L;           // n-gram slots per caption
constexpr int EV_MAX_N = 128;             // samples per image
constexpr int EV_DIV_SLOTS = 16384;       // LDS hash set of ev_image: >= 2 x EV_MAX_N x EV_L occurrences
constexpr unsigned EV_EMPTY = 0xffffffffu;
constexpr int EV_NSCORE = 6, EV_NCOUNT = 10, EV_NIMG = 9;

struct EvLayout {
  size_t key, hkey, w, norm, tf, nu, len, base, rstyle, hdf, flag, total;
  unsigned long long T;
};

EvLayout ev_layout(int I, int nref, int ntok) {
  EvLayout l;
  const size_t S = 4 * (size_t)ntok;
  unsigned long long T = 64;
  while (T < 2 * S) T <<= 1;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = ssc_round_up(o + bytes, 256); return at; };
  l.key = take(S * 8); l.hkey = take(T * 8); l.w = take(S * 8); l.norm = take((size_t)nref * 4 * 8); l.tf = take(S * 4);
  l.nu = take((size_t)nref * 4); l.len = take((size_t)nref * 4); l.base = take((size_t)nref * 4); l.rstyle = take((size_t)I * 4);
  l.hdf = take(T * 4); l.flag = take(4);
  l.total = o; l.T = T;
  return l;
}

struct EvState {
  unsigned long long* key; unsigned long long* hkey; double* w; double* norm; int* tf; int* nu; int* len; int* base; int* rstyle;
  int* hdf; int* flag; unsigned long long mask;
};

EvState ev_state(const ssc_eval_refs* r) {
  const EvLayout l = ev_layout(r->I, r->nref, r->ntok);
  char* b = (char*)r->state;
  return {(unsigned long long*)(b + l.key), (unsigned long long*)(b + l.hkey), (double*)(b + l.w), (double*)(b + l.norm),
          (int*)(b + l.tf), (int*)(b + l.nu), (int*)(b + l.len), (int*)(b + l.base), (int*)(b + l.rstyle), (int*)(b + l.hdf),
          (int*)(b + l.flag), l.T - 1};
}

__device__ __forceinline__ int ev_count(int L) {
  int n = 0;
#pragma unroll
  for (int k = 1; k <= 4; ++k) n += L - k + 1 > 0 ? L - k + 1 : 0;
  return n;
}
// slot j of a caption of L tokens -> order k (1..4) and start s: the orders' n-grams are laid out one after the other
__device__ __forceinline__ void ev_split(int j, int L, int& k, int& s) {
  k = 1;
  int c = L;
  while (j >= c && k < 4) { j -= c; ++k; c = L - k + 1; }
  s = j;
}
__device__ __forceinline__ int ev_order(unsigned long long key) {
  return (key >> 48) ? 4 : (key >> 32) ? 3 : (key >> 16) ? 2 : 1;
}
__device__ __forceinline__ unsigned long long ev_mix(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}
__device__ __forceinline__ unsigned ev_mix32(unsigned k) {
  k ^= k >> 16; k *= 0x7feb352dU; k ^= k >> 15; k *= 0x846ca68bU; k ^= k >> 16;
  return k;
}
// index of `k` among the n sorted keys at `a`, or -1
__device__ __forceinline__ int ev_find(const unsigned long long* a, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < k) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == k) ? lo : -1;
}
__device__ __forceinline__ int ev_df(const unsigned long long* hkey, const int* hdf, unsigned long long mask, unsigned long long k) {
  unsigned long long h = ev_mix(k) & mask;
  for (unsigned long long p = 0; p <= mask; ++p) {
    const unsigned long long s = hkey[h];
    if (s == k) return hdf[h];
    if (s == 0ull) return 0;
    h = (h + 1) & mask;
  }
  return 0;
}
__device__ __forceinline__ double ev_wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int ev_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

bool ev_refs_ok(const ssc_eval_refs* r) {
  return r && r->I >= 1 && r->I <= (1 << 24) && r->nref >= r->I && r->nref <= (1 << 26) && r->ntok >= r->nref &&
         r->ntok <= (1 << 26) && r->W >= 1 && r->W <= 65535 && r->ref_offsets && r->tok_offsets && r->tokens && r->state;
}

int ev_read_flag(const int* flag, hipStream_t st) {
  int h = 0;
  if (hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return SSC_EHIP;
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { ssc_tls_hip_error = (int)e; return SSC_EHIP; }
  return h ? SSC_EINVAL : SSC_OK;
}

// ---- one candidate, one wave ----------------------------------------------------------------------------------------------------

// A candidate's own n-grams as the lanes of its wave hold them: slot lane + 64 q is n-gram q of this lane; tf > 0 only at a distinct
// n-gram's first occurrence (compared on the original ids); key 0 = an n-gram with a word in no reference.
struct EvCand {
  int L;                    // tokens (cut at the first boundary_index, at most EV_L)
  int tfc[4], ordc[4];
  unsigned long long ck[4];
  double wc[4];             // tf (log I - log max(1, df))
  double normc[4];          // per-order norms, the same in every lane
};

// Row `pr` of the prediction tensor -> its tokens in LDS (ot: original ids, ct: compact ids; EV_L entries each) and its n-grams.
// Bad ids and rows of more than EV_L tokens raise `flag` and are clamped.  scored = false: no df lookups (every weight is tf log I).
// Called by the whole 64-thread workgroup.
__device__ __forceinline__ void ev_candidate(const int64_t* pr, int steps, int boundary, int V, const int* id_map, int W, bool scored,
                                             int I, const EvState& st, int* flag, int* ot, int* ct, EvCand& c) {
  const int lane = threadIdx.x;
  // length: the first boundary_index, else the full row
  int L = steps;
  for (int c0 = 0; c0 < steps; c0 += 64) {
    const int col = c0 + lane;
    const unsigned long long m = __ballot(col < steps && pr[col] == (int64_t)boundary);
    if (m) { L = c0 + __builtin_ctzll(m); break; }
  }
  if (L > EV_L) { if (lane == 0) flag[0] = 1; L = EV_L; }
  if (lane < L) {
    int64_t v = pr[lane];
    if (v < 0 || v >= V) { flag[0] = 1; v = 0; }
    int cid = id_map[v];
    if (cid < 0 || cid > W) { flag[0] = 1; cid = 0; }
    ot[lane] = (int)v;
    ct[lane] = cid;
  }
  __syncthreads();
  c.L = L;
  const int n = ev_count(L);
  const double rl = log((double)I);
  double ns[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
    c.tfc[q] = 0; c.ordc[q] = 0; c.ck[q] = 0; c.wc[q] = 0.0;
    if (j >= n) continue;
    int k, s;
    ev_split(j, L, k, s);
    c.ordc[q] = k;
    int tf = 0;
    bool first = true;
    for (int s2 = 0; s2 + k <= L; ++s2) {
      bool eq = true;
      for (int i = 0; i < k; ++i) eq &= ot[s + i] == ot[s2 + i];
      tf += eq;
      if (eq && s2 < s) first = false;
    }
    if (!first) continue;
    c.tfc[q] = tf;
    unsigned long long key = 0;
    for (int i = 0; i < k; ++i) key |= (unsigned long long)ct[s + i] << (16 * i);
    bool any0 = false;
    for (int i = 0; i < k; ++i) any0 |= ct[s + i] == 0;
    c.ck[q] = any0 ? 0ull : key;
    const int df = (scored && c.ck[q]) ? ev_df(st.hkey, st.hdf, st.mask, c.ck[q]) : 0;
    const double w = (double)tf * (rl - log((double)(df > 1 ? df : 1)));
    c.wc[q] = w;
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o == k - 1) ns[o] += w * w;
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) c.normc[o] = sqrt(ev_wsum(ns[o]));
}

// CiderScorer's similarity of the candidate to ONE reference whose nr sorted keys / weights lie in LDS (sk, sw), of lr tokens and
// per-order norms normr[0..4): v[o] = the order's clipped product sum / (norms) x the length Gaussian (sigma 6), the same in every
// lane; x[q] = where this lane's n-gram q lies in the reference, or -1.  One lane assignment and butterfly order per candidate.
__device__ __forceinline__ void ev_cider_ref(const EvCand& c, const unsigned long long* sk, const double* sw, int nr, int lr,
                                             const double* normr, double v[4], int x[4]) {
  double val[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[q] = -1;
    if (c.tfc[q] == 0 || c.ck[q] == 0ull) continue;
    x[q] = ev_find(sk, nr, c.ck[q]);
    if (x[q] < 0) continue;
    const double wr = sw[x[q]];
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o == c.ordc[q] - 1) val[o] += fmin(c.wc[q], wr) * wr;
  }
  const int lenc = c.L > 1 ? c.L - 1 : 0;
  const int lrl = lr > 1 ? lr - 1 : 0;
  const double delta = (double)(lenc - lrl);
  const double g = exp(-(delta * delta) / 72.0);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    double t = ev_wsum(val[o]);
    const double nr_o = normr[o];
    if (c.normc[o] != 0.0 && nr_o != 0.0) t /= c.normc[o] * nr_o;
    v[o] = t * g;
  }
}

}  // namespace
