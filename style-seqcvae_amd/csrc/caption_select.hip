// Diverse subset selection on the device (include/ssc.h: ssc_eval_select): from the N candidate captions of every image the k that
// are good and different from each other, by one of three rules on the caption kernel K that ssc_eval_set leaves and a per-candidate
// quality: MBR (closest to all others), MMR (quality against the largest similarity to a pick) and the greedy MAP inference of a
// DPP (Chen, Zhang & Zhou, NeurIPS 2018).
//
//   sel_image   one wave per image (a 64-thread workgroup: the P problems are independent and a greedy step needs no workgroup
//               barrier).  Lane l owns candidates l and l + 64.  One pass over the eligible rows of K checks every entry the rules
//               may read and leaves MBR's row sums; an argmax is a (value, index) butterfly, ties to the lower index; an ordering
//               (MBR, the fallback) is the stable rank by counting of the consensus order kernel, the other candidates' values
//               arriving by lane broadcast.  Row j of K is read as the lanes' K_ij (coalesced; K is symmetric bit for bit).
//               The DPP vectors c_i lie component-major (component t of candidate i at t * N + i): a lane reads and writes only its
//               own two columns - in LDS for k <= 16, in the workspace beyond - and the picked candidate's component reaches the
//               other lanes by broadcast from its owner, so no lane ever reads what another lane stored.
// fp64 throughout, -ffp-contract=off, sums in ascending order, no atomics: the same bits on every call and for every image with the
// same inputs.  A non-finite input raises the device flag (SSC_EINVAL) and leaves that image's picks at -1.
#include "caption_common.h"

namespace {

constexpr int SEL_LDS_K = 16;            // DPP vectors of up to this many components stay in LDS (16 x 128 doubles = 16 KB)
constexpr int SEL_NONE = 0x7fffffff;     // the index of "no candidate" in an argmax
constexpr size_t SEL_FLAG_BYTES = 256;   // the workspace's head: the device flag; the DPP vectors follow

struct SelArgs {
  int P, N, k, method, normalize;
  const double* kernel; const double* quality; const uint8_t* eligible;
  double lambda, theta, min_gain;
  int* picks; double* gains; int* n_primary; int* flag; double* cvec;
};

// (ov, oi) goes ahead of (v, i): the larger value, the lower index on a tie
__device__ __forceinline__ bool sel_ahead(double ov, int oi, double v, int i) { return ov > v || (ov == v && oi < i); }

// The wave's argmax over the lanes' two candidates: val[q] of candidate lane + 64 q where avail[q] (a NaN counts as not available).
// Every lane gets the same (value, index); index SEL_NONE: no candidate.
__device__ __forceinline__ void sel_argmax(const double val[2], const bool avail[2], int lane, double& v, int& idx) {
  v = -INFINITY;
  idx = SEL_NONE;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const bool ok = avail[q] && val[q] == val[q];
    const double x = ok ? val[q] : -INFINITY;
    const int i = ok ? lane + 64 * q : SEL_NONE;
    if (sel_ahead(x, i, v, idx)) { v = x; idx = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (sel_ahead(ov, oi, v, idx)) { v = ov; idx = oi; }
  }
}

// value of candidate j (held by lane j & 63 as x[j >> 6]) in every lane; j is the same in every lane
__device__ __forceinline__ double sel_bcast(const double x[2], int j) { return __shfl((j >> 6) ? x[1] : x[0], j & 63, 64); }

// The candidates with avail[q] set go to slots base, base + 1, ... by val, stable descending (rank by counting); slots >= k are
// dropped.  gains = the value (report) or 0.  Returns how many candidates were available.
__device__ __forceinline__ int sel_fill_ranked(const double val[2], const bool avail[2], int lane, int N, int base, int k, bool report,
                                               int* picks, double* gains) {
  const unsigned long long m0 = __ballot(avail[0]), m1 = __ballot(avail[1]);
  int rank[2] = {0, 0};
  for (int j = 0; j < N; ++j) {
    if (!(((j < 64 ? m0 : m1) >> (j & 63)) & 1ull)) continue;   // (the same in every lane)
    const double vj = sel_bcast(val, j);
#pragma unroll
    for (int q = 0; q < 2; ++q) rank[q] += vj > val[q] || (vj == val[q] && j < lane + 64 * q);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int slot = base + rank[q];
    if (avail[q] && slot < k) {
      picks[slot] = lane + 64 * q;
      gains[slot] = report ? val[q] : 0.0;
    }
  }
  return __popcll(m0) + __popcll(m1);
}

template <bool LDSC>
__global__ __launch_bounds__(64) void sel_image(SelArgs a) {
  __shared__ double cl[LDSC ? SEL_LDS_K * EV_MAX_N : 1];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int N = a.N, k = a.k;
  const double* K = a.kernel + (size_t)p * N * N;
  int* picks = a.picks + (size_t)p * k;
  double* gains = a.gains + (size_t)p * k;
  double* c = cl;
  if (!LDSC && a.method == 3) c = a.cvec + (size_t)p * N * k;

  bool el[2];
  double qh[2] = {0.0, 0.0};
  bool bad = false;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = lane + 64 * q;
    el[q] = i < N && (!a.eligible || a.eligible[(size_t)p * N + i] != 0);
    if (el[q] && a.quality) {
      qh[q] = a.quality[(size_t)p * N + i];
      bad |= !__builtin_isfinite(qh[q]);
    }
  }
  const unsigned long long m0 = __ballot(el[0]), m1 = __ballot(el[1]);
  const int ne = __popcll(m0) + __popcll(m1);
  // every K_ij of two eligible candidates, row by row: the finiteness check of all a rule may read, and MBR's sums over j ascending
  double s[2] = {0.0, 0.0};
  for (int j = 0; j < N; ++j) {
    if (!(((j < 64 ? m0 : m1) >> (j & 63)) & 1ull)) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = lane + 64 * q;
      if (!el[q]) continue;
      const double x = K[(size_t)j * N + i];
      bad |= !__builtin_isfinite(x);
      if (j != i) s[q] += x;
    }
  }
  if (a.quality && a.normalize && ne > 0) {
    double lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (el[q]) { lo = fmin(lo, qh[q]); hi = fmax(hi, qh[q]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, o, 64));
      hi = fmax(hi, __shfl_xor(hi, o, 64));
    }
    const double span = hi - lo;
    bad |= !__builtin_isfinite(span);
#pragma unroll
    for (int q = 0; q < 2; ++q) qh[q] = span > 0.0 ? (qh[q] - lo) / span : 0.0;
  }
  if (__any(bad)) {
    for (int t = lane; t < k; t += 64) { picks[t] = -1; gains[t] = 0.0; }
    if (lane == 0) { a.n_primary[p] = 0; a.flag[0] = 1; }
    return;
  }

  int filled = 0;   // slots written so far (the same in every lane)
  if (a.method == 1) {
#pragma unroll
    for (int q = 0; q < 2; ++q) s[q] = ne > 1 ? s[q] / (double)(ne - 1) : 0.0;
    sel_fill_ranked(s, el, lane, N, 0, k, true, picks, gains);
    filled = ne < k ? ne : k;
    if (lane == 0) a.n_primary[p] = filled;
  } else if (a.method == 2) {
    bool av[2] = {el[0], el[1]};
    double mx[2] = {-INFINITY, -INFINITY};   // max_{j in S} K_ij
    int t = 0;
    for (; t < k; ++t) {
      double obj[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) obj[q] = t == 0 ? qh[q] : a.lambda * qh[q] - (1.0 - a.lambda) * mx[q];
      double v;
      int j;
      sel_argmax(obj, av, lane, v, j);
      if (j == SEL_NONE) break;
      if (lane == 0) { picks[t] = j; gains[t] = t == 0 ? a.lambda * v : v; }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = lane + 64 * q;
        if (i == j) av[q] = false;
        if (av[q]) mx[q] = fmax(mx[q], K[(size_t)j * N + i]);
      }
    }
    filled = t;
    if (lane == 0) a.n_primary[p] = t;
  } else {
    bool av[2] = {el[0], el[1]};
    double r[2] = {1.0, 1.0}, d2[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = lane + 64 * q;
      if (!el[q]) continue;
      r[q] = exp(a.theta * qh[q]);
      d2[q] = (r[q] * K[(size_t)i * N + i]) * r[q];
    }
    int t = 0;
    for (; t < k; ++t) {
      double v;
      int j;
      sel_argmax(d2, av, lane, v, j);
      if (j == SEL_NONE || !(v >= a.min_gain) || !(v > 0.0)) break;
      if (lane == 0) { picks[t] = j; gains[t] = v; }
      if (t + 1 < k) {   // (after the last slot nothing reads d2)
        const double dj = sqrt(v);
        const double rj = sel_bcast(r, j);
        double dot[2] = {0.0, 0.0};
        for (int u = 0; u < t; ++u) {   // <c_j, c_i> over the components ascending; c_j's come from j's owner
          double ci[2];
#pragma unroll
          for (int q = 0; q < 2; ++q) ci[q] = av[q] ? c[(size_t)u * N + lane + 64 * q] : 0.0;
          const double cj = sel_bcast(ci, j);
#pragma unroll
          for (int q = 0; q < 2; ++q) dot[q] += cj * ci[q];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int i = lane + 64 * q;
          if (!av[q] || i == j) continue;
          const double lji = (rj * K[(size_t)j * N + i]) * r[q];
          const double e = (lji - dot[q]) / dj;
          c[(size_t)t * N + i] = e;
          d2[q] -= e * e;
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (lane + 64 * q == j) av[q] = false;
    }
    if (lane == 0) a.n_primary[p] = t;
    filled = t + sel_fill_ranked(qh, av, lane, N, t, k, false, picks, gains);
    if (filled > k) filled = k;
  }
  for (int t = filled + lane; t < k; t += 64) { picks[t] = -1; gains[t] = 0.0; }
}

bool sel_desc_ok(const ssc_eval_select_desc* d) {
  if (!d || d->P < 1 || d->N < 1 || d->N > EV_MAX_N || d->k < 1 || d->k > d->N || (int64_t)d->P * d->N > (1 << 24)) return false;
  if (d->method < 1 || d->method > 3 || (d->normalize != 0 && d->normalize != 1)) return false;
  if (!d->kernel || !d->picks || !d->gains || !d->n_primary) return false;
  if (!(d->lambda >= 0.0 && d->lambda <= 1.0)) return false;
  if (!(d->theta >= 0.0) || !(d->theta <= 1.7976931348623157e308)) return false;
  if (!(d->min_gain >= 0.0)) return false;
  if (!d->quality && (d->method == 2 || (d->method == 3 && d->theta != 0.0))) return false;
  return true;
}

size_t sel_bytes(const ssc_eval_select_desc* d) {
  size_t n = SEL_FLAG_BYTES;
  if (d->method == 3 && d->k > SEL_LDS_K) n += (size_t)d->P * d->N * d->k * sizeof(double);
  return n;
}

}  // namespace

extern "C" size_t ssc_eval_select_workspace_bytes(const ssc_eval_select_desc* d) { return sel_desc_ok(d) ? sel_bytes(d) : 0; }

extern "C" int ssc_eval_select(const ssc_eval_select_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sel_desc_ok(d) || !workspace || workspace_bytes < sel_bytes(d)) return SSC_EINVAL;
  if (((uintptr_t)workspace) & 7u) return SSC_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  SelArgs a{d->P, d->N, d->k, d->method, d->normalize, d->kernel, d->quality, d->eligible, d->lambda, d->theta, d->min_gain,
            d->picks, d->gains, d->n_primary, (int*)workspace, (double*)((char*)workspace + SEL_FLAG_BYTES)};
  if (hipMemsetAsync(workspace, 0, sizeof(int), st) != hipSuccess) return SSC_EHIP;
  if (d->method == 3 && d->k <= SEL_LDS_K)
    SSC_LAUNCH(sel_image<true>, dim3(d->P), dim3(64), 0, st, a);
  else
    SSC_LAUNCH(sel_image<false>, dim3(d->P), dim3(64), 0, st, a);
  SSC_CHECK_LAUNCH();
  return ev_read_flag(a.flag, st);
}
