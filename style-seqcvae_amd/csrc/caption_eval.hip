// Diverse-caption evaluation on the device: BLEU-1..4 (coco-caption BleuScorer, "closest"), ROUGE-L (coco-caption Rouge),
// CIDEr-D (coco-caption CiderScorer, sigma 6) per candidate, Div-n and style counts per image (the reference's eval/eval.py).
//
// Words are compact ids 1..W (W <= 65535) of the reference words; an n-gram of order k <= 4 is one 64-bit key of k 16-bit ids
// (field i = word i), so the order is the number of nonzero fields and two n-grams are equal iff their keys are.  A candidate's
// own n-grams (its tf, Div-n) are compared on its original ids; words in no reference map to compact id 0 and never match.
//
// Reference preparation (once per reference set):
//   ev_ref_ngrams  one wave per reference: its distinct n-grams sorted by key, with their tf (LDS, O(n^2 / 64) compares)
//   ev_ref_df      one wave per image: the n-grams no earlier reference of the image holds go into an open-addressing table
//                  (integer atomicCAS / atomicAdd only) - df = the number of images whose references hold the n-gram
//   ev_ref_weights one wave per reference: w = tf (log I - log max(1, df)), per-order norms in a fixed order
// Scoring (once per prediction tensor):
//   ev_score       one wave per candidate: n-grams, tf, df lookups, CIDEr-D against each reference (binary search in the
//                  reference's sorted keys, staged in LDS), BLEU clipping, ROUGE-L by bit-parallel LCS (lane = reference position)
//   ev_image       one workgroup per image: distinct 1- / 2-grams of its N captions and of its top 5 by CIDEr (LDS hash sets),
//                  style counts
// Every sum over a candidate's n-grams runs in the same lane assignment and butterfly order whatever the candidate's position, so
// equal captions of an image score bit-equal; no float atomics.  Bad ids / lengths / offsets raise a device flag (SSC_EINVAL) and
// are clamped, never used as indices.
#include "caption_common.h"

namespace {

// ---- reference preparation ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void ev_ref_ngrams(const int* tok_off, const int* tokens, int ntok, int W, EvState st) {
  __shared__ int tk[EV_L];
  __shared__ unsigned long long kk[EV_NG];
  __shared__ int first[EV_NG];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int a = tok_off[r], b = tok_off[r + 1];
  const int L = b - a;
  if (a < 0 || b > ntok || L < 1 || L > EV_L) {
    if (lane == 0) { st.flag[0] = 1; st.nu[r] = 0; st.len[r] = 0; st.base[r] = 0; }
    return;
  }
  int t = 1;
  if (lane < L) {
    t = tokens[a + lane];
    if (t < 1 || t > W) { st.flag[0] = 1; t = 1; }
  }
  tk[lane] = t;
  __syncthreads();
  const int n = ev_count(L);
  for (int j = lane; j < n; j += 64) {
    int k, s;
    ev_split(j, L, k, s);
    unsigned long long key = 0;
    for (int i = 0; i < k; ++i) key |= (unsigned long long)tk[s + i] << (16 * i);
    kk[j] = key;
  }
  __syncthreads();
  for (int j = lane; j < n; j += 64) {
    int f = 1;
    for (int i = 0; i < j; ++i) f &= kk[i] != kk[j];
    first[j] = f;
  }
  __syncthreads();
  int mine = 0;
  for (int j = lane; j < n; j += 64) {
    if (!first[j]) continue;
    ++mine;
    int tf = 0, rank = 0;
    for (int i = 0; i < n; ++i) {
      tf += kk[i] == kk[j];
      rank += first[i] && kk[i] < kk[j];
    }
    st.key[4 * (size_t)a + rank] = kk[j];   // rank < distinct count <= n <= 4 L: inside this reference's 4 L slots
    st.tf[4 * (size_t)a + rank] = tf;
  }
  mine = ev_isum(mine);
  if (lane == 0) { st.nu[r] = mine; st.len[r] = L; st.base[r] = a; }
}

__global__ __launch_bounds__(64) void ev_ref_df(const int* ref_off, int nref, const uint8_t* style, int W, EvState st) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int lo = ref_off[i], hi = ref_off[i + 1];
  if (lo < 0 || hi > nref || hi <= lo) {
    if (lane == 0) { st.flag[0] = 1; st.rstyle[i] = 0; }
    return;
  }
  int sty = 0;
  for (int r = lo; r < hi; ++r) {
    const size_t b = 4 * (size_t)st.base[r];
    const int n = st.nu[r];
    for (int e = lane; e < n; e += 64) {
      const unsigned long long k = st.key[b + e];
      bool dup = false;
      for (int r2 = lo; r2 < r && !dup; ++r2) dup = ev_find(st.key + 4 * (size_t)st.base[r2], st.nu[r2], k) >= 0;
      if (dup) continue;
      unsigned long long h = ev_mix(k) & st.mask;
      bool done = false;
      for (unsigned long long p = 0; p <= st.mask && !done; ++p) {
        const unsigned long long prev = atomicCAS(&st.hkey[h], 0ull, k);
        if (prev == 0ull || prev == k) { atomicAdd(&st.hdf[h], 1); done = true; }
        h = (h + 1) & st.mask;
      }
      if (!done) st.flag[0] = 1;
      if (style && (k >> 16) == 0 && (int)k <= W && style[(int)k]) ++sty;
    }
  }
  sty = ev_isum(sty);
  if (lane == 0) st.rstyle[i] = sty;
}

__global__ __launch_bounds__(64) void ev_ref_weights(int I, EvState st) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const size_t b = 4 * (size_t)st.base[r];
  const int n = st.nu[r];
  const double rl = log((double)I);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = lane; e < n; e += 64) {
    const unsigned long long k = st.key[b + e];
    const int df = ev_df(st.hkey, st.hdf, st.mask, k);
    const double w = (double)st.tf[b + e] * (rl - log((double)(df > 1 ? df : 1)));
    st.w[b + e] = w;
    const int o = ev_order(k) - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q == o) s[q] += w * w;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = ev_wsum(s[q]);
    if (lane == 0) st.norm[4 * (size_t)r + q] = sqrt(v);
  }
}

// ---- scoring ------------------------------------------------------------------------------------------------------------------

struct EvScoreArgs {
  const int64_t* pred; int N, steps, boundary, V, I, nref, W;
  const int* id_map; const uint8_t* style_ids; const int* ref_image; const int* ref_off; const int* tokens;
  double* scores; int* counts; int* image_counts; int* top5; const uint8_t* style; int* flag;
};

__global__ __launch_bounds__(64) void ev_score(EvScoreArgs a, EvState st) {
  __shared__ int ot[EV_L], ct[EV_L];
  __shared__ unsigned long long sk[EV_NG];
  __shared__ double sw[EV_NG];
  __shared__ int stf[EV_NG];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int p = row / a.N;
  const int64_t* pr = a.pred + (size_t)row * a.steps;
  const int img = a.ref_image[p];
  const bool scored = img >= 0 && img < a.I;
  if (img < -1 || img >= a.I) { if (lane == 0) a.flag[0] = 1; }
  // this lane's n-grams: slots lane + 64 q; tf > 0 only at a distinct n-gram's first occurrence
  EvCand c;
  ev_candidate(pr, a.steps, a.boundary, a.V, a.id_map, a.W, scored, a.I, st, a.flag, ot, ct, c);
  const int L = c.L;
  int maxr[4] = {0, 0, 0, 0};
  int* cnt = a.counts + (size_t)row * EV_NCOUNT;
  double* sc = a.scores + (size_t)row * EV_NSCORE;
  int lo = 0, hi = 0;
  if (scored) {
    lo = a.ref_off[img]; hi = a.ref_off[img + 1];
    if (lo < 0 || hi > a.nref || hi <= lo) { if (lane == 0) a.flag[0] = 1; lo = hi = 0; }
  }
  double cid[4] = {0.0, 0.0, 0.0, 0.0};
  double P = 0.0, Q = 0.0;
  int bd = 0x7fffffff, bl = 0;
  for (int r = lo; r < hi; ++r) {
    const size_t b = 4 * (size_t)st.base[r];
    const int nr = min(st.nu[r], EV_NG), lr = min(st.len[r], EV_L);   // (<= 4 len and <= 64 as ev_ref_ngrams wrote them)
    __syncthreads();   // the previous reference's LDS reads are done
    for (int e = lane; e < nr; e += 64) { sk[e] = st.key[b + e]; sw[e] = st.w[b + e]; stf[e] = st.tf[b + e]; }
    const int rt = lane < lr ? a.tokens[st.base[r] + lane] : -1;
    __syncthreads();
    double v[4];
    int x[4];
    ev_cider_ref(c, sk, sw, nr, lr, st.norm + 4 * (size_t)r, v, x);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (x[q] >= 0) maxr[q] = max(maxr[q], stf[x[q]]);
#pragma unroll
    for (int o = 0; o < 4; ++o) cid[o] += v[o];
    // LCS(candidate, reference) by the bit-parallel recurrence V' = (V + (V & M)) | (V & ~M), bit = reference position
    unsigned long long Vb = ~0ull;
    for (int t = 0; t < L; ++t) {
      const int w = ct[t];
      const unsigned long long M = __ballot(w != 0 && rt == w);
      Vb = (Vb + (Vb & M)) | (Vb & ~M);
    }
    const unsigned long long msk = lr >= 64 ? ~0ull : ((1ull << lr) - 1);
    const int l = __popcll(~Vb & msk);
    if (L > 0 && lr > 0) {
      P = fmax(P, (double)l / (double)L);
      Q = fmax(Q, (double)l / (double)lr);
    }
    const int d = lr > L ? lr - L : L - lr;
    if (d < bd || (d == bd && lr < bl)) { bd = d; bl = lr; }
  }
  int corr[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o == c.ordc[q] - 1 && c.tfc[q] > 0) corr[o] += min(c.tfc[q], maxr[q]);
#pragma unroll
  for (int o = 0; o < 4; ++o) corr[o] = ev_isum(corr[o]);
  if (lane == 0) {
    const int reflen = hi > lo ? bl : 0;
    int guess[4];
    for (int o = 0; o < 4; ++o) guess[o] = L - o > 0 ? L - o : 0;
    cnt[0] = L; cnt[1] = reflen;
    for (int o = 0; o < 4; ++o) { cnt[2 + o] = guess[o]; cnt[6 + o] = corr[o]; }
    if (hi > lo) {
      double bleu[4], bb = 1.0;
      for (int o = 0; o < 4; ++o) {
        bb *= ((double)corr[o] + 1e-15) / ((double)guess[o] + 1e-9);
        bleu[o] = pow(bb, 1.0 / (o + 1));
      }
      const double ratio = ((double)L + 1e-15) / ((double)reflen + 1e-9);
      if (ratio < 1.0)
        for (int o = 0; o < 4; ++o) bleu[o] *= exp(1.0 - 1.0 / ratio);
      for (int o = 0; o < 4; ++o) sc[o] = bleu[o];
      const double beta2 = 1.2 * 1.2;
      sc[4] = (L > 0 && P != 0.0 && Q != 0.0) ? ((1.0 + beta2) * P * Q) / (Q + beta2 * P) : 0.0;
      sc[5] = (((cid[0] + cid[1]) + cid[2]) + cid[3]) / 4.0 / (double)(hi - lo) * 10.0;
    } else {
      for (int o = 0; o < EV_NSCORE; ++o) sc[o] = 0.0;
    }
  }
}

// distinct n-grams (n = 1, 2) of the captions sel[0..ns) of prediction image p, over their original ids; with style != NULL the
// new unigrams that are style words are counted (cs) and so are those its references hold (cm)
__device__ void ev_distinct(const EvScoreArgs& a, const EvState& st, int p, const int* sel, int ns, const int* len, int order,
                            unsigned* tab, int* cnt, int lo, int hi, bool style) {
  for (int i = threadIdx.x; i < EV_DIV_SLOTS; i += blockDim.x) tab[i] = EV_EMPTY;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  int nd = 0, cs = 0, cm = 0;
  for (int x = threadIdx.x; x < ns * EV_L; x += blockDim.x) {
    const int n = sel[x / EV_L], t = x % EV_L;
    if (n < 0 || n >= a.N || t + order > len[n]) continue;
    const int64_t* pr = a.pred + ((size_t)p * a.N + n) * a.steps;
    const int64_t v0 = pr[t], v1 = order == 2 ? pr[t + 1] : 0;
    if (v0 < 0 || v0 >= a.V || v1 < 0 || v1 >= a.V) continue;   // (flagged by ev_score)
    const unsigned key = order == 1 ? (unsigned)v0 : (unsigned)v0 * 65536u + (unsigned)v1;
    unsigned h = ev_mix32(key) & (EV_DIV_SLOTS - 1);
    bool fresh = false;
    for (int probe = 0; probe < EV_DIV_SLOTS; ++probe) {
      const unsigned prev = atomicCAS(&tab[h], EV_EMPTY, key);
      if (prev == EV_EMPTY) { fresh = true; break; }
      if (prev == key) break;
      h = (h + 1) & (EV_DIV_SLOTS - 1);
    }
    if (!fresh) continue;
    ++nd;
    if (style && a.style_ids[v0]) {
      ++cs;
      const int c = a.id_map[v0];
      bool held = false;
      if (c > 0 && c <= a.W)
        for (int r = lo; r < hi && !held; ++r) held = ev_find(st.key + 4 * (size_t)st.base[r], st.nu[r], (unsigned long long)c) >= 0;
      cm += held;
    }
  }
  atomicAdd(&cnt[0], nd);
  atomicAdd(&cnt[1], cs);
  atomicAdd(&cnt[2], cm);
  __syncthreads();
}

__global__ __launch_bounds__(256) void ev_image(EvScoreArgs a, EvState st) {
  __shared__ unsigned tab[EV_DIV_SLOTS];
  __shared__ int len[EV_MAX_N], sel[EV_MAX_N], top[5], cnt[3];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int N = a.N;
  for (int n = tid; n < N; n += blockDim.x) {
    len[n] = a.counts[((size_t)p * N + n) * EV_NCOUNT];
    sel[n] = n;
  }
  if (tid < 5) top[tid] = -1;
  const int img = a.ref_image[p];
  const bool scored = img >= 0 && img < a.I;
  int lo = 0, hi = 0;
  if (scored) {
    lo = a.ref_off[img]; hi = a.ref_off[img + 1];
    if (lo < 0 || hi > a.nref || hi <= lo) lo = hi = 0;   // (flagged by ev_score)
  }
  __syncthreads();
  int* out = a.image_counts + (size_t)p * EV_NIMG;
  int words = 0;
  for (int n = 0; n < N; ++n) words += len[n];
  ev_distinct(a, st, p, sel, N, len, 1, tab, cnt, lo, hi, scored && a.style_ids != nullptr);
  if (tid == 0) { out[0] = cnt[0]; out[6] = cnt[1]; out[7] = cnt[2]; }
  __syncthreads();
  ev_distinct(a, st, p, sel, N, len, 2, tab, cnt, lo, hi, false);
  if (tid == 0) { out[1] = cnt[0]; out[2] = words; out[8] = scored ? st.rstyle[img] : 0; }
  if (scored && N >= 5) {
    // top 5 by CIDEr, stable descending: rank = #{j : c_j > c_n, or c_j == c_n and j < n}
    for (int n = tid; n < N; n += blockDim.x) {
      const double c = a.scores[((size_t)p * N + n) * EV_NSCORE + 5];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const double cj = a.scores[((size_t)p * N + j) * EV_NSCORE + 5];
        rank += cj > c || (cj == c && j < n);
      }
      if (rank < 5) top[rank] = n;
    }
    __syncthreads();
    int w5 = 0;
    for (int k = 0; k < 5; ++k) w5 += top[k] >= 0 ? len[top[k]] : 0;
    ev_distinct(a, st, p, top, 5, len, 1, tab, cnt, lo, hi, false);
    if (tid == 0) out[3] = cnt[0];
    __syncthreads();
    ev_distinct(a, st, p, top, 5, len, 2, tab, cnt, lo, hi, false);
    if (tid == 0) { out[4] = cnt[0]; out[5] = w5; }
  } else if (tid == 0) {
    out[3] = out[4] = out[5] = 0;
  }
  if (tid < 5) a.top5[(size_t)p * 5 + tid] = top[tid];
}

// ---- caption-set diversity: the N captions of an image against each other ---------------------------------------------------
//   es_caption  one wave per caption: its distinct n-grams over ORIGINAL ids (key field = id + 1, so id 0 is a word), sorted by
//               key, with tf, the weight tf (log I - log max(1, df)) and the per-order norms - once per caption, in a workspace
//               of S = (n-gram slots of min(steps, 64) tokens) entries per caption
//   es_pair     one wave per (image, i): caption i's keys staged in LDS; against every j the n-grams both hold are found by binary
//               search, ranked among themselves (ballot prefix), and their products summed in rank order - an order that depends on
//               the set of shared n-grams alone, so K_ij == K_ji and equal captions give equal rows bit for bit; BLEU clipping
//               maxima, the "closest" length and "an earlier caption equals this one" ride along
//   es_eigen    one workgroup per image: K in LDS, cyclic Jacobi (round-robin pairing: N / 2 disjoint rotations at a time) in fp64
//               until the largest off-diagonal entry is below 1e-15 max(1, largest diagonal entry); eigenvalues sorted descending

constexpr int ES_THREADS = 256;
constexpr int ES_MAX_SWEEPS = 30;

struct EsLayout { size_t flag, key, w, tf, nu, len, norm, first, kmat, total; int S; };

EsLayout es_layout(int P, int N, int steps, bool own_kmat) {
  EsLayout l;
  const int Lm = steps < EV_L ? steps : EV_L;
  int S = 0;
  for (int k = 1; k <= 4; ++k) S += Lm - k + 1 > 0 ? Lm - k + 1 : 0;
  const size_t rows = (size_t)P * N;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = ssc_round_up(o + bytes, 256); return at; };
  l.flag = take(4); l.key = take(rows * S * 8); l.w = take(rows * S * 8); l.tf = take(rows * S * 4); l.nu = take(rows * 4);
  l.len = take(rows * 4); l.norm = take(rows * 4 * 8); l.first = take(rows * 4);
  l.kmat = take(own_kmat ? rows * N * 8 : 0);
  l.total = o; l.S = S;
  return l;
}

struct EsArgs {
  const int64_t* pred; int N, steps, boundary, V, I, W, S;
  const int* id_map; const int* ref_image;
  unsigned long long* key; double* w; int* tf; int* nu; int* len; double* norm; int* first;
  int* counts; double* kmat; double* eig; int* distinct; int* flag;
};

// the prepared image of prediction image p, or -1; anything else raises the flag
__device__ __forceinline__ int es_image(const EsArgs& a, int p) {
  const int img = a.ref_image[p];
  if (img < -1 || img >= a.I) { a.flag[0] = 1; return -1; }
  return img;
}

__global__ __launch_bounds__(64) void es_caption(EsArgs a, EvState st) {
  __shared__ int ot[EV_L], ct[EV_L];
  __shared__ unsigned long long kk[EV_NG], ck[EV_NG], sk[EV_NG];
  __shared__ double sw[EV_NG];
  __shared__ int first[EV_NG];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int p = row / a.N;
  const int64_t* pr = a.pred + (size_t)row * a.steps;
  int L = a.steps;
  for (int c0 = 0; c0 < a.steps; c0 += 64) {
    const int c = c0 + lane;
    const unsigned long long m = __ballot(c < a.steps && pr[c] == (int64_t)a.boundary);
    if (m) { L = c0 + __builtin_ctzll(m); break; }
  }
  if (L > EV_L) { if (lane == 0) a.flag[0] = 1; L = EV_L; }
  const bool scored = es_image(a, p) >= 0;
  ot[lane] = 0; ct[lane] = 0;
  if (lane < L) {
    int64_t v = pr[lane];
    if (v < 0 || v >= a.V) { a.flag[0] = 1; v = 0; }
    int c = 0;
    if (scored) {
      c = a.id_map[v];
      if (c < 0 || c > a.W) { a.flag[0] = 1; c = 0; }
    }
    ot[lane] = (int)v;
    ct[lane] = c;
  }
  __syncthreads();
  const int n = ev_count(L);   // <= a.S: L <= min(steps, 64)
  for (int j = lane; j < n; j += 64) {
    int k, s;
    ev_split(j, L, k, s);
    unsigned long long key = 0, c = 0;
    bool any0 = false;
    for (int i = 0; i < k; ++i) {
      key |= (unsigned long long)(ot[s + i] + 1) << (16 * i);
      c |= (unsigned long long)ct[s + i] << (16 * i);
      any0 |= ct[s + i] == 0;
    }
    kk[j] = key;
    ck[j] = any0 ? 0ull : c;
  }
  __syncthreads();
  for (int j = lane; j < n; j += 64) {
    int f = 1;
    for (int i = 0; i < j; ++i) f &= kk[i] != kk[j];
    first[j] = f;
  }
  __syncthreads();
  const size_t b = (size_t)row * a.S;
  const double rl = log((double)a.I);
  int mine = 0;
  for (int j = lane; j < n; j += 64) {
    if (!first[j]) continue;
    ++mine;
    int tf = 0, rank = 0;
    for (int i = 0; i < n; ++i) {
      tf += kk[i] == kk[j];
      rank += first[i] && kk[i] < kk[j];
    }
    const int df = (scored && ck[j]) ? ev_df(st.hkey, st.hdf, st.mask, ck[j]) : 0;
    const double w = scored ? (double)tf * (rl - log((double)(df > 1 ? df : 1))) : 0.0;
    sk[rank] = kk[j];   // rank < distinct count <= n <= S
    sw[rank] = w;
    a.key[b + rank] = kk[j];
    a.w[b + rank] = w;
    a.tf[b + rank] = tf;
  }
  mine = ev_isum(mine);
  __syncthreads();
  // per-order norms over the SORTED n-grams: the order depends on the caption's content alone
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = lane; e < mine; e += 64) {
    const int o = ev_order(sk[e]) - 1;
    const double w = sw[e];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q == o) s[q] += w * w;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = ev_wsum(s[q]);
    if (lane == 0) a.norm[4 * (size_t)row + q] = sqrt(v);
  }
  if (lane == 0) { a.nu[row] = mine; a.len[row] = L; }
}

__global__ __launch_bounds__(64) void es_pair(EsArgs a) {
  __shared__ unsigned long long sk[EV_NG];
  __shared__ double sw[EV_NG], sprod[EV_NG];
  __shared__ int stf[EV_NG], smax[EV_NG], sord[EV_NG];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int p = row / a.N, i = row - p * a.N;
  const bool scored = a.ref_image[p] >= 0 && a.ref_image[p] < a.I;   // (out-of-range values were flagged by es_caption)
  const int ni = min(a.nu[row], a.S), L = min(a.len[row], EV_L);
  const size_t bi = (size_t)row * a.S;
  for (int e = lane; e < EV_NG; e += 64) {
    const bool in = e < ni;
    sk[e] = in ? a.key[bi + e] : 0ull;
    sw[e] = in ? a.w[bi + e] : 0.0;
    stf[e] = in ? a.tf[bi + e] : 0;
    smax[e] = 0;
  }
  const int64_t* pri = a.pred + (size_t)row * a.steps;
  const int64_t mytok = lane < L ? pri[lane] : 0;
  double normi[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) normi[o] = a.norm[4 * (size_t)row + o];
  __syncthreads();
  int bd = 0x7fffffff, bl = 0;
  bool dup = false;
  for (int j = 0; j < a.N; ++j) {
    const int rj = p * a.N + j;
    const int nj = min(a.nu[rj], a.S), lj = min(a.len[rj], EV_L);
    const size_t bj = (size_t)rj * a.S;
    int common = 0;
    for (int c0 = 0; c0 < nj; c0 += 64) {
      const int e = c0 + lane;
      int x = -1;
      unsigned long long kj = 0;
      if (e < nj) {
        kj = a.key[bj + e];
        x = ev_find(sk, ni, kj);
      }
      if (x >= 0 && j != i) smax[x] = max(smax[x], a.tf[bj + e]);   // one lane per x: the keys of caption j are distinct
      if (scored) {
        const unsigned long long m = __ballot(x >= 0);
        if (x >= 0) {
          const int r = common + __popcll(m & ((1ull << lane) - 1ull));   // rank among the shared n-grams, in key order
          sprod[r] = sw[x] * a.w[bj + e];
          sord[r] = ev_order(kj) - 1;
        }
        common += __popcll(m);
      }
    }
    if (j != i) {
      const int d = lj > L ? lj - L : L - lj;
      if (d < bd || (d == bd && lj < bl)) { bd = d; bl = lj; }
      if (j < i && lj == L && !dup) {
        const int64_t* prj = a.pred + (size_t)rj * a.steps;
        dup = __all(lane < L ? prj[lane] == mytok : true);
      }
    }
    __syncthreads();
    if (a.kmat) {
      double kij = 0.0;
      if (scored) {
        double val[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = lane; r < common; r += 64) {
          const int o = sord[r];
          const double v = sprod[r];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == o) val[q] += v;
        }
        double c[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const double v = ev_wsum(val[o]);
          const double nj_o = a.norm[4 * (size_t)rj + o];
          c[o] = (normi[o] != 0.0 && nj_o != 0.0) ? v / (normi[o] * nj_o) : 0.0;
        }
        kij = (((c[0] + c[1]) + c[2]) + c[3]) * 0.25;
      }
      if (lane == 0) a.kmat[(size_t)row * a.N + j] = kij;
    }
    __syncthreads();   // sprod / sord / smax are free for the next caption
  }
  int corr[4] = {0, 0, 0, 0};
  for (int e = lane; e < ni; e += 64) {
    const int o = ev_order(sk[e]) - 1;
    const int c = min(stf[e], smax[e]);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q == o) corr[q] += c;
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) corr[o] = ev_isum(corr[o]);
  if (lane == 0) {
    int* cnt = a.counts + (size_t)row * EV_NCOUNT;
    cnt[0] = L; cnt[1] = bl;
    for (int o = 0; o < 4; ++o) { cnt[2 + o] = L - o > 0 ? L - o : 0; cnt[6 + o] = corr[o]; }
    a.first[row] = dup ? 0 : 1;
  }
}

__global__ __launch_bounds__(ES_THREADS) void es_eigen(EsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double es_lds[];
  const int N = a.N, LD = N | 1;        // odd leading dimension: a column walk touches every bank
  double* A = es_lds;                   // [N][LD]
  double* cs = A + (size_t)N * LD;      // [64] rotation cosines, then [64] sines
  double* sn = cs + 64;
  double* red = sn + 64;                // [ES_THREADS]
  int* pp = (int*)(red + ES_THREADS);   // [64] the rotations' rows p < q
  int* qq = pp + 64;
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int nd = 0;
    for (int i = 0; i < N; ++i) nd += a.first[(size_t)p * N + i] != 0;
    a.distinct[p] = nd;
  }
  const int img = a.ref_image[p];
  if (img < 0 || img >= a.I) {   // workgroup-uniform
    for (int i = tid; i < N; i += ES_THREADS) a.eig[(size_t)p * N + i] = 0.0;
    return;
  }
  const double* K = a.kmat + (size_t)p * N * N;
  for (int x = tid; x < N * N; x += ES_THREADS) A[(x / N) * LD + x % N] = K[x];
  if (tid < 64) { cs[tid] = 1.0; sn[tid] = 0.0; pp[tid] = 0; qq[tid] = 0; }
  __syncthreads();
  const int m = N + (N & 1), half = m / 2;   // an odd N plays with a dummy index N that never rotates
  for (int sweep = 0; sweep < ES_MAX_SWEEPS; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int x = tid; x < N * N; x += ES_THREADS) {
      const int r = x / N, c = x - r * N;
      const double v = fabs(A[r * LD + c]);
      if (r == c) dg = fmax(dg, v); else off = fmax(off, v);
    }
    red[tid] = off;
    __syncthreads();
    for (int s = ES_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
      __syncthreads();
    }
    off = red[0];
    __syncthreads();
    red[tid] = dg;
    __syncthreads();
    for (int s = ES_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
      __syncthreads();
    }
    dg = red[0];
    __syncthreads();
    if (off <= 1e-15 * fmax(1.0, dg)) break;   // workgroup-uniform
    for (int step = 0; step < m - 1; ++step) {
      if (tid < half) {
        int u = tid == 0 ? step : (step + tid) % (m - 1);
        int v = tid == 0 ? m - 1 : (step - tid + (m - 1)) % (m - 1);
        if (u > v) { const int t = u; u = v; v = t; }
        double c = 1.0, s = 0.0;
        if (v < N) {
          const double apq = A[u * LD + v];
          if (apq != 0.0) {
            const double theta = (A[v * LD + v] - A[u * LD + u]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
          }
        } else {
          u = v = 0;
        }
        cs[tid] = c; sn[tid] = s; pp[tid] = u; qq[tid] = v;
      }
      __syncthreads();
      for (int x = tid; x < half * N; x += ES_THREADS) {   // rows p, q of J^T A
        const int k = x / N, col = x - k * N;
        const double s = sn[k];
        if (s == 0.0) continue;
        const double c = cs[k];
        double* ap = A + pp[k] * LD + col;
        double* aq = A + qq[k] * LD + col;
        const double x0 = *ap, x1 = *aq;
        *ap = c * x0 - s * x1;
        *aq = s * x0 + c * x1;
      }
      __syncthreads();
      for (int x = tid; x < half * N; x += ES_THREADS) {   // columns p, q of (J^T A) J
        const int k = x / N, r = x - k * N;
        const double s = sn[k];
        if (s == 0.0) continue;
        const double c = cs[k];
        double* ap = A + r * LD + pp[k];
        double* aq = A + r * LD + qq[k];
        const double x0 = *ap, x1 = *aq;
        *ap = c * x0 - s * x1;
        *aq = s * x0 + c * x1;
      }
      __syncthreads();
      if (tid < half && sn[tid] != 0.0) { A[pp[tid] * LD + qq[tid]] = 0.0; A[qq[tid] * LD + pp[tid]] = 0.0; }   // the pivots, exactly
      __syncthreads();
    }
  }
  // descending, stable
  for (int i = tid; i < N; i += ES_THREADS) {
    const double d = A[i * LD + i];
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const double dj = A[j * LD + j];
      rank += dj > d || (dj == d && j < i);
    }
    a.eig[(size_t)p * N + rank] = d;
  }
}

size_t es_eigen_lds(int N) { return ((size_t)N * (N | 1) + 128 + ES_THREADS) * sizeof(double) + 128 * sizeof(int); }

bool es_desc_ok(const ssc_eval_set_desc* d) {
  return d && d->P >= 1 && d->N >= 2 && d->N <= EV_MAX_N && d->steps >= 1 && d->V >= 1 && d->V <= 65535 &&
         (int64_t)d->P * d->N <= (1 << 24) && d->predictions && d->ref_image && d->set_counts && d->eigenvalues && d->distinct;
}

}  // namespace

extern "C" size_t ssc_eval_refs_bytes(int I, int nref, int ntok) {
  if (I < 1 || I > (1 << 24) || nref < I || nref > (1 << 26) || ntok < nref || ntok > (1 << 26)) return 0;
  return ev_layout(I, nref, ntok).total;
}

extern "C" int ssc_eval_prepare_refs(const ssc_eval_refs* r, void* stream) {
  if (!ev_refs_ok(r)) return SSC_EINVAL;
  const EvLayout l = ev_layout(r->I, r->nref, r->ntok);
  if (r->state_bytes < l.total) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const EvState s = ev_state(r);
  if (hipMemsetAsync(r->state, 0, l.total, st) != hipSuccess) return SSC_EHIP;
  SSC_LAUNCH(ev_ref_ngrams, dim3(r->nref), dim3(64), 0, st, r->tok_offsets, r->tokens, r->ntok, r->W, s);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(ev_ref_df, dim3(r->I), dim3(64), 0, st, r->ref_offsets, r->nref, r->style, r->W, s);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(ev_ref_weights, dim3(r->nref), dim3(64), 0, st, r->I, s);
  SSC_CHECK_LAUNCH();
  return ev_read_flag(s.flag, st);
}

extern "C" size_t ssc_eval_score_workspace_bytes(const ssc_eval_refs* r, const ssc_eval_score_desc* d) {
  (void)r; (void)d;
  return 256;
}

extern "C" int ssc_eval_score(const ssc_eval_refs* r, const ssc_eval_score_desc* d, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (!ev_refs_ok(r) || !d) return SSC_EINVAL;
  if (d->P < 1 || d->N < 1 || d->N > EV_MAX_N || d->steps < 1 || d->V < 1 || d->V > 65535 || (int64_t)d->P * d->N > (1 << 24) ||
      !d->predictions || !d->id_map || !d->ref_image || !d->scores || !d->counts || !d->image_counts || !d->top5)
    return SSC_EINVAL;
  if (r->state_bytes < ev_layout(r->I, r->nref, r->ntok).total || !workspace || workspace_bytes < 256) return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const EvState s = ev_state(r);
  EvScoreArgs a{d->predictions, d->N, d->steps, d->boundary_index, d->V, r->I, r->nref, r->W, d->id_map, d->style_ids, d->ref_image,
                r->ref_offsets, r->tokens, d->scores, d->counts, d->image_counts, d->top5, r->style, (int*)workspace};
  if (hipMemsetAsync(workspace, 0, sizeof(int), st) != hipSuccess) return SSC_EHIP;
  SSC_LAUNCH(ev_score, dim3(d->P * d->N), dim3(64), 0, st, a, s);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(ev_image, dim3(d->P), dim3(256), 0, st, a, s);
  SSC_CHECK_LAUNCH();
  return ev_read_flag(a.flag, st);
}

extern "C" size_t ssc_eval_set_workspace_bytes(const ssc_eval_refs* r, const ssc_eval_set_desc* d) {
  if (!es_desc_ok(d) || (r && (!ev_refs_ok(r) || !d->id_map))) return 0;
  return es_layout(d->P, d->N, d->steps, r && !d->kernel).total;
}

extern "C" int ssc_eval_set(const ssc_eval_refs* r, const ssc_eval_set_desc* d, void* workspace, size_t workspace_bytes,
                            void* stream) {
  if (!es_desc_ok(d) || (r && (!ev_refs_ok(r) || !d->id_map))) return SSC_EINVAL;
  const EsLayout l = es_layout(d->P, d->N, d->steps, r && !d->kernel);
  if (!workspace || workspace_bytes < l.total || (r && r->state_bytes < ev_layout(r->I, r->nref, r->ntok).total))
    return SSC_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* b = (char*)workspace;
  // without references no image has a kernel matrix: es_pair skips it, es_eigen writes zero eigenvalues
  double* kmat = r ? (d->kernel ? d->kernel : (double*)(b + l.kmat)) : nullptr;
  EsArgs a{d->predictions, d->N, d->steps, d->boundary_index, d->V, r ? r->I : 0, r ? r->W : 0, l.S, d->id_map, d->ref_image,
           (unsigned long long*)(b + l.key), (double*)(b + l.w), (int*)(b + l.tf), (int*)(b + l.nu), (int*)(b + l.len),
           (double*)(b + l.norm), (int*)(b + l.first), d->set_counts, kmat, d->eigenvalues, d->distinct,
           (int*)(b + l.flag)};
  EvState s{};
  if (r) s = ev_state(r);
  if (hipMemsetAsync(a.flag, 0, sizeof(int), st) != hipSuccess) return SSC_EHIP;
  if (!r && d->kernel && hipMemsetAsync(d->kernel, 0, (size_t)d->P * d->N * d->N * sizeof(double), st) != hipSuccess) return SSC_EHIP;
  SSC_LAUNCH(es_caption, dim3(d->P * d->N), dim3(64), 0, st, a, s);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(es_pair, dim3(d->P * d->N), dim3(64), 0, st, a);
  SSC_CHECK_LAUNCH();
  const size_t lds = es_eigen_lds(d->N);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)es_eigen, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return SSC_EHIP;
  SSC_LAUNCH(es_eigen, dim3(d->P), dim3(ES_THREADS), lds, st, a);
  SSC_CHECK_LAUNCH();
  return ev_read_flag(a.flag, st);
}
