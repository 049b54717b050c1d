// Latent-guided decoding (include/ssc.h: ssc_latent_guide): the z block of a decode step drawn from a caller's per-entry, per-step
// distribution - the stored z path of a posterior forward, an interpolation of two, a jittered exemplar - instead of the configured
// prior, and the caption comparison a reconstruction is judged by.
//
// ssc_latent_guide_rows is the decode step's latent launch (ssc_latent_prior_sample's place): row r belongs to entry
// b = r / rows_per_entry; a guided entry gets z = eps * sqrtf(var[t, b]) + mean[t, b] - the expression of
// latent_prior_sample_pm_kernel (pointwise.hip), so a decode driven step by step with (rows, Z) operands gives the same bits -, an
// unguided one the expression of latent_prior_sample_pm_kernel.  One thread per (row, four columns); whether an entry is guided is read
// once per thread and is the same for every thread of a row.  Each of the three operands (eps, the guide, z) is touched with 16-byte
// accesses where its leading dimension and base allow and with scalar accesses otherwise; the arithmetic is the same either way
// (-ffp-contract=off), so the bits do not depend on the path.  Columns >= Z of the inputs are never read; with var NULL a guided
// row never reads eps.  No atomics.
//
// ssc_caption_match: one thread per (prediction, reference) pair - lengths, equal positions, exact match and the word-level
// Levenshtein distance by the two-row dynamic programme, the row kept in LDS (L <= 128: distances fit 16 bits).  Integer arithmetic
// in a fixed order: two calls give the same bits.
#include <math.h>

#include "decode_loop.h"

namespace {

struct GuideRowsArgs {
  const float* mean; const float* var; const int* len;   // slab t of the guide: (B, ld); var / len may be NULL
  int ld, t;
  const float* eps; int ldeps;
  const float* sent; float pm_scale, sd;
  int rows, rows_per_entry, Z, Q;   // Q = quads per row: ceil(Z / 4)
  float* z; int ldz;
  int vec_eps, vec_guide, vec_z;   // 16-byte accesses allowed on that operand
};

// columns [c, c + 4) of a row: one 16-byte load where allowed and all four columns are below Z, else the columns below Z one by one
__device__ __forceinline__ void guide_load4(const float* __restrict__ row, int c, int Z, bool vec, float (&x)[4]) {
  if (vec && c + 4 <= Z) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = c + u < Z ? row[c + u] : 0.f;
  }
}

__global__ __launch_bounds__(256) void latent_guide_rows_kernel(const GuideRowsArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.rows * a.Q) return;
  const int r = (int)(i / a.Q), c = (int)(i % a.Q) * 4;
  const int b = r / a.rows_per_entry;
  const int Z = a.Z;
  const bool guided = !a.len || a.t < a.len[b];   // (the same for every thread of row r)
  float zz[4];
  if (guided) {
    float m[4];
    guide_load4(a.mean + (size_t)b * a.ld, c, Z, a.vec_guide != 0, m);
    if (a.var) {
      float v[4], e[4];
      guide_load4(a.var + (size_t)b * a.ld, c, Z, a.vec_guide != 0, v);
      guide_load4(a.eps + (size_t)r * a.ldeps, c, Z, a.vec_eps != 0, e);
#pragma unroll
      for (int u = 0; u < 4; ++u) zz[u] = e[u] * sqrtf(v[u]) + m[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) zz[u] = m[u];
    }
  } else {
    float e[4];
    guide_load4(a.eps + (size_t)r * a.ldeps, c, Z, a.vec_eps != 0, e);
    const float pm = a.sent ? a.pm_scale * a.sent[r] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) zz[u] = e[u] * a.sd + pm;
  }
  // pad columns Z .. round4(Z) of a 16-byte padded row are zeroed, as latent_prior_sample_pm_kernel zeroes them
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (c + u >= Z) zz[u] = 0.f;
  float* zr = a.z + (size_t)r * a.ldz;
  if (a.vec_z) {   // (ldz % 4 == 0 and ldz >= Z: the whole quad lies inside the row)
    *reinterpret_cast<float4*>(zr + c) = make_float4(zz[0], zz[1], zz[2], zz[3]);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c + u < a.ldz) zr[c + u] = zz[u];
  }
}

constexpr int MATCH_MAX_L = 128;
constexpr int MATCH_THREADS = 64;

// tokens before the first end_index or negative id
__device__ __forceinline__ int caption_len(const int64_t* __restrict__ c, int L, int end_index) {
  int n = 0;
  while (n < L && c[n] >= 0 && c[n] != end_index) ++n;
  return n;
}

__global__ __launch_bounds__(MATCH_THREADS) void caption_match_kernel(const int64_t* __restrict__ pred, int Lp,
                                                                      const int64_t* __restrict__ ref, int Lr, int n, int end_index,
                                                                      int* __restrict__ out) {
  // the dynamic programme's row of every thread, entry j of thread x at [j][x]: the threads of a wave hit distinct banks
  __shared__ unsigned short row[MATCH_MAX_L + 1][MATCH_THREADS];
  const int x = threadIdx.x;
  const int q = blockIdx.x * MATCH_THREADS + x;
  if (q >= n) return;
  const int64_t* p = pred + (size_t)q * Lp;
  const int64_t* g = ref + (size_t)q * Lr;
  const int np = caption_len(p, Lp, end_index), nr = caption_len(g, Lr, end_index);
  const int nm = np < nr ? np : nr;
  int eq = 0;
  for (int j = 0; j < nm; ++j) eq += p[j] == g[j] ? 1 : 0;
  // row[j] = distance between the first i words of the prediction and the first j words of the reference
  for (int j = 0; j <= nr; ++j) row[j][x] = (unsigned short)j;
  for (int i = 1; i <= np; ++i) {
    const int64_t w = p[i - 1];
    int diag = row[0][x];   // D[i-1][j-1]
    int left = i;           // D[i][j-1]
    row[0][x] = (unsigned short)i;
    for (int j = 1; j <= nr; ++j) {
      const int up = row[j][x];   // D[i-1][j]
      int d = diag + (w == g[j - 1] ? 0 : 1);
      d = d < up + 1 ? d : up + 1;
      d = d < left + 1 ? d : left + 1;
      row[j][x] = (unsigned short)d;
      diag = up;
      left = d;
    }
  }
  int* o = out + (size_t)q * 5;
  o[0] = np; o[1] = nr; o[2] = eq; o[3] = (np == nr && eq == np) ? 1 : 0; o[4] = row[nr][x];
}

bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

}  // namespace

bool ssc_latent_guide_ok(const ssc_model_cfg* cfg, const ssc_latent_guide* g) {
  if (!cfg || !g || cfg->kld_mode == 2) return false;   // (SENTIMENT_VAE = 2: the pooled prior mean also conditions the LSTMs)
  if (g->steps < 1 || !g->mean || g->ld < cfg->Z) return false;
  return aligned4(g->mean) && aligned4(g->var) && aligned4(g->len);
}

extern "C" int ssc_latent_guide_rows(const ssc_latent_guide* g, int t, int rows, int rows_per_entry, int Z, const float* eps,
                                     int ldeps, const float* sent, float pm_scale, float prior_var, float* z, int ldz,
                                     void* stream) {
  if (!eps || !z || rows <= 0 || Z <= 0 || t < 0 || ldeps < Z || ldz < Z) return SSC_EINVAL;
  if (g && g->steps < 1) return SSC_EINVAL;
  if (!g || t >= g->steps)   // no guide at this step: exactly the launch of an unguided decode
    return ssc_latent_prior_sample(eps, ldeps, sent, pm_scale, prior_var, rows, Z, z, ldz, stream);
  if (rows_per_entry <= 0 || rows % rows_per_entry != 0 || !g->mean || g->ld < Z) return SSC_EINVAL;
  if (!aligned4(g->mean) || !aligned4(g->var) || !aligned4(g->len) || !aligned4(eps) || !aligned4(z) || !aligned4(sent)) return SSC_EINVAL;
  const size_t B = (size_t)(rows / rows_per_entry);
  GuideRowsArgs a{};
  a.mean = g->mean + (size_t)t * B * g->ld;
  a.var = g->var ? g->var + (size_t)t * B * g->ld : nullptr;
  a.len = g->len; a.ld = g->ld; a.t = t;
  a.eps = eps; a.ldeps = ldeps; a.sent = sent; a.pm_scale = pm_scale; a.sd = sqrtf(prior_var);
  a.rows = rows; a.rows_per_entry = rows_per_entry; a.Z = Z; a.Q = ssc_cdiv(Z, 4);
  a.z = z; a.ldz = ldz;
  a.vec_eps = ldeps % 4 == 0 && ssc_aligned16(eps);
  a.vec_guide = g->ld % 4 == 0 && ssc_aligned16(a.mean) && (!a.var || ssc_aligned16(a.var));
  a.vec_z = ldz % 4 == 0 && ssc_aligned16(z);
  const long work = (long)rows * a.Q;
  if (work > (1L << 31) - 256) return SSC_EINVAL;
  SSC_LAUNCH(latent_guide_rows_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_caption_match(const int64_t* pred, int Lp, const int64_t* ref, int Lr, int n, int end_index, int* out,
                                 void* stream) {
  if (!pred || !ref || !out || n < 0 || Lp < 1 || Lr < 1 || Lp > MATCH_MAX_L || Lr > MATCH_MAX_L || end_index < 0) return SSC_EINVAL;
  if (n == 0) return SSC_OK;
  SSC_LAUNCH(caption_match_kernel, dim3(ssc_cdiv(n, MATCH_THREADS)), dim3(MATCH_THREADS), 0, (hipStream_t)stream, pred, Lp, ref, Lr, n,
             end_index, out);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
