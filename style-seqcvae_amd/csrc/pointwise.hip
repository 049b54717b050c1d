// Elementwise / small-reduction kernels of the var_updown hot path (gfx950, wave64).
// All of them are HBM-bound byte movers; they are written for coalesced access along the contiguous
// axis and 64-lane shuffle reductions.  Reference citations are on the C entry points in ssc.h.
#include <algorithm>

#include "latent_common.h"
#include "ssc_common.h"

thread_local int ssc_tls_hip_error = 0;

extern "C" int ssc_version(void) { return 4; }
extern "C" int ssc_last_hip_error(void) { return ssc_tls_hip_error; }
extern "C" const char* ssc_arch(void) { return "gfx950"; }

namespace {

// ---------------------------------------------------------------------------------------------
// feat_prep: mask[b,r] = (sum_f |v| > 0) ; avg[b,f] = sum_r mask*v / max(sum_r mask, 1e-8)
// ---------------------------------------------------------------------------------------------
// One workgroup per image, ONE pass over its (R, F) block.  Thread = column (1024 per sweep): it walks the R regions with eight
// loads in flight and sums them in region order - a masked region is an all-zero row and adds exactly zero, so the sum needs no
// mask and no multiply - and every wave flags the regions in which it met a non-zero entry (sum_f |v| > 0 <=> some v != 0).
// Then the workgroup forms the mask and the count and divides the sums it left in avg.
constexpr int kFeatPrepThreads = 1024;
__global__ __launch_bounds__(kFeatPrepThreads) void feat_prep_kernel(const float* __restrict__ feats, int R, int F,
                                                                     float* __restrict__ mask, float* avg) {
  extern __shared__ int nz[];   // [R]
  __shared__ float wave_n[kFeatPrepThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* p = feats + (size_t)b * R * F;
  for (int r = tid; r < R; r += kFeatPrepThreads) nz[r] = 0;
  __syncthreads();
  for (int f0 = 0; f0 < F; f0 += kFeatPrepThreads) {
    const int f = f0 + tid;
    const bool in = f < F;
    const int fc = in ? f : F - 1;
    float s = 0.f;
    for (int r = 0; r < R; r += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = p[(size_t)min(r + u, R - 1) * F + fc];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r + u < R) {
          s += x[u];
          const bool any = __ballot(in && fabsf(x[u]) > 0.f) != 0ull;
          if (any && lane == 0) nz[r + u] = 1;   // (every writer stores the same value)
        }
    }
    if (in) avg[(size_t)b * F + f] = s;
  }
  __syncthreads();
  float n = 0.f;   // a count: exact in any order
  for (int r = tid; r < R; r += kFeatPrepThreads) {
    const float m = nz[r] ? 1.f : 0.f;
    mask[(size_t)b * R + r] = m;
    n += m;
  }
  n = ssc_wave_sum(n);
  if (lane == 0) wave_n[tid >> 6] = n;
  __syncthreads();
  n = 0.f;
  for (int q = 0; q < kFeatPrepThreads / 64; ++q) n += wave_n[q];
  const float d = fmaxf(n, 1e-8f);
  for (int f = tid; f < F; f += kFeatPrepThreads) avg[(size_t)b * F + f] = avg[(size_t)b * F + f] / d;   // this thread's own sums
}

// ---------------------------------------------------------------------------------------------
__global__ void prep_tokens_kernel(const int64_t* __restrict__ caps, int B, int L, int pad, int boundary,
                                   int64_t* __restrict__ tok, float* __restrict__ w, float* __restrict__ nvalid) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int n = 0;
  for (int j = 0; j < L; ++j) n += caps[(size_t)b * L + j] != pad;
  tok[b] = boundary;
  for (int j = 0; j < L; ++j) tok[(size_t)(1 + j) * B + b] = caps[(size_t)b * L + j];
  tok[(size_t)(L + 1) * B + b] = 0;
  tok[(size_t)(n + 1) * B + b] = boundary;
  float nv = 0.f;
  for (int t = 0; t <= L; ++t) {
    float wt = tok[(size_t)(t + 1) * B + b] != pad ? 1.f : 0.f;
    w[(size_t)t * B + b] = wt;
    nv += wt;
  }
  nvalid[b] = nv;
}

__global__ void embed_gather_kernel(const float* __restrict__ table, int ldt, const int64_t* __restrict__ ids, int n, int E,
                                    float* __restrict__ out, int ldo) {
  int i = blockIdx.y;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  out[(size_t)i * ldo + e] = table[(size_t)ids[i] * ldt + e];
}

// Deterministic: float atomics would add a token's rows in whatever order the blocks arrive, so the rounding (and, through the
// next steps, the whole training run) would change from run to run.  Instead the blocks of a token's FIRST position sum the rows
// of all its positions in ascending position order and add that sum with a plain store (once per kEmbedScatterChunk positions);
// the blocks of its later positions exit.  The positions are listed in LDS first so that the sum keeps kEmbedScatterRows loads
// in flight: a frequent token (the boundary token opens every caption) is not a chain of one load after another.
constexpr int kEmbedScatterThreads = 256;
constexpr int kEmbedScatterChunk = 4096;   // positions listed per pass
constexpr int kEmbedScatterBatch = 8;    // ids loaded per thread before comparing
constexpr int kEmbedScatterRows = 32;    // rows of d loaded per thread before adding
__global__ void __launch_bounds__(kEmbedScatterThreads) embed_scatter_kernel(float* __restrict__ dt, int ldt,
                                                                               const int64_t* __restrict__ ids, int n, int E,
                                                                               const float* __restrict__ d, int ldd, int pad) {
  __shared__ unsigned long long s_hit[kEmbedScatterChunk / SSC_WAVE];   // bit b of word w: ids[c0 + 64 w + b] == id
  __shared__ int s_pos[kEmbedScatterChunk + kEmbedScatterRows];         // matching positions - c0, ascending
  __shared__ int s_cnt;
  const int i = blockIdx.y;
  const int e = blockIdx.x * kEmbedScatterThreads + threadIdx.x;
  const int64_t id = ids[i];
  if (id == pad) return;   // (uniform over the block, as is the exit below)
  // both scans over the ids below load kEmbedScatterBatch of them per thread before comparing: one memory latency per
  // 2048 positions instead of one per 256
  constexpr int kSpan = kEmbedScatterBatch * kEmbedScatterThreads;
  bool earlier = false;
  for (int j0 = threadIdx.x; j0 < i; j0 += kSpan) {
    int64_t v[kEmbedScatterBatch];
#pragma unroll
    for (int u = 0; u < kEmbedScatterBatch; ++u) v[u] = ids[min(j0 + u * kEmbedScatterThreads, i - 1)];   // (clamped: no branch per load)
#pragma unroll
    for (int u = 0; u < kEmbedScatterBatch; ++u) earlier |= j0 + u * kEmbedScatterThreads < i && v[u] == id;
  }
  if (__syncthreads_or(earlier)) return;
  const int lane = threadIdx.x % SSC_WAVE;
  for (int c0 = i; c0 < n; c0 += kEmbedScatterChunk) {
    const int cn = min(kEmbedScatterChunk, n - c0);
    for (int k0 = 0; k0 < cn; k0 += kSpan) {   // (k0 is 0 or 2048: word (k0 + 256 u + 64 wave) / 64 < 64)
      int64_t v[kEmbedScatterBatch];
#pragma unroll
      for (int u = 0; u < kEmbedScatterBatch; ++u) v[u] = ids[c0 + min(k0 + u * kEmbedScatterThreads + (int)threadIdx.x, cn - 1)];
#pragma unroll
      for (int u = 0; u < kEmbedScatterBatch; ++u) {
        const unsigned long long hit = __ballot(k0 + u * kEmbedScatterThreads + (int)threadIdx.x < cn && v[u] == id);
        if (lane == 0) s_hit[(k0 + u * kEmbedScatterThreads + threadIdx.x) / SSC_WAVE] = hit;
      }
    }
    __syncthreads();
    const int nw = (cn + SSC_WAVE - 1) / SSC_WAVE;
    if (threadIdx.x < SSC_WAVE) {   // wave 0: word w's positions go behind those of words 0 .. w-1 (prefix sum over the lanes)
      const unsigned long long m0 = lane < nw ? s_hit[lane] : 0ull;
      const int c = __popcll(m0);
      int incl = c;
#pragma unroll
      for (int o = 1; o < SSC_WAVE; o <<= 1) {
        const int t = __shfl_up(incl, o, SSC_WAVE);
        if (lane >= o) incl += t;
      }
      int q = incl - c;
      for (unsigned long long m = m0; m; m &= m - 1) s_pos[q++] = lane * SSC_WAVE + __builtin_ctzll(m);
      if (lane == SSC_WAVE - 1) s_cnt = incl;
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (e < E) {
      float s = 0.f;
      for (int q0 = 0; q0 < cnt; q0 += kEmbedScatterRows) {
        float v[kEmbedScatterRows];
#pragma unroll
        for (int u = 0; u < kEmbedScatterRows; ++u)
          v[u] = q0 + u < cnt ? d[(size_t)(c0 + s_pos[q0 + u]) * ldd + e] : 0.f;
#pragma unroll
        for (int u = 0; u < kEmbedScatterRows; ++u)
          if (q0 + u < cnt) s += v[u];
      }
      dt[(size_t)id * ldt + e] += s;
    }
    __syncthreads();   // (s_hit, s_pos and s_cnt are rewritten by the next chunk)
  }
}

// ---------------------------------------------------------------------------------------------
// latent head: mu / log_var / z / KL of one step and its backward, plain (FB = 0) or with a free-bits floor on the KL
// (FB = 1..3, the modes of include/ssc.h: ssc_free_bits).  Every form is built from the pieces below, so mu / lv / z and the raw KL
// are the same bits in all of them; latent_fb_elem and latent_fb_row are the only place where the modes differ.
// ---------------------------------------------------------------------------------------------
// m, l += slabs [s_lo, s_hi) of element (b, z) in index order, U loads of each in flight: the loads of a round are clamped to the
// last valid slab and all issued before the adds, a term past the range is added as 0
template <int U>
__device__ __forceinline__ void latent_sum_slabs(const ssc_latent_fwd_desc& d, int b, int z, int s_lo, int s_hi, float& m, float& l) {
  for (int s0 = s_lo; s0 < s_hi; s0 += U) {
    float tm[U], tl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* row = d.mulv + (size_t)min(s0 + u, s_hi - 1) * d.slab_stride + (size_t)b * d.ldmulv;
      tm[u] = row[z];
      tl[u] = row[d.Z + z];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m += (s0 + u < s_hi) ? tm[u] : 0.f;
      l += (s0 + u < s_hi) ? tl[u] : 0.f;
    }
  }
}

// the summed (m, l) of element (b, z): biases, the sample, the three stores; returns the element's KL k_tbj
__device__ __forceinline__ float latent_finish_elem(const ssc_latent_fwd_desc& d, int b, int z, float m, float l) {
  const float pm = latent_prior_mean(d.pm, d.ldpm, d.sent, d.pm_scale, b, z);   // (before the stores: no load may be moved across them)
  m += d.bmu[z];
  l += d.blv[z];
  const float var = expf(l);
  const float zz = d.eps[(size_t)b * d.ldeps + z] * sqrtf(var) + m;
  d.mu[(size_t)b * d.ldz + z] = m;
  d.lv[(size_t)b * d.ldz + z] = l;
  d.z[(size_t)b * d.ldz + z] = zz;
  return latent_kl_elem(d.kld_mode, m, l, var, pm, logf(d.prior_var), d.prior_var);
}

// what one (b, j) element adds: to the raw sum, to the floored sum (mode 1) and to the (B, lddim) accumulator (mode 3)
template <int FB>
__device__ __forceinline__ void latent_fb_elem(const ssc_latent_fwd_desc& d, const ssc_free_bits& fb, float k, int b, int z, float& raw,
                                               float& flo) {
  raw += k;
  if (FB == 1) flo += k > fb.lambda ? k : fb.lambda;
  if (FB == 3) fb.dim_acc[(size_t)b * fb.lddim + z] += d.w[b] * k;
}

// the row's sums (already reduced over j) into the accumulators; FB = 0 touches no field of fb.  (The step weight is read where
// it is used, by the one lane that writes the row: read ahead of the slab loads it would hold them back by a memory round trip.)
template <int FB>
__device__ __forceinline__ void latent_fb_row(const ssc_latent_fwd_desc& d, const ssc_free_bits& fb, int b, float raw, float flo) {
  const float wb = d.w[b];
  if (FB == 0) {
    d.kld_acc[b] += wb * raw;
    return;
  }
  fb.kld_raw[b] += wb * raw;
  if (FB == 1) d.kld_acc[b] += wb * flo;
  if (FB == 2) {
    const bool open = raw > fb.lambda;
    d.kld_acc[b] += wb * (open ? raw : fb.lambda);
    fb.gate_step[b] = open ? 1.f : 0.f;
  }
}

// one wave per row, four rows per workgroup
template <int FB>
__global__ void latent_fwd_kernel(const ssc_latent_fwd_desc d, const ssc_free_bits fb) {
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= d.B) return;
  float raw = 0.f, flo = 0.f;
  for (int z = lane; z < d.Z; z += 64) {
    float m = 0.f, l = 0.f;
    latent_sum_slabs<8>(d, b, z, 0, d.nslab, m, l);
    latent_fb_elem<FB>(d, fb, latent_finish_elem(d, b, z, m, l), b, z, raw, flo);
  }
  raw = ssc_wave_sum(raw);
  if (FB == 1) flo = ssc_wave_sum(flo);
  if (lane == 0) latent_fb_row<FB>(d, fb, b, raw, flo);
}

// The form for MANY partial slabs (the cdiv(H,16) partial products of lstm_fwd_p_kernel): one 256-thread workgroup per row; the
// slab list is split into 256 / (64 ceil(Z/64)) contiguous parts that are summed in parallel (each in index order) and combined in
// part order - fixed summation order, four times the loads in flight of the wave-per-row form.  Z <= 256.
template <int FB>
__global__ __launch_bounds__(256) void latent_fwd_wide_kernel(const ssc_latent_fwd_desc d, const ssc_free_bits fb) {
  __shared__ float pm_[4][64], pl_[4][64], kr_[4], kf_[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int Z = d.Z;
  const int ZW = (Z + 63) / 64;            // waves per full z range (1, 2 or 4)
  const int SP = 4 / ZW;                   // slab parts
  const int zw = wave % ZW, part = wave / ZW;
  const int z = zw * 64 + lane;
  const int per = (d.nslab + SP - 1) / SP;
  const int s_lo = part * per, s_hi = min(d.nslab, s_lo + per);
  float m = 0.f, l = 0.f;
  if (z < Z && ZW * SP == 4) latent_sum_slabs<16>(d, b, z, s_lo, s_hi, m, l);
  pm_[wave][lane] = m;
  pl_[wave][lane] = l;
  __syncthreads();
  float raw = 0.f, flo = 0.f;
  if (part == 0 && z < Z) {
    for (int p = 1; p < SP; ++p) { m += pm_[p * ZW + zw][lane]; l += pl_[p * ZW + zw][lane]; }
    latent_fb_elem<FB>(d, fb, latent_finish_elem(d, b, z, m, l), b, z, raw, flo);
  }
  raw = ssc_wave_sum(raw);
  if (FB == 1) flo = ssc_wave_sum(flo);
  if (lane == 0) {
    kr_[wave] = raw;
    if (FB == 1) kf_[wave] = flo;
  }
  __syncthreads();
  if (tid == 0) {
    float r = 0.f, f = 0.f;
    for (int w2 = 0; w2 < ZW; ++w2) {   // waves of part 0, in z order
      r += kr_[w2];
      if (FB == 1) f += kf_[w2];
    }
    latent_fb_row<FB>(d, fb, b, r, f);
  }
}

// z = eps * sd + prior mean, per row g; pm: a per-row, per-dimension prior mean (SENTIMENT_VAE = 2: the attention-pooled attribute
// means, updown_cell.py:160-163), pv: a per-element prior variance in place of sd^2 (a caller of _decode_step that hands its own
// prior, updown_captioner.py:371-381); both optional
__global__ void latent_prior_sample_pm_kernel(const float* __restrict__ eps, int ldeps, const float* __restrict__ pm, int ldpm,
                                              const float* __restrict__ pv, int ldpv, const float* __restrict__ sent, float pm_scale,
                                              float sd, int G, int Z, float* __restrict__ z, int ldz) {
  int g = blockIdx.y;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Z) {   // pad columns of a 16-byte padded row are zeroed (the row is a K-segment of r4(Z) columns in the decode step)
    if (i < ((Z + 3) & ~3) && i < ldz) z[(size_t)g * ldz + i] = 0.f;
    return;
  }
  const float m = latent_prior_mean(pm, ldpm, sent, pm_scale, g, i);
  const float s = pv ? sqrtf(pv[(size_t)g * ldpv + i]) : sd;
  z[(size_t)g * ldz + i] = eps[(size_t)g * ldeps + i] * s + m;
}

// mode 3 after the last step: one workgroup.  K_j over b in index order, the Z gates, then kld_b (one wave per row at a time)
__global__ __launch_bounds__(256) void latent_fb_finish_kernel(const float* __restrict__ acc, int ld, int B, int Z, float lambda,
                                                               float* __restrict__ kdim, float* gate, float* __restrict__ kld) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int j = tid; j < Z; j += 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += acc[(size_t)b * ld + j];
    const float k = s / (float)B;
    kdim[j] = k;
    gate[j] = k > lambda ? 1.f : 0.f;
  }
  __syncthreads();   // (the gates of this workgroup's own stores)
  for (int b = wave; b < B; b += 4) {
    float s = 0.f;
    for (int j = lane; j < Z; j += 64) s += gate[j] != 0.f ? acc[(size_t)b * ld + j] : lambda;
    s = ssc_wave_sum(s);
    if (lane == 0) kld[b] = s;
  }
}

// dz += the split-K slabs of the producing GEMM in index order, eight loads in flight
__device__ __forceinline__ void latent_bwd_sum_slabs(const float* slabs, int n, size_t stride, size_t cell, float& dz) {
  for (int s0 = 0; s0 < n; s0 += 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = slabs[(size_t)min(s0 + u, n - 1) * stride + cell];
#pragma unroll
    for (int u = 0; u < 8; ++u) dz += (s0 + u < n) ? t[u] : 0.f;
  }
}

// FB = 1..3: the KL part of dmu, dlv and dpm is multiplied by the element's gate (mode 1 forms it again from mu / lv with the
// forward's latent_kl_elem, modes 2 and 3 read it); FB = 0 leaves k alone
template <int FB>
__global__ void latent_bwd_kernel(const ssc_latent_bwd_desc d, const ssc_free_bits fb) {
  int b = blockIdx.y;
  int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z >= d.Z) return;
  float k = d.gk[b] * d.w[b];
  float m = d.mu[(size_t)b * d.ldz + z], l = d.lv[(size_t)b * d.ldz + z];
  float dz = 0.f;
  latent_bwd_sum_slabs(d.dz, d.nslab > 1 ? d.nslab : 1, d.slab_stride, (size_t)b * d.lddz + z, dz);
  float e = d.eps[(size_t)b * d.ldeps + z];
  float var = expf(l);
  const float pm = d.kld_mode == 0 ? 0.f : latent_prior_mean(d.pm, d.ldpm, d.sent, d.pm_scale, b, z);
  if (FB != 0) {
    bool open;
    if (FB == 1) open = latent_kl_elem(d.kld_mode, m, l, var, pm, logf(d.prior_var), d.prior_var) > fb.lambda;
    else if (FB == 2) open = fb.gate_step[b] != 0.f;
    else open = fb.gate_dim[z] != 0.f;
    k = open ? k : 0.f;   // a closed gate: the KL part is +0 times its factor, as with gk = 0
  }
  float dmu, dlv;
  if (d.kld_mode == 0) {
    dmu = dz + k * m;
    dlv = dz * e * 0.5f * sqrtf(var) - 0.5f * k * (1.f - var);
  } else {
    float den = d.prior_var + 0.00001f;
    dmu = dz + k * (m - pm) / den;
    if (d.dpm) d.dpm[(size_t)b * d.lddpm + z] = -k * (m - pm) / den;
    dlv = dz * e * 0.5f * sqrtf(var) - 0.5f * k * (1.f - var / den);
  }
  d.dmulv[(size_t)b * d.lddmulv + z] = dmu;
  d.dmulv[(size_t)b * d.lddmulv + d.Z + z] = dlv;
}


// ---------------------------------------------------------------------------------------------
// log-softmax over the vocabulary
// ---------------------------------------------------------------------------------------------
__global__ void log_softmax_kernel(const float* __restrict__ logits, int ldl, int V, float* __restrict__ out, int ldo) {
  __shared__ float sh[16];
  int row = blockIdx.x;
  const float* p = logits + (size_t)row * ldl;
  float* o = out + (size_t)row * ldo;
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, p[v]);
  mx = ssc_block_reduce(mx, sh, true);
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) s += expf(p[v] - mx);
  s = ssc_block_reduce(s, sh, false);
  float l = mx + logf(s);
  for (int v = threadIdx.x; v < V; v += blockDim.x) o[v] = p[v] - l;
}

// ---------------------------------------------------------------------------------------------
// column sums, tanh, fill
// ---------------------------------------------------------------------------------------------
// column sums in two deterministic stages: stage 1 - workgroup (column slice of 256, row chunk) -> partials
// [chunk][N] (thread per column: 1 KiB coalesced row reads); stage 2 - sum the chunks, write out (and out2).
constexpr int COLSUM_CHUNKS = 64;   // 19 column slices x 64 row chunks = 1216 workgroups at N = 4H (latency-bound otherwise)
__global__ __launch_bounds__(256) void colsum_stage1_kernel(const float* __restrict__ X, int ldx, int rows, int N,
                                                            const float* __restrict__ wrow, float* __restrict__ part) {
  int n = blockIdx.x * 256 + threadIdx.x;
  int chunk = blockIdx.y;
  int per = (rows + COLSUM_CHUNKS - 1) / COLSUM_CHUNKS;
  int r0 = chunk * per, r1 = r0 + per < rows ? r0 + per : rows;
  if (n >= N) return;
  float s = 0.f;
  for (int r = r0; r < r1; r += 8) {  // 8 row loads in flight, summed in row order
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rr = min(r + u, r1 - 1);
      x[u] = X[(size_t)rr * ldx + n];
      if (wrow) x[u] *= wrow[rr];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (r + u < r1) ? x[u] : 0.f;
  }
  part[(size_t)chunk * N + n] = s;
}
__global__ __launch_bounds__(256) void colsum_stage2_kernel(const float* __restrict__ part, int N, float* __restrict__ out,
                                                            int out_stride, float* __restrict__ out2, int accumulate) {
  // 64 columns per workgroup; wave q sums chunks 16q .. 16q+15 (16 loads in flight), wave 0 adds the four partial sums
  __shared__ float sh[4][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + c;
  float t = 0.f;
  if (n < N) {
    float x[COLSUM_CHUNKS / 4];
#pragma unroll
    for (int u = 0; u < COLSUM_CHUNKS / 4; ++u) x[u] = part[(size_t)(q * (COLSUM_CHUNKS / 4) + u) * N + n];
#pragma unroll
    for (int u = 0; u < COLSUM_CHUNKS / 4; ++u) t += x[u];
  }
  sh[q][c] = t;
  __syncthreads();
  if (q != 0 || n >= N) return;
  t = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
  float* o = out + (size_t)n * out_stride;
  *o = accumulate ? *o + t : t;
  if (out2) out2[n] = accumulate ? out2[n] + t : t;
}

// small-row fallback (rows < 64): one pass
__global__ void colsum_kernel(const float* __restrict__ X, int ldx, int rows, int N, const float* __restrict__ wrow,
                              float* __restrict__ out, int out_stride, float* __restrict__ out2, int accumulate) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int r = 0; r < rows; r += 8) {  // 8 row loads in flight, summed in row order
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rr = min(r + u, rows - 1);
      x[u] = X[(size_t)rr * ldx + n];
      if (wrow) x[u] = wrow[rr] * x[u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r + u < rows) s += x[u];
  }
  float* o = out + (size_t)n * out_stride;
  *o = accumulate ? *o + s : s;
  if (out2) out2[n] = accumulate ? out2[n] + s : s;
}

__global__ void copy_strided_kernel(const float* __restrict__ src, size_t stride, int n, float* __restrict__ dst) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[(size_t)i * stride];
}

__global__ void bias_tanh_kernel(float* __restrict__ x, int ldx, int N, const float* __restrict__ bias) {
  int r = blockIdx.y;
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float* p = x + (size_t)r * ldx + n;
  *p = tanhf(*p + (bias ? bias[n] : 0.f));
}

__global__ void tanh_bwd_kernel(float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int N) {
  int r = blockIdx.y;
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float yy = y[(size_t)r * ldy + n];
  dy[(size_t)r * lddy + n] *= (1.f - yy * yy);
}

__global__ void fill_kernel(float* __restrict__ p, size_t n, float v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// ---------------------------------------------------------------------------------------------
// clip + SGD on flat buffers
// ---------------------------------------------------------------------------------------------
// NT: the flat gradient / parameter / momentum buffers (0.45 GB each at C2's widths) are touched once per train step - with
// non-temporal loads and stores they pass the caches by (ssc_g_stream_nt, bit 2; same arithmetic, same order, same bits).
// C2 train step 8.17 -> 8.09 ms, sgd_kernel 431 -> 395 us, sq_norm_partial_kernel 99 -> 76 us.
template <bool NT> __device__ __forceinline__ float stream_ld(const float* p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT> __device__ __forceinline__ void stream_st(float* p, float v) {
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
template <bool NT>
__global__ void sq_norm_partial_kernel(const float* __restrict__ g, size_t n, float* __restrict__ scratch) {
  __shared__ float sh[16];
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  float s = 0.f;
  if (ssc_aligned16_dev(g)) {  // 16 B/lane stream over the bulk, scalar tail
    const size_t n4 = n >> 2;
    const ssc_f32x4* g4 = reinterpret_cast<const ssc_f32x4*>(g);
    for (size_t k = i; k < n4; k += stride) {
      const ssc_f32x4 v = NT ? __builtin_nontemporal_load(&g4[k]) : g4[k];
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (size_t k = (n4 << 2) + i; k < n; k += stride) { const float v = stream_ld<NT>(g + k); s += v * v; }
  } else {
    for (; i < n; i += stride) {
      float v = stream_ld<NT>(g + i);
      s += v * v;
    }
  }
  s = ssc_block_reduce(s, sh, false);
  if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

__global__ void sq_norm_final_kernel(const float* __restrict__ scratch, int nb, float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += scratch[i];
  s = ssc_block_reduce(s, sh, false);
  if (threadIdx.x == 0) *out = s;
}

template <bool NT>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t n,
                           const float* __restrict__ sqnorm, float gscale, float max_norm, float lr, float momentum,
                           float wd, int first) {
  float norm = sqrtf(*sqnorm) * gscale;
  float coef = fminf(1.f, max_norm / (norm + 1e-6f)) * gscale;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float pv = stream_ld<NT>(p + i);
    float dd = stream_ld<NT>(g + i) * coef + wd * pv;
    float b = first ? dd : momentum * stream_ld<NT>(buf + i) + dd;
    stream_st<NT>(buf + i, b);
    stream_st<NT>(p + i, pv - lr * b);
  }
}

// ---------------------------------------------------------------------------------------------
// clip + Adam / AdamW on flat buffers (include/ssc.h states the arithmetic; -ffp-contract=off keeps it as written)
// ---------------------------------------------------------------------------------------------
struct AdamArgs {
  float step_size;   // lr / (1 - beta1^step)
  float rsqrt_bc2;   // 1 / sqrt(1 - beta2^step)
  float beta1, omb1, beta2, omb2, eps, wd;
  float decay;       // 1 - lr * wd (AdamW)
};

template <bool DECOUPLED>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float coef, const AdamArgs& a) {
  float d = g * coef;
  if (DECOUPLED) p = p * a.decay;
  else d = d + a.wd * p;
  m = a.beta1 * m + a.omb1 * d;
  v = a.beta2 * v + a.omb2 * d * d;
  p = p - a.step_size * (m / (sqrtf(v) * a.rsqrt_bc2 + a.eps));
}

// Elements [0, head) and [head + 4 * n4, n) go one by one, the n4 groups of four in between as 16-byte loads and stores
// (p + head is 16-byte aligned in all four buffers; head = n, n4 = 0: the scalar path throughout).
template <bool DECOUPLED>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            size_t n, size_t head, size_t n4, const float* __restrict__ sqnorm, float gscale, float max_norm,
                            AdamArgs a) {
  float norm = sqrtf(*sqnorm) * gscale;
  float coef = fminf(1.f, max_norm / (norm + 1e-6f)) * gscale;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  for (size_t k = i; k < n4; k += stride) {
    float4 pv = p4[k], gv = g4[k], mv = m4[k], vv = v4[k];
    adam_elem<DECOUPLED>(pv.x, gv.x, mv.x, vv.x, coef, a);
    adam_elem<DECOUPLED>(pv.y, gv.y, mv.y, vv.y, coef, a);
    adam_elem<DECOUPLED>(pv.z, gv.z, mv.z, vv.z, coef, a);
    adam_elem<DECOUPLED>(pv.w, gv.w, mv.w, vv.w, coef, a);
    p4[k] = pv;
    m4[k] = mv;
    v4[k] = vv;
  }
  const size_t tail = head + (n4 << 2);
  const size_t ns = head + (n - tail);
  for (size_t k = i; k < ns; k += stride) {
    const size_t e = k < head ? k : tail + (k - head);
    float pv = p[e], mv = m[e], vv = v[e];
    adam_elem<DECOUPLED>(pv, g[e], mv, vv, coef, a);
    p[e] = pv;
    m[e] = mv;
    v[e] = vv;
  }
}

inline hipStream_t S(void* s) { return (hipStream_t)s; }

}  // namespace

// =============================================================================================
extern "C" int ssc_feat_prep(const float* feats, int B, int R, int F, float* mask, float* avg, void* stream) {
  if (!feats || !mask || !avg || B <= 0 || R <= 0 || F <= 0) return SSC_EINVAL;
  if ((size_t)R * sizeof(int) > 48 * 1024) return SSC_EINVAL;   // the region flags of one image live in LDS
  SSC_LAUNCH(feat_prep_kernel, dim3(B), dim3(kFeatPrepThreads), (size_t)R * sizeof(int), S(stream), feats, R, F, mask, avg);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_prep_tokens(const int64_t* caps, int B, int L, int pad, int boundary, int64_t* tokens_tm, float* w_tm,
                               float* nvalid, void* stream) {
  if (!caps || !tokens_tm || !w_tm || !nvalid || B <= 0 || L <= 0) return SSC_EINVAL;
  SSC_LAUNCH(prep_tokens_kernel, dim3(ssc_cdiv(B, 64)), dim3(64), 0, S(stream), caps, B, L, pad, boundary,
                     tokens_tm, w_tm, nvalid);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_embed_gather(const float* table, int ldt, const int64_t* ids, int n, int E, float* out, int ldo,
                                void* stream) {
  if (!table || !ids || !out || n <= 0 || E <= 0 || ldt < E || ldo < E) return SSC_EINVAL;
  SSC_LAUNCH(embed_gather_kernel, dim3(ssc_cdiv(E, 256), n), dim3(256), 0, S(stream), table, ldt, ids, n, E, out,
                     ldo);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_embed_scatter_add(float* dtable, int ldt, const int64_t* ids, int n, int E, const float* d, int ldd,
                                     int pad, void* stream) {
  if (!dtable || !ids || !d || n <= 0 || E <= 0 || ldt < E || ldd < E) return SSC_EINVAL;
  SSC_LAUNCH(embed_scatter_kernel, dim3(ssc_cdiv(E, kEmbedScatterThreads), n), dim3(kEmbedScatterThreads), 0, S(stream), dtable,
             ldt, ids, n, E, d, ldd, pad);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// lambda is a finite number >= 0 and, when positive, the mode one of 1..3 (NaN fails the first comparison)
static bool free_bits_ok(const ssc_free_bits* fb) {
  if (!fb || !(fb->lambda >= 0.f) || !(fb->lambda <= 3.402823466e38f)) return false;
  return fb->lambda == 0.f || (fb->mode >= 1 && fb->mode <= 3);
}
// the kernels' template argument: 0 (lambda = 0: the plain kernels, no other field of fb is read or written) or the mode
static int free_bits_form(const ssc_free_bits* fb) { return fb->lambda == 0.f ? 0 : fb->mode; }

static bool latent_fwd_ok(const ssc_latent_fwd_desc* d) {
  return d && d->B > 0 && d->Z > 0 && d->mulv && d->nslab >= 1 && d->bmu && d->blv && d->eps && d->w && d->mu && d->lv && d->z &&
         d->kld_acc;
}
static bool latent_bwd_ok(const ssc_latent_bwd_desc* d) {
  return d && d->B > 0 && d->Z > 0 && d->dz && d->eps && d->mu && d->lv && d->w && d->gk && d->dmulv;
}

template <int FB>
static void latent_fwd_form(const ssc_latent_fwd_desc& d, const ssc_free_bits& fb, hipStream_t st) {
  const int zw = (d.Z + 63) / 64;
  if (d.nslab > 16 && (zw == 1 || zw == 2 || zw == 4))
    SSC_LAUNCH(latent_fwd_wide_kernel<FB>, dim3(d.B), dim3(256), 0, st, d, fb);
  else
    SSC_LAUNCH(latent_fwd_kernel<FB>, dim3(ssc_cdiv(d.B, 4)), dim3(256), 0, st, d, fb);
}
static int latent_fwd_launch(const ssc_latent_fwd_desc& d, const ssc_free_bits& fb, int form, hipStream_t st) {
  if (form == 0) latent_fwd_form<0>(d, fb, st);
  else if (form == 1) latent_fwd_form<1>(d, fb, st);
  else if (form == 2) latent_fwd_form<2>(d, fb, st);
  else latent_fwd_form<3>(d, fb, st);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
static int latent_bwd_launch(const ssc_latent_bwd_desc& d, const ssc_free_bits& fb, int form, hipStream_t st) {
  const dim3 grid(ssc_cdiv(d.Z, 64), d.B), block(64);
  if (form == 0) SSC_LAUNCH(latent_bwd_kernel<0>, grid, block, 0, st, d, fb);
  else if (form == 1) SSC_LAUNCH(latent_bwd_kernel<1>, grid, block, 0, st, d, fb);
  else if (form == 2) SSC_LAUNCH(latent_bwd_kernel<2>, grid, block, 0, st, d, fb);
  else SSC_LAUNCH(latent_bwd_kernel<3>, grid, block, 0, st, d, fb);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_latent_fwd(const ssc_latent_fwd_desc* d, void* stream) {
  if (!latent_fwd_ok(d)) return SSC_EINVAL;
  return latent_fwd_launch(*d, ssc_free_bits{}, 0, S(stream));
}

extern "C" int ssc_latent_fwd_fb(const ssc_latent_fwd_desc* d, const ssc_free_bits* fb, void* stream) {
  if (!free_bits_ok(fb) || !latent_fwd_ok(d)) return SSC_EINVAL;
  const int form = free_bits_form(fb);
  if (form != 0 && (!fb->kld_raw || (form == 2 && !fb->gate_step) || (form == 3 && (!fb->dim_acc || fb->lddim < d->Z))))
    return SSC_EINVAL;
  return latent_fwd_launch(*d, *fb, form, S(stream));
}

extern "C" int ssc_latent_fb_finish(const float* dim_acc, int lddim, int B, int Z, float lambda, float* kdim, float* gate_dim,
                                    float* kld, void* stream) {
  if (!dim_acc || !kdim || !gate_dim || !kld || B <= 0 || Z <= 0 || lddim < Z || !(lambda >= 0.f) || !(lambda <= 3.402823466e38f))
    return SSC_EINVAL;
  SSC_LAUNCH(latent_fb_finish_kernel, dim3(1), dim3(256), 0, S(stream), dim_acc, lddim, B, Z, lambda, kdim, gate_dim, kld);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_latent_bwd(const ssc_latent_bwd_desc* d, void* stream) {
  if (!latent_bwd_ok(d)) return SSC_EINVAL;
  return latent_bwd_launch(*d, ssc_free_bits{}, 0, S(stream));
}

extern "C" int ssc_latent_bwd_fb(const ssc_latent_bwd_desc* d, const ssc_free_bits* fb, void* stream) {
  if (!free_bits_ok(fb) || !latent_bwd_ok(d)) return SSC_EINVAL;
  const int form = free_bits_form(fb);
  if ((form == 2 && !fb->gate_step) || (form == 3 && !fb->gate_dim)) return SSC_EINVAL;
  return latent_bwd_launch(*d, *fb, form, S(stream));
}

// the _pm kernel without a per-element mean or variance: the same expression, the same zeroed pad columns
extern "C" int ssc_latent_prior_sample(const float* eps, int ldeps, const float* sent, float pm_scale, float prior_var,
                                       int G, int Z, float* z, int ldz, void* stream) {
  if (!eps || !z || G <= 0 || Z <= 0) return SSC_EINVAL;
  SSC_LAUNCH(latent_prior_sample_pm_kernel, dim3(ssc_cdiv((Z + 3) & ~3, 64), G), dim3(64), 0, S(stream), eps, ldeps,
             (const float*)nullptr, 0, (const float*)nullptr, 0, sent, pm_scale, sqrtf(prior_var), G, Z, z, ldz);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_latent_prior_sample_pm(const float* eps, int ldeps, const float* pm, int ldpm, const float* pv, int ldpv,
                                          const float* sent, float pm_scale, float prior_var, int G, int Z, float* z, int ldz,
                                          void* stream) {
  if (!eps || !z || G <= 0 || Z <= 0 || ldeps < Z || (pm && ldpm < Z) || (pv && ldpv < Z) || ldz < Z) return SSC_EINVAL;
  SSC_LAUNCH(latent_prior_sample_pm_kernel, dim3(ssc_cdiv((Z + 3) & ~3, 64), G), dim3(64), 0, S(stream), eps, ldeps, pm, ldpm, pv, ldpv, sent,
             pm_scale, sqrtf(prior_var), G, Z, z, ldz);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_log_softmax(const float* logits, int ldl, int rows, int V, float* out, int ldo, void* stream) {
  if (!logits || !out || rows <= 0 || V <= 0 || ldl < V || ldo < V) return SSC_EINVAL;
  SSC_LAUNCH(log_softmax_kernel, dim3(rows), dim3(256), 0, S(stream), logits, ldl, V, out, ldo);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// scratch: COLSUM_CHUNKS*N floats when rows >= 64 (may be null for fewer rows); out2: optional second copy (N, stride 1)
extern "C" int ssc_colsum2(const float* X, int ldx, int rows, int N, const float* wrow, float* out, int out_stride,
                           float* out2, int accumulate, float* scratch, void* stream) {
  if (!X || !out || rows <= 0 || N <= 0 || ldx < N || out_stride < 1) return SSC_EINVAL;
  if (rows >= 64 && scratch) {
    SSC_LAUNCH(colsum_stage1_kernel, dim3(ssc_cdiv(N, 256), COLSUM_CHUNKS), dim3(256), 0, S(stream), X, ldx, rows, N,
                       wrow, scratch);
    SSC_CHECK_LAUNCH();
    SSC_LAUNCH(colsum_stage2_kernel, dim3(ssc_cdiv(N, 64)), dim3(256), 0, S(stream), scratch, N, out, out_stride,
                       out2, accumulate);
    SSC_CHECK_LAUNCH();
    return SSC_OK;
  }
  SSC_LAUNCH(colsum_kernel, dim3(ssc_cdiv(N, 256)), dim3(256), 0, S(stream), X, ldx, rows, N, wrow, out, out_stride,
                     out2, accumulate);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_colsum(const float* X, int ldx, int rows, int N, const float* wrow, float* out, int out_stride,
                          int accumulate, void* stream) {
  return ssc_colsum2(X, ldx, rows, N, wrow, out, out_stride, nullptr, accumulate, nullptr, stream);
}

namespace {
// |x| maxima as unsigned bit patterns (non-negative floats order like their bit patterns): one atomicMax per wave
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, size_t rows, int cols, size_t ld,
                                                     unsigned* __restrict__ out) {
  float m = 0.f;
  const size_t n = rows * (size_t)cols;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / cols;
    m = fmaxf(m, fabsf(x[r * ld + (i - r * cols)]));
  }
  m = ssc_wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}
__global__ void pow2_scale_kernel(const unsigned* __restrict__ mx, int target_log2, float* __restrict__ out, int combine) {
  const float m = __uint_as_float(*mx);
  float sc = 1.f;
  if (m > 0.f && m < INFINITY) {
    int e;
    (void)frexpf(m, &e);           // m = f 2^e, f in [0.5, 1): m <= 2^e
    sc = ldexpf(1.f, target_log2 - e);
  }
  *out = combine ? fminf(*out, sc) : sc;
}
}  // namespace

extern "C" int ssc_pow2_scale(const float* x, size_t rows, int cols, size_t ld, int target_log2, float* out, int combine,
                              float* scratch, void* stream) {
  if (!x || !out || !scratch || rows == 0 || cols <= 0 || ld < (size_t)cols) return SSC_EINVAL;
  if (hipMemsetAsync(scratch, 0, sizeof(float), S(stream)) != hipSuccess) return SSC_EHIP;
  const size_t n = rows * (size_t)cols;
  const int grid = (int)std::min<size_t>((n + 1023) / 1024, 2048);
  SSC_LAUNCH(absmax_kernel, dim3(grid < 1 ? 1 : grid), dim3(256), 0, S(stream), x, rows, cols, ld, reinterpret_cast<unsigned*>(scratch));
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(pow2_scale_kernel, dim3(1), dim3(1), 0, S(stream), reinterpret_cast<const unsigned*>(scratch), target_log2, out, combine);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_copy_strided(const float* src, size_t stride, int n, float* dst, void* stream) {
  if (!src || !dst || n <= 0) return SSC_EINVAL;
  SSC_LAUNCH(copy_strided_kernel, dim3(ssc_cdiv(n, 256)), dim3(256), 0, S(stream), src, stride, n, dst);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// rows ride on gridDim.y, which the runtime limits to 65535: more is refused here, not handed on as an invalid grid
static constexpr int kMaxGridY = 65535;
extern "C" int ssc_bias_tanh(float* x, int ldx, int rows, int N, const float* bias, void* stream) {
  if (!x || rows <= 0 || rows > kMaxGridY || N <= 0 || ldx < N) return SSC_EINVAL;
  SSC_LAUNCH(bias_tanh_kernel, dim3(ssc_cdiv(N, 256), rows), dim3(256), 0, S(stream), x, ldx, N, bias);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_tanh_bwd(float* dy, int lddy, const float* y, int ldy, int rows, int N, void* stream) {
  if (!dy || !y || rows <= 0 || rows > kMaxGridY || N <= 0 || lddy < N || ldy < N) return SSC_EINVAL;
  SSC_LAUNCH(tanh_bwd_kernel, dim3(ssc_cdiv(N, 256), rows), dim3(256), 0, S(stream), dy, lddy, y, ldy, N);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_fill(float* p, size_t n, float v, void* stream) {
  if (!p) return SSC_EINVAL;
  if (n == 0) return SSC_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  SSC_LAUNCH(fill_kernel, dim3((unsigned)blocks), dim3(256), 0, S(stream), p, n, v);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

// Non-temporal policy of the once-per-step streams, a bit mask: 2 = ssc_sgd_step and ssc_sq_norm.  (Bit 1, the weight loads of
// the minibatch gate products, measured slower and is not built: DESIGN.md 6.)  Both policies are compiled forms chosen here.
int ssc_g_stream_nt = ssc_env_int("SSC_STREAM_NT", 2);
extern "C" int ssc_sq_norm(const float* g, size_t n, float* scratch, float* out, void* stream) {
  if (!g || !scratch || !out) return SSC_EINVAL;
  const int nb = 1024;
  const auto partial = (ssc_g_stream_nt & 2) ? sq_norm_partial_kernel<true> : sq_norm_partial_kernel<false>;
  SSC_LAUNCH(partial, dim3(nb), dim3(256), 0, S(stream), g, n, scratch);
  SSC_CHECK_LAUNCH();
  SSC_LAUNCH(sq_norm_final_kernel, dim3(1), dim3(256), 0, S(stream), scratch, nb, out);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_sgd_step(float* p, const float* g, float* buf, size_t n, const float* sqnorm, float gscale,
                            float max_norm, float lr, float momentum, float weight_decay, int first, void* stream) {
  if (!p || !g || !buf || !sqnorm) return SSC_EINVAL;
  if (n == 0) return SSC_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const auto sgd = (ssc_g_stream_nt & 2) ? sgd_kernel<true> : sgd_kernel<false>;
  SSC_LAUNCH(sgd, dim3((unsigned)blocks), dim3(256), 0, S(stream), p, g, buf, n, sqnorm, gscale, max_norm,
                     lr, momentum, weight_decay, first);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_adam_step(float* p, const float* g, float* m, float* v, size_t n, const float* sqnorm, float gscale,
                             float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                             int step, void* stream) {
  if (!p || !g || !m || !v || !sqnorm || step < 1) return SSC_EINVAL;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(lr >= 0.f) || !(weight_decay >= 0.f))
    return SSC_EINVAL;
  const uintptr_t mis = (uintptr_t)p & 15u;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 3u) return SSC_EALIGN;
  if (n == 0) return SSC_OK;
  // the four slices of equally aligned buffers share one misalignment: scalar head up to the first 16-byte boundary, float4
  // bulk, scalar tail; a direct caller's differently aligned pointers take the scalar path throughout
  size_t head = n;
  if (((uintptr_t)g & 15u) == mis && ((uintptr_t)m & 15u) == mis && ((uintptr_t)v & 15u) == mis) {
    head = ((16u - mis) & 15u) >> 2;
    if (head > n) head = n;
  }
  const size_t n4 = (n - head) >> 2;
  AdamArgs a;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  a.step_size = (float)((double)lr / bc1);
  a.rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
  a.beta1 = beta1;
  a.omb1 = (float)(1.0 - (double)beta1);
  a.beta2 = beta2;
  a.omb2 = (float)(1.0 - (double)beta2);
  a.eps = eps;
  a.wd = weight_decay;
  a.decay = (float)(1.0 - (double)lr * (double)weight_decay);
  const size_t work = n4 > n - (n4 << 2) ? n4 : n - (n4 << 2);
  size_t blocks = (work + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (decoupled)
    SSC_LAUNCH(adam_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, S(stream), p, g, m, v, n, head, n4, sqnorm, gscale, max_norm, a);
  else
    SSC_LAUNCH(adam_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, S(stream), p, g, m, v, n, head, n4, sqnorm, gscale, max_norm, a);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
