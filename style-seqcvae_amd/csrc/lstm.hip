// LSTM cell kernels of the var_updown hot path (gfx950, wave64): the torch.nn.LSTMCell pointwise part fused with the split-K slab
// sums of the gate products, forward and backward, plus the forms that contract one more addend inside the kernel.  The cell is
// written ONCE, as the __device__ pieces below; every kernel is built from them, so the kernels agree bit for bit wherever they
// take the same addends.  Reference citations are on the C entry points in ssc.h.
#include <algorithm>

#include "ssc_common.h"

namespace {

inline hipStream_t S(void* s) { return (hipStream_t)s; }

// the four-step v_mfma_f32_16x16x4_f32 contraction of 16 k-values: lane (r = lane & 15, q = lane >> 4) holds 4 consecutive k at
// 16 c + 4 q of row r of either operand; MFMA i takes element i of every lane, i.e. contracts k in {16 c + 4 q + i : q = 0..3} -
// the same for both operands.  Output layout: the lane holds rows 4 q + i (i = 0..3) of column r.
__device__ __forceinline__ ssc_f32x4 mfma_f32_k16(const float4& a, const float4& b, ssc_f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// ---------------------------------------------------------------------------------------------
// the forward cell:  pre[g] = slabs, slabs2, add0, add1, b_ih, b_hh, sent * wcol [, the kernel's own addend]  (in this order)
// ---------------------------------------------------------------------------------------------
// The cell kernels move ~20 MB: they are bound by memory latency, not bandwidth.  Every operand that does not depend on the slab
// sums is requested first and all slabs (up to 16) in one batch, so about one latency is exposed in total.
struct LstmOperands { float a0[4], a1[4], bi[4], bh[4], sw[4], sv, cp; };
enum { LSTM_ROW_TERMS = 1, LSTM_UNIT_TERMS = 2 };   // a0, a1, sv, cp (per row and unit) | bi, bh, sw (per unit: the same for every row)

// CP_ROWS: the kernel honours c_prev_rows.  (b, j) are always readable: a thread without a cell passes clamped indices.
template <bool CP_ROWS, int TERMS = LSTM_ROW_TERMS | LSTM_UNIT_TERMS>
__device__ __forceinline__ void lstm_load_operands(const ssc_lstm_fwd_desc& d, int b, int j, LstmOperands& o) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int n = g * d.H + j;
    if (TERMS & LSTM_ROW_TERMS) {
      o.a0[g] = d.add0 ? d.add0[(size_t)(d.add0_rows ? d.add0_rows[b] : (int64_t)b) * d.ld_add0 + n] : 0.f;
      o.a1[g] = d.add1 ? d.add1[(size_t)(b / d.rows_per_add1) * d.ld_add1 + n] : 0.f;
    }
    if (TERMS & LSTM_UNIT_TERMS) {
      o.bi[g] = d.b_ih ? d.b_ih[n] : 0.f;
      o.bh[g] = d.b_hh ? d.b_hh[n] : 0.f;
      o.sw[g] = d.sent ? d.wcol[(size_t)n * d.ldwcol] : 0.f;
    }
  }
  if (TERMS & LSTM_ROW_TERMS) {
    o.sv = d.sent ? d.sent[b] : 0.f;
    o.cp = d.c_prev ? d.c_prev[(size_t)(CP_ROWS && d.c_prev_rows ? d.c_prev_rows[b] : b) * d.ld_cprev + j] : 0.f;
  }
}

// split-K slabs: summed in index order per gate (a `v += load` loop with a dynamic trip count would serialise one memory latency
// per slab), U loads per gate in flight: slabs s0 .. s0 + U - 1 of cell (srow, j), indices clamped to the last slab and the
// values beyond it masked when they are added.  MAY_BE_EMPTY: for a batch requested whether or not there is a slab at all.
template <int U, bool MAY_BE_EMPTY = false>
__device__ __forceinline__ void lstm_load_slabs(const ssc_lstm_fwd_desc& d, size_t srow, int j, int s0, float (&t)[4][U]) {
  const int H = d.H, H4 = 4 * d.H;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float* sp = d.slabs + (size_t)min(s0 + u, MAY_BE_EMPTY ? max(d.nslab - 1, 0) : d.nslab - 1) * d.slab_stride + srow * H4 + j;
#pragma unroll
    for (int g = 0; g < 4; ++g) t[g][u] = (!MAY_BE_EMPTY || d.nslab > 0) ? sp[g * H] : 0.f;
  }
}
template <int U>
__device__ __forceinline__ void lstm_add_slabs(const ssc_lstm_fwd_desc& d, int s0, const float (&t)[4][U], float (&pre)[4]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int g = 0; g < 4; ++g) pre[g] += (s0 + u < d.nslab) ? t[g][u] : 0.f;
}
// pre += slabs s0 .. nslab - 1, in batches of U
template <int U>
__device__ __forceinline__ void lstm_sum_slabs(const ssc_lstm_fwd_desc& d, size_t srow, int j, int s0, float (&pre)[4]) {
  for (; s0 < d.nslab; s0 += U) {
    float t[4][U];
    lstm_load_slabs<U>(d, srow, j, s0, t);
    lstm_add_slabs<U>(d, s0, t, pre);
  }
}

// the terms behind the slab sums, in their fixed order; absent terms add +0.f, which leaves every value unchanged.  LAST: the
// kernel's own addend (the z product, the image-table contraction) goes last.
template <bool LAST>
__device__ __forceinline__ void lstm_add_terms(const ssc_lstm_fwd_desc& d, const LstmOperands& o, float (&pre)[4], const float (&last)[4]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v = pre[g];
    v += o.a0[g];
    v += o.a1[g];
    v += o.bi[g];
    v += o.bh[g];
    if (d.sent) v += o.sv * o.sw[g];
    if (LAST) v += last[g];
    pre[g] = v;
  }
}
__device__ __forceinline__ void lstm_add_terms(const ssc_lstm_fwd_desc& d, const LstmOperands& o, float (&pre)[4]) {
  lstm_add_terms<false>(d, o, pre, pre);
}

// torch.nn.LSTMCell, gate order i, f, g, o
struct LstmCell { float ig, fg, gg, og, c, h; };
__device__ __forceinline__ LstmCell lstm_cell_update(const float (&pre)[4], float cp) {
  LstmCell r;
  r.ig = ssc_sigmoid(pre[0]); r.fg = ssc_sigmoid(pre[1]); r.gg = tanhf(pre[2]); r.og = ssc_sigmoid(pre[3]);
  r.c = r.fg * cp + r.ig * r.gg;
  r.h = r.og * tanhf(r.c);
  return r;
}

// the halfs of column j of row b in the fp16 planes (ssc_lstm_fwd_desc.h_planes): hi at [0], lo at [32] (per k-block of 32
// columns: 32 hi halfs, then 32 lo halfs)
__device__ __forceinline__ unsigned short* lstm_plane_halfs(const ssc_lstm_fwd_desc& d, int b, int j) {
  return reinterpret_cast<unsigned short*>(d.h_planes) + ((size_t)b * d.ld_hplanes + (j >> 5) * 32) * 2 + (j & 31);
}
// PLANES: the kernel also leaves h as the two fp16 pieces of h * scale
template <bool PLANES>
__device__ __forceinline__ void lstm_store(const ssc_lstm_fwd_desc& d, int b, int j, const LstmCell& r) {
  const int H = d.H;
  if (d.gates_out) {
    float* go = d.gates_out + (size_t)b * 4 * H + j;
    go[0] = r.ig; go[H] = r.fg; go[2 * H] = r.gg; go[3 * H] = r.og;
  }
  d.c_out[(size_t)b * d.ld_cout + j] = r.c;
  d.h_out[(size_t)b * d.ld_hout + j] = r.h;
  if (PLANES && d.h_planes) {
    unsigned short hi, lo;
    ssc_split1_f16(r.h * (d.planes_scale ? *d.planes_scale : 1.f), hi, lo);
    unsigned short* hp = lstm_plane_halfs(d, b, j);
    hp[0] = hi; hp[32] = lo;
  }
}

__global__ void lstm_fwd_kernel(const ssc_lstm_fwd_desc d) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int b = blockIdx.y;
  const bool pad = j >= d.H;   // (only with h_planes: the planes' padding columns H .. roundup(H, 32) are zeroed here)
  if (pad && (!d.h_planes || j >= (d.H + 31) / 32 * 32)) return;
  if (d.rows) {   // only the listed rows (decode: the rows that are read at all)
    if (b >= *d.row_count) return;
    b = d.rows[b];
  }
  if (pad) {
    unsigned short* hp = lstm_plane_halfs(d, b, j);
    hp[0] = 0; hp[32] = 0;
    return;
  }
  LstmOperands o;
  lstm_load_operands<true>(d, b, j, o);
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
  // the batch follows the slab count: the decode step hands ONE slab (the gate product of 5000 rows is not split) and a fixed
  // batch of 16 made it issue 64 loads per cell for the 4 it needs
  const size_t srow = d.slab_rows ? (size_t)d.slab_rows[b] : (size_t)b;   // (decode: the row of this beam's parent in a product over distinct parents)
  if (d.nslab <= 1) lstm_sum_slabs<1>(d, srow, j, 0, pre);
  else if (d.nslab <= 4) lstm_sum_slabs<4>(d, srow, j, 0, pre);
  else if (d.nslab <= 8) lstm_sum_slabs<8>(d, srow, j, 0, pre);
  else lstm_sum_slabs<16>(d, srow, j, 0, pre);
  if (d.nslab2 > 0) {
    const int H = d.H, H4 = 4 * d.H;
    const size_t r2 = d.slab2_rows ? (size_t)d.slab2_rows[b] : (size_t)b;
    for (int sl = 0; sl < d.nslab2; ++sl)
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] += d.slabs2[(size_t)sl * d.slab2_stride + r2 * H4 + g * H + j];
  }
  lstm_add_terms(d, o, pre);
  lstm_store<true>(d, b, j, lstm_cell_update(pre, o.cp));
}

// lstm_fwd_kernel plus one more addend of the gate pre-activations computed IN the kernel: pre[b,n] += z[b,:] . wz[n,:]
// (K = Z: the latent block of the decoder LSTM's input, updown_cell.py:211-229).  z only exists after the latent head of the
// same step, so as a K-segment of the gate product it would tie the whole 88 MB product to the end of the step's dependency
// chain; here the product's other segments are issued earlier (grouped with the encoder product) and the small z block costs
// no launch of its own.  One 512-thread workgroup per (32 batch rows x 16 hidden units) = one cell per thread; every load of
// the kernel (the z rows and the 64 wz rows of the tile, cell operands, slab values) is requested up front, so one memory
// latency is exposed as in lstm_fwd_kernel; wave (rt, g) then forms the 16 x 16 block of row tile rt and gate g on the
// exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) from LDS images and hands it to the cell threads through LDS.  150 workgroups at
// C2: one round of the chip (a first form with 256-thread workgroups of 16 x 16 cells needed 254 VGPRs, one workgroup per CU,
// and its 300 workgroups took two rounds: 16.8 us).
__global__ __launch_bounds__(512, 2) void lstm_fwd_z_kernel(const ssc_lstm_fwd_desc d, const float* __restrict__ z, int ldz,
                                                            const float* __restrict__ wz, int ldwz, int Z) {
  constexpr int TB = 32, TJ = 16, KT = 128, LD = KT + 4, NT = 512;   // k-tile of 128 (one pass for Z <= 128); rows padded by 4 floats
  __shared__ __attribute__((aligned(16))) float sz[TB * LD];       // z[b0 + r, k]
  __shared__ __attribute__((aligned(16))) float sw[4 * TJ * LD];   // wz[g*H + j0 + jj, k], row = g*16 + jj
  __shared__ float st[TB * 65];                                    // product tile [row b][column g*16 + jj]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = d.H;
  const int j0 = blockIdx.x * TJ, b0 = blockIdx.y * TB;
  const int bb = tid >> 4, jj = tid & 15;
  const int b = b0 + bb, j = j0 + jj;
  const bool live = b < d.B && j < H;
  const int bc = live ? b : 0, jc = live ? j : 0;   // clamped: every thread runs the same loads
  // ---- operand tiles of the product: requested first (they are needed first) ---------------------------------------------------
  float zr[TB * KT / NT], wr[4 * TJ * KT / NT];
  auto request_tiles = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < TB * KT / NT; ++u) {   // 8 floats per thread, coalesced along k
      const int idx = tid + NT * u, row = idx / KT, kk = idx % KT, k = k0 + kk, zb = b0 + row;
      zr[u] = (zb < d.B && k < Z) ? z[(size_t)zb * ldz + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4 * TJ * KT / NT; ++u) {   // 16 floats per thread
      const int idx = tid + NT * u, row = idx / KT, kk = idx % KT, k = k0 + kk, wj = j0 + (row & 15);
      wr[u] = (wj < H && k < Z) ? wz[(size_t)((row >> 4) * H + wj) * ldwz + k] : 0.f;
    }
  };
  request_tiles(0);
  // ---- this thread's cell: operands that do not depend on the product ----------------------------------------------------------
  LstmOperands o;
  lstm_load_operands<false>(d, bc, jc, o);
  float t0[4][16];   // first batch of slab values (later batches, if any, after the product)
  lstm_load_slabs<16, true>(d, (size_t)bc, jc, 0, t0);
  // ---- z . wz^T for the workgroup's 32 rows x (4 gates x 16 units) ----------------------------------------------------------
  ssc_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, q4 = lane >> 4;
  const int rt = wave >> 2, gw = wave & 3;   // 8 waves: row tile (0, 1) x gate
  for (int k0 = 0; k0 < Z; k0 += KT) {
    if (k0 > 0) {
      __syncthreads();   // the previous k-tile has been consumed
      request_tiles(k0);
    }
#pragma unroll
    for (int u = 0; u < TB * KT / NT; ++u) { const int idx = tid + NT * u; sz[(idx / KT) * LD + idx % KT] = zr[u]; }
#pragma unroll
    for (int u = 0; u < 4 * TJ * KT / NT; ++u) { const int idx = tid + NT * u; sw[(idx / KT) * LD + idx % KT] = wr[u]; }
    __syncthreads();
    const int kend = min(KT, (Z - k0 + 15) / 16 * 16);   // whole 16-wide chunks; the tail is zero-filled
    for (int c = 0; c < kend; c += 16)
      acc = mfma_f32_k16(*reinterpret_cast<const float4*>(&sz[(rt * 16 + r16) * LD + c + 4 * q4]),
                         *reinterpret_cast<const float4*>(&sw[(gw * 16 + r16) * LD + c + 4 * q4]), acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) st[(rt * 16 + 4 * q4 + i) * 65 + gw * 16 + r16] = acc[i];
  __syncthreads();
  // ---- cell update, the z term added last ------------------------------------------------------------------------------------------
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
  lstm_add_slabs<16>(d, 0, t0, pre);
  lstm_sum_slabs<16>(d, (size_t)bc, jc, 16, pre);
  const float zw[4] = {st[bb * 65 + jj], st[bb * 65 + 16 + jj], st[bb * 65 + 32 + jj], st[bb * 65 + 48 + jj]};
  lstm_add_terms<true>(d, o, pre, zw);
  if (!live) return;
  lstm_store<false>(d, b, j, lstm_cell_update(pre, o.cp));
}

// lstm_fwd_kernel for rows that share per-IMAGE operands (decode: rows_per_image beam rows per image), with one more addend of the
// gate pre-activations formed in the kernel from a per-image table:
//   pre[b, n] += sum_r alpha[b, r] * P[(img(b) R + r) 4H + n],   img(b) = b / rows_per_image
// P[img, r, :] = W_ih^dec[:, :F] v_{img,r} is the decoder-gate contribution of region r, formed ONCE per image
// (ssc_decode_prepare); since the attended feature vector is sum_r alpha_r v_r (updown_cell.py:156-158) and the gate product is
// linear in it, sum_r alpha_r P_r IS the att segment of the decoder gate product (updown_cell.py:211-229) - K = R = 36 against a
// table the image's 100 rows share, instead of K = F = 2048 against the weights in every step: the largest product of a decode
// step loses 45 % of its k-steps (same value up to fp32 reassociation; SURVEY Appendix A.5 / B: per-image terms are computed
// once per image).  One 256-thread workgroup per (image, 16 hidden units): the (R x 4 gates x 16 units) table tile goes to LDS
// once, then the image's rows are taken 16 at a time, one cell per thread, alpha rows through LDS; R <= 128.
constexpr int IMG_MAXR = 128;
// (cpw: 16-row chunks per workgroup - a whole image per workgroup at C4's 50 x 100 rows, one chunk each for a single image, so that
// the grid fills the chip either way; blockIdx.y = image * ceil(chunks / cpw) + chunk group)
// 512 threads = 16 rows x 32 hidden units: a wave reads two full 128-byte lines per row-gate access (the first form had 16 units
// per workgroup: 64-byte half lines whose other half a neighbouring workgroup fetched again later - 198 us for ~300 MB).
__global__ __launch_bounds__(512) void lstm_fwd_img_kernel(const ssc_lstm_fwd_desc d, const float* __restrict__ alpha, int ldalpha,
                                                           const float* __restrict__ P, int R, int rpi, int cpw) {
  constexpr int TJ = 32, TR = 16, PW = 4 * TJ;   // units, rows per chunk, table tile width (4 gates x TJ)
  // dynamic LDS sized by R (R = 36: 20.7 KB)
  extern __shared__ float img_lds[];
  float* sP = img_lds;                     // [R][PW]
  float* sA = img_lds + (size_t)R * PW;    // [TR][R + 1]
  const int LDA = R + 1;
  const int tid = threadIdx.x, rr = tid >> 5, jj = tid & 31;
  const int H = d.H, H4 = 4 * d.H;
  const int chunks = (rpi + TR - 1) / TR, groups = (chunks + cpw - 1) / cpw;
  const int img = blockIdx.y / groups, grp = blockIdx.y - img * groups;
  const int j0 = blockIdx.x * TJ, j = j0 + jj;
  const int jc = j < H ? j : 0;
  for (int idx = tid; idx < R * PW; idx += 512) {
    const int r = idx / PW, c = idx - r * PW, g = c / TJ, ju = j0 + (c - g * TJ);
    sP[idx] = ju < H ? P[((size_t)img * R + r) * H4 + (size_t)g * H + ju] : 0.f;
  }
  LstmOperands o;
  lstm_load_operands<true, LSTM_UNIT_TERMS>(d, 0, jc, o);
  const int row_end = min(d.B, (img + 1) * rpi);
  for (int c0 = grp * cpw * TR; c0 < min(rpi, (grp + 1) * cpw * TR); c0 += TR) {
    const int b = img * rpi + c0 + rr;
    const bool live = c0 + rr < rpi && b < row_end && j < H;
    const int bc = (c0 + rr < rpi && b < row_end) ? b : min(img * rpi, d.B - 1);
    // this thread's cell operands first (independent of the table term); the first slab of either list with them, the slabs
    // beyond it (none in a decode step) one by one
    lstm_load_operands<true, LSTM_ROW_TERMS>(d, bc, jc, o);
    const size_t r1 = d.slab_rows ? (size_t)d.slab_rows[bc] : (size_t)bc;
    const size_t r2 = d.slab2_rows ? (size_t)d.slab2_rows[bc] : (size_t)bc;
    float t0[4], t2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) t0[g] = d.nslab > 0 ? d.slabs[r1 * H4 + g * H + jc] : 0.f;
    if (d.nslab2 > 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) t2[g] = d.slabs2[r2 * H4 + g * H + jc];
    }
    __syncthreads();   // (the previous chunk's alpha rows have been consumed; first pass: sP's writers)
    for (int idx = tid; idx < TR * R; idx += 512) {
      const int row = idx / R, r = idx - row * R, ab = img * rpi + c0 + row;
      sA[row * LDA + r] = (c0 + row < rpi && ab < row_end) ? alpha[(size_t)ab * ldalpha + r] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* ar = sA + rr * LDA;
    for (int r = 0; r < R; ++r) {   // region order: fixed summation order
      const float a = ar[r];
      const float* pr = sP + r * PW + jj;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] += a * pr[g * TJ];
    }
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v = t0[g];
      for (int sl = 1; sl < d.nslab; ++sl) v += d.slabs[(size_t)sl * d.slab_stride + r1 * H4 + g * H + jc];
      v += t2[g];
      for (int sl = 1; sl < d.nslab2; ++sl) v += d.slabs2[(size_t)sl * d.slab2_stride + r2 * H4 + g * H + jc];
      pre[g] = v;
    }
    lstm_add_terms<true>(d, o, pre, acc);
    if (live) lstm_store<false>(d, b, j, lstm_cell_update(pre, o.cp));
  }
}

// The same cell with the table contraction on the fp32 matrix cores (v_mfma_f32_16x16x4_f32; fp32 products and sums, fixed order).
// One workgroup of eight waves per (16 hidden units, image[, row group]); the waves take the 16-row chunks round robin (one each at
// C4's 100 rows per image) and issue their chunk's operand loads before the tile is staged:
//   A operand = the image's table tile transposed, P[img][r][gate*H + u] for 16 units x 4 gates x R regions, staged once per
//               workgroup in LDS (row stride 80 floats: the four k-rows of a k-step fall on disjoint banks) - one ds_read per MFMA;
//               rows R and R + 1 of the tile hold b_ih + b_hh and the sentiment column, contracted with 1 and the row's sentiment;
//   B operand = alpha^T of the 16-row chunk (KS = ceil((R + 2) / 4) values per lane, read straight from global - alpha is L2-resident);
//   D[unit][row]: lane l holds units 4 * (l / 16) .. + 3 of row l % 16 for each gate -> the lane's 16 accumulators are exactly the
//               four gate pre-activations of four adjacent units of one row, so the cell update follows in registers and every
//               slab / state access is a float4 (H % 4 == 0, 16-byte aligned rows - checked by the caller).
// The VALU form above spent ~100 of its 190 us at C4 (5000 rows, R = 36) on LDS reads for the contraction (5 reads per 4 FMAs).
// (A first matrix-core form held the table tile in 36 registers per lane, one wave per image: ~200 registers, two waves per SIMD,
// 96 us; with the next chunk's operands prefetched by hand 114 us.)
// MODE 0: one slab read by row index, no second slab; MODE 1: + a second slab read through slab2_rows and the previous cell state
// through c_prev_rows (the sibling-dedup decode step); MODE 2: every option of the descriptor.  Modes 0 and 1 have NO conditional loads: hipcc turns `p ? *p : 0` into a branch
// with s_waitcnt vmcnt(0) at the join, which serialises the loads of a lane (the first forms of this kernel: 120-135 us).
// The operands are vectors of four units and the biases and the sentiment term ride in the contraction, so this kernel has its own
// operand issue and term sums; the update of each unit is lstm_cell_update.
template <int KS, int MODE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(MODE == 2 ? 2 : KS <= 10 ? 4 : KS <= 17 ? 3 : 2, 8))) void lstm_fwd_img_mfma_kernel(
    const ssc_lstm_fwd_desc d, const float* __restrict__ alpha, int ldalpha, const float* __restrict__ P, int R, int rpi, int cpw) {
  constexpr int LDP = 80, NW = 8;
  constexpr bool RARE = MODE == 2;
  extern __shared__ float img_lds[];   // [4 * KS][LDP], rows >= R + 2 zero
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int H = d.H, H4 = 4 * d.H;
  const int ub = blockIdx.x;
  const int chunks = (rpi + 15) / 16, groups = (chunks + cpw - 1) / cpw;
  const int img = blockIdx.y / groups, grp = blockIdx.y - img * groups;
  const int u = ub * 16 + 4 * lk;   // this lane's four units
  const bool uok = u < H;            // (H % 4 == 0: all four or none)
  const int uc = uok ? u : 0;
  const int row_end = min(d.B, (img + 1) * rpi);
  const int c_end = min(rpi, (grp + 1) * cpw * 16);
  const float* sentp = d.sent ? d.sent : alpha;   // (always a readable address: the value is dropped when there is no sentiment)
  const float sflag = d.sent ? 1.f : 0.f;
  struct Ops { ssc_f32x4 pre[4], t2[4], cp; float al[KS], sv; int b, bc; bool rok; size_t r1, r2; };
  // a chunk's operands: issued before anything that waits (the tile staging and its barrier for a wave's first chunk)
  auto issue = [&](int c0, Ops& o) {
    o.b = img * rpi + c0 + li;
    o.rok = c0 + li < rpi && o.b < row_end;
    o.bc = o.rok ? o.b : img * rpi;
    if (MODE == 2) {
      o.r1 = d.slab_rows ? (size_t)d.slab_rows[o.bc] : (size_t)o.bc;
      o.r2 = d.slab2_rows ? (size_t)d.slab2_rows[o.bc] : (size_t)o.bc;
    } else {
      o.r1 = (size_t)o.bc;
      o.r2 = MODE == 1 ? (size_t)d.slab2_rows[o.bc] : 0;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = g * H + uc;
      if (MODE == 2) o.pre[g] = d.nslab > 0 ? *reinterpret_cast<const ssc_f32x4*>(d.slabs + o.r1 * H4 + n) : ssc_f32x4{0.f, 0.f, 0.f, 0.f};
      else o.pre[g] = *reinterpret_cast<const ssc_f32x4*>(d.slabs + o.r1 * H4 + n);
    }
    if (MODE == 2)
      o.cp = d.c_prev ? *reinterpret_cast<const ssc_f32x4*>(d.c_prev + (size_t)(d.c_prev_rows ? d.c_prev_rows[o.bc] : o.bc) * d.ld_cprev + uc)
                      : ssc_f32x4{0.f, 0.f, 0.f, 0.f};
    else if (MODE == 1) o.cp = *reinterpret_cast<const ssc_f32x4*>(d.c_prev + (size_t)d.c_prev_rows[o.bc] * d.ld_cprev + uc);
    else o.cp = *reinterpret_cast<const ssc_f32x4*>(d.c_prev + (size_t)o.bc * d.ld_cprev + uc);
    const float* ap = alpha + (size_t)o.bc * ldalpha;
    o.sv = sentp[o.bc];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int r = ks * 4 + lk;
      o.al[ks] = ap[min(r, R - 1)];   // (raw: masked in `finish`, after the waits of the tile staging)
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = g * H + uc;
      if (MODE == 2) o.t2[g] = d.nslab2 > 0 ? *reinterpret_cast<const ssc_f32x4*>(d.slabs2 + o.r2 * H4 + n) : ssc_f32x4{0.f, 0.f, 0.f, 0.f};
      else if (MODE == 1) o.t2[g] = *reinterpret_cast<const ssc_f32x4*>(d.slabs2 + o.r2 * H4 + n);
    }
  };
  Ops o;
  int c0 = (grp * cpw + wave) * 16;
  if (c0 < c_end) issue(c0, o);
  // the tile: rows < R from the table, row R the bias sum, row R + 1 the sentiment column, the rest zero
  {
    const int c = lane, g = c >> 4, ua = ub * 16 + (c & 15);
    const bool cok = ua < H;
    const size_t n = (size_t)g * H + (cok ? ua : 0);
    const float* pi = P + (size_t)img * R * H4 + n;
    constexpr int NIT = (4 * KS + NW - 1) / NW;
    float v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) v[it] = pi[(size_t)min(wave + it * NW, R - 1) * H4];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int r = wave + it * NW;
      if (r < 4 * KS && r != R && r != R + 1) img_lds[r * LDP + c] = (r < R && cok) ? v[it] : 0.f;
    }
    if (wave == 0) {
      const float bs = (d.b_ih ? d.b_ih[n] : 0.f) + (d.b_hh ? d.b_hh[n] : 0.f);
      img_lds[R * LDP + c] = cok ? bs : 0.f;
    } else if (wave == 1) {
      img_lds[(R + 1) * LDP + c] = (d.sent && cok) ? d.wcol[n * d.ldwcol] : 0.f;
    }
  }
  __syncthreads();
  const float* sp = img_lds + lk * LDP + li;
  while (c0 < c_end) {
    // alpha^T with the rows beyond R: 1 for the bias row, the sentiment for its column, 0 elsewhere (arithmetic, not a select
    // around the load: the compiler sinks a load whose value is used on one side only into a branch)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int r = ks * 4 + lk;
      const float m = (r < R && o.rok) ? 1.f : 0.f;
      o.al[ks] = o.al[ks] * m + (r == R ? 1.f : r == R + 1 ? o.sv * sflag : 0.f);
    }
    ssc_f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = ssc_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[ks * 4 * LDP + g * 16], o.al[ks], acc[g], 0, 0, 0);
      if ((ks & 1) == 1) __builtin_amdgcn_sched_barrier(0);   // (keeps the tile reads two k-steps ahead at most: registers)
    }
    const int b = o.b, bc = o.bc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = g * H + uc;
      if (MODE >= 1) o.pre[g] += o.t2[g];
      if (RARE) {   // split-K slabs beyond the first, the per-token and per-image rows
        for (int sl = 1; sl < d.nslab; ++sl) o.pre[g] += *reinterpret_cast<const ssc_f32x4*>(d.slabs + (size_t)sl * d.slab_stride + o.r1 * H4 + n);
        for (int sl = 1; sl < d.nslab2; ++sl) o.pre[g] += *reinterpret_cast<const ssc_f32x4*>(d.slabs2 + (size_t)sl * d.slab2_stride + o.r2 * H4 + n);
        if (d.add0) o.pre[g] += *reinterpret_cast<const ssc_f32x4*>(d.add0 + (size_t)(d.add0_rows ? d.add0_rows[bc] : (int64_t)bc) * d.ld_add0 + n);
        if (d.add1) o.pre[g] += *reinterpret_cast<const ssc_f32x4*>(d.add1 + (size_t)(bc / d.rows_per_add1) * d.ld_add1 + n);
      }
      o.pre[g] += acc[g];
    }
    if (o.rok && uok) {
      ssc_f32x4 ig, fg, gg, og, c, h;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float pre[4] = {o.pre[0][v], o.pre[1][v], o.pre[2][v], o.pre[3][v]};
        const LstmCell r = lstm_cell_update(pre, o.cp[v]);
        ig[v] = r.ig; fg[v] = r.fg; gg[v] = r.gg; og[v] = r.og; c[v] = r.c; h[v] = r.h;
      }
      if (RARE && d.gates_out) {
        float* go = d.gates_out + (size_t)b * H4 + u;
        *reinterpret_cast<ssc_f32x4*>(go) = ig;
        *reinterpret_cast<ssc_f32x4*>(go + H) = fg;
        *reinterpret_cast<ssc_f32x4*>(go + 2 * H) = gg;
        *reinterpret_cast<ssc_f32x4*>(go + 3 * H) = og;
      }
      *reinterpret_cast<ssc_f32x4*>(d.c_out + (size_t)b * d.ld_cout + u) = c;
      *reinterpret_cast<ssc_f32x4*>(d.h_out + (size_t)b * d.ld_hout + u) = h;
      if (d.h_planes) {   // (uniform) h also as its two fp16 pieces (ssc_lstm_fwd_desc.h_planes)
        ssc_u32x2 hi, lo;
        ssc_split4_f16(h * (d.planes_scale ? *d.planes_scale : 1.f), hi, lo);
        unsigned* hp = reinterpret_cast<unsigned*>(d.h_planes) + (size_t)b * d.ld_hplanes + ssc_plane_word(u);
        *reinterpret_cast<ssc_u32x2*>(hp) = hi;
        *reinterpret_cast<ssc_u32x2*>(hp + 16) = lo;
      }
    } else if (o.rok && d.h_planes && u < (H + 31) / 32 * 32) {   // the planes' padding columns (the grid then covers roundup(H, 32) units)
      unsigned* hp = reinterpret_cast<unsigned*>(d.h_planes) + (size_t)b * d.ld_hplanes + ssc_plane_word(u);
      *reinterpret_cast<ssc_u32x2*>(hp) = ssc_u32x2{0u, 0u};
      *reinterpret_cast<ssc_u32x2*>(hp + 16) = ssc_u32x2{0u, 0u};
    }
    c0 += NW * 16;
    if (c0 < c_end) issue(c0, o);
  }
}

// lstm_fwd_kernel that also leaves partial products of its OUTPUT: pout[blockIdx.x][b, n] = sum_{j in the workgroup's 16 units}
// h[b,j] wp[n,j]  (wp (NP,H) ld ldwp: an nn.Linear weight; NP <= 256).  The encoder LSTM's h feeds fc_mean | fc_log_var
// (updown_cell.py:196-197) in the same step: as a product of its own that was a 10 us launch on the dependency chain for 1.2 MB
// of weights; here every (32 rows x 16 units) workgroup multiplies the h tile it has just computed with its 16 weight columns
// (exact-fp32 16x16x4 MFMA, K = 16) and the consumer (latent head) sums the cdiv(H,16) partial slabs in index order.
__global__ __launch_bounds__(512, 2) void lstm_fwd_p_kernel(const ssc_lstm_fwd_desc d, const float* __restrict__ wp, int ldwp,
                                                            int NP, float* __restrict__ pout) {
  constexpr int TB = 32, TJ = 16, LD = TJ + 4, NT = 512, NPMAX = 256;
  __shared__ __attribute__((aligned(16))) float sh[TB * LD];      // h[b0 + r, j0 + k]
  __shared__ __attribute__((aligned(16))) float sw[NPMAX * LD];   // wp[n, j0 + k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = d.H;
  const int j0 = blockIdx.x * TJ, b0 = blockIdx.y * TB;
  const int bb = tid >> 4, jj = tid & 15;
  const int b = b0 + bb, j = j0 + jj;
  const bool live = b < d.B && j < H;
  const int bc = live ? b : 0, jc = live ? j : 0;   // clamped: every thread runs the same loads
  // the weight slice is requested first (independent of the cell)
  float wr[NPMAX * TJ / NT];
#pragma unroll
  for (int u = 0; u < NPMAX * TJ / NT; ++u) {   // 8 floats per thread: 16 consecutive threads read 64 contiguous bytes of a row
    const int idx = tid + NT * u, n = idx / TJ, wj = j0 + idx % TJ;
    wr[u] = (n < NP && wj < H) ? wp[(size_t)n * ldwp + wj] : 0.f;
  }
  LstmOperands o;
  lstm_load_operands<false>(d, bc, jc, o);
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
  lstm_sum_slabs<16>(d, (size_t)bc, jc, 0, pre);
  lstm_add_terms(d, o, pre);
  const LstmCell r = lstm_cell_update(pre, o.cp);
  if (live) lstm_store<false>(d, b, j, r);
  // ---- partial product of the h tile with the workgroup's 16 weight columns ------------------------------------------------------
  sh[bb * LD + jj] = live ? r.h : 0.f;
#pragma unroll
  for (int u = 0; u < NPMAX * TJ / NT; ++u) { const int idx = tid + NT * u; sw[(idx / TJ) * LD + idx % TJ] = wr[u]; }
  __syncthreads();
  const int r16 = lane & 15, q4 = lane >> 4;
  float* po = pout + (size_t)blockIdx.x * d.B * NP;
  // 2 row tiles x NP/16 column tiles; wave w takes column tiles 2w, 2w+1 (K = 16: one chunk, 4 MFMAs per tile)
#pragma unroll
  for (int ci = 0; ci < 2; ++ci) {
    const int ct = 2 * wave + ci;
    if (ct * 16 >= NP) break;
    const float4 bv = *reinterpret_cast<const float4*>(&sw[(ct * 16 + r16) * LD + 4 * q4]);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const float4 av = *reinterpret_cast<const float4*>(&sh[(rt * 16 + r16) * LD + 4 * q4]);
      const ssc_f32x4 acc = mfma_f32_k16(av, bv, ssc_f32x4{0.f, 0.f, 0.f, 0.f});
      const int n = ct * 16 + r16;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ob = b0 + rt * 16 + 4 * q4 + i;
        if (ob < d.B && n < NP) po[(size_t)ob * NP + n] = acc[i];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the backward cell
// ---------------------------------------------------------------------------------------------
// latency-bound like the forward cell: the saved activations are requested before the slab sums are consumed
struct LstmSaved { float dcin, ig, fg, gg, og, cp, cn, dh; };
__device__ __forceinline__ LstmSaved lstm_bwd_load(const ssc_lstm_bwd_desc& d, int b, int j) {
  const int H = d.H;
  LstmSaved s;
  s.dcin = d.dc_in ? d.dc_in[(size_t)b * d.ld_dcin + j] : 0.f;
  const float* g = d.gates + (size_t)b * 4 * H + j;
  s.ig = g[0]; s.fg = g[H]; s.gg = g[2 * H]; s.og = g[3 * H];
  s.cp = d.c_prev[(size_t)b * d.ld_cprev + j];
  s.cn = d.c_new[(size_t)b * d.ld_cnew + j];
  s.dh = d.dh ? d.dh[(size_t)b * d.ld_dh + j] : 0.f;
  if (d.dh2) s.dh += d.dh2[(size_t)b * d.ld_dh2 + j];
  return s;
}
// dh += the split-K slabs of the producing GEMMs (lists A, then B), fixed order, up to 16 loads in flight (the batch follows the
// slab count)
template <int U>
__device__ __forceinline__ void lstm_bwd_sum_slabs(const float* slabs, int n, size_t stride, size_t cell, float& dh) {
  for (int s0 = 0; s0 < n; s0 += U) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = slabs[(size_t)min(s0 + u, n - 1) * stride + cell];
#pragma unroll
    for (int u = 0; u < U; ++u) dh += (s0 + u < n) ? t[u] : 0.f;
  }
}
__device__ __forceinline__ void lstm_bwd_add_slabs(const ssc_lstm_bwd_desc& d, int b, int j, float& dh) {
  const size_t cell = (size_t)b * d.H + j;
  if (d.nA > 8) lstm_bwd_sum_slabs<16>(d.slabsA, d.nA, d.strideA, cell, dh);
  else if (d.nA > 0) lstm_bwd_sum_slabs<8>(d.slabsA, d.nA, d.strideA, cell, dh);
  if (d.nB > 8) lstm_bwd_sum_slabs<16>(d.slabsB, d.nB, d.strideB, cell, dh);
  else if (d.nB > 0) lstm_bwd_sum_slabs<8>(d.slabsB, d.nB, d.strideB, cell, dh);
}
// the gradient of cell (b, j) for the summed s.dh, and its stores
__device__ __forceinline__ void lstm_cell_grad(const ssc_lstm_bwd_desc& d, int b, int j, const LstmSaved& s) {
  const int H = d.H, H4 = 4 * d.H;
  float tc = tanhf(s.cn);
  float d_o = s.dh * tc;
  float dc = s.dcin + s.dh * s.og * (1.f - tc * tc);
  float dgi = dc * s.gg * s.ig * (1.f - s.ig);
  float dgf = dc * s.cp * s.fg * (1.f - s.fg);
  float dgg = dc * s.ig * (1.f - s.gg * s.gg);
  float dgo = d_o * s.og * (1.f - s.og);
  float* o = d.dG + (size_t)b * H4 + j;
  o[0] = dgi; o[H] = dgf; o[2 * H] = dgg; o[3 * H] = dgo;
  d.dc_prev[(size_t)b * d.ld_dcprev + j] = dc * s.fg;
  if (d.dgsum) {
    float* sp = d.dgsum + (size_t)b * H4 + j;
    sp[0] += dgi; sp[H] += dgf; sp[2 * H] += dgg; sp[3 * H] += dgo;
  }
}

__global__ void lstm_bwd_kernel(const ssc_lstm_bwd_desc d) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int b = blockIdx.y;
  if (j >= d.H) return;
  LstmSaved s = lstm_bwd_load(d, b, j);
  lstm_bwd_add_slabs(d, b, j, s.dh);
  lstm_cell_grad(d, b, j, s);
}

// lstm_bwd_kernel plus one more addend of dh formed IN the kernel: dh[b,j] += sum_k x[b,k] w[k,j]  (x (B,K) ld ldx; w (K,H) ld ldw,
// j-contiguous; K <= 1024).  Used in BPTT for the encoder LSTM - dh = carried g_he' + (dmu | dlv) . [W_mu ; W_lv], K = 2Z = 256
// (updown_cell.py:196-197 backward) - and for the attention LSTM - dh += dq . Wq, K = A = 768 (attention.py:69 backward): as
// split-K products of their own these were 10-18 us launches on the step's dependency chain for 1-4 MB of weights.  Same shape
// as lstm_fwd_z_kernel: one 512-thread workgroup per (32 batch rows x 16 hidden units), one cell per thread; the x rows and the
// (K x 16) weight slice go through LDS images to the exact-fp32 16x16x4 MFMA: wave w takes row tile w & 1 and the quarter
// w >> 1 of the K range, the four partial tiles are added in quarter order.
template <int KMAX>   // 256 | 768: bounds the staged registers (KMAX / 16 + KMAX / 32 floats per thread)
__global__ __launch_bounds__(512, 2) void lstm_bwd_x_kernel(const ssc_lstm_bwd_desc d, const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ w, int ldw, int K) {
  constexpr int TB = 32, TJ = 16;
  extern __shared__ __attribute__((aligned(16))) float bwdx_lds[];
  const int KP = (K + 63) & ~63;       // four quarters of whole 16-wide chunks
  const int LD = KP + 4;
  float* sx = bwdx_lds;                // x[b0 + r, k]: TB * LD
  float* sw = sx + TB * LD;            // w[k, j0 + jj] stored [jj][k]: TJ * LD
  float* st = sw + TJ * LD;            // partial product tiles [quarter][row b][jj]: 4 * TB * 17
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = d.H;
  const int j0 = blockIdx.x * TJ, b0 = blockIdx.y * TB;
  const int bb = tid >> 4, jj = tid & 15;
  const int b = b0 + bb, j = j0 + jj;
  const bool live = b < d.B && j < H;
  const int bc = live ? b : 0, jc = live ? j : 0;   // clamped: every thread runs the same loads
  // staging without integer division by the run-time K (it cost ~35 instructions per element: 24 us per launch at K = 768):
  // x: thread (row = tid >> 4, t = tid & 15) takes k = t + 16 u of its row; w: thread (k = (tid >> 4) + 32 u, unit tid & 15).
  // Either way 16 consecutive threads read 64 contiguous bytes.
  float xr[KMAX / 16], wr[KMAX / 32];
  {
    const int xb = b0 + (tid >> 4);
    const float* xp = x + (size_t)min(xb, d.B - 1) * ldx;
#pragma unroll
    for (int u = 0; u < KMAX / 16; ++u) {
      const int k = (tid & 15) + 16 * u;
      xr[u] = (k < K && xb < d.B) ? xp[k] : 0.f;
    }
    const int wj = j0 + (tid & 15);
#pragma unroll
    for (int u = 0; u < KMAX / 32; ++u) {
      const int k = (tid >> 4) + 32 * u;
      wr[u] = (k < K && wj < H) ? w[(size_t)k * ldw + wj] : 0.f;
    }
  }
  // ---- the cell's own operands ----------------------------------------------------------------------------------------------------
  LstmSaved s = lstm_bwd_load(d, bc, jc);
  lstm_bwd_add_slabs(d, bc, jc, s.dh);
  // ---- x . w for the workgroup's 32 rows x 16 units ----------------------------------------------------------------------------
#pragma unroll
  for (int u = 0; u < KMAX / 16; ++u) {
    const int k = (tid & 15) + 16 * u;
    if (k < KP) sx[(tid >> 4) * LD + k] = xr[u];
  }
#pragma unroll
  for (int u = 0; u < KMAX / 32; ++u) {
    const int k = (tid >> 4) + 32 * u;
    if (k < KP) sw[(tid & 15) * LD + k] = wr[u];
  }
  __syncthreads();
  {
    ssc_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, q4 = lane >> 4;
    const int rt = wave & 1, kq = wave >> 1;
    const int kspan = KP >> 2;   // a multiple of 16
    for (int c = kq * kspan; c < (kq + 1) * kspan; c += 16)
      acc = mfma_f32_k16(*reinterpret_cast<const float4*>(&sx[(rt * 16 + r16) * LD + c + 4 * q4]),
                         *reinterpret_cast<const float4*>(&sw[r16 * LD + c + 4 * q4]), acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) st[(kq * TB + rt * 16 + 4 * q4 + i) * 17 + r16] = acc[i];
  }
  __syncthreads();
  s.dh += ((st[bb * 17 + jj] + st[(TB + bb) * 17 + jj]) + st[(2 * TB + bb) * 17 + jj]) + st[(3 * TB + bb) * 17 + jj];
  if (!live) return;
  lstm_cell_grad(d, b, j, s);
}

// What a forward entry point's kernel reads of the optional descriptor fields (ssc.h: ssc_lstm_fwd_desc).  A field that is set but
// not read is an error, not silently ignored.
enum : unsigned { LSTM_READS_ROWS = 1u, LSTM_READS_SLAB_ROWS = 2u, LSTM_READS_CPREV_ROWS = 4u, LSTM_READS_SLABS2 = 8u, LSTM_READS_PLANES = 16u };
int lstm_fwd_check(const ssc_lstm_fwd_desc* d, unsigned reads) {
  if (!d || d->B <= 0 || d->H <= 0 || !d->c_out || !d->h_out) return SSC_EINVAL;
  if (d->nslab < 0 || (d->nslab > 0 && !d->slabs)) return SSC_EINVAL;
  if (d->sent && !d->wcol) return SSC_EINVAL;
  if (d->add1 && d->rows_per_add1 <= 0) return SSC_EINVAL;
  if ((d->rows != nullptr) != (d->row_count != nullptr)) return SSC_EINVAL;
  if (d->rows && !(reads & LSTM_READS_ROWS)) return SSC_EINVAL;
  if (d->slab_rows && !(reads & LSTM_READS_SLAB_ROWS)) return SSC_EINVAL;
  if (d->c_prev_rows && !(reads & LSTM_READS_CPREV_ROWS)) return SSC_EINVAL;
  if (d->nslab2 > 0 && (!d->slabs2 || !(reads & LSTM_READS_SLABS2))) return SSC_EINVAL;
  if (d->h_planes && (!(reads & LSTM_READS_PLANES) || d->ld_hplanes < (d->H + 31) / 32 * 32 || (d->ld_hplanes & 3) || !ssc_aligned16(d->h_planes)))
    return SSC_EINVAL;
  return SSC_OK;
}

int lstm_bwd_check(const ssc_lstm_bwd_desc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || !d->gates || !d->c_prev || !d->c_new || !d->dG || !d->dc_prev) return SSC_EINVAL;
  if ((d->nA > 0 && !d->slabsA) || (d->nB > 0 && !d->slabsB) || d->nA < 0 || d->nB < 0) return SSC_EINVAL;
  return SSC_OK;
}

}  // namespace

// =============================================================================================
extern "C" int ssc_lstm_fwd(const ssc_lstm_fwd_desc* d, void* stream) {
  SSC_TRY(lstm_fwd_check(d, LSTM_READS_ROWS | LSTM_READS_SLAB_ROWS | LSTM_READS_CPREV_ROWS | LSTM_READS_SLABS2 | LSTM_READS_PLANES));
  SSC_LAUNCH(lstm_fwd_kernel, dim3(ssc_cdiv(d->H, 128), d->B), dim3(128), 0, S(stream), *d);   // (128 threads per block: the grid covers roundup(H, 32))
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_lstm_fwd_z(const ssc_lstm_fwd_desc* d, const float* z, int ldz, const float* wz, int ldwz, int Z, void* stream) {
  SSC_TRY(lstm_fwd_check(d, 0));
  if (!z || !wz || Z <= 0 || ldz < Z || ldwz < Z) return SSC_EINVAL;
  SSC_LAUNCH(lstm_fwd_z_kernel, dim3(ssc_cdiv(d->H, 16), ssc_cdiv(d->B, 32)), dim3(512), 0, S(stream), *d, z, ldz, wz, ldwz, Z);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_lstm_fwd_p(const ssc_lstm_fwd_desc* d, const float* wp, int ldwp, int NP, float* pout, void* stream) {
  SSC_TRY(lstm_fwd_check(d, 0));
  if (!wp || !pout || NP <= 0 || NP > 256 || ldwp < d->H) return SSC_EINVAL;
  SSC_LAUNCH(lstm_fwd_p_kernel, dim3(ssc_cdiv(d->H, 16), ssc_cdiv(d->B, 32)), dim3(512), 0, S(stream), *d, wp, ldwp, NP, pout);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

int ssc_g_img_mfma = ssc_env_int("SSC_IMG_MFMA", 1);   // 0: the VALU form of lstm_fwd_img_kernel (the fallback for H % 4 != 0)
int ssc_g_img_cpw = ssc_env_int("SSC_IMG_CPW", 0);   // tuning: 16-row chunks per workgroup of lstm_fwd_img_kernel (0 = by grid size)
extern "C" int ssc_lstm_fwd_img(const ssc_lstm_fwd_desc* d, const float* alpha, int ldalpha, const float* P, int R,
                                int rows_per_image, void* stream) {
  SSC_TRY(lstm_fwd_check(d, LSTM_READS_SLAB_ROWS | LSTM_READS_CPREV_ROWS | LSTM_READS_SLABS2 | LSTM_READS_PLANES));
  if (!alpha || !P || R <= 0 || R > IMG_MAXR || ldalpha < R || rows_per_image <= 0 || d->B % rows_per_image != 0) return SSC_EINVAL;
  const int nimg = d->B / rows_per_image, chunks = ssc_cdiv(rows_per_image, 16);
  // matrix-core form: every row access is a float4
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = d->H % 4 == 0 && al16(d->slabs) && al16(d->slabs2) && al16(d->c_prev) && al16(d->c_out) && al16(d->h_out) &&
                   al16(d->gates_out) && al16(d->add0) && al16(d->add1) && al16(d->b_ih) && al16(d->b_hh) && d->ld_cprev % 4 == 0 &&
                   d->ld_cout % 4 == 0 && d->ld_hout % 4 == 0 && d->ld_add0 % 4 == 0 && d->ld_add1 % 4 == 0 &&
                   d->slab_stride % 4 == 0 && d->slab2_stride % 4 == 0;
  if (d->h_planes && !(vec && ssc_g_img_mfma)) return SSC_EINVAL;   // (the pieces are written by the matrix-core form only)
  if (vec && ssc_g_img_mfma) {
    const int gx = ssc_cdiv(d->h_planes ? (d->H + 31) / 32 * 32 : d->H, 16);   // (+ the planes' padding columns)
    int cpw = (int)(((long)gx * nimg * chunks) / 4096);   // >= ~4096 workgroups when the rows allow it (the table tile is staged per row group)
    if (ssc_g_img_cpw > 0) cpw = ssc_g_img_cpw;
    cpw = std::min(std::max(cpw, 8), std::max(chunks, 8));   // (eight waves, a chunk each)
    const dim3 grid(gx, nimg * ssc_cdiv(chunks, cpw));
    // (mode 2: split-K slabs beyond the first, per-token / per-image rows, saved gates, a missing state or slab - the decode step
    // uses none of them)
    const bool rare = d->nslab != 1 || d->nslab2 > 1 || d->add0 || d->add1 || d->gates_out || d->slab_rows || !d->c_prev ||
                      (d->nslab2 == 1 && !(d->slab2_rows && d->c_prev_rows)) || (d->nslab2 == 0 && d->c_prev_rows);
    const int mode = rare ? 2 : d->nslab2 == 1 ? 1 : 0;
#define SSC_IMG_LAUNCH(KS)                                                                                                           \
  do {                                                                                                                             \
    const size_t lds = (size_t)4 * KS * 80 * sizeof(float);                                                                        \
    const void* fn = mode == 2 ? (const void*)lstm_fwd_img_mfma_kernel<KS, 2>                                                      \
                               : mode == 1 ? (const void*)lstm_fwd_img_mfma_kernel<KS, 1> : (const void*)lstm_fwd_img_mfma_kernel<KS, 0>; \
    if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return SSC_EHIP; \
    if (mode == 2) SSC_LAUNCH((lstm_fwd_img_mfma_kernel<KS, 2>), grid, dim3(512), lds, S(stream), *d, alpha, ldalpha, P, R, rows_per_image, cpw); \
    else if (mode == 1) SSC_LAUNCH((lstm_fwd_img_mfma_kernel<KS, 1>), grid, dim3(512), lds, S(stream), *d, alpha, ldalpha, P, R, rows_per_image, cpw); \
    else SSC_LAUNCH((lstm_fwd_img_mfma_kernel<KS, 0>), grid, dim3(512), lds, S(stream), *d, alpha, ldalpha, P, R, rows_per_image, cpw); \
  } while (0)
    if (R <= 38) SSC_IMG_LAUNCH(10);   // (KS k-steps of 4 cover the R regions + the bias and sentiment rows)
    else if (R <= 66) SSC_IMG_LAUNCH(17);
    else SSC_IMG_LAUNCH(33);
#undef SSC_IMG_LAUNCH
    SSC_CHECK_LAUNCH();
    return SSC_OK;
  }
  const int gx = ssc_cdiv(d->H, 32);
  int cpw = (int)(((long)gx * nimg * chunks) / 2048);   // ~2048 workgroups when the rows allow it
  if (ssc_g_img_cpw > 0) cpw = ssc_g_img_cpw;
  if (cpw < 1) cpw = 1;
  if (cpw > chunks) cpw = chunks;
  const size_t lds = ((size_t)R * 128 + 16 * (size_t)(R + 1)) * sizeof(float);   // <= 64 KB + 8 KB at R = 128
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute((const void*)lstm_fwd_img_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) != hipSuccess) return SSC_EHIP;
  }
  SSC_LAUNCH(lstm_fwd_img_kernel, dim3(gx, nimg * ssc_cdiv(chunks, cpw)), dim3(512), lds, S(stream), *d, alpha, ldalpha, P, R,
             rows_per_image, cpw);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_lstm_bwd(const ssc_lstm_bwd_desc* d, void* stream) {
  SSC_TRY(lstm_bwd_check(d));
  SSC_LAUNCH(lstm_bwd_kernel, dim3(ssc_cdiv(d->H, 128), d->B), dim3(128), 0, S(stream), *d);
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}

extern "C" int ssc_lstm_bwd_x(const ssc_lstm_bwd_desc* d, const float* x, int ldx, const float* w, int ldw, int K, void* stream) {
  SSC_TRY(lstm_bwd_check(d));
  if (!x || !w || K <= 0 || K > 768 || ldx < K || ldw < d->H) return SSC_EINVAL;
  const int KP = (K + 63) & ~63;
  const size_t lds = ((size_t)(32 + 16) * (KP + 4) + 4 * 32 * 17) * sizeof(float);
  const dim3 grid(ssc_cdiv(d->H, 16), ssc_cdiv(d->B, 32));
  if (K <= 256) {
    SSC_LAUNCH(lstm_bwd_x_kernel<256>, grid, dim3(512), lds, S(stream), *d, x, ldx, w, ldw, K);
  } else {
    // up to 157 KB of dynamic LDS at K = 768 (one workgroup per CU).  The attribute is per device: set on every call (cheap)
    if (hipFuncSetAttribute((const void*)lstm_bwd_x_kernel<768>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return SSC_EHIP;
    if (lds > 160 * 1024) return SSC_EINVAL;
    SSC_LAUNCH(lstm_bwd_x_kernel<768>, grid, dim3(512), lds, S(stream), *d, x, ldx, w, ldw, K);
  }
  SSC_CHECK_LAUNCH();
  return SSC_OK;
}
