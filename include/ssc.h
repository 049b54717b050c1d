/*
 * ssc.h - C ABI of libssc_hip.so: the MI355X (gfx950) Style-SeqCVAE hot path.
 *
 * The reference (visinf/style-seqcvae) has NO native boundary on this path: its hot path is stock
 * PyTorch ops behind the Python module API var_updown.models.UpDownCaptioner /
 * var_updown.modules.UpDownCell.  This header is the boundary the build creates
 * underneath that API; each entry point cites the reference code it replaces (paths relative to
 * /root/reference).
 *
 * Conventions
 *  - plain C: raw device pointers, ints, floats; no torch / C++ types.
 *  - all tensors fp32 row-major unless noted; token ids int64; `ld*` = leading dimension in floats.
 *  - every buffer is caller-allocated device memory (e.g. torch tensor .data_ptr()), kept alive by
 *    the caller until `stream` is synchronised.  The library allocates nothing and is re-entrant per
 *    stream and safe under hipGraph capture.  Process-wide state: the numerics mode of NT products
 *    (ssc_set_gemm_mode, below) and the opt-in diagnostics / tuning switches of ssc_debug.h, which are
 *    not part of this ABI.
 *  - `stream` is a hipStream_t passed as void* (0 = default stream).
 *  - return value: 0 on success, negative SSC_E* otherwise; never throws.
 */
#ifndef SSC_H
#define SSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSC_OK 0
#define SSC_EINVAL (-1)   /* bad shape / argument */
#define SSC_EALIGN (-2)   /* pointer or leading dimension violates an alignment requirement */
#define SSC_EHIP (-3)     /* a HIP runtime call failed (see ssc_last_hip_error) */
#define SSC_EWORKSPACE (-4) /* workspace too small */

#define SSC_MAX_SEG 6

int ssc_version(void);              /* ABI version (this header: 4) */
int ssc_last_hip_error(void);       /* last hipError_t observed by this thread */
const char* ssc_arch(void);         /* "gfx950" */

/* ------------------------------------------------------------------------------------------------
 * GEMM: C[M,N] (+)= sum_s op(A_s)[M,K_s] * op(B_s)[K_s,N] (+ bias[N])     exact-fp32 MFMA
 * (v_mfma_f32_32x32x2_f32).  Replaces aten::mm / aten::addmm under nn.LSTMCell, nn.Linear
 * (var_updown/var_updown/modules/updown_cell.py:146,192,196-197,227;
 *  updown-baseline/updown/modules/attention.py:69,125; var_updown/.../updown_captioner.py:444-445)
 * and their autograd backward.  K is segmented so that torch.cat inputs (updown_cell.py:143,178,211)
 * are never materialised: segment s multiplies a column block of the weight with its own source.
 *   a_kc=1: A_s is (M,K_s) row-major (lda>=K_s)   a_kc=0: A_s is (K_s,M) row-major (A given transposed)
 *   b_kc=1: B_s is (N,K_s) row-major (weights as stored, out x in)   b_kc=0: B_s is (K_s,N) row-major
 * splits>1 splits the K loop over `splits` workgroups per tile; partial slabs go to `workspace`
 * (>= splits*M*N floats) and are reduced (deterministically) by a second kernel.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* A; const float* B;
  int lda, ldb, K;
  /* Optional, read by the 2xFP16 form only (k-contiguous operands): the SAME operand already split into its two fp16 pieces by
   * ssc_split_f16 with the product's a_scale / b_scale ("planes"; ld in 4-byte words, >= K rounded up to 32, a multiple of 4;
   * 16-byte aligned).  The kernel then copies the pieces instead of forming them once per tile that reads the operand - bit-identical
   * results.  A / B stay mandatory: every other form of the product reads them.  NULL = split inside the kernel. */
  const void* A16; const void* B16;
  int lda16, ldb16;
} ssc_gemm_seg;

typedef struct {
  ssc_gemm_seg seg[SSC_MAX_SEG];
  int nseg;
  int M, N;
  int a_kc, b_kc;
  float* C; int ldc;
  const float* bias;   /* optional (N) */
  int accumulate;      /* 1: C += result */
  int splits;          /* >=1; 0 = choose automatically */
  float* workspace; size_t workspace_floats;
  /* Optional device-side row compaction (all NULL = off).  Counts and index lists live in device memory, so the host
   * needs no synchronisation to know how many rows are active; the launch covers the full M / K and workgroups beyond
   * the device count exit.  Only with 16-B aligned operands (else SSC_EALIGN).
   *   m_count: M = min(M, *m_count); a_rows: row r of the k-contiguous A operand is read from row a_rows[r];
   *   c_rows: row r of the result is written to row c_rows[r]   (NT / NN products)
   *   k_count: K = min(K, *k_count); ka_rows / kb_rows: k-row k of A / B is read from row k?_rows[k]
   *            (single-segment TN products, a_kc = b_kc = 0) */
  const int* m_count; const int* a_rows; const int* c_rows;
  const int* k_count; const int* ka_rows; const int* kb_rows;
  /* Optional, used by the 2xFP16 form only (ssc_model_cfg.gemm_mode 3): device scalars holding POWERS OF TWO the A / B operands are
   * multiplied with before they are split into two fp16 pieces (the result is multiplied with the exact inverse of their product).
   * Choose them so that the operands' largest magnitudes land near 2^6 .. 2^13 (ssc_pow2_scale): fp16 overflows at 65504, and an
   * entry whose lo piece is below 2^-14 keeps an absolute precision of 2^-25 only.  NULL = 1. */
  const float* a_scale; const float* b_scale;
  /* Optional: instead of C (which may then be NULL), every (row, 128-column tile) leaves a record of 6 floats at
   * topk_part[(row * ceil(N / 128) + tile) * 6]: the tile's maximum, sum of exp(x - maximum), best value, its column (int bits),
   * second best, its column; x includes the bias; ties go to the lower column; c_rows applies to the record's row.  The
   * vocabulary head of a decode step then never writes its (rows, V) logits: ssc_beam_step_parts selects from the records.
   * NT products with 16-byte aligned operands under the 3xBF16 / 2xFP16 numerics only (SSC_EINVAL otherwise). */
  float* topk_part;
  /* Optional, ssc_gemm_dw_group only (SSC_EINVAL elsewhere): a second destination (M x N, ld ldc2 >= N) that receives the values
   * stored to C - two gradients that are the same product (an LSTM's W_hh and the recurrent block of its W_ih).  A work-list member
   * stores both from its tile epilogue; any other member is followed by a copy. */
  float* C2; int ldc2;
} ssc_gemm_desc;

/* out[0] = 2^(target_log2 - ceil(log2(max |x|))) over the rows x cols block x (ld), a power of two that brings the block's largest
 * magnitude to [2^(target_log2 - 1), 2^target_log2] (1 when the block is all zero).  combine = 1: out[0] = min(out[0], that).
 * scratch: one float of device memory. */
int ssc_pow2_scale(const float* x, size_t rows, int cols, size_t ld, int target_log2, float* out, int combine, float* scratch,
                   void* stream);

/* The two fp16 pieces of x * scale[0] (rows x K, ld ldx; scale: device scalar, a power of two, NULL = 1) in the plane layout of
 * ssc_gemm_seg.A16 / B16: row r occupies ldo 4-byte words; per 32-k block 32 hi halfs (x truncated to fp16) then 32 lo halfs
 * (x - hi truncated); columns K .. roundup(K, 32) are zero.  ldo >= roundup(K, 32), ldo % 4 == 0, out 16-byte aligned.
 * rows / row_count (optional, device): only the listed rows. */
int ssc_split_f16(const float* x, int rows, int K, int ldx, const float* scale, void* out, int ldo, const int* row_list,
                  const int* row_count, void* stream);

int ssc_gemm(const ssc_gemm_desc* d, void* stream);

/* n <= 32 INDEPENDENT products C_i = A_i^T B_i with direct outputs (a_kc = b_kc = 0, one segment, splits ignored): the weight
 * gradients of a train step.  Members with all three k-row lists (k_count, ka_rows, kb_rows - every member its own), 16-byte
 * aligned operands and no bias run as ONE work list on a persistent grid (one workgroup per compute unit walks the tiles of
 * every member); per output element the operations are those of the single product.  The other members go out as ssc_gemm
 * would issue them (list-less eligible ones in grouped launches).  Errors as ssc_gemm. */
int ssc_gemm_dw_group(const ssc_gemm_desc* const* d, int n, void* stream);

/* Numerics of NT products (a_kc = b_kc = 1, 16-B aligned operands): mode 1 (default) splits every fp32 operand exactly
 * into three bf16 pieces and sums the six partial products of order <= 2 on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation (error ~ one fp32 rounding per product); mode 0 uses the exact-fp32 MFMA v_mfma_f32_32x32x2_f32.
 * Process-wide; returns the previous mode.  Environment default: SSC_GEMM_MODE=x3|f32. */
int ssc_set_gemm_mode(int mode);
int ssc_gemm_auto_splits(int M, int N, int ksteps); /* the split count ssc_gemm picks for splits=0 */

/* ------------------------------------------------------------------------------------------------
 * Per-sequence precompute
 * ---------------------------------------------------------------------------------------------- */
/* region mask + masked mean: UpDownCell._average_image_features (updown_cell.py:233-270) +
 * allennlp masked_mean.  feats (B,R,F) -> mask (B,R) float {0,1}, avg (B,F).  One pass over feats; R <= 12288. */
int ssc_feat_prep(const float* feats, int B, int R, int F, float* mask, float* avg, void* stream);

/* boundary tokens + loss weights: allennlp add_sentence_boundary_token_ids as called at
 * updown_captioner.py:265-278.  caps (B,L) int64 -> tokens_tm (L+2,B) int64 time-major,
 * w_tm (T=L+1,B) float = [tokens[b,t+1] != pad], nvalid (B) float = sum_t w. */
int ssc_prep_tokens(const int64_t* caps, int B, int L, int pad, int boundary, int64_t* tokens_tm, float* w_tm,
                    float* nvalid, void* stream);

/* ssc_prep_tokens plus the two ascending row lists of the train step, in one launch: act = rows t*B+b with w = 1, live = rows
 * with w = 1 at step t or at any later step of caption b.  Each list is int32 [count, 3 unused, rows ... (T*B entries)].
 * ident (optional, B + 4 entries): the list of the rows 0 .. B-1 in the same layout - the k-row list of a product over the B rows
 * of a per-row sum when it joins the work list of ssc_gemm_dw_group. */
int ssc_prep_tokens_rows(const int64_t* caps, int B, int L, int pad, int boundary, int64_t* tokens_tm, float* w_tm,
                         float* nvalid, int* act, int* live, int* ident, void* stream);

/* nn.Embedding forward (updown_captioner.py:430): out[i,:] = table[ids[i],:]  (n rows, E cols). */
int ssc_embed_gather(const float* table, int ldt, const int64_t* ids, int n, int E, float* out, int ldo, void* stream);
/* nn.Embedding backward: dtable[ids[i],:] += d[i,:] for ids[i] != pad (padding_idx row gets no grad).  Deterministic: the rows
   of one id are summed in ascending i and added to the table row once per 4096 positions. */
int ssc_embed_scatter_add(float* dtable, int ldt, const int64_t* ids, int n, int E, const float* d, int ldd, int pad,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * LSTM cell epilogue: torch.nn.LSTMCell pointwise part (gate order i,f,g,o), fused with the split-K
 * slab reduction, the hoisted time-invariant gate terms, both biases and the rank-1 sentiment
 * column (updown_cell.py:146-148,192-194,227-229).
 *   pre[b,n] = sum_{s<nslab} slabs[s][b,n] + add0[row0(b),n] + add1[row1(b),n] + b_ih[n] + b_hh[n]
 *              + sent[b]*wcol[n*ldwcol]
 *   gates_out (B,4H) = activated (i,f,g,o);  c_out = f*c_prev + i*g;  h_out = o*tanh(c_out)
 * add1 is indexed by b / rows_per_add1 (decode: per-image hoisted term).  Any optional pointer may be 0.
 * The four forward entry points share this descriptor; the optional fields each of them reads:
 *                                       ssc_lstm_fwd   ssc_lstm_fwd_img   ssc_lstm_fwd_z / _p
 *   rows, row_count                          yes              -                   -
 *   slab_rows, c_prev_rows                   yes             yes                  -
 *   slabs2, nslab2 (slab2_stride, _rows)     yes             yes                  -
 *   h_planes (ld_hplanes, planes_scale)      yes        yes (H % 4 == 0)          -
 * A field that is set for an entry point that does not read it is SSC_EINVAL (never silently ignored); add0, add0_rows, add1,
 * the biases, the sentiment column, c_prev and gates_out are read by all four.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int B, H;
  const float* slabs; int nslab; size_t slab_stride; /* each slab (B,4H), ld 4H */
  const float* add0; int ld_add0;
  const float* add1; int ld_add1; int rows_per_add1;
  const float* b_ih; const float* b_hh;
  const float* sent; const float* wcol; int ldwcol;
  const float* c_prev; int ld_cprev;
  float* gates_out;            /* (B,4H) activated, ld 4H; may be 0 */
  float* c_out; int ld_cout;
  float* h_out; int ld_hout;
  const int64_t* add0_rows;    /* optional: add0 is indexed by add0_rows[b] instead of b (decode: a per-token table of the
                                * embedding's gate contribution, row = the beam's last token) */
  /* decode, beams that share their parent (ssc_decode_step_desc.parent): row b's slab values are read from row slab_rows[b] of
   * `slabs` (a product formed on the distinct parents only); slabs2: a second slab list with its own row index (0 = row b) */
  const int* slab_rows;
  const float* slabs2; int nslab2; size_t slab2_stride; const int* slab2_rows;
  const int* c_prev_rows;      /* optional: row b's previous cell state is row c_prev_rows[b] of c_prev (decode: states left in the
                                * previous step's row order, ssc_decode_step_desc.ungathered) */
  const int* rows; const int* row_count;   /* optional (ssc_lstm_fwd only): a device-side list of the rows to compute, *row_count of them
                                * (decode: the rows that hold a finite, unfinished beam); the other rows' outputs are left as they are */
  /* optional (ssc_lstm_fwd, ssc_lstm_fwd_img): h_out * planes_scale[0] also leaves the cell split into its two fp16 pieces, in the
   * plane layout of ssc_split_f16 (ld_hplanes 4-byte words per row, >= H rounded up to 32; the padding columns are zeroed) - the
   * operand of the next 2xFP16 product (ssc_gemm_seg.A16) without a pass of its own.  planes_scale NULL = 1.  SSC_EINVAL from
   * ssc_lstm_fwd_z / _p and from the VALU form of ssc_lstm_fwd_img (H % 4 != 0), which do not write them. */
  void* h_planes; int ld_hplanes; const float* planes_scale;
} ssc_lstm_fwd_desc;
int ssc_lstm_fwd(const ssc_lstm_fwd_desc* d, void* stream);
/* The same with one more addend formed inside the kernel: pre[b,n] += z[b,:Z] . wz[n,:Z]  (z (B,Z) ld ldz; wz (4H,Z) ld ldwz;
 * exact-fp32 MFMA).  Used for the latent block of the decoder LSTM input (updown_cell.py:211-229): z exists only after the
 * latent head of the same step, the rest of the gate product does not wait for it. */
int ssc_lstm_fwd_z(const ssc_lstm_fwd_desc* d, const float* z, int ldz, const float* wz, int ldwz, int Z, void* stream);
/* ssc_lstm_fwd that also leaves partial products of its output with an nn.Linear weight wp (NP <= 256 rows of H, ld ldwp):
 *   pout[s][b,n] = sum_{j in [16 s, 16 s + 16)} h_out[b,j] wp[n,j],   s < ceil(H/16), each slab (B,NP) ld NP
 * (the encoder LSTM's h feeds fc_mean | fc_log_var in the same step, updown_cell.py:196-197: ssc_latent_fwd sums the slabs). */
int ssc_lstm_fwd_p(const ssc_lstm_fwd_desc* d, const float* wp, int ldwp, int NP, float* pout, void* stream);
/* ssc_lstm_fwd for rows that share per-image operands (decode), with one more addend from a per-image table:
 *   pre[b,n] += sum_r alpha[b,r] P[(img(b) R + r) 4H + n],  img(b) = b / rows_per_image;  alpha (B,R) ld ldalpha; R <= 128.
 * With P[img,r,:] = W_ih^dec[:, :F] v_{img,r} (ssc_decode_prepare) this IS the attended-feature segment of the decoder gate
 * product (updown_cell.py:156-158,211-229), by linearity of the product in att = sum_r alpha_r v_r. */
int ssc_lstm_fwd_img(const ssc_lstm_fwd_desc* d, const float* alpha, int ldalpha, const float* P, int R, int rows_per_image,
                     void* stream);

/* LSTMCell pointwise backward (SURVEY Appendix A.4 "LSTM^-1"):
 *   dh (B,H) (+ dh2 optional second addend), dc_in (B,H), gates (activated), c_prev, c_new
 *   -> dG (B,4H) pre-activation grads, dc_prev (B,H).  If dgsum != 0: dgsum += dG. */
typedef struct {
  int B, H;
  const float* dh; int ld_dh;
  const float* dh2; int ld_dh2;
  const float* dc_in; int ld_dcin;
  const float* gates;
  const float* c_prev; int ld_cprev;
  const float* c_new; int ld_cnew;
  float* dG;                   /* (B,4H) ld 4H */
  float* dc_prev; int ld_dcprev;
  float* dgsum;                /* optional (B,4H) running sum over time */
  /* optional extra addends of dh given as split-K partial slabs ((B,H), ld H each) of the GEMMs that produce them:
   * dh += sum_s slabsA[s] + sum_s slabsB[s]  (fixed summation order) */
  const float* slabsA; int nA; size_t strideA;
  const float* slabsB; int nB; size_t strideB;
} ssc_lstm_bwd_desc;
int ssc_lstm_bwd(const ssc_lstm_bwd_desc* d, void* stream);
/* The same with one more addend of dh formed inside the kernel: dh[b,j] += sum_k x[b,k] w[k,j]  (x (B,K) ld ldx; w (K,H) ld ldw;
 * exact-fp32 MFMA; K <= 768: its LDS images take (48 (K+4) + 2176) floats).  BPTT of the
 * encoder LSTM: x = (dmu | dlv), w = [W_mu ; W_lv] (fc_mean / fc_log_var, updown_cell.py:196-197); of the attention LSTM:
 * x = dq, w = Wq (the query projection, attention.py:69). */
int ssc_lstm_bwd_x(const ssc_lstm_bwd_desc* d, const float* x, int ldx, const float* w, int ldw, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bottom-up top-down attention step: BottomUpTopDownAttention.forward after the q projection
 * (attention.py:78-95) + allennlp masked_softmax + the weighted sum (updown_cell.py:156-158).
 *   logit[g,r] = wa . tanh(q[g] + pv[img(g),r]);  alpha = masked_softmax(logit, mask[img(g)])
 *   att[g,:]  = sum_r alpha[g,r] feats[img(g),r,:]          img(g) = g / rows_per_image
 * Every entry but ssc_attn_logits takes G <= 65535 (the rows are the grid's second dimension): SSC_EINVAL and no launch beyond.
 * ---------------------------------------------------------------------------------------------- */
int ssc_attn_logits(const float* q, int ldq, const float* pv, const float* wa, int G, int R, int A, int rows_per_image,
                    float* logits, void* stream);
/* logits: scratch (G,R); alpha (G,R); R <= 256 */
int ssc_attn_fwd(const float* q, int ldq, const float* pv, const float* wa, const float* mask, const float* feats,
                 int G, int R, int A, int F, int rows_per_image, float* logits, float* alpha, float* att, int ldatt,
                 void* stream);

/* out (G,D) = sum_r alpha[g,r] x[img(g),r,:]: attention pooling of a per-region tensor x (nimg,R,D) with the step's weights -
 * the grounded style prior of SENTIMENT_VAE = 2 (updown_cell.py:160-163: per-region attribute means obj_atts, D = 150). */
/* the attention weights alone (no weighted feature sum): decode consumes alpha through ssc_lstm_fwd_img */
int ssc_attn_weights(const float* q, int ldq, const float* pv, const float* wa, const float* mask, int G, int R, int A,
                     int rows_per_image, float* logits, float* alpha, void* stream);

int ssc_attn_pool(const float* alpha, const float* x, int G, int R, int D, int rows_per_image, float* out, int ldo,
                  void* stream);
/* ssc_attn_fwd that also pools a second per-region tensor with the same weights, in the same launch:
 *   pool[g, :D] = sum_r alpha[g,r] obj[img(g),r,:D]   (obj (nimg,R,D); pool (G, ldpool), columns D..ldpool-1 set to 0) */
int ssc_attn_fwd_pool(const float* q, int ldq, const float* pv, const float* wa, const float* mask, const float* feats,
                      int G, int R, int A, int F, int rows_per_image, float* logits, float* alpha, float* att, int ldatt,
                      const float* obj, int D, float* pool, int ldpool, void* stream);

/* Attention backward: datt (G,F) -> dq (G,A), dpv_acc (G,R,A) += dpre,
 * dwa_acc (G,A) += sum_r dl_r u_r (caller sums over G at the end).  Training only (rows_per_image=1). */
int ssc_attn_bwd(const float* datt, int lddatt, const float* q, int ldq, const float* pv, const float* wa,
                 const float* alpha, const float* feats, int G, int R, int A, int F, float* dq, int lddq,
                 float* dpv_acc, float* dwa_acc, float* scratch_dalpha, void* stream);
/* The same when the attention weights also pooled obj (ssc_attn_fwd_pool): dalpha[g,r] += (dpool_a[g,:Da] + dpool_b[g,:D]) . obj[g,r,:D]
 * (two addends of the pooled tensor's gradient, e.g. the LSTM input gradients and the KL term; dpool_b may be 0; Da <= D: dpool_a
 * covers the first Da entries only - the conditioning block is the whole pooled vector or its first entry, updown_cell.py:169-172). */
int ssc_attn_bwd_pool(const float* datt, int lddatt, const float* q, int ldq, const float* pv, const float* wa,
                      const float* alpha, const float* feats, int G, int R, int A, int F, float* dq, int lddq,
                      float* dpv_acc, float* dwa_acc, float* scratch_dalpha, const float* obj, int D, const float* dpool_a,
                      int lddpa, int Da, const float* dpool_b, int lddpb, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Latent head epilogue: fc_mean / fc_log_var bias add, reparameterised sample and closed-form KL
 * (updown_cell.py:196-208, updown_captioner.py:295-303).
 *   mulv (B,2Z) raw [h_e Wmu^T | h_e Wlv^T] (ld ldmulv);  mu = mulv[:, :Z]+bmu;  lv = mulv[:, Z:]+blv
 *   z = eps*exp(lv/2)+mu;  kld_t[b] per formula (mode 0: vs N(0,1); mode 1: vs N(prior_mean, prior_var+1e-5))
 *   kld_acc[b] += w[b]*kld_t[b].   prior_mean per row = pm_scale*sent[b] (or 0), prior_var scalar.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int B, Z;
  const float* mulv; int ldmulv; int nslab; size_t slab_stride;
  const float* bmu; const float* blv;
  const float* eps; int ldeps;
  int kld_mode;                 /* 0: SENTIMENT_VAE==0 ; 1: otherwise */
  const float* sent; float pm_scale; float prior_var;
  const float* w;               /* (B) step weights w_bt */
  float* mu; float* lv; float* z; int ldz; /* mu, lv, z: (B, ldz) */
  float* kld_acc;               /* (B) */
  const float* pm; int ldpm;    /* optional per-row, per-dimension prior mean (B, ldpm) instead of pm_scale*sent: SENTIMENT_VAE = 2,
                                 * the attention-pooled attribute means of the step (updown_cell.py:160-163; kld_mode 1) */
} ssc_latent_fwd_desc;
int ssc_latent_fwd(const ssc_latent_fwd_desc* d, void* stream);

/* eval-mode sample: z = eps*sqrt(prior_var) + prior_mean (updown_cell.py:200-208). */
int ssc_latent_prior_sample(const float* eps, int ldeps, const float* sent, float pm_scale, float prior_var, int G, int Z,
                            float* z, int ldz, void* stream);

/* the same with a per-row, per-dimension prior mean pm (G, ldpm) - SENTIMENT_VAE = 2, where the prior mean of a step is the
 * attention-pooled attribute means (updown_cell.py:160-163,200-208) - and / or variance pv (G, ldpv); a NULL pm / pv falls back to
 * pm_scale * sent / prior_var. */
int ssc_latent_prior_sample_pm(const float* eps, int ldeps, const float* pm, int ldpm, const float* pv, int ldpv, const float* sent,
                               float pm_scale, float prior_var, int G, int Z, float* z, int ldz, void* stream);

/* latent backward (Appendix A.4): dz -> dmulv (B,2Z) = [dmu | dlv];  k[b] = gk[b]*w[b]. */
typedef struct {
  int B, Z;
  const float* dz; int lddz;
  const float* eps; int ldeps;
  const float* mu; const float* lv; int ldz;
  int kld_mode; const float* sent; float pm_scale; float prior_var;
  const float* w; const float* gk; /* (B) step weights, (B) upstream grad of kld_b */
  float* dmulv; int lddmulv;
  int nslab; size_t slab_stride; /* nslab > 1: dz is the first of nslab split-K slabs ((B, lddz) each) to be summed */
  const float* pm; int ldpm;     /* optional per-element prior mean (see ssc_latent_fwd_desc) ... */
  float* dpm; int lddpm;         /* ... and its gradient from the KL term, WRITTEN: dpm = -k (mu - pm) / (prior_var + 1e-5) */
} ssc_latent_bwd_desc;
int ssc_latent_bwd(const ssc_latent_bwd_desc* d, void* stream);

/* Free bits on the KL of the latent head: a floor lambda >= 0 (nats) below which a KL term costs lambda and has no gradient.
 * With k_tbj = the per-element closed-form KL of step t, row b, dimension j as ssc_latent_fwd forms it (-0.5 * its bracket, in the
 * formula of kld_mode 0, 1 or 2), w_tb the step weight and S_bj = sum_t w_tb k_tbj:
 *   mode 1 "element": kld_b = sum_t w_tb sum_j max(lambda, k_tbj)        gate g_tbj = [k_tbj > lambda]
 *   mode 2 "step":    kld_b = sum_t w_tb max(lambda, sum_j k_tbj)        gate g_tb  = [sum_j k_tbj > lambda]
 *   mode 3 "dim":     kld_b = sum_j (g_j ? S_bj : lambda)                gate g_j   = [K_j > lambda],  K_j = (1/B) sum_b S_bj
 *                     (Kingma et al. 2016: the floor is on the minibatch mean of each dimension, mean_b kld_b = sum_j max(lambda, K_j)
 *                     - B is the rows of THIS call, under data parallelism the rank's own minibatch)
 * The comparison is strict: a term at or below the floor contributes lambda to the value and nothing to the gradient.
 *   ssc_latent_fwd_fb: one step.  mu, lv and z are the bits of ssc_latent_fwd on the same descriptor (same slab summation order,
 *     both kernel forms).  kld_raw[b] += w[b] * sum_j k_tbj in every mode (the bits ssc_latent_fwd adds to kld_acc).  Modes 1 and 2
 *     add the floored step to d->kld_acc[b], mode 2 also writes gate_step[b] (1.0 or 0.0) for this step.  Mode 3 leaves d->kld_acc
 *     alone and adds w[b] * k_tbj to dim_acc[b * lddim + j] (the lane that holds (b, j) owns the element), the caller zeroes
 *     dim_acc before the first step and calls ssc_latent_fb_finish after the last.
 *   ssc_latent_fb_finish (mode 3): K_j = (1/B) sum_b dim_acc[b, j] with b in index order -> kdim (Z), gate_dim[j] = K_j > lambda
 *     (1.0 or 0.0), kld[b] = sum_j (gate ? dim_acc[b, j] : lambda), WRITTEN.  One launch.
 *   ssc_latent_bwd_fb: ssc_latent_bwd with the KL part of dmu, dlv and dpm multiplied by the gate - mode 1 forms k_tbj again from
 *     mu / lv with the device function the forward used, modes 2 and 3 read gate_step (B, this step's) / gate_dim (Z).  The
 *     reparameterisation part (dz) is untouched, gk stays the gradient of the objective with respect to the returned kld_b.
 * No atomics: two calls on the same inputs are bit-identical.
 * SSC_EINVAL and no launch: what ssc_latent_fwd / ssc_latent_bwd refuse, a NULL fb, lambda negative, NaN or infinite, lambda > 0
 * with a mode outside 1..3, kld_raw NULL (forward), gate_step NULL in mode 2, dim_acc NULL or lddim < Z (forward) or gate_dim NULL
 * (backward) in mode 3.  lambda = 0 means off whatever the mode: the two calls launch the kernels of ssc_latent_fwd / ssc_latent_bwd,
 * the fields of fb other than lambda are then not read or written. */
typedef struct {
  float lambda; int mode;
  float* kld_raw;                /* forward: (B) raw KL accumulator */
  float* gate_step;              /* mode 2: (B) gates of this step, written by the forward, read by the backward */
  float* dim_acc; int lddim;     /* mode 3, forward: (B, lddim) accumulator of w k_tbj */
  const float* gate_dim;         /* mode 3, backward: (Z) gates from ssc_latent_fb_finish */
} ssc_free_bits;
int ssc_latent_fwd_fb(const ssc_latent_fwd_desc* d, const ssc_free_bits* fb, void* stream);
int ssc_latent_bwd_fb(const ssc_latent_bwd_desc* d, const ssc_free_bits* fb, void* stream);
int ssc_latent_fb_finish(const float* dim_acc, int lddim, int B, int Z, float lambda, float* kdim, float* gate_dim, float* kld,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vocabulary cross-entropy: allennlp sequence_cross_entropy_with_logits(average=None) times the
 * target length (updown_captioner.py:457-466).  logits (T*B, V) time-major rows (row = t*B+b).
 *   fwd: nll[row] = lse - logits[row,target];  loss[b] = n_b * sum_t w*nll / (n_b + 1e-13)
 *        `lse` must hold 2*T*B floats: [lse | w*nll]
 *   bwd (in place): logits[row,:] <- (softmax - onehot) * gl[b] * w[row] * n_b/(n_b+1e-13)
 * ---------------------------------------------------------------------------------------------- */
int ssc_ce_fwd(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
               int V, float* lse, float* loss, void* stream);
int ssc_ce_bwd(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
               const float* gl, int T, int B, int V, void* stream);
/* Label-smoothed vocabulary cross-entropy: the same loss with torch.nn.functional.cross_entropy's label_smoothing = eps in
 * [0, 1) on every row - the eps mass is uniform over ALL V classes, the target, the pad / unknown index and the boundary included:
 *   row(eps) = lse - (1-eps) * logits[row,target] - (eps/V) * sum_v logits[row,v]
 *   fwd: loss[b] = n_b * sum_t w*row(eps) / (n_b + 1e-13);   nll[b] (optional, may be NULL) = the same with row(0): the
 *        unsmoothed loss of the same forward, at no extra pass.  `lse` must hold 3*T*B floats: [lse | w*row(eps) | w*row(0)]
 *   bwd (in place): logits[row,:] <- (softmax - (1-eps) * onehot - eps/V) * gl[b] * w[row] * n_b/(n_b+1e-13)
 * Rows with w = 0 are skipped as in ssc_ce_fwd / ssc_ce_bwd: their logits are never read (they may hold anything), the forward
 * writes 0 into their three slots, the backward a zero row.  Columns V .. ldl-1 of a padded row are neither read nor written.
 * The forward scans a row ONCE (one workgroup per row: running maximum, rescaled sum of exponentials and sum_v (x[v] -
 * x[target]) together; row(eps) = (lse - x[target]) - (eps/V) * that sum, so no large lse - mean(x) difference is formed); the
 * backward is one in-place stream.  Both move 16 bytes per lane when ldl % 4 == 0: a scalar head up to the first 16-byte
 * boundary of the row (every row then shares the misalignment of `logits`), the 16-byte bulk, a scalar tail; any other ldl
 * takes the scalar path throughout.  No atomics: two calls on the same inputs are bit-identical.
 * eps = 0 launches the kernels of ssc_ce_fwd / ssc_ce_bwd: lse, loss and the gradient are bit-identical to theirs, the third
 * block of `lse` is a copy of the second and nll equals loss.
 * SSC_EINVAL and no launch, before anything touches memory: eps outside [0, 1) or NaN, a NULL pointer other than nll, T, B or
 * V < 1, ldl < V; SSC_EALIGN: logits no multiple of 4. */
int ssc_ce_fwd_smooth(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
                      int V, float eps, float* lse, float* loss, float* nll, void* stream);
int ssc_ce_bwd_smooth(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
                      const float* gl, int T, int B, int V, float eps, void* stream);
/* row-wise log_softmax (updown_captioner.py:450, nn.LogSoftmax(dim=1)); in place allowed. */
int ssc_log_softmax(const float* logits, int ldl, int rows, int V, float* out, int ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small reductions / elementwise
 * ---------------------------------------------------------------------------------------------- */
/* out[n] (+)= sum_rows wrow[row]*X[row,n]  (bias grads: wrow=0 -> weights 1; sentiment column grads) */
int ssc_colsum(const float* X, int ldx, int rows, int N, const float* wrow, float* out, int out_stride, int accumulate,
               void* stream);
/* same, two-stage for many rows: scratch >= 64*N floats; out2 (optional, stride 1) receives a second copy
 * (nn.LSTMCell's bias_ih / bias_hh gradients are the same vector). */
int ssc_colsum2(const float* X, int ldx, int rows, int N, const float* wrow, float* out, int out_stride, float* out2,
                int accumulate, float* scratch, void* stream);
/* dst[i] = src[i*stride]: one weight column made contiguous (the rank-1 sentiment column, updown_cell.py:181-184) */
int ssc_copy_strided(const float* src, size_t stride, int n, float* dst, void* stream);
/* y = tanh(x + bias) (tied output projection, updown_captioner.py:115-117) and its backward dy*(1-y^2) */
/* both: SSC_EINVAL and no launch for a leading dimension below N or rows > 65535 (rows are the grid's second dimension) */
int ssc_bias_tanh(float* x, int ldx, int rows, int N, const float* bias, void* stream);
int ssc_tanh_bwd(float* dy, int lddy, const float* y, int ldy, int rows, int N, void* stream);
int ssc_fill(float* p, size_t n, float v, void* stream);

/* clip_grad_norm_ + SGD(momentum, weight_decay) (var_updown/scripts/train.py:126-131,173-175) on flat buffers.
 *   ssc_sq_norm: partial sums of g^2 -> out (1 float, accumulated deterministically via 2 passes; scratch>=1024 floats)
 *   ssc_sgd_step: g' = g*gscale*min(1, max_norm/(sqrt(*sqnorm)*gscale+1e-6)); d = g' + wd*p;
 *                 buf = first ? d : mom*buf + d;  p -= lr*buf.     gscale folds the 1/world_size of DP. */
int ssc_sq_norm(const float* g, size_t n, float* scratch, float* out, void* stream);
int ssc_sgd_step(float* p, const float* g, float* buf, size_t n, const float* sqnorm, float gscale, float max_norm,
                 float lr, float momentum, float weight_decay, int first, void* stream);

/* clip_grad_norm_ + torch.optim.Adam / AdamW (amsgrad = False, maximize = False) on flat buffers: update number `step` >= 1 of
 * these n elements, m / v their first / second moment.  Per element, in fp32 and in this order (no fused multiply-add):
 *   coef = min(1, max_norm / (sqrt(*sqnorm) * gscale + 1e-6)) * gscale            (as ssc_sgd_step)
 *   d = g * coef
 *   decoupled = 0 (Adam, L2 folded into the gradient):  d = d + weight_decay * p
 *   decoupled = 1 (AdamW):                              p = p * (1 - lr * weight_decay)     (before anything else)
 *   m = beta1 * m + (1 - beta1) * d
 *   v = beta2 * v + ((1 - beta2) * d) * d
 *   p = p - (lr / bc1) * (m / (sqrt(v) * (1 / sqrt(bc2)) + eps)),     bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * The host forms 1 - beta1, 1 - beta2, 1 - lr * weight_decay, lr / bc1 and 1 / sqrt(bc2) in double and hands them to the kernel
 * rounded to float; sqrt and the division are the IEEE-rounded ones.  Elements with p = g = m = v = 0 (the padding columns of
 * a flat parameter layout) stay exactly 0.
 * One grid-stride stream over 16-byte loads and stores (reads p, g, m, v, writes p, m, v: 7 words per element).  Slices whose
 * start is not 16-byte aligned are fine as long as the four pointers share one misalignment: a scalar head up to the first
 * aligned element, the 16-byte bulk, a scalar tail; pointers that do not share it take the scalar path throughout.  No atomics:
 * two calls on the same inputs are bit-identical.
 * SSC_EINVAL and no launch: a NULL pointer, step < 1, a beta outside [0, 1), eps <= 0, lr < 0 or weight_decay < 0 (NaNs
 * included); SSC_EALIGN: a pointer that is no multiple of 4.  n = 0: nothing to do, SSC_OK. */
int ssc_adam_step(float* p, const float* g, float* m, float* v, size_t n, const float* sqnorm, float gscale, float max_norm,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, int step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model / sequence level: the T-step teacher-forced training forward and its BPTT
 * (UpDownCaptioner.forward training branch, updown_captioner.py:228-323; _decode_step :371-455;
 *  UpDownCell.forward updown_cell.py:86-231; backward = what autograd derives, Appendix A.4).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int V, E, H, A, F, Z;
  int S;            /* conditioning columns on the language LSTMs (updown_cell.py:47-81): 0, 1 (the sentiment column) or, with
                     * kld_mode 2 (SENTIMENT_VAE = 2: the attention-pooled attribute means, Z wide), Z (LATENT_EMBEDDING "glove") or
                     * 1 ("senti_word_net": their first entry, updown_cell.py:169-172) */
  int tied;         /* 1: frozen tied embedding + Linear/Tanh projection (updown_captioner.py:112-119) */
  int kld_mode;     /* 0: SENTIMENT_VAE==0 formula; 1: otherwise (updown_captioner.py:298-303); 2: the formula of 1 with the
                     * prior mean of step t = sum_r alpha_tr obj_atts_r (SENTIMENT_VAE = 2, updown_cell.py:160-163) */
  float pm_scale;   /* prior_mean = pm_scale * sentiment (0 for SENTIMENT_VAE 0 / SIMPLE_VAE) */
  float prior_var;  /* PRIOR_STD^2 */
  int pad, boundary;
  int gemm_mode;    /* numerics of the 16-byte aligned NT / NN / TN products issued by the sequence-level calls made with THIS cfg
                     * (ssc_train_*, ssc_decode_*): 0 = the process default (ssc_set_gemm_mode), 1 = 3xBF16 (three bf16 pieces per
                     * fp32 operand, six partial products on the bf16 matrix cores, fp32 accumulate), 2 = exact-fp32 MFMA */
  float label_smoothing;  /* eps of the cross-entropy in ssc_train_fwd / ssc_train_bwd / ssc_train_bwd_phases (phase 16), see
                           * ssc_ce_fwd_smooth: 0 = the plain masked NLL (the kernels of ssc_ce_fwd / ssc_ce_bwd); outside [0, 1):
                           * SSC_EINVAL from those three calls.  The decode, score and self-critical paths ignore it */
} ssc_model_cfg;

/* Parameter (or gradient) table: device pointers + leading dimensions of 2-D weights. */
typedef struct {
  float* emb; int ld_emb;                         /* _embedding_layer.weight (V,E) */
  float* att_w_ih; int ld_att_w_ih;               /* (4H, E+F+2H) */
  float* att_w_hh; int ld_att_w_hh;               /* (4H, H) */
  float* att_b_ih; float* att_b_hh;               /* (4H) */
  float* wq; int ld_wq;                           /* (A,H) */
  float* wv; int ld_wv;                           /* (A,F) */
  float* wa;                                      /* (A) */
  float* enc_w_ih; int ld_enc_w_ih;               /* (4H, F+2H+S) */
  float* enc_w_hh; int ld_enc_w_hh;
  float* enc_b_ih; float* enc_b_hh;
  float* dec_w_ih; int ld_dec_w_ih;               /* (4H, F+2H+S+Z) */
  float* dec_w_hh; int ld_dec_w_hh;
  float* dec_b_ih; float* dec_b_hh;
  float* fc_mean_w; int ld_fc_mean_w;             /* (Z,H) */
  float* fc_mean_b;
  float* fc_lv_w; int ld_fc_lv_w;
  float* fc_lv_b;
  float* out_w; int ld_out_w;                     /* untied: _output_layer.weight (V,H); tied: unused */
  float* out_b;                                   /* untied: (V) */
  float* proj_w; int ld_proj_w;                   /* tied: _output_projection.0.weight (E,H) */
  float* proj_b;                                  /* tied: (E) */
} ssc_params;

typedef struct {
  int B, R, L;                 /* minibatch rows, regions, caption length (T = L+1 steps) */
  const float* feats;          /* (B,R,F) */
  const int64_t* caps;         /* (B,L) 0-padded, no boundary tokens */
  const float* sentiment;      /* (B) (ignored when cfg.S==0 and pm_scale==0) */
  const float* eps;            /* (T,B,Z) standard normal noise, ld Z */
  const float* obj_atts;       /* (B,R,S) per-region attribute means; kld_mode 2 only (else ignored, may be 0) */
} ssc_batch;

size_t ssc_train_workspace_bytes(const ssc_model_cfg* cfg, int B, int R, int L);

/* forward: fills loss (B), kld (B); keeps activations in `workspace` for ssc_train_bwd.  With cfg->label_smoothing > 0 loss is
 * the smoothed one; the unsmoothed loss of the same forward is kept in the workspace either way (ssc_train_workspace_view 12).
 * The backward must be given the cfg of its forward. */
int ssc_train_fwd(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace,
                  size_t workspace_bytes, float* loss, float* kld, void* stream);

/* backward: gl (B), gk (B) = upstream grads of loss_b, kld_b.  Gradients are WRITTEN (not
 * accumulated) into `g` (same layout as p); a null pointer in `g` skips that parameter's gradient
 * (frozen decoder LSTM, train.py:156-161; frozen tied embedding).  */
int ssc_train_bwd(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace,
                  size_t workspace_bytes, const float* gl, const float* gk, const ssc_params* g, void* stream);

/* The same backward in stream-ordered phases (bit mask): 1 = vocabulary head + BPTT time loop, or its two halves
 * 16 = vocabulary head (output-head gradients final) and 32 = BPTT time loop; 2 = embedding / attention-LSTM /
 * attention-projection gradients (or its halves 64 = the embedding gradient alone, 128 = the rest), 4 = encoder-LSTM and
 * latent-head gradients, 8 = decoder-LSTM gradients; 16 then 32 first, then 2 (64, 128) / 4 / 8 in any order.  Lets the caller overlap the RCCL all-reduce of a finished gradient range with the next phases. */
int ssc_train_bwd_phases(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace,
                         size_t workspace_bytes, const float* gl, const float* gk, const ssc_params* g, unsigned phases,
                         void* stream);

/* read-back of saved per-step activations for tests: which = 0:h1 1:c1 2:h_enc 3:c_enc 4:h_dec 5:c_dec
 * (each (T+1,B,H), index 0 = initial zeros), 6: alpha (T,B,R), 7: mu (T,B,Zp), 8: lv (T,B,Zp), 9: logits (T*B,V),
 * 10: tokens (L+2,B) int64, 11: att (T,B,F), 12: nll (B): the unsmoothed loss_b of the last forward (= loss with
 * label_smoothing 0).  Returns pointer into the workspace (and its ld) or 0. */
void* ssc_train_workspace_view(const ssc_model_cfg* cfg, int B, int R, int L, void* workspace, int which, int* ld);

/* The train step with a free-bits floor on the KL (see ssc_latent_fwd_fb): ssc_train_fwd_opts / ssc_train_bwd_opts (below) with
 * lambda = opts->free_bits (nats) and opts->free_bits_mode 1 element, 2 step, 3 dim.  free_bits 0 = off whatever the mode: the
 * kernels of ssc_latent_fwd / ssc_latent_bwd run and every output keeps its bits.  With free_bits > 0 kld is the floored KL and
 * the backward (the latent backward sits in phase 32) gates the KL gradient.  Mode 3 costs one launch after the time loop
 * (ssc_latent_fb_finish), B is the rows of the call.
 * SSC_EINVAL and no launch: what the plain calls refuse, free_bits negative, NaN or infinite, a mode outside 1..3 while
 * free_bits > 0.  The buffers are reserved at the end of the train workspace for any cfg and any option:
 * ssc_train_workspace_bytes does not depend on them; the numbering of ssc_train_workspace_view is pinned, so they have a view of
 * their own.
 * ssc_train_free_bits_view: what a forward with free_bits > 0 left, which = 0: the raw KL (B), 1: K_j (Z; mode 3), 2: the step
 * gates (T,B; mode 2), 3: the dimension gates (Z; mode 3), gates as 1.0 / 0.0.  Returns pointer into the workspace (and its ld) or 0. */
void* ssc_train_free_bits_view(const ssc_model_cfg* cfg, int B, int R, int L, void* workspace, int which, int* ld);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange without RCCL: direct reduce-scatter + all-gather over peer-mapped buffers (hipIpc), all
 * xGMI links of a GPU busy at once (replaces nn.DataParallel's reduce-add, var_updown/scripts/train.py:123-124).
 * buf[j] / flags[j]: rank j's flat fp32 buffer and its flag block (3*SSC_XGMI_MAX_RANKS uint32, zero-initialised) as mapped in
 * THIS process (entry `rank` = the local ones).  ssc_xgmi_allreduce enqueues, on `stream`, the in-place sum over all ranks of
 * floats [lo, hi) (multiples of 4): every rank calls it with the same (lo, hi, seq), seq strictly increasing from call to call.
 * Waits are bounded by `timeout` polls (0 = default); a rank that gives up writes a non-zero stage number to *err (device int).
 * ---------------------------------------------------------------------------------------------- */
#define SSC_XGMI_MAX_RANKS 8
typedef struct {
  int world, rank;
  float* buf[SSC_XGMI_MAX_RANKS];
  unsigned* flags[SSC_XGMI_MAX_RANKS];
} ssc_xgmi_comm;
int ssc_xgmi_enable_peer(int peer_device);   /* hipDeviceEnablePeerAccess from the current device (idempotent) */
/* hipIpc plumbing: export the allocation containing `ptr` (64-byte handle + ptr's offset in it); open a handle in another
 * process UNDER THE CALLER'S CURRENT DEVICE (the device whose kernels will read the mapping); close it again. */
int ssc_xgmi_ipc_export(const void* ptr, void* handle64, size_t* offset);
int ssc_xgmi_ipc_open(const void* handle64, void** base_out);
int ssc_xgmi_ipc_close(void* base);
int ssc_xgmi_peek(const void* src, void* dst_host, size_t bytes);   /* hipMemcpy D2H from a (peer-mapped) device pointer */
int ssc_xgmi_allreduce(const ssc_xgmi_comm* c, size_t lo, size_t hi, unsigned seq, unsigned timeout, int* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Eval-mode decode step (UpDownCaptioner._decode_step with training=False, updown_captioner.py:371-455;
 * UpDownCell.forward training=False branch, updown_cell.py:200-229).  G rows, batch-major:
 * row g belongs to image g / rows_per_image; per-image terms (mask, avg, pv, hoisted gate term)
 * come from ssc_decode_prepare and are computed once per image instead of per step.
 * ---------------------------------------------------------------------------------------------- */
size_t ssc_decode_image_bytes(const ssc_model_cfg* cfg, int nimg, int R);
int ssc_decode_prepare(const ssc_model_cfg* cfg, const ssc_params* p, const float* feats, int nimg, int R, void* imgbuf,
                       size_t imgbuf_bytes, void* stream);
/* The same; `prev_imgbuf` (optional) is the image buffer of an EARLIER context (prev_nimg images, prev_R regions) prepared with
 * the SAME parameter values - the caller's promise: weights fixed over an inference run -; what depends on the weights alone (the
 * per-token gate table, V x 4H) is copied from it instead of being formed again. */
int ssc_decode_prepare_from(const ssc_model_cfg* cfg, const ssc_params* p, const float* feats, int nimg, int R, void* imgbuf,
                            size_t imgbuf_bytes, const void* prev_imgbuf, int prev_nimg, int prev_R, void* stream);

typedef struct {
  int G, R, rows_per_image;
  const float* feats;        /* (nimg,R,F) */
  const void* imgbuf;        /* from ssc_decode_prepare */
  const int64_t* tokens;     /* (G) previous predictions */
  const float* sentiment;    /* (G) per-row sentiment */
  const float* eps;          /* (G,Z) ld Z */
  /* states in (G,H) each, ld H; h_encoder / c_encoder are carried untouched by the caller */
  const float* h1; const float* c1; const float* hd; const float* cd;
  float* h1_out; float* c1_out; float* hd_out; float* cd_out;
  float* alpha;              /* (G,R) */
  float* log_probs;          /* (G,V) ld V; NULL: stop after the cell (UpDownCell.forward) */
  int raw_logits;            /* 1: leave the vocabulary logits un-normalised in log_probs (for ssc_beam_*_logits) */
  int emb_override;          /* 1: p->emb of THIS call is not the embedding ssc_decode_prepare saw (a caller that hands token
                              * embeddings instead of ids, UpDownCell.forward): the per-token gate table of the image context
                              * is not used, the embedding goes through the gate product */
  const int64_t* parent;     /* optional (G): after a beam re-ordering, parent[g] = index WITHIN row g's group of `group` consecutive rows of
                              * the beam it descends from (the back-pointer of cbs.py:231).  Rows of a group with equal parent[] hold
                              * identical recurrent states, so the products fed only by h1 / hd of the previous step are formed on
                              * the distinct parents (device-side row lists) and every beam reads its parent's row: at beam 5 /
                              * per-node 2 a third of the rows of those products go away.  0 = every row on its own */
  int group;                 /* rows per group (S * beam); used with `parent` */
  int att_table;             /* attended-feature term of the decoder gates (updown_cell.py:156-158,211-229): 0 = weighted feature sum +
                              * K = F segment of the gate product; 1 = from the per-image table P[img,r,:] = W_ih^dec[:, :F] v_r in the
                              * image buffer (ssc_lstm_fwd_img, K = R; R <= 128); 2 = form that table first (once per image
                              * context, by the first step that uses it), then as 1.  Pays from ~500 rows with >= 16 rows per image */
  int ungathered;            /* 1: h1 / c1 / hd / cd are the previous step's OUTPUTS in that step's row order - the caller has not
                              * re-ordered them by back-pointer (cbs.py:236-250); row g's previous state is row
                              * (g - g % group) + parent[g].  Every reader goes through the row lists the parent sharing builds
                              * anyway, so the four (G,H) gathers per step go away.  Only where ssc_decode_ungathered_ok() says
                              * so (parent sharing and the attended-feature table both in use); SSC_EINVAL otherwise */
  const float* row_lp;       /* optional (G): the running log-prob of every row's beam.  A row with row_lp <= -1e19 (no finite beam: what
                              * ssc_beam_desc.skip_dead scores without its logits) or whose token is end_index (an ended beam re-emits
                              * END whatever its logits are, cbs.py:177-181) is SKIPPED: no product is formed for it, its outputs
                              * (states, alpha, log_probs row) are unspecified.  Honoured where parent sharing and the attended-feature
                              * table are in use (untied head); elsewhere every row is computed */
  int end_index;             /* used with row_lp */
  const float* obj_atts;     /* cfg->kld_mode 2 (SENTIMENT_VAE = 2): per-region attribute means (nimg, R, Z) of the image context.  The step's
                              * prior mean is their attention-weighted sum (updown_cell.py:160-163), z = eps sqrt(prior_var) + that
                              * (:200-208), and its leading cfg->S entries (all Z: LATENT_EMBEDDING "glove"; 1: "senti_word_net",
                              * :169-172) condition the decoder LSTM (:219-222) */
  float* prior_mean_out;     /* optional (G, Z) ld Z: the pooled prior mean of every row (what the cell returns, updown_cell.py:231) */
  const float* prior_mean;   /* optional (G, Z) ld Z: the caller's own prior mean instead of pm_scale * sentiment (_decode_step's
                              * prior_mean argument, updown_captioner.py:371-381); ignored with kld_mode 2, whose cell replaces it */
  const float* prior_var;    /* optional (G, Z) ld Z: the caller's own prior variance instead of cfg->prior_var */
  float* topk_part;          /* optional (G, ceil(V / 128), 6): the vocabulary head leaves per-tile records (ssc_gemm_desc.topk_part) here INSTEAD
                              * of writing log_probs (which may then be NULL); untied head, 16-byte aligned H, not under the exact-fp32
                              * numerics (SSC_EINVAL otherwise).  For ssc_beam_step_parts */
  /* 2xFP16 numerics, large calls (cfg->gemm_mode 3, parent sharing + attended-feature table in use): the step's products read the
   * recurrent states already split into their fp16 pieces (ssc_split_f16 layout, ssc_decode_planes_ld(cfg) words per row, G rows).
   * h1_planes_out / hd_planes_out (optional): where the cells leave the pieces of h1_out / hd_out (default: the step workspace);
   * h1_planes / hd_planes (optional): the pieces of h1 / hd, i.e. what the PREVIOUS step left in its *_planes_out - without them the
   * step splits h1 / hd itself.  Ignored by every other form of the step. */
  const void* h1_planes; const void* hd_planes;
  void* h1_planes_out; void* hd_planes_out;
} ssc_decode_step_desc;
/* words (4 bytes) per row of the state pieces above: H rounded up to 32 */
int ssc_decode_planes_ld(const ssc_model_cfg* cfg);
/* 1 if a step of G rows in groups of `group` (0: group size not known yet - any divisor of G above 1 will do) over an image context of
 * nimg images with this att_table mode can take un-gathered states */
int ssc_decode_ungathered_ok(const ssc_model_cfg* cfg, int nimg, int G, int group, int att_table);
size_t ssc_decode_step_workspace_bytes(const ssc_model_cfg* cfg, int G, int R);
int ssc_decode_step(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_decode_step_desc* d, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Constrained beam search bookkeeping on device (updown-baseline/updown/modules/cbs.py:59-277).
 *   ssc_beam_first : first step (:127-145): per (b, state s) top-`beam` of log_probs[b,:] masked by fsm[b,0,s,:]
 *   ssc_beam_step  : one later step (:170-234): ended beams forced to end_index, per target state i the
 *                    masked (-1e20) top-`per_node` per row, + running log-prob, top-`beam` over S*beam*per_node;
 *                    backpointer = idx / per_node (floor).  Ties resolve to the lowest index.
 *   ssc_gather_rows: state re-ordering by backpointer (:236-250).  SSC_EINVAL and no launch for B * rows_per_batch > 65535
 *                    (the rows are the grid's second dimension) and for src == dst.
 * fsm (B,S,S,V) uint8, or NULL with S = 1 for the trivial one-state machine (every transition allowed; what
 * MAX_GIVEN_CONSTRAINTS: 0 produces).  Row order (batch, fsm_state, beam).
 * ---------------------------------------------------------------------------------------------- */
int ssc_beam_first(const float* log_probs, int ldlp, const uint8_t* fsm, int B, int S, int V, int beam,
                   int64_t* pred, float* lp_out, void* stream);
int ssc_beam_step(const float* log_probs, int ldlp, const uint8_t* fsm, const int64_t* last_pred, const float* last_lp,
                  int B, int S, int V, int beam, int per_node, int end_index, int64_t* pred, float* lp_out,
                  int64_t* backptr, float* scratch_val, int64_t* scratch_idx, void* stream);
/* Same selections from UN-normalised vocabulary logits: every row's log-sum-exp is taken inside the selection kernel
 * (row staged in LDS, same arithmetic and summation order as ssc_log_softmax followed by the calls above, so the results
 * are bit-identical) - saves a full write + read of the (G,V) log-probability matrix per step. */
int ssc_beam_first_logits(const float* logits, int ldlp, const uint8_t* fsm, int B, int S, int V, int beam,
                          int64_t* pred, float* lp_out, void* stream);
int ssc_beam_step_logits(const float* logits, int ldlp, const uint8_t* fsm, const int64_t* last_pred, const float* last_lp,
                         int B, int S, int V, int beam, int per_node, int end_index, int64_t* pred, float* lp_out,
                         int64_t* backptr, float* scratch_val, int64_t* scratch_idx, void* stream);
int ssc_gather_rows(const float* src, int ld, const int64_t* backptr, int B, int rows_per_batch, int W, float* dst,
                    void* stream);
/* back-trace (cbs.py:252-277): preds (steps,B,SB) int64, backptrs (steps-1,B,SB) int64 -> out (B,SB,steps). */
int ssc_beam_backtrace(const int64_t* preds, const int64_t* backptrs, int steps, int B, int SB, int64_t* out,
                       void* stream);


/* ------------------------------------------------------------------------------------------------
 * Compiled finite-state machines for constrained beam search.
 * The reference keeps a machine as a dense adjacency tensor fsm[from, to, token] (uint8, (S,S,V):
 * updown-baseline/updown/utils/constraints.py:328-478) and its search scans every row's V log-probs and V mask
 * bytes once per TARGET state (cbs.py:157-250: `for i in range(num_fsm_states)` masked_fill + topk).
 * The machines the reference builds send almost every token of a from-state to ONE target set (the self-loop
 * of a main state, the reset state of a sub-state); only the word forms of the constraint words differ.
 * ssc_fsm_compile turns each (machine, from-state) into
 *     default target set (bit i = state i) | <= E exception tokens, ascending, each with its target set |
 *     an "is exception" bitmap over V | the P smallest non-exception tokens,
 * and ssc_beam_step_fsm makes ONE scan per row - the top per_node non-exception tokens - and then selects, per
 * target state, among those, the exception tokens and the -1e20 fill.  The result is the dense kernels' bit for
 * bit (same order: value descending, token ascending).  A from-state that is not "default + <= E exceptions" is
 * flagged and its rows take the dense per-target scans inside the same launch.  S <= 32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int M;   /* machines */
  int S;   /* states per machine (<= 32) */
  int V;   /* vocabulary */
  int E;   /* exception capacity per (machine, from-state) */
  int P;   /* fill tokens kept per (machine, from-state): >= the per_node of every later ssc_beam_step_fsm */
} ssc_fsm_dims;
size_t ssc_fsm_tables_bytes(const ssc_fsm_dims* d);
/* fsm (M,S,S,V) uint8 -> tables (device, ssc_fsm_tables_bytes) */
int ssc_fsm_compile(const uint8_t* fsm, const ssc_fsm_dims* d, void* tables, size_t tables_bytes, void* stream);

/* One descriptor for both search steps.  Batch entry b uses machine mach[b] (NULL: machine b), so the N_Z latent
 * samples of an image share its machine instead of carrying a copy each. */
typedef struct {
  const float* scores; int ld;   /* first: (B,V); step: (B*S*beam, V); log-probs, or un-normalised logits with raw_logits = 1 */
  int raw_logits;
  const uint8_t* fsm;            /* dense (M,S,S,V); NULL only for the trivial machine (S = 1, every transition allowed) */
  const void* tables;            /* from ssc_fsm_compile, or NULL: dense scans */
  ssc_fsm_dims dims;             /* of `tables` / `fsm` (M, S, V used when tables is NULL) */
  const int* mach;               /* (B) or NULL; every entry in [0, dims.M) - the kernels index the machines with it unchecked */
  int B, beam, per_node, end_index;
  const int64_t* last_pred;      /* step: (B, S*beam) previous predictions */
  const float* last_lp;          /* step: (B, S, beam) running log-probs */
  int64_t* pred; float* lp_out;  /* (B, S*beam), (B, S, beam) */
  int64_t* backptr;              /* step: (B, S*beam) */
  float* scratch_val; int64_t* scratch_idx;   /* step: B*S*S*beam*per_node each */
  int skip_dead;                 /* step: a row whose running log-prob is <= -1e19 (no finite beam: only -1e20 fills led to it) is
                                  * scored as if all its log-probs were 0 and its `scores` row is NOT read.  Every log-prob of the
                                  * search and every beam with a finite log-prob stay bit-identical (x + (-1e20) == -1e20 in fp32);
                                  * only the token ids of beams that are themselves <= -1e19 can differ.  Lets the caller skip the
                                  * decode step for such rows (ssc_decode_step_desc.live_*) */
  /* early stop without a host round trip (cbs.py:167 asks `(last_predictions == end).all()` before every step):
   * ctl = device int32[2 + 2*max_steps], zero-filled by the caller before the first step except ctl[0] = max_steps;
   * step t (1-based index of the column it writes, first = 0) counts the beams that have not ended, and the last workgroup of
   * the step to finish sets ctl[0] = min(ctl[0], t + 1) when there are none and writes t + 1 to host_flag[0]; it also notes its
   * own completion, host_flag[1] = t (host_flag: a device-visible pointer to TWO ints of pinned host memory, zeroed by the caller,
   * optional - ssc_decode_search bounds the host's run-ahead with [1]).  A step that finds ctl[0] <= t (the search had already stopped) emits END at +0
   * for every beam with the identity back-pointer, so that surplus steps queued by a host that polls *host_flag late change
   * nothing: columns [0, ctl[0]) of the back-trace ARE the reference's output. */
  int* ctl; int step_index; int max_steps; int* host_flag;
} ssc_beam_desc;
int ssc_beam_first_fsm(const ssc_beam_desc* d, void* stream);
int ssc_beam_step_fsm(const ssc_beam_desc* d, void* stream);
/* ssc_beam_step_fsm for the trivial machine (S = 1, fsm NULL) and per_node <= 2 from the RECORDS a vocabulary head launched with
 * ssc_gemm_desc.topk_part left (rows B*beam, ceil(V / 128) tiles of 6 floats each) instead of from the (rows, V) logits: the
 * row's log-sum-exp is combined from the tiles' partials, its best tokens from the tiles' best two.  Same selections as
 * ssc_beam_step_fsm on the logits unless two candidates collide after the subtraction of the log-sum-exp (which here is
 * summed in tile order); log-probs agree to rounding (~1e-6).  d->scores is not read.  SSC_EINVAL and no launch for S != 1, a
 * machine, tables, per_node > 2 or per_node > V (as ssc_beam_step_fsm: a row has no more candidates than tokens). */
int ssc_beam_step_parts(const ssc_beam_desc* d, const float* parts, void* stream);
/* back-trace with the step count taken from ctl[0] on the device: out (B,SB,max_steps); columns >= ctl[0] are filled with end_index */
int ssc_beam_backtrace_ctl(const int64_t* preds, const int64_t* backptrs, const int* ctl, int max_steps, int B, int SB,
                           int end_index, int64_t* out, void* stream);
/* device-visible address of a pinned (hipHostMalloc / torch pin_memory) host word, for ssc_beam_desc.host_flag */
int ssc_host_device_ptr(void* host_ptr, void** device_ptr);

/* Attention trace of a one-call decode (ssc_search_desc.attn, ssc_score_desc.attn): which regions every word looked at.  With it set,
 * step t's attention weights are written by the step itself to hist + t * rows * R instead of to the workspace block the next step
 * overwrites (no copy, no launch), and one small kernel behind the call's last step writes anc.  `steps` is max_steps (max_len for
 * ssc_decode_score), `rows` the row count of the later steps - B*S*beam for the searches, B for ssc_decode_sample, G for
 * ssc_decode_score - and n_caps = rows.  A search's first step has B rows: they are the head of slab 0.  Both buffers are the
 * caller's; neither the workspace layout nor *_workspace_bytes depend on it.  anc[q, t] is the row of slab t that holds the weights
 * behind word t of returned caption q: for a search b*S*beam + a_{t-1} with a_{T-1} = q's beam, a_{t-1} = backptr[t-1][b, a_t]
 * (word 0: b), for the two row decodes q itself.  It is -1 - the word read nothing, its slab row is unspecified - for t >= ctl[0],
 * for t >= 1 when word t - 1 of the caption is end_index (a forced END; the first END itself keeps its attention, as token_lp keeps
 * its log-prob), for every word of a beam whose final log-prob is <= -1e19, and in ssc_decode_score after a caption's end, for an
 * absent slot and from a negative id on.  Read it with ssc_attn_gather. */
typedef struct {
  float* hist;   /* (steps, rows, R): step t's alpha, written by the step itself */
  int*   anc;    /* (n_caps, steps) int32: the row of slab t whose alpha belongs to word t of caption q, or -1 */
} ssc_attn_record;

/* ------------------------------------------------------------------------------------------------
 * One diverse-decode call = ONE entry point: the whole constrained beam search over nimg images x n_samples latent
 * samples (batch entry b = (image, sample), rows (b, fsm state, beam)), every step launched from the library:
 * ConstrainedBeamSearch.search (updown-baseline/updown/modules/cbs.py:59-277) around the eval _decode_step
 * (var_updown/var_updown/models/updown_captioner.py:371-455), what var_updown/scripts/inference.py:117-189 runs per image
 * and sample.  Noise is handed in for all steps (the reference draws (rows, Z) per step, updown_cell.py:206), so the
 * random state a call consumes does not depend on where the search stops.
 * ---------------------------------------------------------------------------------------------- */
/* Where a one-call decode starts (ssc_search_desc.start): the arguments start_predictions / start_state of
 * ConstrainedBeamSearch.search (cbs.py:59).  The driver copies the four blocks into the generation of states its first step reads
 * (in place of zeroing it) and `tokens` into the first step's fed tokens (in place of filling them with end_index); nothing else
 * in its loop changes.  The first step never treats its fed token as "ended", even where it is end_index.  What the search
 * returns is the CONTINUATION: a constraint machine starts in its start state (constraint words that led to the start state do
 * not count), the decode rules' and the logit rules' histories, minimum length, length penalty and penalties, the samplers' step
 * counter and max_steps all start at the search's own step 0, and log_probs sums the continuation only (ssc_prefix_join adds a
 * prefix).  ssc_decode_prime makes one from a forced prefix.  Honoured by ssc_decode_search, the stochastic, sampled-node, diverse
 * and rules searches and ssc_decode_sample / ssc_decode_sample_opts.  SSC_EINVAL before any launch: a NULL member; `start` together
 * with a latent guide (ssc_decode_*_guided, ssc_sample_opts.guide) or with an ensemble (ssc_decode_search_ensemble). */
typedef struct {
  const float* h1; const float* c1; const float* hd; const float* cd;   /* (B, H) each, ld H: the states the FIRST step reads */
  const int64_t* tokens;                                                /* (B): the word the first step is fed; an id outside [0, V) is fed as end_index, never used as an index */
} ssc_start_state;
typedef struct {
  int nimg, R, n_samples;        /* image context (ssc_decode_prepare over nimg images of R regions); B = nimg * n_samples */
  int S, beam, per_node, max_steps, end_index;
  const float* feats;            /* (nimg, R, F) */
  const void* imgbuf;            /* from ssc_decode_prepare */
  const float* sentiment;        /* (B) or NULL */
  const float* eps0;             /* (B, Z): noise of the first step */
  const float* eps;              /* (max_steps - 1, B*S*beam, Z): noise of the later steps */
  const float* obj_atts;         /* cfg->kld_mode 2: (nimg, R, Z) per-region attribute means (ssc_decode_step_desc.obj_atts); else NULL */
  const uint8_t* fsm;            /* (M, S, S, V) dense machines; NULL with S = 1: the trivial machine */
  const void* tables;            /* ssc_fsm_compile of `fsm`, or NULL: dense scans */
  ssc_fsm_dims dims;             /* of `tables` */
  const int* mach;               /* (B) machine of every batch entry (each in [0, M): not checked on the device), or NULL: machine b */
  int skip_dead;                 /* ssc_beam_desc.skip_dead + ssc_decode_step_desc.row_lp: rows without a finite beam (needs `tables`) and rows
                                  * whose beam has ended (any machine; with the trivial machine these are the only ones) are neither
                                  * stepped nor scored from logits */
  int early_stop;                /* cbs.py:167 */
  int64_t* predictions;          /* out (B, S*beam, max_steps): columns [0, ctl[0]) are the search's; the rest holds end_index */
  float* log_probs;              /* out (B, S, beam) */
  int* ctl;                      /* device int32[2 + 2*max_steps], initialised by the call; ctl[0] = number of columns (steps) */
  int* host_flag;                /* optional: device-visible address of TWO pinned host ints (ssc_host_device_ptr), zeroed by the caller:
                                  * [0] = the stop flag, [1] = the last step the device has completed */
  const int* host_flag_host;     /* the same words' host address: read between steps - the host stops queueing once [0] is set and
                                  * stays at most two steps ahead of [1] (plain memory reads, no event, no synchronisation call) */
  const ssc_start_state* start;  /* optional start state and start token (above); NULL: zero states and end_index, as without the field -
                                  * the same launches, the same bits.  (In front of attn, which stays the descriptor's last field) */
  const ssc_attn_record* attn;   /* optional attention trace (above); NULL: off - the same launches and the same bits as without the field.
                                  * Set with a NULL hist or anc: SSC_EINVAL before any launch.  Honoured by ssc_decode_search, the
                                  * stochastic, sampled-node, diverse and rules searches and ssc_decode_sample */
} ssc_search_desc;
size_t ssc_decode_search_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d);
int ssc_decode_search(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ensemble decoding: ONE beam search over M parameter sets of one architecture (checkpoints of one configuration: seeds,
 * cross-entropy / self-critical, SGD / Adam), the members' word distributions averaged at every step of the search.
 * ---------------------------------------------------------------------------------------------- */
#define SSC_ENSEMBLE_MAX 8
/* M (rows, V) matrices of raw logits -> one (rows, V) matrix of log-probs.  Per row g and member m, lp_m[v] = logits_m[g, v] - lse_m
 * with lse_m formed exactly as ssc_log_softmax forms it (the same device function, the same summation order).
 *   mode 0 "prob":    out[v] = mx_v + log sum_m exp(lp_m[v] + logw_m - mx_v), mx_v = max_m (lp_m[v] + logw_m), members in index
 *                     order: the log of the weighted mean of the members' probabilities.  M = 1 (logw 0) is bit-equal to ssc_log_softmax
 *   mode 1 "logprob": s[v] = sum_m w_m lp_m[v] (w_m = exp(logw_m), taken once on the host), out[v] = s[v] - logsumexp_v s (the
 *                     log-softmax of s, in ssc_log_softmax's arithmetic): the normalised weighted geometric mean
 * A member row that holds a NaN has a NaN log-sum-exp, as under ssc_log_softmax: the whole output row is NaN in both modes.
 * A row with last_pred[g] == end_index or row_lp[g] <= -1e19 (either pointer may be NULL) is SKIPPED: neither read nor written -
 * the rows ssc_decode_step_desc.row_lp leaves unspecified.  One workgroup per row, no atomics, bit-reproducible; out may not alias
 * an input.  SSC_EINVAL before any launch for M outside 1 .. SSC_ENSEMBLE_MAX, a NULL member, V < 1, ld < V, ldo < V, a mode
 * other than 0 / 1 or a non-finite logw. */
typedef struct {
  int M;                       /* members, 1 .. SSC_ENSEMBLE_MAX */
  const float* const* logits;  /* host array of M device pointers, each (rows, V) raw logits, leading dimension ld */
  int ld;
  const float* logw;           /* host array (M): log of the members' weights, weights > 0 and summing to 1 (the caller normalises) */
  int mode;                    /* 0 "prob", 1 "logprob" */
} ssc_ensemble_rows_desc;
int ssc_ensemble_combine_rows(const ssc_ensemble_rows_desc* e, int rows, int V, const int64_t* last_pred, const float* row_lp,
                              int end_index, float* out, int ldo, void* stream);

/* ssc_decode_search over M members.  Per step every member runs ssc_decode_step on its own two generations of states (its own
 * fp16 pieces, attended-feature-table decision and step workspace) and leaves raw logits in its own (G, V) block; one
 * ssc_ensemble_combine_rows (given the step's last_pred / row_lp under skip_dead) turns them into log-probs and the selection of
 * ssc_decode_search reads those with raw_logits = 0; the back-pointers re-order (or are read through by) every member's states
 * alike.  Shared by the members: features, noise (every member decodes the same latent sample), sentiment, obj_atts, the parent
 * lists and row_lp.  Takes the ssc_search_desc of ssc_decode_search - any machine, mach, skip_dead, early_stop, every
 * SENTIMENT_VAE - with d->imgbuf == imgbufs[0]; the records head (ssc_decode_step_desc.topk_part) is never used, and a set d->attn
 * is SSC_EINVAL (no attention trace of an ensemble).  The stochastic, sampled-node, diverse and rules searches, ssc_decode_sample
 * and ssc_decode_score take ONE parameter set. */
typedef struct {
  int M;                             /* members, 1 .. SSC_ENSEMBLE_MAX */
  const ssc_params* const* params;   /* M parameter sets of ONE ssc_model_cfg (same architecture) */
  const void* const* imgbufs;        /* M image buffers: ssc_decode_prepare of the SAME feats under each member's params.  Two members
                                      * may share a buffer only if it was prepared under the params both of them use (not checked) */
  const float* weights;              /* (M) > 0, any scale: normalised by the call; NULL: uniform */
  int mode;                          /* as ssc_ensemble_rows_desc.mode */
} ssc_ensemble_desc;
size_t ssc_decode_search_ensemble_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_ensemble_desc* e);
int ssc_decode_search_ensemble(const ssc_model_cfg* cfg, const ssc_ensemble_desc* e, const ssc_search_desc* d, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Word-level sampling decoders (MultinomialSampler / TopKSampler / TopPSampler.sample_nodes,
 * var_updown/var_updown/modules/beam_search.py:103-293, at one draw per row).  With log_probs = log_softmax(logits):
 *   kind 0 multinomial(T): draw from softmax(log_probs / T)
 *   kind 1 top-k(k, T):    keep the k largest log_probs (ties at the k-th place: lower index first), draw from softmax(kept / T)
 *   kind 2 top-p(p, T):    sort log_softmax(log_probs / T) descending (ties: lower index first); a token is kept iff it is first or
 *                          the tempered mass strictly ahead of it is < p (p = 0: the top token only; p >= 1: every token)
 * The draw is Gumbel-max over the kept set: token = argmax_v logit_v / T + g_v (ties to the lower index), g_v = -log(-log(u_v)),
 * u_v from Philox4x32-10 with key = seed and counter (v / 4, step, row id, 0), word v % 4, mapped to (0, 1) as
 * (2 * (x >> 9) + 1) * 2^-24.  Reproducible bit for bit; no atomics in the choice.  The log-prob returned for a draw is the
 * UNTEMPERED log_probs[token].  temperature > 0 (the runtime maps a top-k / top-p temperature of 0 to 1); 1 <= top_k <= V;
 * 0 <= top_p <= 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int kind;            /* 0 multinomial, 1 top-k, 2 top-p */
  int top_k;
  float top_p;
  float temperature;
  uint64_t seed;
} ssc_sampler_desc;
/* One word per row from raw logits (rows, V) ld `ld`.  row_ids (rows) or NULL (row r): the batch entry of each row, the third
 * Philox counter word.  last_pred (rows) or NULL: a row whose previous token is end_index has ended - it emits end_index at
 * log-prob 0 and its logits are not read.  row_lp (rows) or NULL: the running caption log-prob, += the step log-prob.
 * pred_out / lp_out (rows): the token and its untempered log-prob.  probs_out (rows, V) or NULL: the filtered, renormalised
 * distribution of every row in vocabulary order (an ended row: one-hot at end_index). */
int ssc_sample_rows(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const int64_t* row_ids, int step,
                    const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out, float* probs_out,
                    void* stream);
/* The whole sampled decode of one diverse-decode call as ONE library call: the loop of ssc_decode_search with S = 1, beam = 1 and
 * no machine (d->S = d->beam = 1, d->fsm = d->tables = d->mach = NULL; per_node is not used), ssc_sample_rows in place of the
 * beam selection.  Batch entry b = (image, sample) is row b; step 0 feeds end_index (@@BOUNDARY@@).  d->skip_dead: ended rows
 * are not stepped (ssc_decode_step_desc.row_lp).  d->early_stop / ctl / host_flag / host_flag_host: the protocol of
 * ssc_beam_desc.ctl and ssc_decode_search (ctl[0] = number of columns; surplus queued steps are no-ops; bounded run-ahead).
 * Out: d->predictions (B, max_steps) - columns >= ctl[0] hold end_index -, d->log_probs (B): each caption's summed log-prob.
 * These two ARE ssc_decode_sample_opts_workspace_bytes / ssc_decode_sample_opts (ssc_sample_opts, below) with opts NULL. */
size_t ssc_decode_sample_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d);
int ssc_decode_sample(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scheduled sampling in the cross-entropy train step (Bengio et al. 2015): with probability `prob` the attention LSTM's embedding
 * input of a step is a word the model draws from its own logits of the previous step of the SAME forward, not the ground truth.
 * tok is (L+2, B) time-major, w[t, b] = [tok[t+1, b] != pad].  The target of step t is tok[t+1], always: targets, weights, nvalid,
 * the loss formula and the KL are what they are without it.  Only the input in[t, b] changes:
 *   in[0, b] = tok[0, b] (the boundary token; step 0 never samples).
 *   t >= 1: the row is ELIGIBLE iff w[t, b] == 1 and w[t-1, b] == 1 - the step has a target, and the previous step's logits row is
 *     one the head projects.  A row that is not eligible is fed tok[t, b] (padded tails; the step after an in-caption @@UNKNOWN@@,
 *     which is id 0, the pad index).
 *   An eligible row FIRES iff u[t, b] < prob, u from Philox4x32-10 with key = sampler.seed and counter (0, t, b, 1), word 0, mapped
 *     to (0, 1) as the samplers map it, (2 * (x >> 9) + 1) * 2^-24 (the word draws use a last counter word of 0: the two streams
 *     never meet).  prob = 1 fires every eligible row, prob = 0 none.
 *   A fired row is fed the token ssc_sample_rows draws from the logits row (t-1, b) of this forward with `sampler` (multinomial,
 *     top-k or top-p, with temperature; top-k with k = 1 is the arg-max variant), step = t, row id b and the same seed.  The id is
 *     fed as it is: a drawn boundary token or a drawn id 0 is treated as that id is anywhere else - id 0 gets the pad row of the
 *     table and no embedding gradient.  (A logits row without one comparable entry - all NaN - has no draw: the row keeps tok[t, b].)
 *   The drawn token is a constant: no gradient flows through the draw or the decision.
 * The logits row cross-entropy reads for (t-1, b) is bit for bit the row the draw read: the head of step t-1 is computed once,
 * inside the time loop, into the workspace's logits block, and nothing recomputes it after the loop.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float prob;                 /* in [0, 1] */
  ssc_sampler_desc sampler;   /* its seed is the one seed of the feature */
} ssc_sched_sampling;
/* The kernel of one step, one workgroup per row: logits (rows, V) ld `ld` are the previous step's, truth (rows) the ground-truth
 * inputs tok[step], w_prev / w_cur (rows) the weights of steps step-1 / step, table (*, E) ld ldt the embedding table.  Out:
 * tok_out (rows) the fed ids, fed_out (rows) 1.0 where the model's word was fed else 0.0, emb_out (rows, E) ld ldo the embedding
 * row of every fed id, gathered in the same launch.  A row that does not fire never reads its logits.  Stream-ordered, no
 * read-back.  SSC_EINVAL before any launch: prob outside [0, 1] or NaN, the sampler limits of ssc_sample_rows, a NULL pointer,
 * ld < V, ldt < E, ldo < E, step < 1. */
int ssc_sched_mix_rows(const float* logits, int ld, int rows, int V, const int64_t* truth, const float* w_prev, const float* w_cur,
                       const float* table, int ldt, int E, int step, const ssc_sched_sampling* ss, int64_t* tok_out, float* fed_out,
                       float* emb_out, int ldo, void* stream);
/* The train step with scheduled sampling: ssc_train_fwd_opts (below) with opts->sched.  sched == NULL or prob == 0: teacher
 * forcing - the same launches, the same bits.
 * Otherwise, for t >= 1, inside the time loop and in this order: the vocabulary head on h_dec of step t-1 (tied: its projection /
 * tanh / emb^T chain), ssc_sched_mix_rows, the (B x E x 4H) block of emb_t W_ih^att[:, :E] for step t; after the loop only the last
 * step's head remains.  Step 0 and everything that does not depend on the fed word stay hoisted.  The fed ids and the fed mask
 * are kept in the workspace (ssc_train_sched_view 13 / 14), behind every other block; the workspace's embedding rows hold the
 * fed words' rows.  The backward of such a forward (ssc_train_bwd_opts with the same opts) scatters the embedding gradient
 * (phase 64) by the fed ids of the workspace (id 0 receives none), not by the ground-truth inputs tok[:-1]; nothing else differs,
 * the workspace's embedding and gate rows already hold the fed words' values.  Label smoothing, free bits and the caller's KL
 * weight compose unchanged.
 * SSC_EINVAL and no launch, from the forward and the backward alike: what the plain calls refuse; with sched != NULL, prob
 * outside [0, 1] or NaN and the sampler limits.
 * ssc_train_posterior, the scoring, decode and self-critical paths never sample. */
/* read-back of what the last forward with sched->prob > 0 left, numbered on from ssc_train_workspace_view (whose own numbering
 * is pinned at 0..12, so - as the free-bits buffers - these have a view of their own): which = 13: the fed ids (T,B) int64,
 * 14: 1.0 where such an id was the model's own word, else 0.0 (T,B) float; both undefined after any other forward.  Returns
 * pointer into the workspace (and its ld) or 0. */
void* ssc_train_sched_view(const ssc_model_cfg* cfg, int B, int R, int L, void* workspace, int which, int* ld);

/* ------------------------------------------------------------------------------------------------
 * Knowledge distillation in the cross-entropy train step (Hinton et al. 2015; Kim & Rush 2016, word-level): the student's rows
 * are trained against a teacher's per-word distribution beside the (label-smoothed) hard targets.  Rows, weights w, counts n_b
 * and targets are those of ssc_ce_fwd_smooth.  Per row with w != 0, x the student's logits row, s the teacher's scores row (raw
 * logits or log-probs: only differences within a row matter), tau the temperature, alpha the mixing weight:
 *   q      = softmax(s / tau)                                 (an entry s[v] = -inf has q[v] = 0)
 *   p_tau  = softmax(x / tau)
 *   kd_row = tau^2 * sum_{v: q[v] > 0} q[v] * (log q[v] - log p_tau[v])       (tau^2 KL(q || p_tau) >= 0)
 *   row    = (1 - alpha) * row(eps) + alpha * kd_row          row(eps): the label-smoothed row of ssc_ce_fwd_smooth
 *   loss_b = n_b * sum_t w*row / (n_b + 1e-13)
 *   kd_b   = n_b * sum_t w*kd_row / (n_b + 1e-13)             (reported beside the loss, not weighted by alpha)
 *   bwd (in place): x[v] <- ((1 - alpha) * (softmax(x)[v] - (1-eps)[v==y] - eps/V) + alpha * tau * (p_tau[v] - q[v]))
 *                            * gl_b * w * n_b/(n_b + 1e-13)
 * The teacher is a constant (no gradient flows into it); nll, the unsmoothed hard loss of the same forward, is what it is without
 * distillation.  Rows with w = 0 are never read in either matrix: their slots are written as 0, the backward writes a zero row.
 * kd_row is formed relative to the rows' maxima - sum_v q[v] ((s[v]-max s) - (x[v]-max x))/tau - (log sum exp((s-max s)/tau) -
 * log sum exp((x-max x)/tau)), q[v] = 0 terms skipped -, so no large quantities cancel and a teacher that is a bit copy of the
 * student gives exactly 0.  A teacher row with a NaN gives a NaN loss for its caption; a student entry at -inf under positive
 * teacher mass gives +inf.  One workgroup per row; the forward reads each row from HBM once (a second scan finds it in L2), the
 * backward is one in-place stream; 16 bytes per lane when ldl % 4 == ldt % 4 == 0 and the two matrices share one misalignment,
 * else element by element; columns V .. ld-1 are never touched.  No atomics: two calls on the same inputs are bit-identical.
 * kd == NULL or alpha == 0: the calls ARE ssc_ce_fwd_smooth / ssc_ce_bwd_smooth (in the train step: the cross-entropy as it is
 * without opts->distill) - the same launches, the same bits, and no buffer of kd is read or written.
 * SSC_EINVAL and no launch, before anything touches memory: what the plain calls refuse; alpha outside [0, 1] or NaN; a
 * temperature <= 0, NaN or infinite; with alpha > 0 a NULL teacher or rows, ldt < V, or a teacher range that overlaps the logits
 * range.  SSC_EALIGN: a pointer that is no multiple of 4.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* teacher; int ldt;   /* (T*B, V) scores, ldt >= V; must not overlap the student's logits */
  float alpha;                     /* in [0, 1] */
  float temperature;               /* > 0, finite */
  float* rows;                     /* caller-owned, 3*T*B floats: [lse(x/tau) | lse(s/tau) | w*kd_row], written by the forward, read by the backward */
  float* kd;                       /* (B) or NULL: kd_b */
} ssc_distill;
/* `lse` holds 3*T*B floats, [lse | w*row | w*row(0)], as for ssc_ce_fwd_smooth; the backward is given the kd of its forward. */
int ssc_ce_fwd_distill(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
                       int V, float eps, const ssc_distill* kd, float* lse, float* loss, float* nll, void* stream);
int ssc_ce_bwd_distill(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
                       const float* gl, int T, int B, int V, float eps, const ssc_distill* kd, void* stream);
/* The train step with distillation: ssc_train_fwd_opts / ssc_train_bwd_opts (below) with opts->distill; the scratch is the
 * caller's, so ssc_train_workspace_bytes does not change.  Only the two cross-entropy calls of the step change - the forward's
 * after the vocabulary head, the backward's at the start of phase 16; the backward reads `rows` as its forward left it.  Label
 * smoothing, free bits and the caller's KL weight compose unchanged.  Distillation does not compose with scheduled sampling (the
 * student would be fed its own words while the teacher was fed the ground truth): both on is SSC_EINVAL.  The self-critical,
 * posterior, scoring and decode paths never distil. */

/* ------------------------------------------------------------------------------------------------
 * Token-level unlikelihood training in the cross-entropy train step (Welleck et al. 2020, "Neural Text Generation with
 * Unlikelihood Training"): beside the (label-smoothed) likelihood of its target, a row lowers the probability of the words its
 * caption has already used.  Rows, weights w, counts n_b, targets y and eps are those of ssc_ce_fwd_smooth; rows are time-major,
 * row = t*B + b.  Per row with w != 0, x the logits row, alpha the weight, delta = min_one_minus:
 *   C(t,b) = the distinct ids y[s,b] over s < t with w[s,b] != 0, minus y[t,b]        (the candidates; step 0 has none; a context
 *            position with w = 0 - padding, an in-caption unknown - contributes none; no id is special-cased beyond that)
 *   p      = softmax(x),  om_c = 1 - p[c], formed as -expm1f(x[c] - lse)
 *   ul_row = - sum_{c in C} log(max(om_c, delta))            (a clamped candidate contributes -log(delta) and no gradient)
 *   g_c    = p[c] / om_c where om_c > delta, else 0;  G = sum_c g_c
 *   row    = row(eps) + alpha * ul_row                        row(eps): the label-smoothed row of ssc_ce_fwd_smooth
 *   loss_b = n_b * sum_t w*row / (n_b + 1e-13)
 *   ul_b   = n_b * sum_t w*ul_row / (n_b + 1e-13)             (reported beside the loss, not weighted by alpha)
 *   bwd (in place): x[v] <- (softmax(x)[v] - (1-eps)[v==y] - eps/V - alpha*G*softmax(x)[v] + alpha*g_v [v in C])
 *                            * gl_b * w * n_b/(n_b + 1e-13)
 * nll, the unsmoothed hard loss of the same forward, is what it is without the option.  Rows with w = 0 are never read: their
 * slots are written as 0, the backward writes a zero row.  Columns V .. ld-1 are never touched.  One workgroup per row, one lane per
 * context position (hence T <= 256); the forward scans the row once as ssc_ce_fwd_smooth does and then gathers the candidates'
 * logits, the backward gathers them before its in-place stream and patches them after it; 16 bytes per lane when ldl % 4 == 0.
 * No atomics, every sum in a fixed order: two calls on the same inputs are bit-identical.
 * ul == NULL or alpha == 0: the calls ARE ssc_ce_fwd_smooth / ssc_ce_bwd_smooth (in the train step: the cross-entropy as it is
 * without the descriptor) - the same launches, the same bits, and no buffer of the descriptor is read or written.
 * SSC_EINVAL and no launch, before anything touches memory: what the smoothed calls refuse; alpha negative, NaN or infinite;
 * min_one_minus outside (0, 1) or NaN; with alpha > 0 a NULL rows or T > 256.  SSC_EALIGN: rows or ul no multiple of 4.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float alpha;            /* >= 0, finite; 0 = off */
  float min_one_minus;    /* delta, in (0, 1); the host's default is 1e-5, the clamp of fairseq's implementation */
  float* rows;            /* caller-owned, 2*T*B floats: [G | w*ul_row], written by the forward, read by the backward */
  float* ul;              /* (B) or NULL: ul_b */
} ssc_unlikelihood;
/* `lse` holds 3*T*B floats, [lse | w*row | w*row(0)], as for ssc_ce_fwd_smooth; the backward is given the descriptor of its forward. */
int ssc_ce_fwd_unlike(const float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, int T, int B,
                      int V, float eps, const ssc_unlikelihood* ul, float* lse, float* loss, float* nll, void* stream);
int ssc_ce_bwd_unlike(float* logits, int ldl, const int64_t* targets, const float* w, const float* nvalid, const float* lse,
                      const float* gl, int T, int B, int V, float eps, const ssc_unlikelihood* ul, void* stream);
/* The train step with unlikelihood training: ssc_train_fwd_unlike / ssc_train_bwd_unlike (behind ssc_train_opts, below); the
 * scratch is the caller's, so ssc_train_workspace_bytes does not change.  Only the two cross-entropy calls of the step change - the
 * forward's after the vocabulary head, the backward's at the start of phase 16; the backward reads `rows` as its forward left it.
 * Label smoothing, free bits, the caller's KL weight and scheduled sampling compose unchanged (under scheduled sampling the
 * candidates are the ground-truth targets, as the loss's targets are).  It does not compose with distillation: both on (alpha of
 * both > 0) is SSC_EINVAL.  The self-critical, posterior, scoring and decode paths never apply it. */

/* ------------------------------------------------------------------------------------------------
 * The options of one train step.  The layout of ssc_model_cfg is pinned, so an option travels beside the cfg, in this
 * descriptor - free bits (ssc_latent_fwd_fb), scheduled sampling and distillation (above) today; the next option is a field here,
 * never an entry of its own.  opts == NULL or every option off: the calls ARE ssc_train_fwd / ssc_train_bwd_phases - the same
 * launches, the same bits (those are these with opts NULL, ssc_train_bwd with phases 15 besides).  One rule for the backward: it
 * is given the cfg and the opts of its forward, with every buffer the opts point to as that forward left it.
 * phases: the mask of ssc_train_bwd_phases; 15 is the whole backward; 0 or > 255 is SSC_EINVAL.
 * SSC_EINVAL and no launch, from both entries: what the plain calls and each option's block refuse; sched on (prob > 0) together
 * with distill on (alpha > 0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float free_bits; int free_bits_mode;   /* lambda in nats and 1 element | 2 step | 3 dim; free_bits 0 = off whatever the mode */
  const ssc_sched_sampling* sched;       /* NULL or prob 0 = teacher forcing */
  const ssc_distill* distill;            /* NULL or alpha 0 = off */
} ssc_train_opts;
int ssc_train_fwd_opts(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace, size_t workspace_bytes,
                       float* loss, float* kld, const ssc_train_opts* opts, void* stream);
int ssc_train_bwd_opts(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace, size_t workspace_bytes,
                       const float* gl, const float* gk, const ssc_params* g, unsigned phases, const ssc_train_opts* opts,
                       void* stream);
/* The same two entries with an ssc_unlikelihood (above) beside the opts.  While ssc_version() is 4 the 24 bytes of ssc_train_opts
 * are as pinned as ssc_model_cfg is - a caller built against them hands the library exactly those, so a field behind `distill`
 * would be read out of that caller's memory -, so this descriptor is an argument of its own; when the version next moves it becomes
 * a field of ssc_train_opts and these entries go.  ul == NULL or alpha == 0: the calls ARE ssc_train_fwd_opts / ssc_train_bwd_opts.
 * The backward is given the ul of its forward, `rows` as that forward left it.  SSC_EINVAL and no launch, from both entries: what
 * those refuse and what ssc_unlikelihood's block refuses (T = L + 1 > 256 with alpha > 0 among it); distill on (alpha > 0) together
 * with unlikelihood on (alpha > 0). */
int ssc_train_fwd_unlike(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace, size_t workspace_bytes,
                         float* loss, float* kld, const ssc_train_opts* opts, const ssc_unlikelihood* ul, void* stream);
int ssc_train_bwd_unlike(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_batch* batch, void* workspace, size_t workspace_bytes,
                         const float* gl, const float* gk, const ssc_params* g, unsigned phases, const ssc_train_opts* opts,
                         const ssc_unlikelihood* ul, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring GIVEN captions under the model (teacher forcing): how likely is a caption that came from elsewhere - a ground-truth
 * caption, another decoder's or another checkpoint's output.
 * ---------------------------------------------------------------------------------------------- */
/* The forced counterpart of ssc_sample_rows: per row of raw logits (rows, V) ld `ld`, lp = logits[target] - logsumexp(logits), the
 * row read once.  An ENDED row - last_target[r] == end_index (last_target (rows), or NULL: no row has ended), or target[r] < 0 - is
 * not read: lp_out = 0, rank_out = -1, row_lp unchanged.  An id >= V is never used as an index: lp_out = -inf, rank_out = -1, and
 * row_lp, where given, becomes -inf (a caption that holds such an id has no finite log-prob).  row_lp (rows) or NULL: the running
 * caption log-prob, += lp.  rank_out (rows) or NULL: the number of entries strictly greater than the target's logit plus the equal
 * entries at a lower index - 0: the target is the arg-max.  No float atomics: the same bits on every run. */
int ssc_score_rows(const float* logits, int ld, int rows, int V, const int64_t* target, const int64_t* last_target, int end_index,
                   float* row_lp, float* lp_out, int* rank_out, void* stream);
/* One scoring call = ONE entry point: nimg images x n_captions (C) captions x n_samples (N) latent samples, row g = (image, caption,
 * sample), G = nimg * C * N rows of ssc_decode_step with rows_per_image = C * N, in the form the beam-1 drivers give the steps
 * (ssc_decode_sample).  Step 0 feeds end_index (@@BOUNDARY@@) from zero states, step t feeds target t - 1; each step leaves raw
 * logits and ssc_score_rows reads the target's log-prob from them.  max_len steps, known on the host: no early-stop protocol.
 * From step 1 on ended and absent rows are not stepped (ssc_decode_step_desc.row_lp). */
typedef struct {
  int nimg, R, n_captions, n_samples, max_len, end_index;
  const float* feats;            /* (nimg, R, F) */
  const void* imgbuf;            /* from ssc_decode_prepare */
  const float* sentiment;        /* (G) per row, or NULL */
  const float* obj_atts;         /* cfg->kld_mode 2: (nimg, R, Z) per-region attribute means; else NULL */
  const int64_t* targets;        /* (nimg, C, max_len): the caption's words, then end_index from the caption's end on (a caption with no
                                  * end_index inside max_len is scored over max_len tokens).  A slot whose first entry is negative is
                                  * ABSENT: log-prob 0, no tokens.  A negative id further on ends the caption there; an id >= V gives
                                  * the caption the log-prob -inf.  Neither is ever used as an index */
  const float* eps0;             /* (G, Z): noise of the first step */
  const float* eps;              /* (max_len - 1, G, Z): noise of the later steps */
  float* log_probs;              /* out (G): each (caption, sample)'s summed log-prob, the END included */
  float* token_lp;               /* out (G, max_len), optional: the log-prob of every token; 0 after the caption's end */
  int* token_rank;               /* out (G, max_len), optional: ssc_score_rows' rank of every token; -1 after the caption's end */
  int* n_tokens;                 /* out (nimg, C): the scored tokens of every caption, the END included */
  const ssc_attn_record* attn;   /* optional attention trace (ssc_attn_record: steps = max_len, rows = n_caps = G); NULL: off */
} ssc_score_desc;
size_t ssc_decode_score_workspace_bytes(const ssc_model_cfg* cfg, const ssc_score_desc* d);
int ssc_decode_score(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_score_desc* d, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Latent-guided decoding: decode under a caption's posterior instead of the configured prior.  A guide gives every batch entry of a
 * one-call decode - b = (image, sample) for the search and the sampled decode, row g = (image, caption, sample) for scoring - and every
 * step t < min(steps, len[b]) the distribution its latent is drawn from: reconstruction (the stored z path of a posterior forward,
 * var NULL), style transfer (an exemplar's path on another image), interpolation (a mix of two paths), sampling around an exemplar.
 * Decode step t - step 0 feeds @@BOUNDARY@@ - uses slab t: the train forward's step index.  The guide is a z, not a prior mean:
 * SIMPLE_VAE's zeroing of the prior mean does not apply to it.
 *   guided row r of entry b = r / rows_per_entry:  z[r, j] = eps[r, j] * sqrtf(var[t, b, j]) + mean[t, b, j]   (the expression of
 *     ssc_latent_prior_sample_pm: a decode driven step by step with the guide expanded to (rows, Z) gives the same bits);
 *     var NULL: z = mean, and eps is NOT read for guided (t, b).  A negative variance gives NaN.
 *   unguided row (t >= steps, or t >= len[b]):  what ssc_latent_prior_sample gives, eps * sqrtf(cfg->prior_var) + pm_scale * sent[r].
 * Pad columns Z .. round4(Z) of z are zeroed; columns >= Z of mean / var are never read.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int steps;           /* slabs in mean / var */
  const float* mean;   /* (steps, B, ld) */
  const float* var;    /* (steps, B, ld), or NULL: 0 - z = mean and eps is NOT read for guided (t, b) */
  int ld;              /* >= Z */
  const int* len;      /* (B), or NULL: every entry is guided for all `steps` */
} ssc_latent_guide;
/* The latent launch of one decode step under a guide: `rows` rows in entries of rows_per_entry consecutive rows (B = rows /
 * rows_per_entry entries: 1 row per entry in a search's first step, S * beam in its later steps, 1 in the sampled decode and in
 * scoring).  eps (rows, ldeps), sent (rows) or NULL, z (rows, ldz), ldeps, ldz >= Z.  g NULL or t >= g->steps: exactly the launch
 * of ssc_latent_prior_sample.  16-byte accesses on each operand whose leading dimension and base allow them, scalar accesses
 * otherwise; the result does not depend on which are taken.  No atomics.  SSC_EINVAL and no launch: a NULL eps or z, rows, Z or
 * rows_per_entry < 1, rows no multiple of rows_per_entry, t < 0, steps < 1, a NULL mean, ld, ldeps or ldz < Z, a pointer that is
 * not 4-byte aligned. */
int ssc_latent_guide_rows(const ssc_latent_guide* g, int t, int rows, int rows_per_entry, int Z, const float* eps, int ldeps,
                          const float* sent, float pm_scale, float prior_var, float* z, int ldz, void* stream);
/* The one-call decodes under a guide: ssc_decode_search and ssc_decode_score through the two entries below, the sampled decode
 * through the `guide` field of its ssc_sample_opts (further below) - step t's z block drawn by ssc_latent_guide_rows, one launch in
 * place of one launch; every machine, mach, skip_dead, early_stop, attention traces and every numerics mode as without a guide,
 * and the same *_workspace_bytes.  guide NULL: the unguided call - the same launches, the same bits.  B of the guide:
 * nimg * n_samples (search, sample), nimg * n_captions * n_samples (score).  SSC_EINVAL before any launch: what the unguided call
 * refuses; steps < 1, a NULL mean, ld < cfg->Z, a mean, var or len that is not 4-byte aligned, cfg->kld_mode == 2
 * (SENTIMENT_VAE = 2: the pooled prior mean there also conditions the LSTMs). */
int ssc_decode_search_guided(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_latent_guide* guide,
                             void* workspace, size_t workspace_bytes, void* stream);
int ssc_decode_score_guided(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_score_desc* d, const ssc_latent_guide* guide,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Comparing captions: per pair q of pred (n, Lp) and ref (n, Lr) int64, the length of each the tokens before its first end_index
 * or negative id, out (n, 5) int32 = { n_pred, n_ref, equal positions below min(n_pred, n_ref), exact (0 / 1: equal lengths, every
 * position equal), word-level Levenshtein distance }.  One thread per pair, integer arithmetic, no atomics: two calls give the same
 * bits.  SSC_EINVAL and no launch: a NULL pointer, n < 0, Lp or Lr outside [1, 128], end_index < 0.  n = 0: nothing to do. */
int ssc_caption_match(const int64_t* pred, int Lp, const int64_t* ref, int Lr, int n, int end_index, int* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Posterior scoring of given captions: what the encoder branch q(z_t | x) = N(mu_tb, exp(lv_tb)) of the TRAIN forward says about a
 * caption - the pieces of the ELBO and of the importance-weighted bound with q as the proposal (Burda et al. 2016).
 * Rows r = t * B + b (step t of caption row b).  w (T*B): the train forward's step weight.  The generative prior is the one the
 * eval decode samples: p(z_t) = N(pm_tb, prior_var), pm = the explicit `pm` where given (kld_mode 2: the pooled attribute means of
 * the step), else pm_scale * sent[b] (0 without `sent`).  z = eps * exp(lv / 2) + mu as the forward stored it.  Per row b:
 *   log_ratio[b]      = sum_t w_tb sum_j 1/2 (eps^2 + lv - log prior_var - (z - pm)^2 / prior_var)
 *                     = sum_t w_tb [log p(z_t) - log q(z_t | x)]        (the 2 pi terms cancel; z - pm uses the STORED z)
 *   kl[b]             = sum_t w_tb sum_j k_tbj, the training KL in the formula of kld_mode, as ssc_latent_fwd has it:
 *                         0:    k = -1/2 (1 + lv - mu^2 - exp(lv))                 (against N(0, 1) whatever prior_var is)
 *                         1, 2: k = -1/2 (1 + lv - log prior_var - ((mu - pm)^2 + exp(lv)) / (prior_var + 1e-5))
 *   kl_dim[b, j]      = sum_t w_tb k_tbj          step_kl[t*B+b] = w_tb sum_j k_tbj
 *   step_ratio[t*B+b] = the step's part of log_ratio
 * One wave per caption row, lanes over j with a stride of 64, t sequential; the per-dimension sums stay in registers and the row
 * scalars are one ssc_wave_sum of them: a fixed summation order, no float atomics, the same bits on every run.  A step with
 * w == 0 is SKIPPED, not multiplied by zero: its rows of mu / lv / z / eps / pm are not read (they may hold anything), its step
 * outputs are 0; a row without a live step gives 0 everywhere.  Columns j >= Z are never read.  Z <= 512.
 * SSC_EINVAL and no launch: a NULL descriptor or required pointer, T, B or Z <= 0, Z > 512, ldz / ldeps / ldpm / ld < Z,
 * prior_var <= 0 (NaN included), kld_mode outside 0..2, kld_mode 2 without pm. */
typedef struct {
  int T, B, Z;
  const float* mu;               /* (T*B, ldz) */
  const float* lv;               /* (T*B, ldz) */
  const float* z;                /* (T*B, ldz) */
  int ldz;
  const float* eps;              /* (T*B, ldeps) */
  int ldeps;
  const float* w;                /* (T*B) */
  const float* pm;               /* (T*B, ldpm) prior mean of every step, or NULL */
  int ldpm;
  int kld_mode;
  const float* sent;             /* (B) or NULL */
  float pm_scale, prior_var;
  float* log_ratio;              /* out (B) */
  float* kl;                     /* out (B) */
  float* kl_dim;                 /* out (B, ld), optional */
  int ld;
  float* step_kl;                /* out (T*B), optional */
  float* step_ratio;             /* out (T*B), optional */
} ssc_posterior_rows_desc;
int ssc_posterior_rows(const ssc_posterior_rows_desc* d, void* stream);
/* The same for the forward that LAST ran in `workspace` (ssc_train_fwd with this cfg and a batch of these B, R, L): the descriptor
 * is filled from that forward's mu, lv, z, step weights, pooled prior means (kld_mode 2) and batch->eps, then
 *   log_w[b] = log_ratio[b] - nll[b]      (nll: the unsmoothed loss of that forward, ssc_train_workspace_view 12)
 * = log p(x | z, image) + log p(z) - log q(z | x) at the sampled z: the log importance weight of row b.  kl equals the forward's
 * kld.  log_w, log_ratio and kl (B) are required; kl_dim (B, ld), step_kl (T*B), step_ratio (T*B) may be NULL.  No state of its
 * own; nothing in the workspace is written. */
int ssc_train_posterior(const ssc_model_cfg* cfg, const ssc_batch* batch, void* workspace, size_t workspace_bytes, float* log_w,
                        float* log_ratio, float* kl, float* kl_dim, int ld, float* step_kl, float* step_ratio, void* stream);
/* read-back, for tests, of what ssc_train_posterior reads besides ssc_train_workspace_view's mu (7), lv (8) and nll (12):
 * which = 0: the stored z (T,B,Zp), 1: the pooled prior means (T,B,Dp) of kld_mode 2 (else 0), 2: the step weights w (T,B).
 * Returns pointer into the workspace (and its ld) or 0. */
void* ssc_train_posterior_view(const ssc_model_cfg* cfg, int B, int R, int L, void* workspace, int which, int* ld);

/* ------------------------------------------------------------------------------------------------
 * Stochastic beam search (GumbelSampler driving BeamSearch._search, var_updown/var_updown/modules/beam_search.py:294-432,
 * :592-768; Kool et al. 2019): `beam` = k distinct captions per batch entry, sampled without replacement with sequence-level
 * probabilities.  lp = the untempered log_softmax of a row's logits, lpT = log_softmax(logits / T) (= lp at T = 1);
 * gmax(phi, Tp): g_v = phi_v + Gumbel(u_v), Z = max_v g_v, G_v = Tp - softplus(Tp - g_v + log1p(-exp(g_v - Z))).
 *   step 0: one row per entry, G = gmax(lp, 0) (untempered, target 0); the top k by G, re-ordered by lp descending.
 *   step t >= 1: row (b, j) with running log-prob phi (ssc_beam_desc.last_lp) and state G_bj: G = gmax(phi + lpT, G_bj), the top
 *     n = per_node tokens by G, each with the summed UNTEMPERED log-prob phi + lp[token].  Per entry, the top k of the k * n
 *     candidates by G, sorted by summed log-prob descending (stable); back-pointer = candidate / n.
 *   An ended beam (last token end_index) is one-hot at end_index: its one candidate is end_index with G = G_bj exactly and
 *   log-prob phi; its logits are not read and it takes no noise.
 *   Ties: equal G - lower token, lower candidate index; equal log-probs keep the G order.  G_v is strictly increasing in g_v, so
 *   the top n by G are the top n by g (only the survivors are transformed; the order is the exact one).
 * u_v: Philox4x32-10, key = seed, counter (v / 4, step, row, 0), word v % 4, mapped to (0, 1) as for ssc_sampler_desc; row = b at
 * step 0, b * k + j after.  Limits: trivial machine only (dims.S = 1, fsm / tables / mach NULL), 1 <= per_node <= k <= 32,
 * k <= V, B * k <= 2^24, temperature > 0 and finite - SSC_EINVAL beyond them.  A slot with no finite candidate emits end_index
 * at -inf with the identity back-pointer.  ctl / host_flag: the early-stop protocol of ssc_beam_desc (step 0 included).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float temperature;   /* T > 0: tempers the perturbed scores of steps >= 1 only (the reference's sample_nodes) */
  uint64_t seed;
} ssc_gumbel_desc;
/* Step 0 from d->scores (B, V) ld d->ld (logits or log-probs: the row's log_softmax is taken).  Uses B, beam, dims.V,
 * end_index, pred / lp_out (B, k), scratch_val (>= 2 * B * k floats), scratch_idx (>= B * k), ctl / max_steps / host_flag.
 * g_out (B, k): the beams' G. */
int ssc_beam_first_gumbel(const ssc_beam_desc* d, const ssc_gumbel_desc* s, float* g_out, void* stream);
/* Step d->step_index >= 1 from d->scores (B * k, V): last_pred / last_lp (= phi) / g_last (B, k) -> pred / lp_out / g_out /
 * backptr (B, k).  scratch_val >= 2 * B * k * per_node floats, scratch_idx >= B * k * per_node. */
int ssc_beam_step_gumbel(const ssc_beam_desc* d, const ssc_gumbel_desc* s, const float* g_last, float* g_out, void* stream);
/* The whole stochastic beam search of one diverse-decode call as ONE library call: the loop of ssc_decode_search with S = 1,
 * beam k, per_node n and no machine (d->fsm = d->tables = d->mach = NULL), the Gumbel selection above in place of
 * ssc_beam_first_fsm / ssc_beam_step_fsm; the same step forms (attention table, parent lists, un-gathered states, state planes),
 * skip_dead, early stop and bounded run-ahead.  d->eps (max_steps - 1, B * k, Z).  Out: d->predictions (B, k, max_steps) -
 * columns >= ctl[0] hold end_index -, d->log_probs (B, k) sorted descending: beam 0 is the best caption. */
size_t ssc_decode_stochastic_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d);
int ssc_decode_stochastic_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_gumbel_desc* s,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sampled-node beam search (BeamSearch._search driven by MultinomialSampler / TopKSampler / TopPSampler,
 * var_updown/var_updown/modules/beam_search.py:103-293, :592-768): every live beam samples per_node = n candidate tokens from
 * the filtered, tempered distribution of ssc_sampler_desc; the k * n candidates of a batch entry are merged deterministically.
 * lp = the untempered log_softmax of a row's logits.
 *   step 0: the word samplers keep sample_beams = torch.topk: ssc_beam_first_fsm with the trivial machine (ties: lower token).
 *   step t >= 1, row (b, j) with running log-prob phi (ssc_beam_desc.last_lp): score s_v = logit_v / T + g_v over the kept set of
 *     kind 0 / 1 / 2 (as ssc_sample_rows; top-p WITHOUT replacement also keeps the first n tokens of the sorted distribution).
 *     Without replacement: the n tokens of largest s_v (Gumbel-top-n), in descending order (ties: lower token).  With replacement:
 *     n independent Gumbel-max draws, draw d with noise word d, in draw order (duplicates allowed).  Each candidate carries the
 *     summed UNTEMPERED log-prob phi + lp[token].  Per entry, the top k of the k * n candidates by summed log-prob, descending
 *     (ties: lower candidate index = j * n + slot); back-pointer = candidate / n.
 *   An ended beam (last token end_index) is one-hot at end_index: its logits are not read and it takes no noise.  Without
 *   replacement its candidates are (end_index, phi), then (end_index, -inf); with replacement all n are (end_index, phi).
 * g_v = -log(-log(u_v)), u_v: Philox4x32-10, key = seed, counter (v / 4, step, row, d), word v % 4, mapped to (0, 1) as for
 * ssc_sampler_desc; row = b * k + j, d = the draw (0 without replacement).  At k = n = 1 a step is ssc_sample_rows on the same row
 * id and step, bit for bit.  Limits: trivial machine only (dims.S = 1, fsm / tables / mach NULL), 1 <= k <= 32, 1 <= n <= 32,
 * k, n <= V, top-k with n <= top_k <= V, B * k <= 2^24, temperature > 0 and finite - SSC_EINVAL beyond them.  A slot with no
 * finite candidate emits end_index at -inf with the identity back-pointer.  ctl / host_flag: the early-stop protocol of
 * ssc_beam_desc (step 0 included).
 * ---------------------------------------------------------------------------------------------- */
/* Step d->step_index >= 1 from raw logits d->scores (B * k, V) ld d->ld: last_pred / last_lp (B, k) -> pred / lp_out / backptr
 * (B, k).  scratch_val >= B * k * per_node floats, scratch_idx >= B * k * per_node: the rows' candidates. */
int ssc_beam_step_sampled(const ssc_beam_desc* d, const ssc_sampler_desc* s, int with_replacement, void* stream);
/* The whole sampled-node beam search of one diverse-decode call as ONE library call: the loop of ssc_decode_search with S = 1,
 * beam k, per_node n and no machine, ssc_beam_first_fsm for step 0 and the sampled step after it; the same step forms, skip_dead,
 * early stop and bounded run-ahead.  d->eps (max_steps - 1, B * k, Z).  Out: d->predictions (B, k, max_steps) - columns >= ctl[0]
 * hold end_index -, d->log_probs (B, k) sorted descending: beam 0 is the best caption. */
size_t ssc_decode_sampled_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d);
int ssc_decode_sampled_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                            int with_replacement, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diverse beam search (Vijayakumar et al., "Diverse Beam Search", AAAI 2018: the "Div-BS" rows of the diverse-captioning papers).
 * Deterministic: the k beams of a batch entry are `groups` = Gr groups of k' = k / Gr consecutive beams (beam g * k' + j), searched
 * in order g = 0 .. Gr - 1 inside every step.  lp = the log_softmax of a row's logits exactly as ssc_beam_step_fsm takes it with
 * raw_logits = 1 (bit-equal to ssc_log_softmax); with raw_logits = 0 the scores are log-probs as given.  c_g[v] = the number of
 * beams of groups 0 .. g - 1 of this entry whose token selected AT THIS STEP is v (the forced END of an ended beam and an empty
 * slot are not counted).
 *   step t >= 1, live beam (g, j) with running TRUE log-prob phi (ssc_beam_desc.last_lp): r_v = lp_v - (strength * c_g[v]) (one
 *     fp32 multiply, one fp32 subtract; c = 0 leaves lp_v untouched); its candidates are the n = per_node tokens of largest r_v,
 *     descending (ties: lower token), each with the augmented sum a = phi + r_v and the true sum s = phi + lp_v.
 *   An ended beam (last token end_index): one candidate, end_index, with a = s = phi exactly; its scores are not read.
 *   Group merge: the k' candidates of largest a among the group's k' * n, descending (ties: lower candidate index j * n + slot);
 *     output slot g * k' + i gets that candidate's token, back-pointer g * k' + j and the TRUE sum s: penalties steer a step's
 *     choice and never accumulate.
 *   step 0: one row per entry; every group takes the k' tokens of largest r_v of that row (phi = 0, ties: lower token).
 * A slot with no finite candidate emits end_index at -inf with the identity back-pointer.  ctl / host_flag: the early-stop protocol
 * of ssc_beam_desc (step 0 included).  Outputs are group-major and NOT sorted across groups: the best caption of an entry is the
 * arg-max of its log-probs.  groups = 1 is ssc_beam_first_fsm / ssc_beam_step_fsm with the trivial machine, bit for bit;
 * strength = 0 runs every group as a beam-k' search on its own rows.
 * Limits: trivial machine only (dims.S = 1, fsm / tables / mach NULL), 1 <= k <= 32, 1 <= n <= 32, k, n <= V, k % groups == 0,
 * B * k <= 2^24, strength >= 0 and finite - SSC_EINVAL beyond them.  No atomics in the choice: two calls on the same inputs are
 * bit-identical.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int groups;       /* Gr >= 1, divides the beam */
  float strength;   /* lambda >= 0: the Hamming penalty per earlier selection of a token at the same step */
} ssc_diverse_desc;
/* Step 0 from d->scores (B, V) ld d->ld.  Uses B, beam, dims.V, raw_logits, end_index, pred / lp_out (B, k), scratch_val
 * (>= B * k floats) and scratch_idx (>= B * k): every row's k best (lp, token), ctl / max_steps / host_flag. */
int ssc_beam_first_diverse(const ssc_beam_desc* d, const ssc_diverse_desc* s, void* stream);
/* Step d->step_index >= 1 from d->scores (B * k, V): last_pred / last_lp (B, k) -> pred / lp_out / backptr (B, k).  With
 * m = min(per_node + k - k / groups, V): scratch_val >= B * k * m floats, scratch_idx >= B * k * m - every live row's m best
 * (lp, token), which hold its per_node best under any penalty of the other groups. */
int ssc_beam_step_diverse(const ssc_beam_desc* d, const ssc_diverse_desc* s, void* stream);
/* The whole diverse beam search of one diverse-decode call as ONE library call: the loop of ssc_decode_search with S = 1, beam k,
 * per_node n and no machine (d->fsm = d->tables = d->mach = NULL), the two steps above in place of ssc_beam_first_fsm /
 * ssc_beam_step_fsm on the raw logits; the same step forms (attention table, parent lists, un-gathered states, state planes),
 * skip_dead, early stop and bounded run-ahead.  d->eps (max_steps - 1, B * k, Z).  Out: d->predictions (B, k, max_steps)
 * group-major - columns >= ctl[0] hold end_index -, d->log_probs (B, k): the true summed log-probs, not sorted across groups. */
size_t ssc_decode_diverse_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_diverse_desc* s);
int ssc_decode_diverse_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_diverse_desc* s,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Beam search under the DECODE RULES: blocking of repeated n-grams, a minimum caption length, a list of tokens that are never
 * emitted, and a length penalty in the ranking (what captioning code bases, fairseq and HF switch on before a best-1 caption is
 * trusted).  Deterministic beam search with the trivial machine.  lp = the log_softmax of a row's logits exactly as
 * ssc_beam_step_fsm takes it with raw_logits = 1 (bit-equal to ssc_log_softmax); with raw_logits = 0 the scores are used as given.
 * A ban removes a token from a row's candidates AFTER the log-softmax: the log-probs of all other tokens are untouched and
 * nothing is renormalised.  Every beam carries its true summed log-prob phi, its token history w_0 .. w_{t-1} (the tokens of
 * steps 0 .. t - 1), its length len and its score.  With n = no_repeat_ngram, m = min_length and step t:
 *   Banned tokens of a live row at step t >= 1: the suppress list; END if t < m; with n >= 1 every token v such that the n-gram
 *     (w_{t-n+1}, .., w_{t-1}, v) already occurs in w_0 .. w_{t-1} (n = 1: every word already used; fewer than n - 1 tokens of
 *     history: nothing).  END is never banned by the n-gram rule; a live history holds no END.
 *   Live row: its candidates are the per_node unbanned tokens of largest lp, descending (ties: lower token), each with the sum
 *     s = phi + lp[v] (one fp32 add), the length L = t + 1 and the key s / length_penalty[L - 1] (one IEEE fp32 division).
 *   Ended row (last token END): one candidate, END, with s = phi and L = len of the beam; its key phi / length_penalty[len - 1]
 *     has the bits of its score of the step before.  Its scores are not read.
 *   Merge per batch entry: the k candidates of largest key among the k * per_node, descending (ties: lower candidate index
 *     j * per_node + slot).  Slot i gets that candidate's token, the back-pointer j, the true sum s, len = L and score = key; its
 *     history is the parent's first t tokens with the new token appended.
 *   Step 0: one row per entry with an empty history; the suppress list and min_length apply.  The k best unbanned tokens, with
 *     len = 1 and score = lp / length_penalty[0].
 *   A slot with no finite candidate emits END at -inf with the identity back-pointer, the history of the beam in that slot plus
 *     END, len = t + 1 and score -inf.
 * ctl / host_flag: the early-stop protocol of ssc_beam_desc (step 0 included).  A step that finds the search already stopped emits
 * END from the same beam and leaves phi, len and score as they were.  Outputs are sorted by key: beam 0 is the best caption under
 * the length penalty.  With no_repeat_ngram = 0, min_length = 0, n_suppress = 0 and every penalty 1.0f a step is
 * ssc_beam_first_fsm / ssc_beam_step_fsm with the trivial machine on the logits, bit for bit (x / 1.0f is x).
 * The library knows no penalty formula: the caller fills the table (the runtime offers L ** alpha).
 * Limits: trivial machine only (dims.S = 1, fsm / tables / mach NULL), 1 <= k, per_node <= 32, k, per_node <= V, B * k <= 2^24,
 * 0 <= n <= 64, m >= 0, 0 <= n_suppress <= 8, every suppressed id in [0, V) and not end_index, every one of the 64 penalties
 * finite and positive, 1 <= step_index <= 63 for the later step - SSC_EINVAL with no launch beyond them or with a NULL required
 * pointer.  No float atomics: two calls on the same inputs are bit-identical.  d->scores is never written.
 * ---------------------------------------------------------------------------------------------- */
#define SSC_RULES_MAX_LEN 64
#define SSC_RULES_MAX_SUPPRESS 8
typedef struct {
  int no_repeat_ngram;   /* n: 0 = off, else 1..SSC_RULES_MAX_LEN */
  int min_length;        /* m >= 0: END is banned at steps t < m (a caption has >= m words before END) */
  int n_suppress; int suppress[SSC_RULES_MAX_SUPPRESS];   /* ids in [0, V), != end_index: never candidates */
  float length_penalty[SSC_RULES_MAX_LEN];   /* entry L-1: the divisor of a caption of L tokens, END counted; > 0, finite;
                                                all 1.0f = ranking by the raw sum */
} ssc_rules_desc;
typedef struct {          /* running per-beam state; two generations are the caller's */
  const int* hist; const int* len;        /* in:  (B, k, ld_hist), (B, k); NULL at step 0 */
  int* hist_out; int* len_out; float* score_out;   /* out: same shapes, (B, k) */
  int ld_hist;            /* >= step_index + 1 */
} ssc_rules_state;
/* Step 0 from d->scores (B, V) ld d->ld.  Uses B, beam, dims.V, raw_logits, end_index, pred / lp_out (B, k), scratch_val
 * (>= B * k floats) and scratch_idx (>= B * k): every row's k best unbanned (lp, token), ctl / max_steps / host_flag. */
int ssc_beam_first_rules(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, void* stream);
/* Step d->step_index in 1..63 from d->scores (B * k, V): last_pred / last_lp (B, k) and the state's input generation -> pred /
 * lp_out / backptr (B, k) and its output generation (a different one).  scratch_val >= B * k * per_node floats, scratch_idx
 * >= B * k * per_node: every live row's per_node best unbanned (lp, token). */
int ssc_beam_step_rules(const ssc_beam_desc* d, const ssc_rules_desc* r, const ssc_rules_state* s, void* stream);
/* The whole search of one diverse-decode call as ONE library call: the loop of ssc_decode_search with S = 1, beam k, per_node n and
 * no machine (d->fsm = d->tables = d->mach = NULL), the two steps above in place of ssc_beam_first_fsm / ssc_beam_step_fsm on
 * the raw logits (never the per-tile records: a ban can remove both records of a tile); the same step forms (attention table,
 * parent lists, un-gathered states, state planes), skip_dead, early stop and bounded run-ahead.  max_steps <= 64.  d->eps
 * (max_steps - 1, B * k, Z).  Out: d->predictions (B, k, max_steps) - columns >= ctl[0] hold end_index -, d->log_probs (B, k): the
 * true summed log-probs, scores (B, k): the keys, descending along k, lengths (B, k): tokens of every caption, END counted. */
size_t ssc_decode_rules_beam_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d);
int ssc_decode_rules_beam(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_rules_desc* r,
                          float* scores, int* lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Logit rules for the word samplers (ssc_sample_rows / ssc_decode_sample): a word bias, repetition / presence / frequency
 * penalties, and bans - blocked n-grams, a minimum length, suppressed tokens.  The decode rules above ban a token AFTER the
 * log-softmax and renormalise nothing: right for ranking beams, wrong for a sampler, which needs the edited distribution.  These
 * rules edit the RAW logits of a row in place, in front of the draw; they are a second mechanism with names of their own and share
 * only the two limits SSC_RULES_MAX_LEN / SSC_RULES_MAX_SUPPRESS with ssc_rules_desc.
 * A live row r at step t has the history w_0 .. w_{t-1}: the tokens it emitted at steps 0 .. t - 1 (the BOUNDARY fed at step 0 is
 * not counted).  Its logits x[0 .. V) are edited in this order, every arithmetic step one fp32 operation:
 *   1. Bias:      x[v] = x[v] + bias[bias_row[r]][v] for every v < V.  An entry of -inf is a ban of any size.  +inf and NaN are
 *                 the caller's error (the library cannot see device memory; the runtime refuses them on the host).
 *   2. Penalties: for every distinct token c of the history, occurring n_c times:
 *                   first x[c] = x[c] > 0 ? x[c] / theta : x[c] * theta           (repetition_penalty theta)
 *                   then  x[c] = x[c] - (presence + frequency * (float)n_c)       (one multiplication, one addition, one subtraction)
 *   3. Bans (x[v] = -inf): the suppress list; END while t < min_length; with n = no_repeat_ngram >= 1 every v such that the
 *                 n-gram (w_{t-n+1}, .., w_{t-1}, v) already occurs in the history - the wording of ssc_rules_desc: n = 1 bans every
 *                 used word, fewer than n - 1 tokens of history bans nothing, END is never banned by this rule.
 * A row whose last token is END (t >= 1 and w_{t-1} == end_index) has ended: it is neither read nor written.  Columns V .. ld - 1
 * are never touched; the bias matrix is never written.  A history id outside [0, V) is skipped: never indexed with (it still
 * takes part in the n-gram comparison as a value).  ssc_sample_rows then draws from the edited row, unchanged: the log-prob it
 * returns and sums is the untempered log-softmax of the EDITED row - of the distribution the word was drawn from
 * (ssc_decode_score gives the model's own likelihood of the result).  A banned token has a perturbed score of -inf and is never
 * drawn while one entry of the row is finite.  So that the rules alone cannot empty a row, V > t + n_suppress + 1 is required;
 * emptying a row through the bias is the caller's responsibility.
 * Two kernel forms, chosen on the host.  With a bias one workgroup per row streams the row once (16-byte accesses where both rows
 * allow them, scalar ones otherwise; the sum does not depend on which), then makes the sparse edits.  Without a bias no thread
 * walks the row: one wave per row touches at most t + n_suppress + 1 elements.  No atomics: two calls on equal inputs are
 * bit-identical.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int no_repeat_ngram;        /* n: 0 = off, else 1..SSC_RULES_MAX_LEN */
  int min_length;             /* m >= 0: END is banned at steps t < m */
  int n_suppress; int suppress[SSC_RULES_MAX_SUPPRESS];   /* ids in [0, V), != end_index */
  float repetition_penalty;   /* theta > 0, finite; 1 = off */
  float presence_penalty;     /* finite; 0 = off */
  float frequency_penalty;    /* finite; 0 = off */
  const float* bias; int ld_bias; int n_bias;   /* (n_bias, V), ld_bias >= V; NULL = none */
  const int* bias_row;        /* (rows): the bias row of each logits row; NULL = row 0 for all;
                                 a value outside [0, n_bias) = no bias for that row (never indexed) */
} ssc_logit_rules;
/* The edit of `rows` rows of raw logits (rows, V) ld `ld` at step t.  Token j of row i is hist[j * ld_hist + i] - the
 * (max_steps, B) block the sampled decode keeps; hist may be NULL at t = 0.  SSC_EINVAL before any launch: a NULL logits or r, a
 * NULL hist at t >= 1, rows < 0, V < 1, ld < V, ld_hist < rows, t outside 0 .. SSC_RULES_MAX_LEN - 1, end_index outside [0, V),
 * a field beyond its limits above, a suppressed id outside [0, V) or equal to end_index, a bias with ld_bias < V or n_bias < 1,
 * V <= t + n_suppress + 1.  SSC_EALIGN: logits, hist, bias or bias_row no multiple of 4.  Every control off and no bias: SSC_OK
 * with no launch. */
int ssc_logit_rules_rows(float* logits, int ld, int rows, int V, const ssc_logit_rules* r, const int64_t* hist, int ld_hist, int t,
                         int end_index, void* stream);
/* As the `rules` field of ssc_sample_opts (below): one ssc_logit_rules_rows launch per step of the sampled decode, step 0 included.
 * The history is the call's own block of chosen words, so the workspace does not grow.  bias_row (B) is indexed by batch entry
 * b = (image, sample).  rules NULL or inactive (every control off, no bias): the launches and the bits of the call without them.
 * Composes unchanged with a guide, an attention trace, skip_dead, early_stop and every numerics mode: only the contents of the
 * logits block change.  d->log_probs sums the log-probs under the edited distributions.  SSC_EINVAL before any launch: a field of
 * `rules` beyond its limits (as above, with V = cfg->V); active rules with max_steps > SSC_RULES_MAX_LEN or
 * V <= max_steps + n_suppress.  SSC_EALIGN: bias or bias_row no multiple of 4. */

/* ------------------------------------------------------------------------------------------------
 * Truncation for the word samplers: cuts that adapt to each step's entropy - locally typical sampling (Meister et al. 2022), min-p
 * (Nguyen et al. 2024), eta and epsilon sampling (Hewitt et al. 2022).  Like the logit rules, a truncation edits the RAW logits of
 * a row in place, in front of the unchanged draw: ssc_sample_rows then draws from the edited row and its log-prob is the
 * untempered log-softmax of the EDITED row.  ssc_sampler_desc and the samplers are untouched; ssc_version() stays 4.
 * With T the sampler's temperature, over the finite entries of x[0 .. V): q = softmax(x / T), s_v = -log q_v,
 * H = -sum_v q_v log q_v (nats).  The kinds:
 *   0  off.
 *   1  typical(tau), tau in (0, 1]: the entries in ascending order of d_v = |s_v - H|, equal d by the lower index first; v is kept
 *      iff it is first in that order or the mass q strictly ahead of it is < tau - the rule of top-p, on another order.  Masses in
 *      2^-40 fixed point; entries that share the cut's d are taken to share one mass (top-p's rule, exact for equal logits).
 *      tau = 1 keeps every finite entry.
 *   2  min-p(m), m in (0, 1]: kept iff (x_v - max x) / T >= log m, i.e. q_v >= m max_u q_u.  Every maximal entry is kept.
 *   3  eta(eps), eps in (0, 1): eta = min(eps, sqrt(eps) exp(-H)); kept iff log q_v >= log eta, or v is the lowest-index maximum.
 *   4  epsilon(eps), eps in (0, 1): kept iff log q_v >= log eps, or v is the lowest-index maximum.
 * A dropped entry becomes -inf, a kept one keeps its bits.  An entry that arrives as -inf (a ban of the logit rules) stays dropped
 * and weighs nothing in Z and H.  A row without a finite entry is left as it is (statistics 0); NaN and +inf are the caller's
 * error (the call still ends and stays inside the row).  A row whose last token is END (last_pred[r] == end_index) is neither read
 * nor written (statistics 0); columns V .. ld - 1 are never touched.  One workgroup per row, the row staged in LDS for
 * V <= 32768 and walked in global memory above; 16-byte accesses where the row is 16-byte aligned with V % 4 == 0, scalar ones
 * otherwise - the result does not depend on which.  Reductions in a fixed order, integer histograms: two calls on equal inputs are
 * bit-identical.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int kind;          /* 0 off, 1 typical, 2 min-p, 3 eta, 4 epsilon */
  float value;       /* tau / m in (0, 1]; eps in (0, 1) */
  float* entropy;    /* per row: H in nats, or NULL */
  int* kept;         /* per row: the number of entries left finite, or NULL */
} ssc_truncation;
/* The edit of `rows` rows of raw logits (rows, V) ld `ld`; entropy / kept: (rows) or NULL.  last_pred (rows) or NULL: the rows'
 * previous tokens.  SSC_EINVAL before any launch: a NULL logits or tr, kind outside 0 .. 4, a value outside its range or NaN
 * (kind 0 reads none), temperature <= 0 or not finite, rows < 0, V < 1, ld < V, end_index outside [0, V) with a last_pred.
 * SSC_EALIGN: logits, last_pred, entropy or kept no multiple of 4.  kind 0: SSC_OK with no launch. */
int ssc_truncate_rows(float* logits, int ld, int rows, int V, const ssc_truncation* tr, float temperature, const int64_t* last_pred,
                      int end_index, void* stream);
/* As the `trunc` field of ssc_sample_opts (below): one ssc_truncate_rows launch per step of the sampled decode, step 0 included;
 * the truncation and then the sampler's own top-k / top-p both act on the distribution tempered by s->temperature; last_pred is the
 * previous step's words.  There trunc->entropy / trunc->kept are (max_steps, B) blocks or NULL: step t writes slab t, slabs of steps
 * never queued (early_stop) are not written.  trunc NULL or kind 0: the launches and the bits of the call without it.  The edit is
 * in place and keeps nothing between the steps, so the workspace does not grow.  d->log_probs sums the log-probs under the edited
 * distributions.  SSC_EINVAL before any launch: kind outside 0 .. 4; a value outside its range.  SSC_EALIGN: entropy or kept no
 * multiple of 4. */

/* ------------------------------------------------------------------------------------------------
 * Contrastive decoding for the word samplers (Li et al. 2023; with a degraded image as the amateur: visual contrastive decoding,
 * Leng et al. 2023): a second, AMATEUR stream is decoded in lock-step with the normal EXPERT stream, fed the same words, and the
 * expert's raw logits are contrasted with the amateur's in front of the draw - what the image, the latent, the style or the later
 * checkpoint contributes to the next word is sampled more.  With lp_e = log_softmax(x_e), lp_a = log_softmax(x_a) (untempered),
 * m = max_u lp_e[u] and logb = log(beta), every live row becomes, in place over the expert's,
 *     y[v] = lp_e[v] + alpha * (lp_e[v] - lp_a[v])    if beta == 0 or lp_e[v] >= logb + m   (the plausibility cut)
 *     y[v] = -inf                                     otherwise
 * Each log-sum-exp is formed as ssc_log_softmax forms it (the same device function, the same summation order): x - lse is bit-equal
 * to ssc_log_softmax.  logb is taken once on the host (log in double, rounded to fp32), logb + m is one fp32 addition; the edit is
 * one subtraction, one multiplication and one addition, never an fma; alpha == 0 stores lp_e itself.  Every maximal expert entry is
 * kept.  Downstream y is a row of RAW logits: the logit rules, the truncation and the draw - at the sampler's temperature - are
 * unchanged, and the log-prob a draw reports is the log-softmax of the edited row.
 * A row whose last token is END (last_pred[r] == end_index) is neither read nor written (statistics 0); columns V .. ld - 1 of
 * either row are never touched; the amateur's rows are never written and may not overlap the expert's.  NaN or +-inf in either row
 * is the caller's error (the call still ends and stays inside the rows).  amateur may be NULL iff alpha == 0: the plausibility cut
 * alone.  kept (rows) or NULL: the entries left finite; divergence (rows) or NULL: KL(p_e || p_a) = sum_v p_e[v] (lp_e[v] - lp_a[v])
 * in nats over all V entries - how much the word depended on what the amateur lacks; 0 without an amateur.
 * One workgroup per row; each row is read from HBM once, the later passes find it in L2 (no row is staged in LDS, so no bound on
 * V); 16-byte accesses where both rows are 16-byte aligned with V % 4 == 0, scalar ones otherwise - the result does not depend on
 * which.  Reductions in a fixed order, no atomics: two calls on equal inputs are bit-identical.
 * SSC_EINVAL before any launch: a NULL logits, a NULL amateur with alpha != 0, alpha < 0 or not finite, beta outside [0, 1) or NaN,
 * rows < 0, V < 1, ld < V, ld_amateur < V with an amateur, end_index outside [0, V) with a last_pred.  SSC_EALIGN: logits, amateur,
 * last_pred, kept or divergence no multiple of 4.  alpha == 0 && beta == 0: SSC_OK with no launch.
 * ---------------------------------------------------------------------------------------------- */
int ssc_contrast_rows(float* logits, int ld, const float* amateur, int ld_amateur, int rows, int V, float alpha, float beta,
                      const int64_t* last_pred, int end_index, int* kept, float* divergence, void* stream);
/* The amateur of a contrastive sampled decode.  A NULL member is the expert's own: an amateur differs from the expert in what is
 * set - its parameter set (a weak checkpoint), its image context (degraded features), its sentiment, its noise (zero noise: z at
 * the prior mean), its attribute means, or whether it follows the call's latent guide. */
typedef struct {
  float alpha, beta;             /* as ssc_contrast_rows; both 0: off */
  const ssc_params* params;      /* the amateur's parameter set (of the call's ssc_model_cfg); NULL: the expert's */
  const float* feats;            /* (nimg, R, F) the amateur's features, and ... */
  const void* imgbuf;            /* ... ssc_decode_prepare of them under the amateur's params.  Both or neither (SSC_EINVAL); NULL: the
                                  * expert's context.  params without them: SSC_EINVAL (the expert's buffer was prepared under the
                                  * expert's params) */
  const float* sentiment;        /* (B), or NULL: the expert's */
  const float* eps0;             /* (B, Z), or NULL: the expert's.  Zero noise gives z at the prior mean */
  const float* eps;              /* (max_steps - 1, B, Z), or NULL: the expert's */
  const float* obj_atts;         /* cfg->kld_mode 2: (nimg, R, Z), or NULL: the expert's */
  int guide_mode;                /* with a latent guide: 0 - the amateur follows the guide too (with its own noise where the guide has a
                                  * variance); 1 - the amateur ignores it and decodes under its prior with its noise */
  const ssc_start_state* start;  /* the amateur's start state: only the four state blocks are read, the fed tokens are the expert's
                                  * (tokens may be NULL).  Required iff d->start is set (SSC_EINVAL); not read with alpha == 0 */
  int* kept;                     /* (max_steps, B) or NULL: step t writes slab t with ssc_contrast_rows' kept; slabs of steps never ... */
  float* divergence;             /* ... queued (early_stop) are not written.  (max_steps, B) or NULL: ssc_contrast_rows' divergence */
} ssc_contrast;
/* As the `contrast` field of ssc_sample_opts (below): the sampled decode with an amateur stream.  Per step the amateur's decode step
 * is fed the expert's tokens, on its own two generations of states, its own alpha scratch, logits block, attended-feature-table
 * decision and step workspace (as a member of ssc_decode_search_ensemble has), sharing row_lp / skip_dead with the expert; then one
 * ssc_contrast_rows launch.  Everything runs on `stream`.  With alpha == 0 the amateur is not stepped and the workspace does not
 * grow.  The attention trace records the expert; early stop, the pacer, ctl and host_flag are untouched.  contrast NULL, or
 * alpha == 0 && beta == 0: the launches and the bits of the call without it.  d->log_probs sums the log-probs under the edited
 * distributions.  SSC_EINVAL before any launch: alpha or beta outside their ranges; feats without imgbuf or imgbuf without feats;
 * params without them; guide_mode outside 0 / 1; with alpha != 0 a start on one side only or with a NULL state block.  SSC_EALIGN:
 * kept or divergence no multiple of 4. */

/* ------------------------------------------------------------------------------------------------
 * The options of one sampled decode: the latent guide, the logit rules, the truncation and the contrast (their blocks above), beside
 * the search and sampler descriptors.  While ssc_version() is 4 the five pointers of this struct are fixed (its size is part of what
 * version 4 promises), so a later option travels BESIDE it, as ssc_unlikelihood travels beside ssc_train_opts: ssc_mirostat and
 * ssc_decode_sample_mirostat, below.  At the next move of ssc_version() such descriptors become fields appended here.
 * Per step, for a live row, in this order: the expert's decode step (its z block from slab t of the guide); the amateur's decode
 * step; the contrast; the logit rules; the truncation; the draw.
 * The `bytes` rule: `bytes` is sizeof(ssc_sample_opts) as the CALLER was built.  A field is read only if it lies wholly inside the
 * first `bytes` bytes; otherwise it is NULL.  So a caller built before an option existed keeps working against a later library.
 * SSC_EINVAL before anything else is read: bytes < sizeof(size_t); bytes no multiple of the pointer size; bytes above this library's
 * sizeof(ssc_sample_opts) - such a caller knows an option this library would silently drop.
 * opts NULL, or every field NULL or off: the calls ARE ssc_decode_sample_workspace_bytes / ssc_decode_sample - the same launches, the
 * same bits.  ssc_decode_sample_opts_workspace_bytes grows over the plain call's only by an amateur that is stepped (contrast
 * alpha != 0); it is 0 for a `bytes` it refuses.  SSC_EINVAL before any launch: what ssc_decode_sample and each option's block
 * refuse; a start state (d->start) together with a guide.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  size_t bytes;                     /* sizeof(ssc_sample_opts) as the caller was built */
  const ssc_latent_guide* guide;    /* NULL: the prior */
  const ssc_logit_rules*  rules;    /* NULL or every control off: no edit */
  const ssc_truncation*   trunc;    /* NULL or kind 0: no cut */
  const ssc_contrast*     contrast; /* NULL or alpha == beta == 0: no amateur, no contrast */
} ssc_sample_opts;
size_t ssc_decode_sample_opts_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_sample_opts* opts);
int ssc_decode_sample_opts(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                           const ssc_sample_opts* opts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mirostat for the word samplers (Basu et al., ICLR 2021, algorithm 2, "Mirostat 2.0"): the surprise of the generated words is held
 * at a target tau by feedback.  Every word whose surprise exceeds a running threshold mu is cut; after each draw mu moves by the
 * error between the drawn word's surprise and tau.  The one edit of the sampled decode with STATE: mu is a value per row carried
 * from step to step.  All quantities are in nats, as `entropy` and `divergence` are.  Like the truncation, the cut edits the RAW
 * logits of a row in place in front of the unchanged draw; ssc_sampler_desc and the samplers are untouched; ssc_version() stays 4.
 * With T the sampler's temperature and the row x[0 .. V) as it arrives (behind the contrast, the logit rules and the truncation),
 * over its finite entries, formed as ssc_truncate_rows forms them: mx = max x, a_v = (x_v - mx) / T, logz = log sum_v exp(a_v),
 * first = the lowest index with x_v == mx.
 *   The CUT, given the row's mu (ssc_mirostat_rows): thr = logz - mu (one fp32 subtraction); v is kept iff a_v >= thr or v == first -
 *   surprise -log q_v <= mu, or the top word.  A dropped entry becomes -inf, a kept one keeps its bits; an entry that arrives as
 *   -inf stays dropped and weighs nothing.  Per row: kept (the entries left finite, or NULL) and norm[0][r] = mx, norm[1][r] = logz
 *   (`norm` is 2 * rows floats).
 *   The UPDATE, after the draw of token w (ssc_mirostat_update): s = logz - (x_w - mx) / T, e = s - tau, mu' = mu - eta * e; each
 *   one fp32 operation, never an fma.  s is the surprise under the tempered distribution BEFORE Mirostat's own cut - the choice of
 *   the authors' reference implementation, not the surprise under the renormalised, cut distribution.  x_w is read from the edited
 *   row: a drawn word is a kept word and still holds its bits.  Per row: mu' and surprise = s (or NULL).  mu_out may be mu_in.
 * Rows that pass through: a row whose last token is END (last_pred[r] == end_index) is neither read nor written; so is a row
 * without a finite entry, and at the update a row with x_w == -inf or with pred[r] outside [0, V) (the host cannot see it: the
 * device checks it).  For these kept = 0, surprise = 0, mu' = mu, and norm is left alone.  Columns V .. ld - 1 are never touched.
 * NaN and +inf are the caller's error (the calls still end and stay inside the rows): every trip count depends on V alone, every
 * index is a loop index or a checked token id.  One workgroup per row for the cut, the row staged in LDS for V <= 32768 and walked
 * in global memory above; 16-byte accesses where the row is 16-byte aligned with V % 4 == 0, scalar ones otherwise - the result
 * does not depend on which; one thread per row for the update.  Reductions in a fixed order, no atomics: two calls on equal inputs
 * are bit-identical.
 * SSC_EINVAL before any launch: a NULL logits, mu_in, norm (and, at the update, pred or mu_out); rows < 0, V < 1, ld < V;
 * temperature <= 0 or not finite; end_index outside [0, V) with a last_pred; at the update tau < 0 or eta < 0 or either not finite.
 * SSC_EALIGN: any block that is no multiple of 4.  rows == 0: SSC_OK with no launch.
 * ---------------------------------------------------------------------------------------------- */
int ssc_mirostat_rows(float* logits, int ld, int rows, int V, float temperature, const float* mu_in, const int64_t* last_pred,
                      int end_index, int* kept, float* norm, void* stream);
int ssc_mirostat_update(const float* logits, int ld, int rows, int V, float temperature, float tau, float eta, const float* norm,
                        const int64_t* pred, const int64_t* last_pred, int end_index, const float* mu_in, float* mu_out,
                        float* surprise, void* stream);
/* Mirostat in the sampled decode: the descriptor travels BESIDE ssc_sample_opts (see there). */
typedef struct {
  float tau;         /* the surprise target in nats; 0: off (no other field is read) */
  float eta;         /* the learning rate of mu, >= 0; 0: a fixed surprise cut at mu0 */
  float mu0;         /* every row's mu at the first step (the paper: 2 tau) */
  float* mu;         /* (max_steps + 1, B), required: the call fills slab 0 with mu0, step t cuts with slab t and writes slab t + 1 */
  float* surprise;   /* (max_steps, B) or NULL: step t writes slab t with ssc_mirostat_update's surprise */
  int* kept;         /* (max_steps, B) or NULL: step t writes slab t with ssc_mirostat_rows' kept */
} ssc_mirostat;
/* ssc_decode_sample_opts_workspace_bytes / ssc_decode_sample_opts with one argument more.  With m NULL or m->tau == 0 they ARE those
 * calls: the same launches, the same bits, the same workspace size.  Otherwise, per step and for a live row, in this order: the
 * decode steps, the contrast, the logit rules, the truncation, the Mirostat cut (ssc_mirostat_rows with slab t of mu), the draw,
 * the Mirostat update (ssc_mirostat_update, slab t -> slab t + 1); last_pred is the previous step's words, the temperature is
 * s->temperature.  Slabs of steps never queued (early_stop) are not written.  The workspace grows by the cut's `norm` alone: 2 B
 * floats rounded up to 256 bytes, appended behind everything else - no existing offset moves.  Under d->start (a prompt) the control
 * starts at mu0 at the continuation's first step.  skip_dead, early_stop, the pacer, ctl, the attention trace, the guide, the rules,
 * the truncation and the contrast (amateur included) are untouched; d->log_probs sums the log-probs under the edited rows.
 * SSC_EINVAL before any launch: what ssc_decode_sample_opts refuses; tau < 0, NaN or infinite; with tau > 0: eta < 0 or not finite,
 * mu0 not finite, a NULL mu.  SSC_EALIGN: mu, surprise or kept no multiple of 4. */
size_t ssc_decode_sample_mirostat_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_sample_opts* opts,
                                                  const ssc_mirostat* m);
int ssc_decode_sample_mirostat(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                               const ssc_sample_opts* opts, const ssc_mirostat* m, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Arithmetic sampling for the word samplers (Vilnis et al., ICML 2023, "Arithmetic Sampling: Parallel Diverse Decoding for Large
 * Language Models"): every caption decodes along a CODE POINT in [0, 1) by inverse CDF in vocabulary order, the code renormalised
 * into the chosen word's interval after every step.  Each caption is on its own an exact draw from the sampler's distribution; the
 * N codes of an image form a randomly shifted lattice, so the set is stratified - fewer repeated captions, lower-variance estimates
 * over the N samples - while the rows stay independent of each other.  It replaces only the DRAW of the sampled decode: every edit
 * in front of it (guide, contrast, logit rules, truncation, the Mirostat cut) works as before; ssc_sampler_desc is read as the
 * samplers read it, except the seed, which only ssc_arith_codes uses; ssc_version() stays 4.  Like Mirostat it carries one value
 * per row from step to step.  A code is a uint64 c, meaning c / 2^64.  The arithmetic that decides a word is exact integer
 * arithmetic, so device and a host restatement (tests/arithref.py) agree bit for bit.
 * For a live row x[0 .. V), as it arrives behind all edits, with the sampler s (kind, top_k, top_p, temperature T):
 *   1. mx, the untempered log-sum-exp lse and the top-k / top-p cut are formed exactly as ssc_sample_rows forms them: the kept set
 *      is the set ssc_sample_rows keeps.
 *   2. The MASS of a kept entry is w_v = llrintf(expf((x_v - mx) / T) * 2^40) in fp32, that of a cut or -inf entry 0; the top entry
 *      has w = 2^40 exactly.  W = sum_v w_v in 64-bit integers, which does not depend on the summation order.  An entry whose mass
 *      rounds to 0 - a probability below 2^-41 of the top word's - CANNOT BE DRAWN.
 *   3. With (t, lo) the high and low 64 bits of the 128-bit product c * W, the token is the unique v, in vocabulary order, with
 *      cum(v) <= t < cum(v) + w_v, cum(v) = sum_{u < v} w_u.
 *   4. The new code is c' = floor(((t - cum(v)) * 2^64 + lo) / w_v), below 2^64 because t - cum(v) < w_v.
 *   5. The returned log-prob is the untempered x_v - lse, as for ssc_sample_rows; row_lp (or NULL) accumulates it.
 * Rows that pass through, with c' = c: a row whose last token is END (last_pred[r] == end_index) emits end_index at log-prob 0 and
 * its logits are not read; a row with W == 0 (no finite entry) yields what ssc_sample_rows yields for it - the lowest-index kept
 * entry, log-prob x_v - lse.  mass_out ((rows, V) int64, or NULL; for tests and diagnostics, like probs_out) receives the w_v - for
 * an ended row 2^40 at end_index and 0 elsewhere.  code_out may be code_in.  NaN and +inf are the caller's error (the call still
 * ends and stays inside its rows): a mass that is no positive number counts as 0, every trip count depends on V alone, every index
 * is a loop index; if no lane claims t, the lowest-index maximum is emitted and the code passes through.  One workgroup per row,
 * the row staged in LDS for V <= 32768 and walked in global memory above; the walk of step 3 is a 64-bit prefix scan in tiles in
 * vocabulary order, the division of step 4 a shift-subtract loop of one thread.  No float atomics, no order-dependent float
 * reduction decides anything: two calls on equal inputs are bit-identical.
 * The codes of a call (ssc_arith_codes): for image i with N = n_samples, row i N + j starts at c = u_i + floor(j 2^64 / N) (mod 2^64);
 * u_i = word 0 + 2^32 * word 1 of Philox4x32-10 with key = seed and counter (0, 0, i, 0x41524954).  The last counter word ("ARIT")
 * is used by no other stream of the library: the word draws and the stochastic beam use 0, the scheduled-sampling coin 1, the
 * sampled-node beam its draw index 0 .. 31.
 * SSC_EINVAL before any launch: a NULL logits, code_in, pred_out, lp_out or code_out; rows < 0, V < 1, ld < V; a sampler the word
 * samplers refuse; end_index outside [0, V) with a last_pred; for ssc_arith_codes a NULL code_out, nimg < 0, n_samples outside
 * [1, 2^24] or more than 2^31 rows.  SSC_EALIGN: a code (or mass) block that is no multiple of 8.  rows == 0 (nimg == 0): SSC_OK
 * with no launch.
 * ---------------------------------------------------------------------------------------------- */
int ssc_arith_codes(uint64_t seed, int nimg, int n_samples, uint64_t* code_out, void* stream);
int ssc_arith_rows(const float* logits, int ld, int rows, int V, const ssc_sampler_desc* s, const uint64_t* code_in,
                   const int64_t* last_pred, float* row_lp, int end_index, int64_t* pred_out, float* lp_out, uint64_t* code_out,
                   int64_t* mass_out, void* stream);
/* Arithmetic sampling in the sampled decode: the descriptor travels BESIDE ssc_sample_opts, as ssc_mirostat does. */
typedef struct {
  int mode;         /* 0: off (no other field is read); 1: the call fills slab 0 with ssc_arith_codes(s->seed, nimg, n_samples);
                       2: the caller has filled slab 0 */
  uint64_t* code;   /* (max_steps + 1, B), required when on: step t draws with slab t and writes slab t + 1 */
} ssc_arith;
/* ssc_decode_sample_mirostat_workspace_bytes / ssc_decode_sample_mirostat with one argument more.  With a NULL or a->mode == 0 they
 * ARE those calls: the same launches, the same bits, the same workspace size.  Otherwise the draw launch of every step is
 * ssc_arith_rows' kernel - last_pred the previous step's words, row_lp the running caption log-probs -, carrying the early-stop
 * protocol of the sampler's own draw kernel.  Everything else is untouched: skip_dead, early_stop, ctl / host_flag, the pacer, the
 * attention trace, the guide, the contrast with its amateur, the rules, the truncation, the Mirostat cut and update, d->start.
 * Under d->start (a prompt) the codes start at the continuation's first step.  Slabs of steps never queued (early_stop) are not
 * written.  The workspace does not grow.  SSC_EINVAL before any launch: what ssc_decode_sample_mirostat refuses; a mode outside
 * 0 .. 2; with mode 1 or 2 a NULL code.  SSC_EALIGN: code no multiple of 8. */
size_t ssc_decode_sample_arith_workspace_bytes(const ssc_model_cfg* cfg, const ssc_search_desc* d, const ssc_sample_opts* opts,
                                               const ssc_mirostat* m, const ssc_arith* a);
int ssc_decode_sample_arith(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_search_desc* d, const ssc_sampler_desc* s,
                            const ssc_sample_opts* opts, const ssc_mirostat* m, const ssc_arith* a, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prompted decoding: start the one-call decodes from a forced prefix ("a happy ...").  ssc_decode_prime teacher-forces the prefix
 * on the B = nimg * n_samples rows of a call - the loop of ssc_decode_score, leaving STATES instead of only scores -, its outputs
 * are an ssc_start_state for any search or sampled decode over the same B entries, and ssc_prefix_join puts prefix and
 * continuation together.  The prefix costs max_len steps of B rows, before a search enlarges to B * S * beam rows.
 * ---------------------------------------------------------------------------------------------- */
/* Row b = (image, sample).  len_b = the number of leading ids of prefix[b, :] that lie in [0, V) and are not end_index: the first
 * other id (-1 padding, an id >= V, end_index) ends the prefix and is never used as an index.  Step t < max_len feeds the rows with
 * len_b > t end_index (t = 0: from zero states) or prefix[b, t-1] and scores them against prefix[b, t] (ssc_score_rows):
 * log_probs[b] += log p(prefix[b, t]), token_lp[b, t] likewise.  After step t every row with len_b == t + 1 is CAPTURED: the
 * step's four output states go to h1 / c1 / hd / cd and tokens[b] = prefix[b, t].  A row with len_b == 0 gets zero states,
 * tokens[b] = end_index, log_probs 0: the start of an unprefixed call.  Rows with len_b <= t are not stepped from step 1 on
 * (ssc_decode_step_desc.row_lp); nothing of theirs is read afterwards.  token_lp is 0 from column len_b on.  max_len steps, known
 * on the host.  Every SENTIMENT_VAE, every numerics mode.  SSC_EINVAL before any launch: a NULL required pointer, an extent < 1,
 * B > 2^24, end_index outside [0, V), what the configuration's prior needs (sentiment / obj_atts) missing. */
typedef struct {
  int nimg, R, n_samples, max_len, end_index;
  const float* feats;            /* (nimg, R, F) */
  const void* imgbuf;            /* from ssc_decode_prepare */
  const float* sentiment;        /* (B) or NULL */
  const float* obj_atts;         /* cfg->kld_mode 2: (nimg, R, Z); else NULL */
  const int64_t* prefix;         /* (B, max_len) int64 */
  const float* eps;              /* (max_len, B, Z): noise of step t at eps + t * B * Z */
  float* h1; float* c1; float* hd; float* cd;   /* out (B, H) each */
  int64_t* tokens;               /* out (B) */
  int* lengths;                  /* out (B) int32: len_b */
  float* log_probs;              /* out (B): the prefix's summed log-prob */
  float* token_lp;               /* out (B, max_len), optional */
} ssc_prime_desc;
size_t ssc_decode_prime_workspace_bytes(const ssc_model_cfg* cfg, const ssc_prime_desc* d);
int ssc_decode_prime(const ssc_model_cfg* cfg, const ssc_params* p, const ssc_prime_desc* d, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Prefix + continuation.  prefix (B, Lp) and lengths (B) as ssc_decode_prime took and left them, predictions (B, Q, steps) and
 * log_probs (B, Q) a search's (Q = S * beam; 1 for the sampled decode), ctl the search's or NULL: columns >= ctl[0] are read as
 * end_index.  captions (B, Q, Lp + steps): caption q of entry b is prefix[b, :len_b], then the search's words, then end_index to the
 * end.  total (B, Q) = prefix_lp[b] + log_probs[b, q]; a log_probs value <= -1e19 (a beam that does not exist) stays as it is.
 * One small kernel, no atomics, the same bits on every run.  SSC_EINVAL and no launch: a NULL pointer other than ctl, B, Q, Lp or
 * steps < 1, B * Q > 2^24, end_index < 0. */
int ssc_prefix_join(const int64_t* prefix, const int* lengths, int Lp, const int64_t* predictions, const int* ctl, int steps,
                    const float* log_probs, const float* prefix_lp, int B, int Q, int end_index, int64_t* captions, float* total,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diverse-caption evaluation (eval/eval.py:95-472 with the coco-caption scorers it calls): BLEU-1..4 (BleuScorer, option
 * "closest"), ROUGE-L (Rouge, beta 1.2) and CIDEr-D (CiderScorer, sigma 6) of every candidate; distinct 1- / 2-grams of every
 * image's N captions and of its top 5 by CIDEr (Div-n), and style-word counts.  The reductions over candidates (oracle argmax,
 * corpus BLEU, means) are the caller's.  Exact: n-grams are compared by their full word tuples; fp64 scores, integer counts;
 * integer atomics only; two calls on the same inputs are bit-identical, and equal captions of one image score bit-equal.
 * Reference words are compact ids 1..W, W <= 65535; a reference holds 1..64 tokens.  Both calls read a device error flag back,
 * so they synchronise `stream` (not capturable): every out-of-range id, length or offset gives SSC_EINVAL, nothing is indexed
 * with it.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int I;                     /* images: the evaluated set (CIDEr-D's document frequencies and log I run over it) */
  int nref;                  /* reference captions, >= I */
  int ntok;                  /* tokens over all references */
  int W;                     /* compact word ids 1..W */
  const int* ref_offsets;    /* (I + 1): the references of image i are ref_offsets[i] .. ref_offsets[i + 1] - 1 (at least one) */
  const int* tok_offsets;    /* (nref + 1): the tokens of reference r are tokens[tok_offsets[r] .. tok_offsets[r + 1]) */
  const int* tokens;         /* (ntok): compact ids 1..W */
  const uint8_t* style;      /* optional (W + 1): 1 = a style word */
  void* state;               /* ssc_eval_refs_bytes(I, nref, ntok) bytes, written by ssc_eval_prepare_refs and read by ssc_eval_score */
  size_t state_bytes;
} ssc_eval_refs;

typedef struct {
  const int64_t* predictions; /* (P, N, steps): a row is cut at its first boundary_index, else kept whole; at most 64 tokens */
  int P, N, steps;            /* 1 <= N <= 128 */
  int boundary_index;
  int V;                      /* prediction ids 0..V-1, V <= 65535 */
  const int* id_map;          /* (V): compact id of prediction id v, 0 = in no reference (the vocabulary's UNK maps to 0) */
  const uint8_t* style_ids;   /* optional (V): 1 = a style word (the same words as ssc_eval_refs.style) */
  const int* ref_image;       /* (P): the prepared image of prediction image p, or -1: Div-n counts only */
  double* scores;             /* (P, N, 6): B1, B2, B3, B4, ROUGE-L, CIDEr-D (0 where ref_image is -1) */
  int* counts;                /* (P, N, 10): testlen, reflen, guess[4], correct[4] (BleuScorer's statistics) */
  int* image_counts;          /* (P, 9): distinct 1-grams, distinct 2-grams, words of the N captions; the same of the top 5;
                               * candidate style words, those of them the references hold, reference style words */
  int* top5;                  /* (P, 5): sample indices by CIDEr-D, stable descending; -1 where N < 5 or ref_image is -1 */
} ssc_eval_score_desc;

size_t ssc_eval_refs_bytes(int I, int nref, int ntok);   /* 0 for arguments out of range */
/* n-grams, tf, document frequencies, weights and norms of the references (three kernels). */
int ssc_eval_prepare_refs(const ssc_eval_refs* r, void* stream);
size_t ssc_eval_score_workspace_bytes(const ssc_eval_refs* r, const ssc_eval_score_desc* d);
/* every candidate's scores and statistics, then every image's counts (two kernels) */
int ssc_eval_score(const ssc_eval_refs* r, const ssc_eval_score_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Caption-SET diversity: the N captions of an image compared with each other (Wang & Chan, "Describing like humans", CVPR 2019;
 * the numbers Seq-CVAE / COS-CVAE / POS / AG-CVAE report).  Per image p and sample i:
 *   set_counts  BleuScorer's ten integers (testlen, reflen "closest", guess[4], correct[4]) of caption i against the other N - 1
 *               captions of p as its references (by index: a duplicate at another index is a reference).  mBLEU-k is the caller's
 *               reduction: corpus BLEU-k of the statistics summed over the images at sample index i, averaged over i.
 *   kernel      K_ij = 1/4 sum_{n=1..4} cos(g_i^n, g_j^n), g_i^n = the caption's n-grams weighted tf (log I - log max(1, df)) with
 *               the prepared references' df and I (no CIDEr-D clipping, no length Gaussian); a cosine with a zero vector is 0,
 *               on the diagonal too.  Symmetric bit for bit, positive semi-definite up to rounding, entries in [0, 1].
 *   eigenvalues of K, descending (cyclic Jacobi in fp64).  Self-CIDEr = -log(sqrt(l_1) / sum_i sqrt(l_i)) / log N is the caller's.
 *   distinct    the number of distinct captions (token tuples) among the N; every empty caption is the same caption.
 * A caption's n-grams are compared on its original ids 0..V-1 (id 0 is a word like any other); df is looked up through id_map
 * as ssc_eval_score does.  Exact and deterministic as the calls above: integer counts, fp64, no float atomics, one summation
 * order per pair whatever its position (equal captions give bit-equal rows), two calls bit-identical.  Reads a device flag
 * back (synchronises `stream`): out-of-range ids, rows of more than 64 tokens or ref_image values give SSC_EINVAL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const int64_t* predictions; /* (P, N, steps): as ssc_eval_score_desc */
  int P, N, steps;            /* 2 <= N <= 128 */
  int boundary_index;
  int V;                      /* prediction ids 0..V-1, V <= 65535 */
  const int* id_map;          /* (V): as ssc_eval_score_desc; may be NULL when refs is NULL */
  const int* ref_image;       /* (P): the prepared image of prediction image p, or -1: no kernel / eigenvalues for it */
  int* set_counts;            /* (P, N, 10) */
  double* kernel;             /* optional (P, N, N): 0 where ref_image is -1 */
  double* eigenvalues;        /* (P, N) descending; 0 where ref_image is -1 */
  int* distinct;              /* (P) */
} ssc_eval_set_desc;

/* refs may be NULL when every ref_image is -1 (set_counts and distinct only). */
size_t ssc_eval_set_workspace_bytes(const ssc_eval_refs* refs, const ssc_eval_set_desc* d);   /* 0 for arguments out of range */
/* every caption's sorted n-grams and weights, every ordered pair of an image's captions, every image's eigenvalues (three kernels) */
int ssc_eval_set(const ssc_eval_refs* refs, const ssc_eval_set_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Consensus re-ranking (Devlin et al. 2015, Mao et al. 2015; the "best-1 after consensus re-ranking" numbers of AG-CVAE /
 * Seq-CVAE / COS-CVAE): for every query image the k nearest images of a bank of training images by cosine similarity of the
 * pooled features (ssc_feat_prep's avg), then every candidate caption's mean CIDEr-D against the pooled references of those
 * images, with the bank's document frequencies.  The similarities are an NT product of unit rows: ssc_gemm (a_kc = b_kc = 1) on a
 * chunk of the bank at a time, followed by ssc_knn_merge on the same stream.
 * ---------------------------------------------------------------------------------------------- */
/* out row r = x row r / |x row r| (rows x F, leading dimensions ld / ldo >= F); a zero row stays zero.  One pass, fixed reduction
 * order.  out may be x. */
int ssc_l2_normalize_rows(const float* x, int rows, int F, int ld, float* out, int ldo, void* stream);

/* Merges the (Q x Mc) chunk `sims` (ld >= Mc; column c is bank row bank_offset + c) into the running top-k lists best_sim /
 * best_idx (Q, k), which the caller initialises to -inf / -1 and which stay sorted: similarity descending, equal similarities by
 * bank index ascending; unused slots (-inf, -1) last.  exclude (optional, (Q)): a bank row the query skips, or -1.  k <= 128,
 * Mc <= 2^22.  Exact selection (radix select on order-preserving keys, integer histograms): the lists after the last chunk are the
 * k largest of the whole bank under that order whatever the chunking, bit for bit.  -0 counts as +0; a NaN as -inf. */
int ssc_knn_merge(const float* sims, int ld, int Q, int Mc, int bank_offset, int k, const int* exclude, float* best_sim,
                  int* best_idx, void* stream);

typedef struct {
  const int64_t* predictions; /* (P, N, steps): as ssc_eval_score_desc */
  int P, N, steps;            /* 1 <= N <= 128 */
  int boundary_index;
  int V;                      /* prediction ids 0..V-1, V <= 65535 */
  const int* id_map;          /* (V): as ssc_eval_score_desc */
  const int* neighbours;      /* (P, k): prepared images of refs whose references form query p's pool, in this order; -1 = unused
                               * slot; every query needs at least one valid entry (an image listed twice counts twice) */
  int k;                      /* 1 <= k <= 128 */
  double* scores;             /* (P, N): 10 / |R(p)| sum_{r in R(p)} sim(c, r), CiderScorer's per-reference similarity (CIDEr-D of
                               * the candidate with the pool as its reference list and refs' document frequencies and log I) */
  int* pool_refs;             /* (P): |R(p)| */
  int* pick;                  /* (P): the sample of highest score, the lowest index on a tie */
  int* order;                 /* (P, N): the samples by score, stable descending */
} ssc_eval_consensus_desc;

/* 0 for arguments out of range */
size_t ssc_eval_consensus_workspace_bytes(const ssc_eval_refs* refs, const ssc_eval_consensus_desc* d);
/* Every candidate's n-grams and weights once, then the references of the listed images in list order (one wave per candidate, fp64,
 * one accumulation order: equal captions of a query score bit-equal, two calls are bit-identical); then every query's order (two
 * kernels).  Reads a device flag back (synchronises `stream`): out-of-range ids, rows of more than 64 tokens, neighbour indices
 * outside -1..I-1 and queries without a valid neighbour give SSC_EINVAL; nothing is indexed with them. */
int ssc_eval_consensus(const ssc_eval_refs* refs, const ssc_eval_consensus_desc* d, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Diverse subset selection: from the N candidate captions of every image the k that are good AND different from each other,
 * chosen from a similarity kernel K (ssc_eval_set_desc.kernel) and a per-candidate quality q (consensus scores, caption
 * log-probs) with no test reference.  Everything is fp64; every argmax resolves ties to the lowest candidate index; every sum
 * runs over j (or over the components of a vector) ascending.  K is read as a symmetric matrix: K_ij is taken from row j.
 * q^ is the quality the rules use: q itself (normalize 0) or (q - min) / (max - min) over the image's eligible candidates
 * (normalize 1; all equal: 0); with quality NULL q^ = 0.  n_e = the image's eligible candidates.
 *   MBR (1)   s_i = (sum_{j != i, eligible} K_ij) / (n_e - 1), 0 with n_e = 1: the candidate closest to all others (minimum Bayes
 *             risk under the kernel).  picks = the k eligible candidates of highest s_i, stable descending; gains = s_i.
 *   MMR (2)   maximal marginal relevance: the first pick is argmax q^_i (gain lambda q^_i), each later one
 *             argmax_{i not in S} lambda q^_i - (1 - lambda) max_{j in S} K_ij; gains = that objective.
 *   DPP (3)   greedy MAP inference of the determinantal point process L_ij = r_i K_ij r_j, r_i = exp(theta q^_i) (Chen, Zhang &
 *             Zhou, NeurIPS 2018).  d_i^2 = L_ii and an empty vector c_i per candidate; at each step j = argmax_{i not in S}
 *             d_i^2; the rule stops when d_j^2 < min_gain or d_j^2 is not greater than 0; otherwise j is picked and for every
 *             i not in S: e_i = (L_ji - <c_j, c_i>) / d_j, c_i gets e_i appended, d_i^2 -= e_i^2.  gains = d_j^2 at the pick
 *             (= det L_{S + j} / det L_S): a duplicate of a picked caption (K_ij = K_jj, equal q) is left with gain 0 up to
 *             rounding and a candidate with a zero diagonal is never picked by the rule.
 *   fallback  the slots a rule left open (DPP after its stop) are filled with the remaining eligible candidates by q^, stable
 *             descending (quality NULL: by index); their gain is reported as 0.  Slots beyond n_e hold -1 (gain 0).
 * n_primary = the picks the rule itself made (MBR, MMR: min(k, n_e)).
 * One wave per image; each lane owns candidates lane and lane + 64; (value, index) butterflies for the argmax; the DPP vectors
 * lie component-major (k x N per image) in LDS for k <= 16 and in the workspace beyond, each lane touching only its own two
 * columns.  No atomics: two calls on the same inputs are bit-identical, images with bit-equal inputs get bit-equal outputs.
 * SSC_EINVAL before any launch: a NULL descriptor, P < 1, P * N > 2^24, N outside 1..128, k outside 1..N, a method outside
 * 1..3, normalize outside {0, 1}, NULL picks, gains, n_primary or kernel, a NULL quality for MMR or for DPP with theta != 0,
 * lambda outside [0, 1] or NaN, theta < 0 or not finite, min_gain < 0 or NaN (the three are checked whatever the method), a
 * NULL workspace or one smaller than ssc_eval_select_workspace_bytes.  The call reads one device flag back (synchronises
 * `stream`): a non-finite quality of an eligible candidate, a non-finite K_ij of two eligible candidates or a quality range
 * max - min that overflows give SSC_EINVAL; that image's picks are all -1 (gains 0, n_primary 0), the other images' are valid.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int P, N, k;               /* 1 <= k <= N <= 128 */
  int method;                /* 1 MBR | 2 MMR | 3 greedy DPP */
  const double* kernel;      /* (P, N, N) similarity, as ssc_eval_set_desc.kernel leaves it (symmetric, entries in [0,1]) */
  const double* quality;     /* (P, N) finite; may be NULL for MBR and for DPP with theta == 0 */
  int normalize;             /* 1: per image q^ = (q - min) / (max - min), all equal -> 0; 0: q^ = q */
  double lambda;             /* MMR trade-off in [0, 1] */
  double theta;              /* DPP quality weight >= 0 */
  double min_gain;           /* DPP: stop the primary rule when the best remaining gain is < min_gain (>= 0) */
  const uint8_t* eligible;   /* optional (P, N): 0 = never pick this candidate (an empty caption, a filtered one) */
  int* picks;                /* (P, k) candidate indices in pick order; -1 when fewer than k are eligible */
  double* gains;             /* (P, k) the rule's value of each pick at the time it was picked (0 for fallback picks and -1 slots) */
  int* n_primary;            /* (P) how many picks the rule itself made before the fallback filled up */
} ssc_eval_select_desc;
size_t ssc_eval_select_workspace_bytes(const ssc_eval_select_desc* d);   /* 0 for arguments out of range */
int ssc_eval_select(const ssc_eval_select_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-critical sequence training (Rennie et al. 2017; Luo 2020): the step between the sampled decode (ssc_decode_sample), the
 * per-caption reward (ssc_eval_score) and the train step (ssc_train_fwd / ssc_train_bwd).  P images x N samples, G = P * N rows,
 * row g = p * N + i.  The sampled captions become the train step's `caps`; row g's reward is r_g = sum_k reward_weights[k] *
 * scores[g][k] and its upstream gradients are gl_g = loss_scale * (r_g - b_g), gk_g = kld_scale.  Baseline b_g: 0 (baseline 0),
 * the mean reward of the image's other N - 1 samples, (S_p - r_g) / (N - 1) with S_p summed in sample order (1), or the reward of
 * the image's row of base_scores (2).  All of it in fp64, in column / sample order, rounded to fp32 once per output.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int P, N;                   /* 1 <= N <= 128 (as ssc_eval_score) */
  int steps, L;               /* columns of predictions and of caps: L >= steps >= 1 */
  int end_index;
  const int64_t* predictions; /* (G, steps): as ssc_decode_sample leaves them */
  const double* scores;       /* (P, N, 6): ssc_eval_score_desc.scores */
  const double* base_scores;  /* (P, 6): the scores of one baseline caption per image; NULL unless baseline is 2 */
  double reward_weights[6];   /* B1, B2, B3, B4, ROUGE-L, CIDEr-D */
  int baseline;               /* 0 none, 1 leave-one-out (N >= 2), 2 given per image */
  double loss_scale;          /* 1 / G for the mean over the rows */
  double kld_scale;           /* 1 / (G * KLD_WEIGHT) */
  int64_t* caps;              /* (G, L): the row's tokens before its first end_index (all `steps` tokens where it has none), then
                               * 0.  Ids are copied as they are: an id 0 inside a caption is a 0 of the train step's caps */
  int* lengths;               /* (G): the number of tokens kept */
  float* reward;              /* (G): r */
  float* advantage;           /* (G): r - b */
  float* gl;                  /* (G) */
  float* gk;                  /* (G) */
  double* stats;              /* (4): mean r, mean b, mean |r - b|, share of rows with no end_index */
} ssc_scst_desc;

/* A pack kernel (one wave per row) and an advantage kernel (one workgroup per image, one more for the statistics).  Stream-ordered,
 * no read-back (capturable), no atomics: two calls are bit-identical, and two samples of an image with bit-equal scores get
 * bit-equal outputs (N = 2, leave-one-out: advantage exactly 0).  SSC_EINVAL and nothing written: a NULL pointer, N outside
 * 1..128, L < steps, baseline 1 with N = 1, baseline 2 without base_scores. */
int ssc_scst_prepare(const ssc_scst_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reading an attention trace (ssc_attn_record): per selected caption and step the attention map of the word and its summary.
 * A call of its own because the caller picks the captions it returns after the search (the best beam, a diverse group's arg-max):
 * only those are gathered.  Row i of the outputs is caption q = sel[i] (sel NULL: q = i and n_sel must equal n_caps).  With
 * a = anc[q, t]:
 *   maps[i, t, 0:R]   a bit-for-bit copy of hist[t, a, :]; exact zeros - hist is NOT read - where a is outside [0, rows) (the -1 of
 *                     ssc_attn_record) or q is outside [0, n_caps).  Columns [R, ld_maps) are left untouched.
 *   top_region[i, t]  the arg-max of that row, ties to the lowest index; -1 on a zero row
 *   top_weight[i, t]  the weight at the arg-max; 0 on a zero row
 *   entropy[i, t]     -sum alpha ln alpha over alpha > 0, in nats; 0 on a zero row
 * One wave per (caption, step) row, four rows per workgroup, lanes over R (16-byte accesses where R, ld_maps and the pointers allow);
 * the arg-max and the entropy sum are wave butterflies in a fixed order: no atomics, the same bits on every call.  Stream-ordered.
 * SSC_EINVAL before any launch: NULL d, hist or anc; every output NULL; ld_maps < R with maps set; a non-positive rows, R, steps,
 * n_caps or n_sel; sel NULL with n_sel != n_caps.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* hist; int rows, R, steps;
  const int* anc; int n_caps;
  const int64_t* sel; int n_sel;      /* optional caption list; NULL: all, n_sel = n_caps */
  float* maps; int ld_maps;           /* optional out (n_sel, steps, ld_maps >= R) */
  int* top_region; float* top_weight; float* entropy;   /* optional out (n_sel, steps) */
} ssc_attn_gather_desc;
int ssc_attn_gather(const ssc_attn_gather_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSC_H */
