/*
 * ssc_debug.h - diagnostics, profiling and tuning switches of libssc_hip.so.  NOT part of the product ABI (ssc.h):
 * nothing here is needed to run the hot path, and everything here is process-global and not thread-safe.
 * Used by bench.py (roofline leg), tools/ and the kernel-form tests.
 */
#ifndef SSC_DEBUG_H
#define SSC_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* In-situ GEMM profiling: while enabled every GEMM launch is bracketed by a hipEvent pair on its stream.
 * ssc_prof_collect synchronises the device and writes up to max_records x 8 floats
 * {kind (0 NT, 1 NN, 3 TN), M, N, sum K, splits, milliseconds, algorithmic bytes, flops}; returns the record count.  A grouped
 * launch is ONE record: its bytes (every operand and result of every member once) and flops (2 M N K per member) are exact,
 * its N / K are nominal (widest member, summed K). */
int ssc_prof_enable(int on);
int ssc_prof_collect(float* out, int max_records);

/* Time-loop timing of ssc_train_fwd / ssc_train_bwd: while enabled a hipEvent pair brackets the T-step loop itself
 * (precompute, hoisted products, vocabulary head and the weight-gradient products are outside).  ssc_prof_loop_ms
 * synchronises the events of the LAST forward / backward call and returns the loop times in milliseconds
 * (negative when that call has not run since the switch was turned on). */
int ssc_prof_loop_enable(int on);
int ssc_prof_loop_ms(float* fwd_loop_ms, float* bwd_loop_ms);

/* Named switches between kernel forms that compute the same product (A/B measurements, kernel-form tests).
 * Keys (default; environment variable read once at load):
 *   "large_form"  large products: 0 64-wide kernels | 1 by grid size: wave-specialised from 768 workgroups on (default) |
 *                 2 wave-specialised 128x128 | 3 4-wave 128x128 3xBF16 kernel                       (SSC_X3B)
 *   "x3w_skinny"  minibatch products on the wave-specialised 64x256 kernel: 0 | 1 NT+NN (default) | 2 NN only (SSC_X3W_SKINNY)
 *   "gemm_f16"    op-level products outside a sequence-level call: the wave-specialised 128x128 NT form takes the 2xFP16
 *                 split (0)                                                                        (SSC_GEMM_F16)
 *   "f16_npw"     producer waves of the 2xFP16 kernel: 4 (default: two workgroups per CU) | 8     (SSC_F16_NPW)
 *   "store_wt"    write-through (sc1) output stores of the wave-specialised kernels (1)            (SSC_STORE_WT)
 *   "tile_gm"     tile rows per group of the XCD-aware tile order (8; 0 = row-major)               (SSC_TILE_GM)
 *   "stream_nt"   non-temporal loads and stores on data a train step touches once, a bit mask: 2 = the streams of ssc_sgd_step
 *                 and ssc_sq_norm (default) | 0 = default cache policy; bit-identical results         (SSC_STREAM_NT)
 *   "dw_one_flush"  ssc_train_bwd issues the weight gradients of all phases as one work list (1) | 0 one launch per phase,
 *                 as ssc_train_bwd_phases does                                                     (SSC_DW_ONE_FLUSH)
 *   decode (ssc_decode_step and the beam kernels; every form gives the same captions):
 *   "dec_att_table"  attended-feature term of the decoder gates from the per-image table (1)      (SSC_DEC_ATT_TABLE)
 *   "dec_dedup"      products fed only by the parent's states on the distinct parents (1)         (SSC_DEC_DEDUP)
 *   "dec_ungathered" ssc_decode_ungathered_ok() may say yes: states read through the parent lists (1)   (SSC_DEC_UNGATHERED)
 *   "img_mfma"       table contraction of ssc_lstm_fwd_img on the fp32 matrix cores (1 | 0 = VALU form)  (SSC_IMG_MFMA)
 *   "beam_reg"       beam selection with the vocabulary row in registers for V <= 10240 (1)       (SSC_BEAM_REG)
 *   "dec_planes"     2xFP16 products of a large call read states and weights pre-split into fp16 pieces (1)   (SSC_DEC_PLANES)
 *   "dec_parts"      vocabulary head of a one-state search leaves per-tile records instead of logits (1)      (SSC_DEC_PARTS)
 * The environment variables are honoured only with SSC_DEBUG=1.  Returns SSC_EINVAL for an unknown key. */
int ssc_debug_set(const char* key, int value);
int ssc_debug_get(const char* key, int* value);

/* Test hook of the attention trace (ssc_attn_record): where a one-call decode keeps, in the workspace it has just run in, the words
 * it chose and their ancestry - what the anc of its trace is derived from.  driver 0: the searches (ssc_decode_search and the
 * stochastic, sampled-node, diverse and rules searches), 1: ssc_decode_sample.  which 0: the chosen words, (max_steps, rows) int64
 * time-major; 1: the back-pointers, (max_steps - 1, rows) int64 (searches only).  cfg and desc are those of the call.  Returns a
 * pointer into `workspace`, or 0 for a bad argument. */
void* ssc_debug_decode_view(const void* cfg, const void* desc, void* workspace, int driver, int which);

#ifdef __cplusplus
}
#endif
#endif
