/*
 * uniir_hip.h -- C ABI of libuniir_hip.so, the MI355X (gfx950) hot path of the UniIR
 * contrastive-train / embed / brute-force-retrieve pipeline.
 *
 * Boundary contract: plain pointers and sizes only, no torch types.  Every
 * entry point is asynchronous on the caller's hipStream_t (passed as void*), never allocates device
 * memory, never synchronises the host (the two top-k helpers that return host-visible counts say so),
 * returns 0 (UNIIR_OK) or a negative UNIIR_E* code and never throws.  All pointers are DEVICE pointers
 * unless the parameter name ends in _host.  bf16 / fp16 tensors are passed as const void*.
 *
 * Each group names the reference code it replaces (paths relative to the UniIR tree):
 *   [ENC]   openai/CLIP VisionTransformer / Transformer forward+backward as called from
 *           src/models/uniir_clip/clip_scorefusion/clip_sf.py:43-47 (encode_text / encode_image)
 *   [FUSE]  clip_sf.py:53-63 (mask * emb fuse), :88-97 (row select + F.normalize)
 *   [NCE]   clip_sf.py:133-144 (similarity * exp(logit_scale), CrossEntropy, argmax accuracy)
 *   [OPT]   clip_scorefusion/train.py:52-61,195-199 (two-group AdamW) + uniir_clip/engine.py:41-46
 *   [TOPK]  src/common/mbeir_retriever.py:76,85-103 (normalize_L2 + IDMap,Flat IP index),
 *           :188-232 (search_index: normalize queries, exact top-k by inner product)
 */
#ifndef UNIIR_HIP_H
#define UNIIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNIIR_OK 0
#define UNIIR_EINVAL (-1)       /* null pointer / negative size / bad enum */
#define UNIIR_ESHAPE (-2)       /* shape not supported by the kernels (see each function) */
#define UNIIR_EALIGN (-3)       /* pointer or leading dimension not 16-byte aligned */
#define UNIIR_ELAUNCH (-4)      /* HIP launch failed */
#define UNIIR_EUNSUPPORTED (-5)

const char* uniir_strerror(int code);
/* ABI version; bumped on any signature or struct-layout change (3: uniir_clip_tower.recompute; 4: uniir_reduce_stats;
 * 5: uniir_image_*; 6: uniir_attention_fwd_long / _bwd_long; still 6, new entry points only: uniir_attention_rel_fwd_long /
 * _rel_bwd_long; uniir_attention_one_fwd / _one_bwd, and the value 2 of uniir_clip_tower.pool_last_block; uniir_layernorm_fwd_f16,
 * uniir_patchify_f16, uniir_vit_assemble_f16: no layout changes; 7: uniir_attn_rel_fwd_f16, uniir_attn_rel_fwd_long_f16 and
 * uniir_rmsnorm_fwd_f16 -- new entry points only, a caller that needs them asks for >= 7; still 7, a new entry point only:
 * uniir_attn_f32_rel_fwd, which a caller finds by its symbol; still 7, new entry points and a new struct of their own only:
 * uniir_grad_guard*, uniir_adamw_step_guarded and uniir_grad_ctl, found by their symbols). */
int uniir_abi_version(void);
/* Reproducible reductions (round 6).  Bias, LayerNorm-weight and token-embedding gradients are sums over every row of a batch taken by
 * many workgroups; added with fp32 atomics they depend on the arrival order, and two runs of one training step differ in their last
 * bits.  Register a caller-owned device buffer for a stream (256-byte aligned; 64 MiB covers ViT-L/14 at 1024 items; buf NULL removes
 * the entry) and every such reduction launched on that stream -- uniir_gemm's colsum / a_rowsum, uniir_layernorm_bwd*, uniir_colsum_bf16,
 * uniir_text_embed_bwd* and the tower entry points that use them -- stores per-workgroup partials there and adds them in a fixed
 * order (one extra small launch each): same inputs, same bits.  Kernels on one stream run one after the other, so one buffer per
 * stream is enough.  A reduction that needs more than the buffer holds keeps its atomics, and is counted (uniir_reduce_stats).  Also
 * covered since ABI 4: the relative-position-bias gradient of uniir_attention_rel_bwd and _rel_bwd_long (per-workgroup bucket partials).
 * Thread safety: the host-side table (64 entries, one per (device, stream); when it is full the entry used longest ago goes) and the
 * counters are guarded by one mutex, so uniir_reduce_scratch, uniir_reduce_stats and the lookups that launches make may run on any
 * threads at once.  NOT covered: the buffer itself -- two threads that launch reductions on the SAME stream share its scratch and
 * must order their launches themselves, and a buffer must stay alive until the entry is replaced or removed and the stream's work
 * that used it has finished. */
int uniir_reduce_scratch(void* buf, int64_t bytes, void* stream);
/* process-wide, since the last reset: fallbacks = reduction launches that took the arrival-order (atomic) form because the stream
 * had no scratch or too small a one; max_request = the largest scratch size any reduction asked for, in bytes.  Either pointer may be
 * NULL.  An explicit UNIIR_EPI_ATOMIC_F32 epilogue is the caller's request and is not counted.  A caller that grows a stream's buffer
 * to max_request whenever fallbacks moved has at most the first step of a new geometry in arrival order. */
int uniir_reduce_stats(int64_t* fallbacks, int64_t* max_request, int32_t reset);

/* ------------------------------------------------------------------------------------------------
 * [ENC] building block 1: 16-bit MFMA GEMM with fused epilogues.
 *   C[M,N] = alpha * op(A)[M,K] . op(B)[K,N]  (+ epilogue)
 * a_tmaj = 0: A stored [M][lda] (K contiguous);  1: A stored [K][lda] (M contiguous)
 * b_tmaj = 0: B stored [N][ldb] (K contiguous; torch Linear weight layout);  1: B stored [K][ldb]
 * v = alpha * (op(A) . op(B))[m][n] in fp32; every epilogue below starts from it.
 * Requirements: K-contiguous operands need K % 8 == 0, M/N-contiguous ones need that extent % 8 == 0,
 * N % 8 == 0, all base pointers and leading dimensions multiples of 8 elements (16 B).
 * ---------------------------------------------------------------------------------------------- */
enum {
    UNIIR_EPI_BF16 = 0,          /* C(bf16) = v + bias?                                          */
    UNIIR_EPI_BIAS_ACT = 1,      /* f = bf16(v + bias) -> C ; act(f) -> C2 (both bf16)           */
    UNIIR_EPI_RESID_F32 = 2,     /* C(f32) = v + bias? + resid(f32, ldc) ; C2(bf16 copy) optional */
    UNIIR_EPI_DACT = 3,          /* C(bf16) = (v + bias?) * act'(aux[m][n]) (aux bf16, ldaux); C2(bf16, ldaux) = act(aux) opt. */
    UNIIR_EPI_F32 = 4,           /* C(f32) = v + bias?  (beta = 0)                                */
    UNIIR_EPI_ATOMIC_F32 = 5,    /* C(f32) += v via atomics; enables split-K (wgrad accumulate); bias must be NULL
                                    (UNIIR_EUNSUPPORTED otherwise)                                  */
    UNIIR_EPI_ACT_ONLY = 6       /* C(bf16) = act(bf16(v + bias)): BIAS_ACT without the pre-activation output (forward-only
                                    passes: embedding extraction); same rounding as BIAS_ACT's second output */
};
enum { UNIIR_ACT_QUICKGELU = 0, UNIIR_ACT_GELU_ERF = 1, UNIIR_ACT_RELU = 2 };
enum { UNIIR_DT_BF16 = 0, UNIIR_DT_F16 = 1 };

typedef struct {
    const void* A;
    const void* B;
    void* C;
    void* C2;            /* optional second output */
    const float* bias;   /* [N] or NULL */
    const float* resid;  /* [M][ldc] f32 or NULL */
    const void* aux;     /* [M][ldaux] bf16 or NULL */
    int32_t M, N, K;
    int64_t lda, ldb, ldc, ldaux;
    int32_t a_tmaj, b_tmaj;
    int32_t epilogue, act, dtype;
    int32_t k_splits;    /* >= 1; > 1 only with UNIIR_EPI_ATOMIC_F32 */
    float alpha;
    void* splitk_ws;          /* optional scratch for split-K: when it holds k_splits*M*N floats the splits write */
    int64_t splitk_ws_bytes;  /* plain fp32 slabs that one reduce kernel adds into C (no atomics)               */
    float* colsum;            /* optional [N] fp32: += column sums of the result before rounding (bias gradient);
                                 EPI_RESID_F32 / EPI_DACT / EPI_F32 on the 256x256 kernel; EPI_DACT on the general
                                 kernel sums the rounded bf16 result in a separate pass (needs ldc % 8 == 0)     */
    const float* row_scale;   /* optional [M] fp32, EPI_RESID_F32 only: C = (v + bias) * row_scale[m] + resid -- DropPath /
                                 stochastic depth of a residual branch (BLIP ViT, backbone/vit.py:79-80) without a separate pass */
    float* a_rowsum;          /* optional [M] fp32, a_tmaj only: += sum over K of op(A)'s rows -- the bias gradient of a
                                 weight-gradient GEMM dW = dy^T x, taken from the dy fragments inside the 256x256 transposed
                                 kernel (bf16, b_tmaj) and by a separate pass over A otherwise; not scaled by alpha       */
} uniir_gemm_desc;

int uniir_gemm(const uniir_gemm_desc* d, void* stream);
/* k_splits for a weight gradient dW += dy^T x over `rows` rows whose output has `tiles` 256 x 256 tiles: the smallest count that
 * fills the 256 compute units to 90 % while every split keeps >= 16 K steps of 64 rows (host arithmetic, no device involved) */
int32_t uniir_gemm_wgrad_splits(int32_t rows, int32_t tiles);
/* measurement hook (bench.py): stride > 0 brackets every stride-th uniir_gemm call -- from any caller, the tower entry
 * points included -- with HIP events on its launch stream; 0 switches it off.  uniir_gemm_timing_read (after a stream
 * synchronise) returns the sums over the sampled launches: 2 M N K, elapsed ms, count.  Single measuring thread.
 * uniir_gemm_timing_on: the same, counting and sampling only the calls launched on `stream`.  An event pair measures a kernel's own
 * duration only while no other stream shares the device: with the towers on two streams the measurement follows one of them, the
 * uniir_gemm calls on other streams are bracketed as "device shared" windows, and the read functions leave out the samples that
 * intersect a window (uniir_gemm_timing_read_ex also returns their count in *shared; shared may be NULL).  Windows closer than two
 * mean sample durations (at most 3 ms) count as one; when fewer than 8 samples (or than all, if fewer were taken) would be left the
 * sums cover ALL samples and *fallback (may be NULL) is 1 -- a read after at least one sampled launch never returns zero launches.
 * uniir_gemm_timing_filter is that rule alone on caller-supplied times, no device involved: windows = nwin x (begin, end) ms,
 * samples = n x (begin, duration) ms on the same axis, merge_ms < 0 = the automatic gap; writes keep[n] (1 = counts) and returns the
 * number kept (negative UNIIR_E* on bad arguments). */
int uniir_gemm_timing(int32_t stride);
int uniir_gemm_timing_on(int32_t stride, void* stream);
int uniir_gemm_timing_read(double* flop, double* ms, int32_t* launches);
int uniir_gemm_timing_read_ex(double* flop, double* ms, int32_t* launches, int32_t* shared, int32_t* fallback);
int uniir_gemm_timing_filter(const float* windows, int32_t nwin, const float* samples, int32_t n, float merge_ms, uint8_t* keep,
                             int32_t* fallback);

/* ------------------------------------------------------------------------------------------------
 * [ENC] building block 2: LayerNorm over the last dim (fp32 statistics, CLIP eps 1e-5).
 * x is the fp32 residual stream [rows][x_stride]; y is bf16 [rows][width] (GEMM operand) and/or f32.
 * bwd: dx_f32 = (dres ? dres : 0) + LN'(dy); also writes a bf16 copy when dx_bf16 != NULL;
 * dgamma/dbeta are ACCUMULATED (+=) in fp32 (zero them once per optimizer step); dx_colsum (optional, [width]) +=
 * the column sums of dx_f32 as written (the bias gradient of the linear layer that produced x).
 * dy may be bf16 (dy_is_f32 = 0) or fp32.
 * Strides: x rows are x_stride floats apart; dx_f32 AND dres rows are dx_stride floats apart (dres is read at dres + row * dx_stride:
 * it is the gradient of the same residual stream dx_f32 belongs to; a dense dres needs dx_stride == width); y, dy and dx_bf16 are
 * dense [rows][width].  width % 4 == 0, width <= 2048, x_stride % 4 == 0, dx_stride % 4 == 0 (UNIIR_ESHAPE otherwise).
 * ---------------------------------------------------------------------------------------------- */
int uniir_layernorm_fwd(const float* x, int64_t x_stride, const float* gamma, const float* beta,
                        void* y_bf16, float* y_f32, int32_t rows, int32_t width, float eps, void* stream);
/* the forward with an fp16 16-bit output (the fp16 forward of an embedding tower, forward only): the same checks; y_f32 has the
 * bits of uniir_layernorm_fwd's y_f32, y_f16 is that value rounded to fp16.  Either output may be NULL, not both. */
int uniir_layernorm_fwd_f16(const float* x, int64_t x_stride, const float* gamma, const float* beta,
                            void* y_f16, float* y_f32, int32_t rows, int32_t width, float eps, void* stream);
int uniir_layernorm_bwd(const float* x, int64_t x_stride, const float* gamma, const void* dy,
                        int32_t dy_is_f32, const float* dres, float* dx_f32, int64_t dx_stride,
                        void* dx_bf16, float* dgamma, float* dbeta, float* dx_colsum, int32_t rows,
                        int32_t width, float eps, void* stream);
/* the same with a per-row factor (fp32 [rows]) for what leaves towards the next residual branch: dx_bf16 = bf16(branch_scale[r] *
 * dx) and dx_colsum += branch_scale[r] * dx; dx_f32 stays the unscaled residual-stream gradient (DropPath in backward) */
int uniir_layernorm_bwd_ex(const float* x, int64_t x_stride, const float* gamma, const void* dy,
                           int32_t dy_is_f32, const float* dres, float* dx_f32, int64_t dx_stride,
                           void* dx_bf16, float* dgamma, float* dbeta, float* dx_colsum, const float* branch_scale,
                           int32_t rows, int32_t width, float eps, void* stream);
/* A weight gradient (uniir_gemm of `d`) and an INDEPENDENT LayerNorm backward (the arguments of uniir_layernorm_bwd_ex) as one launch
 * of one workgroup per compute unit: `side_cus` of the 256 run the LayerNorm rows, the others the product as fp32 split-K slabs in
 * d->splitk_ws (added to C in K order afterwards).  The product is bound by the matrix pipes and the LayerNorm by HBM, so each runs
 * in the other's shadow.  Results: dx_f32 / dx_bf16 are bitwise those of uniir_layernorm_bwd_ex; dgamma / dbeta / dx_colsum and C are
 * fixed-order sums (the same bits in every run; C bitwise uniir_gemm's at the same split count).  The fused launch needs a bf16
 * product with both operands K-major and the accumulating epilogue on 256 x 256 tiles, bf16 dy, a width of 512 / 768 / 1024, a chunk
 * plan (uniir_gemm_wgrad_side_plan > 0) and a workspace that holds its slabs; whenever one of these fails the call IS uniir_gemm
 * followed by uniir_layernorm_bwd_ex, so callers never branch.  side_cus <= 0: always the two launches. */
int uniir_gemm_wgrad_ln_bwd(const uniir_gemm_desc* d, const float* x, int64_t x_stride, const float* gamma, const void* dy,
                            int32_t dy_is_f32, const float* dres, float* dx_f32, int64_t dx_stride, void* dx_bf16,
                            float* dgamma, float* dbeta, float* dx_colsum, const float* branch_scale, int32_t rows,
                            int32_t width, float eps, int32_t side_cus, void* stream);
/* the split count of that launch for a weight gradient over `rows` rows with `tiles` 256 x 256 output tiles when `side_cus` compute
 * units are given to the side rows: the smallest count with tiles * splits a multiple of 256 - side_cus and >= 16 K steps of 64 rows
 * in every split; 0 = no such count (host arithmetic) */
int32_t uniir_gemm_wgrad_side_plan(int32_t rows, int32_t tiles, int32_t side_cus);

/* ------------------------------------------------------------------------------------------------
 * [ENC] building block 3: fused multi-head attention, head_dim 64.
 * Sequence limits per entry point (anything beyond is UNIIR_ESHAPE):
 *   uniir_attention_fwd / _bwd with causal = 0 : seq <= 1024 (513 .. 1024: K / V or Q / dO streamed through LDS; the backward stays
 *                                                bitwise reproducible); the uniir_clip_tower vision towers use this form
 *   uniir_attention_fwd / _bwd with causal = 1 : seq <= 512
 *   _packed, _ex, _rows, _rel_fwd / _rel_bwd   : seq, tq, tk <= 512 (mask, key_len, dropout, packed rows, relative bias)
 *   uniir_attention_fwd_long / _bwd_long       : tq, tk <= 1024: the general form without the causal mask (Q separate from K | V,
 *                                                key_len, dropout, packed query rows), K / V or Q / dO streamed through LDS at
 *                                                every size; bitwise reproducible.  BLIP MED cross-attention over 577 image tokens
 *   uniir_attention_rel_fwd_long / _rel_bwd_long: seq <= 1024: the relative bias (and dropout) on packed qkv, streamed at every size;
 *                                                dqkv bitwise reproducible, drel too with scratch on the stream.  The CLIP_FF
 *                                                fusion stack over the 577 + 77 tokens of ViT-L/14@336px
 *   uniir_attention_one_fwd / _one_bwd         : ONE query row per item against tk <= 1024 dense keys (the pooled last block of a
 *                                                tower); the backward is one pass over K and V, bitwise reproducible
 *   uniir_onequery_fwd / _bwd                  : ONE query row per item against tk <= 1024 keys with key_len or packed keys and dropout
 *                                                at the coordinates of the full call (the class row of BLIP's last BERT layer)
 *   Still 512 at most: the causal mask, fully packed rows (_packed, _rows with kv_packed).
 *   On fp16 tensors (forward only): uniir_attention_fwd_f16 with the limits of uniir_attention_fwd / _fwd_packed (causal = 0 and
 *   dense rows: seq <= 1024, the BLIP ViT at 384 pixels; else 512), uniir_attention_one_fwd with f16 = 1, and the general form
 *   (_ex, _rows, _long without the causal mask and dropout) as uniir_attn_general_fwd_f16 with its one-query form
 *   uniir_onequery_fwd_f16: the BLIP MED BERT's eval-mode forward; the relative bias as uniir_attn_rel_fwd_f16 (seq <= 512) and
 *   uniir_attn_rel_fwd_long_f16 (seq <= 1024): the CLIP_FF fusion stack's eval-mode forward.  There is no fp16 backward.
 * qkv bf16 [batch*seq][3*heads*64] as produced by nn.MultiheadAttention.in_proj ([q | k | v] per row);
 * out bf16 [batch*seq][heads*64]; lse f32 [batch][heads][seq] (natural log-sum-exp of scaled scores).
 * causal = 1 applies CLIP's build_attention_mask (key <= query).
 * ---------------------------------------------------------------------------------------------- */
int uniir_attention_fwd(const void* qkv, void* out, float* lse, int32_t batch, int32_t seq,
                        int32_t heads, int32_t causal, void* stream);
int uniir_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                        void* dqkv, int32_t batch, int32_t seq, int32_t heads, int32_t causal,
                        void* stream);
/* Packed rows: item m owns rows row_off[m] .. row_off[m + 1] - 1 (its own length <= max_seq) of qkv / out / dqkv; lse stays
 * [batch][heads][max_seq].  Every live row's result is bitwise that of the dense call on zero-padded-behind items under causal = 1. */
int uniir_attention_fwd_packed(const void* qkv, void* out, float* lse, const int32_t* row_off, int32_t batch,
                               int32_t max_seq, int32_t heads, int32_t causal, void* stream);
int uniir_attention_bwd_packed(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                               const int32_t* row_off, int32_t batch, int32_t max_seq, int32_t heads, int32_t causal, void* stream);
/* Every packed item has at least one row (row_off[m + 1] > row_off[m]) and every key_len[m] below is >= 1: the kernels stage an
 * item's row T - 1 for the padding behind it, so a length of 0 is not an input. */
/* The forward on fp16 tensors (qkv / out fp16, lse f32): row_off == NULL is uniir_attention_fwd (causal = 0: seq <= 1024, causal = 1:
 * seq <= 512), otherwise uniir_attention_fwd_packed (seq = max_seq <= 512).  There is no fp16 backward. */
int uniir_attention_fwd_f16(const void* qkv, void* out, float* lse, const int32_t* row_off, int32_t batch, int32_t seq,
                            int32_t heads, int32_t causal, void* stream);
/* General form: separate Q [batch*tq][q_ld] and K/V [batch*tk][kv_ld] tensors (head h at column h*64) for the BLIP
 * MED cross-attention (uniir_blip/backbone/med.py:160-232 with encoder_hidden_states), and an optional per-item key
 * length (keys >= key_len[m] masked: the BERT padding mask, med.py:687-688 "(1 - mask) * -10000"; 1 <= key_len[m], values above
 * tk count as tk: a row with no valid key is not an input).
 * lse is [batch][heads][tq].  bwd writes dq [batch*tq][dq_ld], dk / dv [batch*tk][dkv_ld]. */
int uniir_attention_fwd_ex(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out,
                           int64_t out_ld, float* lse, const int32_t* key_len, int32_t batch, int32_t tq,
                           int32_t tk, int32_t heads, int32_t causal, float drop_p, uint32_t drop_seed, void* stream);
int uniir_attention_bwd_ex(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld,
                           const void* out, const void* dout, int64_t out_ld, const float* lse,
                           const int32_t* key_len, void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld,
                           int32_t batch, int32_t tq, int32_t tk, int32_t heads, int32_t causal, float drop_p,
                           uint32_t drop_seed, void* stream);
/* drop_p > 0 (BERT attention_probs_dropout_prob in train mode): P V uses P * mask / (1 - drop_p), mask regenerated from
 * (drop_seed, ((item * heads + head) * tq + query) * tk + key); backward must get the same pair. */
/* The general form on PACKED QUERY ROWS (BLIP's MED BERT on the tokens up to each caption's valid length only; replaces the padded
 * rows of backbone/med.py:160-232, whose keys are masked by (1 - m) * -10000, :687-688): item m owns the rows q_row_off[m] ..
 * q_row_off[m + 1] - 1 of q / out / dout / dq (length <= tq).  kv_packed != 0: self-attention -- k / v / dk / dv are rows of the same
 * packed numbering, the item's key count is its own length (what key_len is in the padded call; key_len must be NULL, tq == tk);
 * kv_packed == 0: cross-attention -- k / v / dk / dv stay dense [batch][tk] rows, key_len optional.  lse keeps the dense
 * [batch][heads][tq] layout; the dropout mask is drawn at the dense coordinates above, so every live row equals the padded call's
 * bit for bit, train mode included. */
int uniir_attention_fwd_rows(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld,
                             float* lse, const int32_t* q_row_off, int32_t kv_packed, const int32_t* key_len, int32_t batch,
                             int32_t tq, int32_t tk, int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
int uniir_attention_bwd_rows(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, const void* out,
                             const void* dout, int64_t out_ld, const float* lse, const int32_t* q_row_off, int32_t kv_packed,
                             const int32_t* key_len, void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch,
                             int32_t tq, int32_t tk, int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
/* The general form for 1 <= tq, tk <= 1024 (bf16, head_dim 64, scale 1/8, no causal mask).  q_row_off == NULL: the call is
 * uniir_attention_fwd_ex / _bwd_ex with causal = 0 (dense [batch][tq] query rows).  q_row_off != NULL: the call is
 * uniir_attention_fwd_rows / _bwd_rows with kv_packed = 0: item m's queries are the rows q_row_off[m] .. q_row_off[m + 1] - 1 of q /
 * out / dout / dq, K / V / dk / dv stay dense [batch][tk].  lse is dense [batch][heads][tq]; entries of rows an item does not have
 * are not written.  key_len[m] >= 1 (NULL: all tk keys); the dk / dv rows of masked keys are written as exact zeros.  The dropout
 * factor of an element is drawn at the dense coordinate ((m * heads + h) * tq + query) * tk + key, the softmax statistics come from
 * the undropped P, so a packed call's live rows are bitwise the dense call's.  Every size runs the streaming kernels (128 query
 * rows per workgroup, K / V in 128-key chunks; dK / dV: 128 keys per workgroup, Q / dO in 64-query chunks); nothing is atomic.
 * As for _rows, every item has at least one query row (q_row_off[m + 1] > q_row_off[m]): an item without queries is not an input.
 * (The kernels would launch no work on its rows and write zeros to its dk / dv rows, but the contract does not promise it and no
 * test covers it.)  The dropout coordinate is taken modulo 2^32, as in the 512-token kernels: a head's extent tq * tk reaches 2^20
 * here, so the coordinates of a call wrap -- and items far apart share masks -- once batch * heads * tq * tk exceeds 2^32 (batch *
 * heads > 4096 at 1024 x 1024, > 12900 at 577 x 577, > 74000 at 100 x 577).
 * UNIIR_EINVAL: a NULL operand, heads <= 0, batch < 0, drop_p outside [0, 1); UNIIR_ESHAPE: tq or tk outside 1 .. 1024;
 * UNIIR_EALIGN: a leading dimension that is no multiple of 8 or a pointer that is not 16-byte aligned.  A refused call writes
 * nothing; batch == 0 is UNIIR_OK. */
int uniir_attention_fwd_long(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld,
                             float* lse, const int32_t* q_row_off, const int32_t* key_len, int32_t batch, int32_t tq, int32_t tk,
                             int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
int uniir_attention_bwd_long(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, const void* out,
                             const void* dout, int64_t out_ld, const float* lse, const int32_t* q_row_off, const int32_t* key_len,
                             void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch, int32_t tq, int32_t tk,
                             int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
/* ONE query row per item (head_dim 64, scale 1/8, no mask, no dropout, no bias) against 1 <= tk <= 1024 dense keys: the attention of
 * a tower's last block when only one row per item leaves it (uniir_clip_tower.pool_last_block).  q / out / dout are dense
 * [batch][heads*64] rows, lse is [batch][heads]; k / v are the rows [batch*tk] of a buffer with leading dimension kv_ld (head h at
 * column h*64: e.g. the K and V thirds of a packed [q | k | v] buffer, kv_ld = 3*heads*64); dq is [batch] rows with leading dimension
 * dq_ld, dk / dv are [batch*tk] rows with leading dimension dkv_ld.  Only the heads*64 columns of a row are read or written: what lies
 * between them (the other two thirds of a [q | k | v] shaped gradient buffer, pad columns) is left alone.
 * _one_fwd: bf16, or fp16 with f16 != 0 (q / k / v / out fp16).  tk <= 512 runs the resident kernel of uniir_attention_fwd_ex, 513 ..
 * 1024 the streaming kernel of uniir_attention_fwd at one query row.  In both ranges out and lse are bitwise row 0 of
 * uniir_attention_fwd (uniir_attention_fwd_f16) on a packed qkv whose row 0 of every item is this query: a query row's result
 * never depends on the rows that share its tile.
 * _one_bwd: bf16; ONE kernel at every tk, one pass over K and V (dV[j] = p_j dO and dK[j] = scale dS_j q are rank-1 products, only
 * dQ = scale sum_j dS_j k_j is a sum): one wave per (item, head), operands straight to registers, no LDS, no atomics.  Products and
 * sums are fp32 and every sum has a fixed order, so two calls give the same bits; values are rounded to bf16 only where dq / dk / dv
 * are stored (the tiled kernels also round P and dS to bf16 for their MFMAs, so the two agree to bf16 rounding, not bit for bit).
 * UNIIR_EINVAL: a NULL operand, heads <= 0, batch < 0; UNIIR_ESHAPE: tk outside 1 .. 1024; UNIIR_EALIGN: a leading dimension that is
 * no multiple of 8 or a pointer that is not 16-byte aligned.  A refused call writes nothing; batch == 0 is UNIIR_OK. */
int uniir_attention_one_fwd(const void* q, const void* k, const void* v, int64_t kv_ld, void* out, float* lse, int32_t batch,
                            int32_t tk, int32_t heads, int32_t f16, void* stream);
int uniir_attention_one_bwd(const void* q, const void* k, const void* v, int64_t kv_ld, const void* out, const void* dout,
                            const float* lse, void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch, int32_t tk,
                            int32_t heads, void* stream);
/* ONE query row per item that STANDS FOR ROW drop_q OF A CALL WITH drop_tq QUERY ROWS (bf16, head_dim 64, scale 1/8, no causal mask, no
 * bias): per-item key counts, packed keys and probability dropout in the one-query form.  BLIP's last BERT layer on the class row
 * (BLIPFeatureFusion.pool_last_layer): only row 0 of every caption leaves the encoder.
 * q / out / dout: [batch] rows with leading dimensions q_ld / out_ld (a dense BERT passes row m*L of its [q | k | v] buffer with q_ld =
 * L*3*heads*64 and copies nothing); lse [batch][heads]; dq [batch] rows with leading dimension dq_ld.
 * Keys, one of two forms (both given: UNIIR_EINVAL):
 *   dense : k / v / dk / dv are [batch][tk] rows (kv_ld / dkv_ld), key_len optional: 1 <= key_len[m], values above tk count as tk,
 *           keys at or behind it are masked as in uniir_attention_fwd_ex; the backward writes exact zeros to their dk / dv rows;
 *   packed: kv_row_off[batch + 1]: item m's keys are the rows kv_row_off[m] .. kv_row_off[m + 1] - 1 of k / v / dk / dv, its key count
 *           its own length (1 <= length <= tk).  No row of another item is read or written.
 * 1 <= tk <= 1024.  Dropout: the factor of key j is drawn at the dense coordinate ((m * heads + h) * drop_tq + drop_q) * tk + j (modulo
 * 2^32) -- the coordinate of that row in uniir_attention_fwd_ex / _fwd_rows / _fwd_long with tq = drop_tq; the softmax statistics come
 * from the undropped P.  1 <= drop_tq, 0 <= drop_q < drop_tq.
 * _fwd: out and lse are bitwise row drop_q of the full call on the same operands and seed with tq = drop_tq: uniir_attention_fwd_ex
 * (key_len) or uniir_attention_fwd_rows (kv_packed = 1 for packed keys, 0 for dense ones) up to 512 keys, uniir_attention_fwd_long
 * above.  Kernels by key range: tk <= 512 the resident kernel of those entry points at one query row (a head's keys whole in LDS);
 * 513 .. 1024 the streaming kernel of uniir_attention_fwd_long at one query row (keys in 128-key chunks), which alone also takes
 * packed keys here.  A query row's result never depends on the rows that share its tile.
 * _bwd: the one-pass kernel of uniir_attention_one_bwd at every tk, extended by the key count and the dropout factor (dV[j] = p_j f_j
 * dO, dP_j = f_j dO . v_j, delta = dO . O): one wave per (item, head), no LDS, no atomics, every sum in a fixed order -- two calls
 * give the same bits.  Without key_len, kv_row_off and dropout it launches the kernel of uniir_attention_one_bwd itself.
 * UNIIR_EINVAL: a NULL operand (key_len and kv_row_off may be NULL), heads <= 0, batch < 0, drop_p outside [0, 1) (a NaN included),
 * drop_tq < 1, drop_q outside 0 .. drop_tq - 1, both key forms; UNIIR_ESHAPE: tk outside 1 .. 1024; UNIIR_EALIGN: a leading
 * dimension that is no multiple of 8 or a pointer that is not 16-byte aligned.  A refused call writes nothing; batch == 0 is UNIIR_OK. */
int uniir_onequery_fwd(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld, float* lse,
                       const int32_t* key_len, const int32_t* kv_row_off, int32_t batch, int32_t tk, int32_t heads, float drop_p,
                       uint32_t drop_seed, int32_t drop_tq, int32_t drop_q, void* stream);
int uniir_onequery_bwd(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, const void* out, const void* dout,
                       int64_t out_ld, const float* lse, const int32_t* key_len, const int32_t* kv_row_off, void* dq, int64_t dq_ld,
                       void* dk, void* dv, int64_t dkv_ld, int32_t batch, int32_t tk, int32_t heads, float drop_p, uint32_t drop_seed,
                       int32_t drop_tq, int32_t drop_q, void* stream);
/* The general form ON FP16 TENSORS, forward only (q / k / v / out fp16, lse f32 [batch][heads][tq]; head_dim 64, scale 1/8, no causal
 * mask, no dropout): the eval-mode embedding forward of the BLIP MED BERT under use_fp16.  One call for what uniir_attention_fwd_ex,
 * _fwd_rows and _fwd_long are in bf16: q_row_off == NULL: dense [batch][tq] query rows; q_row_off != NULL: packed query rows, with
 * kv_packed != 0 K / V in the same packed numbering (self-attention: key_len NULL, tq == tk), with kv_packed == 0 K / V dense
 * [batch][tk] and key_len optional.  q_row_off, kv_packed and key_len mean what they mean there: every item has at least one row,
 * key_len[m] >= 1, lse entries of rows an item does not have are not written, a packed call's live rows are bitwise the dense call's.
 * Kernels: max(tq, tk) <= 512 the resident kernel of uniir_attention_fwd_f16 (with tq == tk, no key_len and the thirds of one packed
 * [q | k | v] buffer the two give the same bits); above it, with kv_packed == 0, the streaming kernel of uniir_attention_fwd_long on
 * fp16 operands (128 query rows per workgroup, K / V in 128-key chunks).
 * The checks, in this order: (1) UNIIR_EINVAL: a NULL q, k, v, out or lse, heads <= 0, batch < 0; (2) UNIIR_EINVAL: kv_packed != 0 with
 * a NULL q_row_off, a non-NULL key_len or tq != tk; (3) batch == 0 is UNIIR_OK; (4) UNIIR_ESHAPE: tq or tk outside 1 .. 1024, or
 * kv_packed != 0 with tq > 512; (5) UNIIR_EALIGN: a leading dimension that is no multiple of 8, then a pointer among q, k, v, out
 * that is not 16-byte aligned.  A refused call writes nothing. */
int uniir_attn_general_fwd_f16(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld,
                               float* lse, const int32_t* q_row_off, int32_t kv_packed, const int32_t* key_len, int32_t batch,
                               int32_t tq, int32_t tk, int32_t heads, void* stream);
/* uniir_onequery_fwd on fp16 tensors, without its four dropout arguments and with its check order otherwise (both key forms:
 * UNIIR_EINVAL, before batch == 0 and the sizes).  The two kernels of uniir_attn_general_fwd_f16 at one query row -- packed keys above
 * 512 take the streaming kernel, as in the bf16 twin -- so out and lse are bitwise row 0 of that call on the same operands. */
int uniir_onequery_fwd_f16(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, void* out, int64_t out_ld,
                           float* lse, const int32_t* key_len, const int32_t* kv_row_off, int32_t batch, int32_t tk, int32_t heads,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * [ENC] small fused pieces of the towers.
 * ---------------------------------------------------------------------------------------------- */
/* images f32 NCHW [n][3][res][res] -> patches bf16 [n*grid*grid][kpad], k = c*P*P + py*P + px (the
 * Conv2d weight's own flattening), zero-padded to kpad (multiple of 64). */
int uniir_patchify(const float* images, void* patches, int32_t n, int32_t res, int32_t patch,
                   int32_t kpad, void* stream);
/* x[n][1+g][w] (f32) = concat(class_emb, patch_out[n][g][w] (bf16)) + pos_emb[1+g][w] */
int uniir_vit_assemble(const void* patch_out, const float* class_emb, const float* pos_emb, float* x,
                       int32_t n, int32_t tokens, int32_t width, void* stream);
/* the two with fp16 in place of bf16 (the fp16 forward of a vision tower: fp16 patch rows for a UNIIR_DT_F16 patch-embedding GEMM,
 * whose fp16 patch_out is read back here); the same checks, no backward */
int uniir_patchify_f16(const float* images, void* patches, int32_t n, int32_t res, int32_t patch,
                       int32_t kpad, void* stream);
int uniir_vit_assemble_f16(const void* patch_out, const float* class_emb, const float* pos_emb, float* x,
                           int32_t n, int32_t tokens, int32_t width, void* stream);
/* backward of uniir_vit_assemble: dpatch bf16 [n*g][w] = dx[:,1:,:]; dclass += sum_n dx[:,0,:]; dpos += sum_n dx */
int uniir_vit_assemble_bwd(const float* dx, void* dpatch_out, float* dclass, float* dpos, int32_t n,
                           int32_t tokens, int32_t width, void* stream);
/* x[n][ctx][w] (f32) = token_emb[text[n][t]] + pos_emb[t]; also eot[n] = argmax_t text[n][t] (first max) */
int uniir_text_embed(const int32_t* text, const float* token_emb, const float* pos_emb, float* x,
                     int32_t* eot, int32_t n, int32_t ctx, int32_t width, int32_t vocab, void* stream);
/* dtoken_emb[text[n][t]] += dx[n][t], dpos[t] += sum_n dx[n][t].  With a scratch buffer on the stream (uniir_reduce_scratch) the rows
 * of a token id are added in ascending row order whatever their number (ids with more than 4096 rows: in row slices whose partials
 * are added in slice order): reproducible bit for bit.  Without one, or for a shape that form does not take (width % 4, a pointer
 * that is not 16-byte aligned, vocab > 65536, n * ctx > 65535 * 4096), fp32 atomics in arrival order, counted by
 * uniir_reduce_stats.  The same holds for the packed form below. */
int uniir_text_embed_bwd(const int32_t* text, const float* dx, float* dtoken_emb, float* dpos,
                         int32_t n, int32_t ctx, int32_t width, int32_t vocab, void* stream);
/* the same on packed rows: x row row_off[n] + t for t < row_off[n + 1] - row_off[n]; last_row[n] (optional) = the item's last row */
int uniir_text_embed_packed(const int32_t* text, const float* token_emb, const float* pos_emb, const int32_t* row_off,
                            float* x, int32_t* last_row, int32_t n, int32_t ctx, int32_t width, int32_t vocab, void* stream);
int uniir_text_embed_bwd_packed(const int32_t* text, const float* dx, const int32_t* row_off, float* dtoken_emb,
                                float* dpos, int32_t n, int32_t ctx, int32_t width, int32_t vocab, void* stream);
/* out[i][:] = x[(i*seq + idx[i])][:] (idx NULL -> 0, the class token): rows for ln_post / ln_final */
int uniir_gather_rows(const float* x, const int32_t* idx, float* out, int32_t n, int32_t seq,
                      int32_t width, void* stream);
/* dx[(i*seq + idx[i])][:] += dout[i][:] ; all other rows of dx must have been zeroed by the caller */
int uniir_scatter_rows(const float* dout, const int32_t* idx, float* dx, int32_t n, int32_t seq,
                       int32_t width, void* stream);
/* act / colsum / casts */
int uniir_act_fwd(const void* f_bf16, void* g_bf16, int64_t count, int32_t act, void* stream);
/* out[n] += sum_m x[m][n]  (x bf16 [rows][ld]) */
int uniir_colsum_bf16(const void* x, int64_t ld, float* out, int32_t rows, int32_t cols, void* stream);
int uniir_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream);
int uniir_cast_f32_to_f16(const float* src, void* dst, int64_t count, void* stream);     /* the fp16 forward's weight copies */
int uniir_cast_bf16_to_f32(const void* src, float* dst, int64_t count, void* stream);
/* dst bf16 [rows][ld_dst] (zero padded) = src f32 [rows][cols] */
int uniir_cast_pad_rows(const float* src, void* dst, int32_t rows, int32_t cols, int32_t ld_dst,
                        void* stream);
int uniir_cast_pad_rows_f16(const float* src, void* dst, int32_t rows, int32_t cols, int32_t ld_dst,
                            void* stream);      /* the same into fp16 (the fp16 forward's patch-embedding weight) */
/* dst f32 [rows][cols] += src f32 [rows][ld_src][:cols]  (un-pad a wgrad result) */
int uniir_unpad_add(const float* src, float* dst, int32_t rows, int32_t cols, int32_t ld_src,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * [FUSE] emb = txt_emb * txt_mask[:,None] + img_emb * img_mask[:,None]  (clip_sf.py:61-63), then
 * q = normalize(emb[idx_q]), p = normalize(emb[idx_p])  (clip_sf.py:88-97; F.normalize eps 1e-12).
 * Masks are int64 like the collator's (mbeir_dataset.py:427-434).  All fp32.
 * ---------------------------------------------------------------------------------------------- */
int uniir_fuse_embeddings(const float* txt_emb, const float* img_emb, const int64_t* txt_mask,
                          const int64_t* img_mask, float* emb, int32_t n, int32_t dim, void* stream);
int uniir_select_normalize(const float* emb, const int32_t* idx, float* out, float* inv_norm,
                           int32_t rows, int32_t dim, void* stream);
/* demb[idx[i]] += (dout[i] - out[i] * <out[i], dout[i]>) * inv_norm[i]  (demb zeroed by the caller).  idx may repeat: the rows that
 * share a destination are added in ascending i by a single writer, so the result is reproducible bit for bit. */
int uniir_select_normalize_bwd(const float* out, const float* inv_norm, const float* dout,
                               const int32_t* idx, float* demb, int32_t rows, int32_t dim, void* stream);
/* dtxt = demb * txt_mask, dimg = demb * img_mask */
int uniir_fuse_embeddings_bwd(const float* demb, const int64_t* txt_mask, const int64_t* img_mask,
                              float* dtxt, float* dimg, int32_t n, int32_t dim, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [NCE] in-batch InfoNCE, fp32 end to end (f32 MFMA 16x16x4: exact fp32 fma chains).
 *   score[i][j] = <q[i], all_p[j]> * scale            (scale = exp(logit_scale), device scalar)
 *   loss = mean_i( logsumexp_j score[i][:] - score[i][t_i] ),  t_i = target_offset + i
 *   acc  = mean_i( argmax_j score[i][:] == t_i )      (first max on ties, torch.max semantics)
 * score may be NULL only in uniir_infonce_bwd (it is required by fwd as the stash for bwd).
 * bwd: with g = dloss (device scalar), G = (softmax(score) - onehot) * g / b,
 *   dq = scale * G . all_p,  d_all_p = scale * G^T . q,  dscale = sum(G * score) / scale.
 * ---------------------------------------------------------------------------------------------- */
int uniir_infonce_fwd(const float* q, const float* all_p, const float* scale, int32_t b, int32_t B,
                      int32_t dim, int32_t target_offset, float* score, float* row_lse, float* loss,
                      float* acc, void* stream);
int uniir_infonce_bwd(const float* q, const float* all_p, const float* scale, const float* score,
                      const float* row_lse, const float* dloss, int32_t b, int32_t B, int32_t dim,
                      int32_t target_offset, float* gbuf, float* dq, float* d_all_p, float* dscale,
                      void* stream);
/* Hard-negative branch of the same loss (clip_sf.py:105-131).  q, p [b][dim], n [b][N][dim] are L2-normalised fp32 rows;
 * the logit row of query i is [<q_i,p_i>, <q_i,n_i,0..N-1>, I more copies of <q_i,p_i>] * scale, I = min(b - 1,
 * in_batch_neg_num): the reference's expand/mask expression for the "in-batch negatives" yields the query's own
 * positive I times, which is reproduced as is (golden G3).  fwd: logits [b][1+N+I], row_lse, row_loss (= -log_softmax(row)[0]) and
 * row_hit (first arg-max == 0) per query; loss = mean(row_loss), accuracy = mean(row_hit).
 * bwd (dloss: device scalar): dq, dn written; dp and dscale ACCUMULATED (zero them first).  Reproducible bit for bit: every dp element
 * has one writer, and dscale is one fixed-order sum over the b rows added to dscale by a single thread. */
int uniir_hardneg_fwd(const float* q, const float* p, const float* n, const float* scale, int32_t b, int32_t N,
                      int32_t I, int32_t dim, float* logits, float* row_lse, float* row_loss, float* row_hit,
                      void* stream);
int uniir_hardneg_bwd(const float* q, const float* p, const float* n, const float* scale, const float* logits,
                      const float* row_lse, const float* dloss, int32_t b, int32_t N, int32_t I, int32_t dim,
                      float* dq, float* dp, float* dn, float* dscale, void* stream);
/* generic strided fp32 MFMA GEMM used by the two above (exported for tests):
 * C[m][n] (ldc) = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn]  */
int uniir_sgemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, float alpha, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [TOWER] a whole CLIP tower per call: what the reference's FFI for this path would bind for
 * `clip_model.encode_image(image)` / `clip_model.encode_text(text)` (clip_sf.py:44,47; openai/CLIP
 * VisionTransformer.forward / CLIP.encode_text) and their autograd backward.  The per-layer launch sequence lives in the
 * library (csrc/tower.hip); the op-level entry points above stay available.
 *   weights / gradients : raw device pointers in the POD structs below.  "16" fields are the bf16 shadow of the fp32
 *                         master weights (kept fresh by uniir_adamw_step or uniir_cast_f32_to_bf16); g_* are fp32
 *                         gradients, ACCUMULATED (+=), may be NULL for a forward-only description.
 *   activations         : ONE caller-owned workspace of uniir_clip_tower_workspace_bytes() bytes (256-B aligned); with
 *                         save_for_backward it is the activation stash and must be passed unchanged to the bwd calls.
 *   forward             : input = images f32 NCHW [batch][3][res][res] (vision) or token ids int32 [batch][tokens] (text)
 *                         -> emb_out f32 [batch][embed_dim].
 *   backward            : demb f32 [batch][embed_dim].  uniir_clip_tower_bwd = head + all blocks + stem; the three stages
 *                         are exported so that a caller can hand finished layers to its gradient all-reduce between
 *                         uniir_clip_tower_bwd_blocks calls (descending ranges [lo, hi) covering all layers).
 * Asynchronous on `stream`, no allocation, no host synchronisation; 0 or a negative UNIIR_E* code.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;                 /* [W] */
    const void *wqkv16, *wo16, *wfc16, *wproj16;                /* bf16 [3W][W], [W][W], [4W][W], [W][4W] */
    const float *bqkv, *bo, *bfc, *bproj;                       /* [3W], [W], [4W], [W] */
    float *g_ln1_w, *g_ln1_b, *g_ln2_w, *g_ln2_b;
    float *g_wqkv, *g_bqkv, *g_wo, *g_bo, *g_wfc, *g_bfc, *g_wproj, *g_bproj;
} uniir_clip_block;

typedef struct {
    int32_t is_text;                          /* 0: vision tower, 1: text tower (causal attention, EOT pooling) */
    int32_t layers, width, heads, tokens;     /* width = 64 * heads; tokens = 1 + (resolution/patch)^2 or context_length */
    int32_t embed_dim;
    int32_t resolution, patch, kpad;          /* vision: kpad = 3*patch*patch rounded up to 64 */
    int32_t vocab;                            /* text */
    const uniir_clip_block* blocks;           /* HOST array [layers] */
    const void* conv16;                       /* vision: bf16 [W][kpad] (conv1.weight flattened, zero padded) */
    const float *class_emb, *pos_emb;         /* vision [W], [tokens][W]; text: pos_emb [tokens][W] */
    const float *ln_pre_w, *ln_pre_b;         /* vision */
    const float* token_emb;                   /* text [vocab][W] */
    const float *ln_post_w, *ln_post_b;       /* visual.ln_post / ln_final */
    const void* proj16;                       /* bf16 [W][embed_dim]: visual.proj / text_projection */
    float *g_conv;                            /* fp32 [W][3*patch*patch] (conv1.weight.grad) */
    float *g_class, *g_pos, *g_ln_pre_w, *g_ln_pre_b, *g_token, *g_ln_post_w, *g_ln_post_b, *g_proj;
    void* splitk_ws;                          /* optional scratch for the weight-gradient GEMMs' split-K slabs */
    int64_t splitk_ws_bytes;
    int32_t ln_bwd_side;                      /* 1 = in uniir_clip_tower_bwd_blocks the backward of ln_2 runs inside the launch of
                                                 the c_fc weight gradient and the backward of ln_1 inside that of the in_proj weight
                                                 gradient (uniir_gemm_wgrad_ln_bwd: a few compute units stream the LayerNorm rows while the
                                                 others feed the matrix pipes); each of the two activation-gradient GEMMs then runs before
                                                 its layer's weight gradient.  Same activation gradients bit for bit; those two weight
                                                 gradients are summed over more split-K slabs (needs splitk_ws: 7 x 4W x W and 13 x 3W x W
                                                 floats at ViT-L/14 x 1024 images), the LayerNorm parameter gradients over other row
                                                 groups -- other valid fp32 orders, the same bits in every run.  Pairs without a chunk
                                                 plan or slab room run as the two launches they replace.  0 = the separate launches.
                                                 This field sits in front of the four flags below, which stay the struct's last
                                                 fields.  Any other value is UNIIR_EINVAL */
    int32_t stash_act;                       /* with save_for_backward: 0 = the MLP's act(f) lives in one scratch buffer and the
                                                 backward re-materialises it from the stashed pre-activation f inside the c_proj dgrad
                                                 epilogue; 1 = act(f) is stashed per layer next to f (round 4: +2 bytes x rows x 4 width
                                                 per layer of workspace; that epilogue loses its second output: 3.31 -> 2.99 ms at ViT-L/14 x
                                                 1024 items).  Same forward bit for bit; the c_proj weight gradient reads the forward's
                                                 act(f) instead of the backward's recomputation (equal up to rare one-ulp differences).
                                                 Part of the workspace layout: every call on one workspace must see the same value */
    int32_t dtype16;                          /* 0 = bf16 (training and the default forward); 1 = fp16, FORWARD ONLY: wqkv16 .. proj16 /
                                                 conv16 then point at fp16 copies of the weights (uniir_cast_f32_to_f16) and every
                                                 16-bit activation is fp16 -- the reference embedder's autocast(fp16),
                                                 mbeir_embedder.py:52-56; save_for_backward with it is UNIIR_EUNSUPPORTED */
    int32_t pool_last_block;                  /* 1 = the LAST residual block runs its Q projection, attention, out_proj, ln_2 and MLP on
                                                 the one pooled row of every item only (class token / EOT row; ln_1 and the K | V
                                                 projection still see every row): the reference computes the other rows' outputs of
                                                 that block and discards them (VisionTransformer.forward: ln_post(x[:, 0, :]);
                                                 CLIP.encode_text: x[arange, text.argmax(-1)]).  Same embedding bit for bit; the same
                                                 gradient sums without their exact-zero terms (the one-query attention backward is the
                                                 general kernel: at 193..288 tokens, where the full block runs the pair-tile kernel,
                                                 upstream gradients agree to bf16 rounding, 4e-3); 10 of the block's 12 WxW GEMM units
                                                 leave the step.  Part of the
                                                 workspace layout like stash_act.  0 = every row through every sublayer.
                                                 Value 1 pools up to 512 tokens: above that (a vision tower at 577 tokens) the full
                                                 last block runs and the workspace is that of 0.
                                                 2 = the pooled last block at EVERY token count the tower takes (<= 1024): above 512
                                                 tokens the one-query attention is uniir_attention_one_fwd / _one_bwd (the streaming
                                                 forward at one query row, the one-pass backward); training, recomputation and the
                                                 fp16 forward follow.  Contract of that mode: embeddings are bitwise those of the full
                                                 block; parameter gradients agree to bf16 rounding for everything upstream of the
                                                 last block's attention (two valid bf16 backward kernels, as at 193..288 tokens), the
                                                 last block's out_proj, ln_2 and MLP and the head keep theirs up to the order of fp32
                                                 sums.  At <= 512 tokens 2 behaves as 1: same kernels, same workspace layout */
    int32_t recompute;                        /* activation recomputation (ABI 3).  0 = the training forward stashes every block's
                                                 intermediates (28 - 36 bytes per row x width element per layer).  1 = with
                                                 save_for_backward the forward keeps only the fp32 residual stream that ENTERS each
                                                 block (`layers` slots of rows x width x 4 bytes) and runs all blocks through ONE shared
                                                 set of the other layer buffers (qkv, attention out, LSE, x2, f, act(f), h1, h2);
                                                 uniir_clip_tower_bwd_blocks[_packed] rebuilds block i's set from its stored input
                                                 right before block i's backward, with the forward's own function and arguments (same
                                                 kernels, shapes and inputs; every kernel is deterministic), so the set holds the bits
                                                 the forward produced and the gradients are those of the stored run.  The block's
                                                 c_proj GEMM is not re-run (no backward reads a block's output): 8 of the block's 12
                                                 WxW GEMM units + attention forward + two LayerNorms per block; with pool_last_block
                                                 the last block re-runs ln_1 and its K | V projection only (its [batch]-row buffers
                                                 are kept).  stash_act has no effect on the layout or the arithmetic in this mode:
                                                 act(f) exists once in the shared set, so the backward always reads the forward-formula
                                                 act(f) and takes the one-output c_proj dgrad epilogue, i.e. the stash_act = 1
                                                 arithmetic.  The staged backward keeps its contract (descending ranges covering all
                                                 layers, one call per layer or one for all: identical results); every block is rebuilt
                                                 from its slot, none is assumed to be still in the shared set.  Without
                                                 save_for_backward the flag changes nothing.  Part of the workspace layout like
                                                 stash_act and pool_last_block: every call on one workspace must see the same value.
                                                 Any other value is UNIIR_EINVAL (the workspace query returns -1) */
} uniir_clip_tower;

int64_t uniir_clip_tower_workspace_bytes(const uniir_clip_tower* t, int32_t batch, int32_t save_for_backward);
int uniir_clip_tower_fwd(const uniir_clip_tower* t, const void* input, int32_t batch, float* emb_out, void* workspace,
                         int64_t workspace_bytes, int32_t save_for_backward, void* stream);
int uniir_clip_tower_bwd(const uniir_clip_tower* t, const void* input, const float* demb, int32_t batch, void* workspace,
                         int64_t workspace_bytes, void* stream);
int uniir_clip_tower_bwd_head(const uniir_clip_tower* t, const float* demb, int32_t batch, void* workspace,
                              int64_t workspace_bytes, void* stream);
int uniir_clip_tower_bwd_blocks(const uniir_clip_tower* t, int32_t batch, int32_t layer_lo, int32_t layer_hi, void* workspace,
                                int64_t workspace_bytes, void* stream);
int uniir_clip_tower_bwd_stem(const uniir_clip_tower* t, const void* input, int32_t batch, void* workspace,
                              int64_t workspace_bytes, void* stream);
/* Where the calls above keep what in the workspace: the plan they carve it with, as data (csrc/tower.hip plan(); this call copies
 * that plan's fields, it computes nothing itself).  Host arithmetic only -- no device, no stream, like uniir_topk_plan.
 * live_rows = -1: the dense layout (batch x tokens rows); >= 0: the packed text layout of that many live rows.  Every offset is in
 * bytes from the workspace base and 256-byte aligned; a region the description does not have is -1 (the vision stem of a text tower,
 * the pl_* buffers without a pooled last block, every backward transient without save_for_backward, o_x with recompute, o_f / o_g
 * where they are not stashed).  `total` equals uniir_clip_tower_workspace_bytes[_packed] of the same arguments.
 *   head / stem   eot int32 [batch]; pooled_rows f32 [batch][W] (the pooled row of the last block's output); pooled bf16 [batch][W]
 *                 (ln_post of it); patches bf16 [batch G][kpad]; po bf16 [batch G][W] (G = tokens - 1); x0 f32 [rows][W]
 *   layer i       set base = lay0 + i * lay_stride (lay_stride 0: ONE shared set -- forward-only and recompute); inside a set:
 *                 o_x f32 [rows][W] (the stream that enters the block), o_qkv bf16 [rows][3W], o_ao bf16 [rows][W],
 *                 o_lse f32 [batch][heads][tokens], o_x2 f32 [rows][W], o_f / o_g bf16 [rows][4W], o_h1 / o_h2 bf16 [rows][W].
 *                 recompute: block i's input is at xs0 + i * xs_stride instead.  x_last f32 [rows][W]: the stream after the last block
 *   pooled block  pl_q, pl_h1, pl_ao, pl_h2 bf16 [batch][W]; pl_x, pl_x2 f32 [batch][W]; pl_lse f32 [batch][heads]; pl_f, pl_g bf16
 *                 [batch][4W]
 *   transients    from `tmp` on: g bf16 [rows][4W] (act(f) when it is not stashed), then with save_for_backward df bf16 [rows][4W],
 *                 dh bf16 [rows][W], dx / dx2 f32 [rows][W], dxb bf16 [rows][W], dqkv bf16 [rows][3W], demb16 bf16 [batch][E],
 *                 dpooled bf16 [batch][W], drows f32 [batch][W], pl_dxb / pl_dh / pl_dhq bf16 [batch][W], pl_df bf16 [batch][4W],
 *                 pl_dx2 f32 [batch][W], pl_dqkv bf16 [batch][3W], dx0 f32 [rows][W], dpo bf16 [batch G][W], dconv f32 [W][kpad].
 * No two regions overlap (with lay_stride 0 every layer uses the one set in turn).  The forward's and the backward's transients are one union behind `tmp`: a forward-only layout ends after
 * `g`, the training layout continues behind it, and `g` is the only transient both directions write. */
typedef struct {
    int64_t total;
    int64_t rows;                             /* rows of the residual stream: batch x tokens, or live_rows */
    int32_t save, pool_last, stash_act, recompute;          /* the flags as plan() resolved them (0 / 1) */
    int64_t eot, pooled_rows, pooled, patches, po, x0;
    int64_t lay0, lay_stride, o_x, o_qkv, o_ao, o_lse, o_x2, o_f, o_g, o_h1, o_h2;
    int64_t xs0, xs_stride, x_last;
    int64_t pl_q, pl_h1, pl_x, pl_ao, pl_lse, pl_x2, pl_h2, pl_f, pl_g;
    int64_t tmp, g, df, dh, dx, dx2, dxb, dqkv, demb16, dpooled, drows;
    int64_t pl_dxb, pl_df, pl_dh, pl_dx2, pl_dqkv, pl_dhq;
    int64_t dx0, dpo, dconv;
} uniir_clip_tower_layout_t;
int uniir_clip_tower_layout(const uniir_clip_tower* t, int32_t batch, int32_t live_rows /* -1 = dense */, int32_t save_for_backward,
                            uniir_clip_tower_layout_t* out);
/* The TEXT tower on packed rows (exact): only the tokens up to and including each caption's EOT are rows of the residual stream.
 * Under CLIP's causal mask nothing behind the EOT reaches the pooled feature (clip_sf.py:43-44 -> CLIP.encode_text pools at
 * argmax(tokens)), so embeddings and activation gradients are bitwise those of the dense calls above and the weight gradients the same
 * sums without their zero terms (equal up to the order of fp32 additions).  row_off: device int32 [batch + 1], prefix sums of the
 * live lengths (argmax + 1); live_rows = row_off[batch] as known to the host.  Same workspace discipline as the dense calls. */
int64_t uniir_clip_tower_workspace_bytes_packed(const uniir_clip_tower* t, int32_t batch, int32_t live_rows,
                                                int32_t save_for_backward);
int uniir_clip_tower_fwd_packed(const uniir_clip_tower* t, const void* tokens, int32_t batch, const int32_t* row_off,
                                int32_t live_rows, float* emb_out, void* workspace, int64_t workspace_bytes,
                                int32_t save_for_backward, void* stream);
int uniir_clip_tower_bwd_head_packed(const uniir_clip_tower* t, const float* demb, int32_t batch, const int32_t* row_off,
                                     int32_t live_rows, void* workspace, int64_t workspace_bytes, void* stream);
int uniir_clip_tower_bwd_blocks_packed(const uniir_clip_tower* t, int32_t batch, const int32_t* row_off, int32_t live_rows,
                                       int32_t layer_lo, int32_t layer_hi, void* workspace, int64_t workspace_bytes, void* stream);
int uniir_clip_tower_bwd_stem_packed(const uniir_clip_tower* t, const void* tokens, int32_t batch, const int32_t* row_off,
                                     int32_t live_rows, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [FP32] forward path of the encoders in fp32 ("model.float()" of the reference: clip_sf.py:25-26 keeps fp32 weights,
 * the embedder only autocasts when use_fp16 is set).  Linear layers = uniir_sgemm (exact fp32 MFMA) followed by
 * uniir_bias_act_f32: y = (resid ? resid : 0) + act(y + bias) in place (act < 0: none, else UNIIR_ACT_*);
 * uniir_vit_assemble_f32 = uniir_vit_assemble on an fp32 patch projection; uniir_attention_f32_fwd = softmax(scale q k^T
 * [causal / key_len masks]) v with separate Q / K / V views like uniir_attention_fwd_ex, fp32 in and out, any seq.
 * Forward only; 157 TFLOP/s peak -- reference precision, not throughput.
 * ---------------------------------------------------------------------------------------------- */
int uniir_bias_act_f32(float* y, const float* bias, const float* resid, int64_t rows, int32_t cols, int32_t act,
                       void* stream);
int uniir_vit_assemble_f32(const float* patch_out, const float* class_emb, const float* pos_emb, float* x, int32_t n,
                           int32_t tokens, int32_t width, void* stream);
int uniir_attention_f32_fwd(const float* q, int64_t q_ld, const float* k, const float* v, int64_t kv_ld, float* out,
                            int64_t out_ld, const int32_t* key_len, int32_t batch, int32_t tq, int32_t tk,
                            int32_t heads, int32_t causal, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [OPT] fused AdamW over one flat fp32 parameter group (torch.optim.AdamW semantics, no amsgrad):
 *   p *= 1 - lr*wd ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ;
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * grad_scale multiplies g first (1/accumulation_steps or 1/world); also refreshes the bf16 shadow.
 * ---------------------------------------------------------------------------------------------- */
int uniir_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     void* param_bf16, int64_t count, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int32_t step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [OPT] gradient guard: the part of the reference's scaler.step(optimizer) that is not the loss scale (uniir_clip/engine.py:34-42,
 * uniir_blip/engine.py:44-52: a step whose gradients hold Inf or NaN is not applied), plus torch's clip_grad_norm_, decided on the
 * device.  uniir_grad_guard reads the AdamW ranges of one step (host arrays of device pointers and counts) and fills a control
 * block; uniir_adamw_step_guarded is uniir_adamw_step behind that block.  Nothing here reads device memory on the host.
 *   x = fl32(g * grad_scale) per element (what AdamW consumes); sumsq = sum of the exact fp64 squares of the finite x, in one fixed
 *   order: chunks of uniir_grad_guard_chunk() elements per range (a compile-time constant, independent of grid, chip and stream),
 *   one workgroup and one fp64 partial per chunk, the partials of all ranges added in index order by a fixed tree.  No atomics:
 *   same input, same bits.  Any order of n exact non-negative terms is within n * 2^-53 * sumsq of the exact sum.
 *   norm = fl32(sqrt(sumsq)) (the f64 root); nonfinite = a non-finite x anywhere, or norm == Inf; skip = nonfinite && skip_nonfinite;
 *   coef = 0 when skip; else min(1, max_norm / (norm + 1e-6)) in fp32 when max_norm > 0 and !nonfinite (clip_grad_norm_); else 1.
 *   first_bad_range / first_bad_chunk / first_bad_index: the lowest (range, element) that was non-finite -- its range, its chunk in
 *   the range and its element offset in the range; -1 without one.  steps_seen += 1 and steps_skipped += skip on the device: the
 *   caller zeroes (or restores) the block once and never writes it again.
 * uniir_grad_guard: one launch per non-empty range plus the finish; max_norm <= 0: no clipping; no ranges or all counts 0: norm 0,
 * coef 1, skip 0.  UNIIR_EINVAL: a NULL operand (grads[r] may be NULL where counts[r] == 0; workspace may be NULL where it needs no
 * bytes), a negative count or one of 2^40 and more, more than 2^20 ranges, a NaN or negative grad_scale, a NaN max_norm, a workspace
 * below uniir_grad_guard_workspace_bytes (which returns -1 for counts it refuses); UNIIR_EALIGN: a range pointer or the control block
 * not 16-byte aligned, a workspace not 256-byte aligned.  All of it before anything is launched: a refused call writes nothing.
 * uniir_adamw_step_guarded: skip != 0 -- no thread touches param, the moments or the shadow; otherwise g' = fl32(fl32(g * grad_scale)
 * * coef), so coef == 1 gives uniir_adamw_step's bits.  `step` is the caller's count of APPLIED steps (+1): a caller that learns of
 * a skip takes its count back by one, as torch does when scaler.step() leaves optimizer.step() out.  Errors as uniir_adamw_step,
 * plus a NULL (UNIIR_EINVAL) or misaligned (UNIIR_EALIGN) control block.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uniir_grad_ctl {      /* 64 bytes, 16-byte aligned, device memory */
    double sumsq;
    float norm;
    float coef;
    int32_t nonfinite;
    int32_t skip;
    int32_t first_bad_range;
    int32_t first_bad_chunk;
    int64_t first_bad_index;
    int64_t steps_seen;
    int64_t steps_skipped;
    int64_t reserved;
} uniir_grad_ctl;
int64_t uniir_grad_guard_chunk(void);
int64_t uniir_grad_guard_workspace_bytes(const int64_t* counts, int32_t nranges);
int uniir_grad_guard(const float* const* grads, const int64_t* counts, int32_t nranges, float grad_scale, float max_norm,
                     int32_t skip_nonfinite, uniir_grad_ctl* ctl_dev, void* workspace, int64_t workspace_bytes, void* stream);
int uniir_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                             int64_t count, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                             float grad_scale, const uniir_grad_ctl* ctl_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [BLIP] extra pieces of the BLIP_FF path (src/models/uniir_blip): tanh pooler (backbone/med.py:499-511), momentum
 * EMA p_m = m p_m + (1-m) p (blip_featurefusion/blip_ff.py:288-292) over a flat buffer (+ bf16 shadow), and the
 * soft-target contrastive loss of blip_ff.py:219-231 on one matrix of dot products sim [b][n] (n = b + queue) with
 * logits = sim / *temp (temp NULL -> 1):
 *   target = alpha * softmax(sim_m / temp) + (1-alpha) * pos / sum(pos), pos_j = (ids_all[j] == ids_row[i]);
 *   row_loss[i] = -sum_j log_softmax(logits[i])_j target_j;
 *   with g = (softmax(logits) - target) * gscale * (dloss ? *dloss : 1):
 *     dsim = g / temp (optional), row_dtemp[i] = -sum_j g_j logits_j / temp (optional);
 *   row_hit[i] = pos[argmax_j sim[i][j]]  (accuracy of blip_ff.py:250-252, first max).
 * ---------------------------------------------------------------------------------------------- */
int uniir_tanh_fwd(const float* x, float* y, int64_t count, void* stream);
int uniir_tanh_bwd(const float* y, const float* dy, float* dx, int64_t count, void* stream);
int uniir_ema_update(float* param_m, const float* param, void* param_m_bf16, int64_t count, float momentum,
                     void* stream);
int uniir_softce(const float* sim, const float* sim_m, const float* temp, const int64_t* ids_row,
                 const int64_t* ids_all, int32_t b, int32_t n, float alpha, float gscale, const float* dloss,
                 float* row_loss, float* row_hit, float* dsim, float* row_dtemp, void* stream);
/* uniir_sgemm with C += instead of C = (dq = dsim[:, :b] p_m + dsim[:, b:] queue^T without a concatenated copy) */
int uniir_sgemm_acc(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                    float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, float alpha, void* stream);
/* The same product for a LONG reduction with few output tiles (BLIP: d feat = dsim[b][K] x queue[K][E], K = 57 344): deterministic
 * split-K -- slices of whole K steps into slabs of the caller's workspace, added in slice order.  Reproducible run to run; differs
 * from uniir_sgemm's k-ordered chain in the last bits (so the logits never take it).  accumulate != 0: C += alpha * A B.
 * Falls back to the plain kernel when there is nothing to split. */
int64_t uniir_sgemm_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K);
int uniir_sgemm_splitk(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
                       int64_t ldc, int32_t M, int32_t N, int32_t K, float alpha, int32_t accumulate, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [DROPOUT] train-mode dropout / DropPath of the BLIP and T5 stacks.  Masks are counter based: element idx of a call
 * with seed s is kept iff fmix32(idx * 0x9E3779B1 ^ s) >= p * 2^32 (kept values are scaled by 1 / (1 - p)); backward
 * regenerates the mask from the same (seed, idx).  idx = row * cols + col of the logical [rows][cols] tensor.
 *   dropout_f32 : y = (resid ? resid : 0) + x * mask [* rowscale[row / rows_per_scale]]  -> fp32 and / or bf16
 *   dropout_bf16: y = x * mask [* rowscale[...]]  (bf16 rows of pitch ld; in place allowed)
 *   dropout_mask: out[idx] = mask value (0 or 1 / (1 - p)); for tests
 * rowscale (optional) is the per-item DropPath factor (0 or 1 / keep) of blip's ViT-large.
 * ---------------------------------------------------------------------------------------------- */
int uniir_dropout_f32(const float* x, const float* resid, float* y_f32, void* y_bf16, int64_t rows, int32_t cols, float p,
                      uint32_t seed, const float* rowscale, int32_t rows_per_scale, void* stream);
int uniir_dropout_bf16(const void* x, void* y, int64_t rows, int32_t cols, int64_t ld, float p, uint32_t seed,
                       const float* rowscale, int32_t rows_per_scale, void* stream);
int uniir_dropout_mask(float* out, int64_t count, float p, uint32_t seed, void* stream);
/* the same on PACKED rows (no rowscale): row r of x / resid / y is row row_map[r] of the logical tensor, idx = row_map[r] * cols + col
 * -- a BERT that runs on the live rows of its captions only draws the mask elements those rows have in the padded batch */
int uniir_dropout_f32_rows(const float* x, const float* resid, float* y_f32, void* y_bf16, int64_t rows, int32_t cols, float p,
                           uint32_t seed, const int32_t* row_map, void* stream);
int uniir_dropout_bf16_rows(const void* x, void* y, int64_t rows, int32_t cols, int64_t ld, float p, uint32_t seed,
                            const int32_t* row_map, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [CLIP_FF] pieces of the feature-fusion stack of src/models/uniir_clip/clip_featurefusion/clip_ff.py:80-96,161-192
 * (transformers T5Stack, encoder mode): RMS norm (T5LayerNorm: y = gamma * x * rsqrt(mean(x^2) + eps), no bias; same
 * argument meaning as uniir_layernorm_*), self-attention with logits = scale * q.k + rel_emb[rel_bucket[key - query +
 * seq - 1]][head] on packed qkv (T5Attention: scale 1, bucketed relative position bias; rel_bucket is the host-computed
 * bucket of every offset, [2 seq - 1] int32; bwd ACCUMULATES d rel_emb into drel [buckets][heads]), and the mean over the
 * tokens of an item.
 * ---------------------------------------------------------------------------------------------- */
int uniir_rmsnorm_fwd(const float* x, int64_t x_stride, const float* gamma, void* y_bf16, float* y_f32, int32_t rows,
                      int32_t width, float eps, void* stream);
int uniir_rmsnorm_bwd(const float* x, int64_t x_stride, const float* gamma, const void* dy, int32_t dy_is_f32,
                      const float* dres, float* dx_f32, int64_t dx_stride, void* dx_bf16, float* dgamma, int32_t rows,
                      int32_t width, float eps, void* stream);
int uniir_attention_rel_fwd(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                            int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, float drop_p,
                            uint32_t drop_seed, void* stream);
/* drel [nbuckets][heads] (fp32) += d loss / d rel_emb (accumulated: the layers of a T5 stack share one table; zero it once per
 * step).  With a scratch buffer of batch * heads * nbuckets floats on the stream the sum has one fixed order (64-bit fixed-point sums
 * of 2^-40 units inside a workgroup: |sum| < 2^23 per (item, head, bucket); the items' partials added in item order) and is
 * reproducible bit for bit; otherwise one float atomic per (item, head, bucket), counted by uniir_reduce_stats.  dqkv never depends
 * on arrival order. */
int uniir_attention_rel_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                            const float* rel_emb, const int32_t* rel_bucket, int32_t nbuckets, float scale, float* drel,
                            int32_t batch, int32_t seq, int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
/* The same two calls for 1 <= seq <= 1024 (bf16, rel_bucket [2 seq - 1]).  Every size runs the streaming kernels of
 * uniir_attention_fwd_long (128 query rows per workgroup, K / V in 128-key chunks; dK / dV: 128 keys per workgroup, Q / dO in 64-query
 * chunks), nothing is forwarded to the 512-token kernels; the bias of every diagonal sits in LDS.  drel is ACCUMULATED as above.  A dK /
 * dV workgroup sums dS along the diagonals its 128 keys see and then per bucket in the 64-bit fixed point of uniir_attention_rel_bwd,
 * and stores its nbuckets sums, zeros included, as the partial of (item, key block) in the stream's scratch: batch * ceil(seq / 128) *
 * nbuckets * heads floats, added into drel in that fixed order.  Without that much scratch: one float atomic per (item, key block, head,
 * bucket), counted by uniir_reduce_stats.  dqkv never depends on arrival order.  Dropout coordinates and their wrap beyond 2^32
 * elements per call: as for uniir_attention_fwd_long.
 * UNIIR_EINVAL: a NULL operand (drel may be NULL: no bias gradient), heads <= 0, batch < 0, drop_p outside [0, 1), nbuckets outside
 * 1 .. 64; UNIIR_ESHAPE: seq outside 1 .. 1024; UNIIR_EALIGN: qkv, out, dout or dqkv not 16-byte aligned.  A refused call writes
 * nothing; batch == 0 is UNIIR_OK. */
int uniir_attention_rel_fwd_long(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                                 int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, float drop_p,
                                 uint32_t drop_seed, void* stream);
int uniir_attention_rel_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                 const float* rel_emb, const int32_t* rel_bucket, int32_t nbuckets, float scale, float* drel,
                                 int32_t batch, int32_t seq, int32_t heads, float drop_p, uint32_t drop_seed, void* stream);
/* The fp16 forward of the stack (eval mode only: no dropout arguments; there is no fp16 backward).
 * uniir_rmsnorm_fwd_f16: uniir_rmsnorm_fwd with an fp16 16-bit output -- y_f32 has the bits of uniir_rmsnorm_fwd's, y_f16 is that fp32
 * value rounded once to fp16 (round to nearest even; beyond 65504 it becomes inf, as in every fp16 kernel here: nothing is clamped).
 * uniir_attn_rel_fwd_f16 / uniir_attn_rel_fwd_long_f16: uniir_attention_rel_fwd / _rel_fwd_long without dropout on fp16 qkv / out
 * (lse and rel_emb stay fp32): 1 <= seq <= 512 on the resident kernel, 1 <= seq <= 1024 on the streaming kernel at every size.  The
 * same codes for the same conditions as their bf16 twins (the resident form tests no alignment, the streaming one refuses a qkv or
 * out that is not 16-byte aligned with UNIIR_EALIGN); a refused call writes nothing; batch == 0 is UNIIR_OK.  The names start with
 * uniir_attn_, not uniir_attention_: the set of uniir_attention_* entry points is closed. */
int uniir_rmsnorm_fwd_f16(const float* x, int64_t x_stride, const float* gamma, void* y_f16, float* y_f32, int32_t rows,
                          int32_t width, float eps, void* stream);
int uniir_attn_rel_fwd_f16(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                           int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, void* stream);
int uniir_attn_rel_fwd_long_f16(const void* qkv, void* out, float* lse, const float* rel_emb, const int32_t* rel_bucket,
                                int32_t nbuckets, float scale, int32_t batch, int32_t seq, int32_t heads, void* stream);
/* The fp32 forward of the stack (CLIPFeatureFusion.precision = "fp32": uniir_rmsnorm_fwd's y_f32, uniir_sgemm, uniir_bias_act_f32).
 * uniir_attn_f32_rel_fwd: the fp32 twin of uniir_attn_rel_fwd_f16, without lse -- fp32 packed qkv [batch*seq, 3*heads*64] -> fp32 out
 * [batch*seq, heads*64], logit(i, j) = scale * <q_i, k_j> + rel_emb[rel_bucket[j - i + seq - 1]][head], softmax over j, times V;
 * rel_bucket has 2 seq - 1 entries in [0, nbuckets), rel_emb is [nbuckets][heads].  The kernel of uniir_attention_f32_fwd ([FP32])
 * with the head's diagonal biases in LDS: fp32 VALU, one rounding more per logit; with an all-zero rel_emb it has the bits of
 * uniir_attention_f32_fwd on the same buffer.  1 <= seq <= 1024 at one kernel.  UNIIR_EINVAL: a NULL operand, heads <= 0, batch < 0,
 * nbuckets outside 1..64; UNIIR_ESHAPE: seq outside 1..1024; a refused call writes nothing; batch == 0 is UNIIR_OK.  No alignment
 * requirement beyond that of a float. */
int uniir_attn_f32_rel_fwd(const float* qkv, float* out, const float* rel_emb, const int32_t* rel_bucket, int32_t nbuckets,
                           float scale, int32_t batch, int32_t seq, int32_t heads, void* stream);
int uniir_meanpool_fwd(const float* x, float* out, int32_t n, int32_t tokens, int32_t width, void* stream);
int uniir_meanpool_bwd(const float* dout, float* dx, int32_t n, int32_t tokens, int32_t width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [TOPK] exact brute-force inner-product top-k over an fp16 pool (FAISS "IDMap,Flat" + normalize_L2).
 *   uniir_pool_inv_norms: inv[i] = 1/sqrt(sum_j x[i][j]^2) in the oracle's summation order
 *                         (sequential fp32, no fma), 0 for an all-zero row (FAISS leaves it untouched).
 *   uniir_topk_coarse:    MFMA fp16 scan; per query a shortlist of uniir_topk_ncand(nq, kc) pool rows that is
 *                         guaranteed to contain the kc best by approximate score; kc >= k, kc <= 64.
 *   uniir_topk_rescore:   exact fp32 re-score of a shortlist in the oracle's summation order, sort by
 *                         (score desc, id asc), keep k.  exact_ws: nq*ncand floats of scratch.  A row may
 *                         appear at most once in a query's shortlist.
 * Layouts: pool fp16 [n][dim], queries fp16 [nq][dim] as stored by the embedder (un-normalised), ids
 * int64 [n].  dim % 32 == 0 for uniir_topk_coarse, dim % 8 == 0 for uniir_topk_rescore, dim % 64 == 0 for
 * uniir_topk_ip; n * dim * 2 < 2 GiB for the scans (UNIIR_ESHAPE otherwise); pool, queries and inverse norms
 * 16-byte aligned (UNIIR_EALIGN).  Outputs: cand_idx int32 [nq][ncand] pool-row indices (-1 = empty),
 * out_scores f32 [nq][k] descending, out_ids int64 [nq][k] (-1 padded like FAISS).
 * workspace: uniir_topk_workspace_bytes(nq, kc, rows) bytes, 16-byte aligned.
 * MASS TIES.  The scans keep one maximum per group of 16 rows and the selection keeps at most 2 (k + 8)
 * groups per query.  When more groups than that tie EXACTLY at the k-th best score (a zero query, whose
 * scores are all 0; a pool of identical rows), the tied groups kept are those of the lowest row index, so
 * the ids returned are the smallest among the rows of the kept groups, not the smallest of the whole pool
 * as an exhaustive (score desc, id asc) sort gives them.  The answer is still a valid one: the scores are
 * those of the exhaustive search at every rank, bit for bit, every (score, id) returned is the exact score
 * of that row, ids are distinct and ascend among equal scores.  Near-ties (scores that differ) and fewer
 * tied groups than 2 (k + 8) are ordered exactly (tests/topk_cases.py, tests/test_topk_paths_gpu.py).
 * ---------------------------------------------------------------------------------------------- */
int uniir_pool_inv_norms(const void* x_f16, int64_t n, int32_t dim, float* inv_norm, void* stream);
int64_t uniir_topk_workspace_bytes(int32_t nq, int32_t kc, int64_t rows);
/* candidates per query that uniir_topk_coarse writes into cand_idx (group path: 2*kc groups of 16 rows) */
int32_t uniir_topk_ncand(int32_t nq, int32_t kc);
int uniir_topk_coarse(const void* pool_f16, const float* pool_inv_norm, int64_t rows, int32_t dim,
                      const void* queries_f16, int32_t nq, int32_t kc, int32_t* cand_idx,
                      float* cand_score, void* workspace, int64_t workspace_bytes, void* stream);
int uniir_topk_rescore(const void* pool_f16, const float* pool_inv_norm, const int64_t* pool_ids,
                       int64_t rows, int32_t dim, const void* queries_f16, const float* query_inv_norm,
                       int32_t nq, const int32_t* cand_idx, int32_t ncand, int32_t k, float* exact_ws,
                       float* out_scores, int64_t* out_ids, void* stream);
/* The whole search of one pool shard in ONE call -- what the reference's FFI for this path would bind
 * (mbeir_retriever.py:188-232 search_index: faiss.normalize_L2(queries); index.search(queries, k)):
 * per chunk of <= 1024 queries one sweep of the shard (MFMA group-max scan: queries in registers and the pool streamed once for
 * <= 256 queries, GEMM-shaped above), then a fused group selection + query norm + exact re-score launch and the final sort.
 * k <= 56.  Candidates: behind the streaming / ping-pong scans every group whose maximum lies within the proven rounding bound of
 * the k-th best group maximum (GselBound, csrc/topk_select.h; at most 2 (k + 8) groups), not the fixed k + 8 groups of
 * uniir_topk_coarse -- the results are those of the exhaustive search either way (MASS TIES above excepted), bit for bit.
 * Which kernels a shape gets: the table of DESIGN.md "Top-k host layer"; uniir_topk_plan below answers for one shape.
 * rows * dim * 2 must stay below 2 GiB (UNIIR_ESHAPE otherwise: the shard is addressed through 31-bit buffer offsets); a larger
 * resident shard -- the whole 5.6 M x 768 M-BEIR pool on one GPU -- is searched as equal row ranges and merged with
 * uniir_topk_merge (uniir_amd/retrieval.py subshard_bounds), which is the search of the whole shard.
 * workspace: uniir_topk_ip_workspace_bytes_ex(nq, k, rows, dim) bytes (the exact requirement; the dim-agnostic form is an upper
 * bound over the sweep widths), 256-B aligned. */
int64_t uniir_topk_ip_workspace_bytes(int32_t nq, int32_t k, int64_t rows);
int64_t uniir_topk_ip_workspace_bytes_ex(int32_t nq, int32_t k, int64_t rows, int32_t dim);
int uniir_topk_ip(const void* pool_f16, const float* pool_inv_norm, const int64_t* pool_ids, int64_t rows,
                  int32_t dim, const void* queries_f16, int32_t nq, int32_t k, float* out_scores,
                  int64_t* out_ids, void* workspace, int64_t workspace_bytes, void* stream);
/* The same for ONE resident shard of any size (round 5) -- the whole 5.6 M x 768 M-BEIR pool on one GPU: equal logical sub-shards of
 * uniir_topk_subshard_rows(rows, dim) rows (a multiple of 32, below the 2-GiB buffer bound and within the fused tail's 786 432 rows;
 * = rows when the shard needs no cut), per sweep one scan launch per sub-shard, then ONE fused tail, ONE sort and ONE merge launch
 * for all of them; identical to the merge of per-sub-shard uniir_topk_ip searches, bit for bit.  pool_ids must be given (unique). */
int64_t uniir_topk_subshard_rows(int64_t rows, int32_t dim);
int64_t uniir_topk_ip_multi_workspace_bytes(int32_t nq, int32_t k, int64_t rows, int32_t dim);
int uniir_topk_ip_multi(const void* pool_f16, const float* pool_inv_norm, const int64_t* pool_ids, int64_t rows,
                        int32_t dim, const void* queries_f16, int32_t nq, int32_t k, float* out_scores,
                        int64_t* out_ids, void* workspace, int64_t workspace_bytes, void* stream);
/* queries per sweep inside uniir_topk_ip: 0 (default) = automatic -- 256 where the streaming scan applies (dim 768, >= 32768 rows,
 * shard < 2 GiB), else 1024 = the maximum.  Results never depend on it: the hook exists so that tests can drive the sweep loop with
 * small inputs, and for tuning.  Process-wide host setting.  uniir_topk_ip_sweep_queries: the value a search of this shape uses. */
int uniir_topk_set_chunk(int32_t queries_per_sweep);
int32_t uniir_topk_ip_sweep_queries(int32_t dim, int64_t rows);
/* What a uniir_topk_ip / uniir_topk_ip_multi search of (rows, dim, nq, k) launches on a device with ncu compute units, and the
 * scratch it uses: the library's own plan (csrc/topk.h TkPlan; the dispatch table it implements is DESIGN.md "Top-k host layer"),
 * read-only, no device needed.  New entry point only, found by its symbol.  A search runs full sweeps of sweep_queries queries and,
 * when nq is no multiple, one remainder sweep of rem_queries (0: none); a shard of >= 2 GiB runs them per sub-shard (the fields
 * then describe a FULL sub-shard; ask again with last_rows for the shorter last one) or, batched == 1, with one tail, one sort and
 * one merge launch per sweep for all sub-shards.  UNIIR_EINVAL: null / non-positive argument; UNIIR_ESHAPE: k > 56, dim % 64,
 * rows >= 2^31 (what the searches refuse). */
enum {                              /* scan: the group-max scan of a sweep */
    UNIIR_TK_SCAN_STREAM = 0,       /* topk_stream_kernel<dim / 32>: <= 64 queries in LDS, dim 768 | 512, small shards */
    UNIIR_TK_SCAN_STREAM2 = 1,      /* topk_stream2_kernel<dim / 32, 2>: <= 64 queries in registers, >= 2048 groups */
    UNIIR_TK_SCAN_SHARED2 = 2,      /* topk_stream5_kernel<2, 2>: 65 .. 128 queries, dim 768, >= 2048 groups */
    UNIIR_TK_SCAN_SHARED4 = 3,      /* topk_stream5_kernel<4, 2>: 129 .. 256 */
    UNIIR_TK_SCAN_PP_HALF = 4,      /* topk_gmax_pp_kernel<true, 2>: 65 .. 128 queries, dim % 64 == 0, dim >= 192 */
    UNIIR_TK_SCAN_PP_NT = 5,        /* topk_gmax_pp_kernel<false, 2>: 129 .. 256 */
    UNIIR_TK_SCAN_PP = 6,           /* topk_gmax_pp_kernel<false, 0>: 257 .. 1024 */
    UNIIR_TK_SCAN_GMAX = 7,         /* topk_gmax_kernel<2>: everything else */
    UNIIR_TK_SCAN_COARSE = 8        /* topk_coarse_kernel: uniir_topk_coarse with more than 1024 queries (never inside a search) */
};
enum { UNIIR_TK_TAIL_UNFUSED = 0,   /* tail: stand-alone selection (select = UNIIR_TK_SEL_*), query norms, uniir_topk_rescore */
       UNIIR_TK_TAIL_FUSED = 1 };   /* topk_tail_select_rescore_kernel<select, ..> (select = 4 | 2 | 1 workgroups per query) + sort */
enum {
    UNIIR_TK_SEL_1024_REG = 0,      /* topk_gsel_kernel<1024, true>: an even number of groups, <= 49 152 */
    UNIIR_TK_SEL_1024 = 1,          /* topk_gsel_kernel<1024, false>: <= 64 queries */
    UNIIR_TK_SEL_256 = 2,           /* topk_gsel_kernel<256> */
    UNIIR_TK_SEL_MERGE_PARTIAL = 3  /* topk_merge_partial_kernel, behind UNIIR_TK_SCAN_COARSE */
};
typedef struct {
    int64_t scan, waves, tail, select;                                  /* a full sweep; waves: wave maxima written by the scan (0: none) */
    int64_t rem_queries, rem_scan, rem_waves, rem_tail, rem_select;     /* the remainder sweep */
    int64_t sweep_queries, ncand;                                       /* ncand: shortlist entries per query */
    int64_t nsub, batched, subshard_rows, last_rows;
    int64_t workspace_bytes;                                            /* = uniir_topk_ip_multi_workspace_bytes */
    /* regions (batched: of all sub-shards): group [+ wave] maxima, wave maxima where they have a region of their own, query
     * inverse norms, candidate rows, exact scores, the sub-shards' k-lists (scores and ids) */
    int64_t gmax_bytes, wmax_bytes, qinv_bytes, cand_bytes, exact_bytes, lists_bytes;
} uniir_topk_plan_t;
int uniir_topk_plan(int64_t rows, int32_t dim, int32_t nq, int32_t k, int32_t ncu, uniir_topk_plan_t* out);
/* The same search over an fp32 pool (an extraction with use_fp16 = False kept as fp32 rows: UNIIR_POOL_FP32).  New entry points only,
 * found by their symbols.  The arithmetic is that of uniir_topk_ip with fp32 inputs where it converts fp16 to fp32: inverse norms
 * (float)(1.0 / (double)sqrtf(s)), s the sequential fp32 sum of squares without fma, 0 when s is not > 0; query and row elements
 * scaled by them and rounded to fp32; score s = s + qn[j] * xn[j] sequentially without fma; order (score desc, id asc), missing
 * results (-inf, -1).  Bit for bit for finite inputs in the normal range.
 *   uniir_pool_inv_norms_f32: dim % 4 == 0, x 16-byte aligned.
 *   uniir_topk_ip_f32: k <= 56, dim % 64 == 0, rows * dim * 4 < 2 GiB (UNIIR_ESHAPE otherwise, before anything is launched; a larger
 *     shard is searched as the row ranges of retrieval.subshard_bounds(n, dim, 4) and merged with uniir_topk_merge); pool, queries
 *     and inverse norms 16-byte, workspace 256-byte aligned (UNIIR_EALIGN); workspace of uniir_topk_ip_f32_workspace_bytes (0 for
 *     nq == 0 or k == 0).  Sweeps of <= 1024 queries, or of uniir_topk_set_chunk's value. */
int uniir_pool_inv_norms_f32(const float* x, int64_t n, int32_t dim, float* inv_norm, void* stream);
int64_t uniir_topk_ip_f32_workspace_bytes(int32_t nq, int32_t k, int64_t rows, int32_t dim);
int uniir_topk_ip_f32(const float* pool_f32, const float* pool_inv_norm, const int64_t* pool_ids, int64_t rows, int32_t dim,
                      const float* queries_f32, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* k-way merge of per-shard results (score desc, id asc): in [nshard][nq][k] -> out [nq][k] */
int uniir_topk_merge(const float* scores, const int64_t* ids, int32_t nshard, int32_t nq, int32_t k,
                     float* out_scores, int64_t* out_ids, void* stream);
/* the same for lists of k_in entries per shard merged into the k_out best (k_out may exceed k_in) */
int uniir_topk_merge_ex(const float* scores, const int64_t* ids, int32_t nshard, int32_t nq, int32_t k_in,
                        int32_t k_out, float* out_scores, int64_t* out_ids, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [IMAGE] device-side image transform (input pipeline).  Replaces, for a decoded RGB uint8
 * image [h][w][3] already in HBM, the CPU chain of upstream clip._transform (preprocess returned by clip.load, used at
 * src/models/uniir_clip/clip_scorefusion/clip_sf.py:25-26 and applied in src/data/mbeir_dataset.py:92-100) and of BLIP's
 * eval transform (src/models/uniir_blip/backbone/transform/blip_transform.py:41-48):
 *   PIL resize to (oh, ow) with BICUBIC -> crop rows [top, top+n) x columns [left, left+n) -> x / 255 ->
 *   (v - mean[c]) / std[c] -> out fp32 [3][n][n].
 * The resize is bit-exact with Pillow's 8-bit resample; mean3 / std3 are HOST pointers to 3 floats (read at call time).
 * (oh, ow, top, left) are the caller's geometry (torchvision Resize + CenterCrop: short side n, long side
 * int(n * long / short), offsets round-half-even((size - n) / 2); BLIP: oh = ow = n, no crop).
 * ---------------------------------------------------------------------------------------------- */
int64_t uniir_image_workspace_bytes(int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t n);
int uniir_image_preprocess(const void* rgb_u8, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t top, int32_t left,
                           int32_t n, const float* mean3, const float* std3, float* out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Batched form: one table of per-image geometry, a constant number of launches per batch (three kernels, whatever `count`).
 * All images sit in ONE packed uint8 buffer; image i is RGB [h][w][3] at byte `offset` (a multiple of 16).  Per image:
 *   crop the source box (box_left, box_top, box_w, box_h) -> PIL resize of the BOX to (oh, ow) with BICUBIC -> rows
 *   [top, top+n) x columns [left, left+n) of the resized box -> mirror the n kept columns when flip -> x / 255 ->
 *   (v - mean[c]) / std[c] -> out[out_index] fp32 [3][n][n].
 * This is Pillow's image.crop(box).resize((ow, oh), BICUBIC): the resample windows are clamped at the BOX edges, never
 * reading pixels outside it (Image.resize(box=...) does read them and gives other bytes).  A pass is skipped when its
 * axis keeps its size (box_w == ow / box_h == oh), as Pillow and uniir_image_preprocess do.  Both older chains are
 * special cases: CLIP = whole-image box + Resize / CenterCrop geometry, flip 0; BLIP eval = whole-image box, oh = ow = n;
 * BLIP train = the RandomResizedCrop box, oh = ow = n, the drawn flip.
 *
 * uniir_image_batch_plan is HOST-ONLY arithmetic (no HIP call): it validates the host copy of the table, fills one
 * uniir_image_plan per image and the batch summary.  Errors: null pointers, non-positive sizes, a flip other than 0 / 1, an
 * offset that is negative or no multiple of 16, out_index outside [0, out_items), two descriptors with one out_index ->
 * UNIIR_EINVAL; box outside the image, window outside (oh, ow), image bytes outside [0, packed_bytes) -> UNIIR_ESHAPE; a
 * box whose touched row segment exceeds the staging buffer of the horizontal pass (16384 pixels) -> UNIIR_EUNSUPPORTED.
 * count == 0 is valid (workspace_bytes 0).
 *
 * uniir_image_preprocess_batch takes DEVICE copies of the pixels and of both tables, and the HOST summary `info` of the plan
 * call that produced the plan table; it trusts them.  It checks only its own arguments: null pointers, workspace smaller
 * than info->workspace_bytes or not 256-byte aligned -> UNIIR_EINVAL.  It allocates nothing, copies nothing and never
 * synchronises; slots of `out` that no descriptor names are left untouched; info->count == 0 returns UNIIR_OK without a
 * launch.  mean3 / std3 are HOST pointers to 3 floats. */
typedef struct uniir_image_desc {
    int64_t offset;                             /* byte offset of the image in the packed buffer, multiple of 16 */
    int32_t h, w;                               /* image size */
    int32_t box_left, box_top, box_w, box_h;    /* source box inside the image */
    int32_t oh, ow;                             /* size the box is resized to */
    int32_t top, left;                          /* n x n window inside (oh, ow) */
    int32_t flip;                               /* 1: mirror the kept columns */
    int32_t out_index;                          /* [3][n][n] slot of `out` */
} uniir_image_desc;
typedef struct uniir_image_plan {
    int64_t bx_off, by_off;     /* workspace byte offsets: (first, count) window bounds per kept column / row, int32 [n][2] */
    int64_t cx_off, cy_off;     /* 22-bit fixed-point weights, int32 [n][kx] / [n][ky] */
    int64_t tmp_off;            /* horizontal-pass result, uint8 [rows][n][3] */
    int32_t kx, ky;             /* window capacity per axis (Pillow's ksize); 0 for a skipped pass */
    int32_t y0, rows;           /* box rows [y0, y0 + rows) that the vertical windows of the kept rows touch */
    int32_t x0, cols;           /* box columns [x0, x0 + cols) that the horizontal windows of the kept columns touch */
} uniir_image_plan;
typedef struct uniir_image_batch_info {
    int64_t workspace_bytes;    /* what uniir_image_preprocess_batch needs, 256-byte aligned */
    int32_t count, n, out_items;
    int32_t max_rows;           /* largest plan.rows: the row extent of the horizontal pass's grid */
    int32_t launches;           /* kernel launches of the batched call for this batch: the same for every count >= 1 */
    int32_t reserved;
} uniir_image_batch_info;
int uniir_image_batch_plan(const uniir_image_desc* descs, int32_t count, int32_t n, int32_t out_items, int64_t packed_bytes,
                           uniir_image_plan* plans, uniir_image_batch_info* info);
int uniir_image_preprocess_batch(const void* packed_u8, const uniir_image_desc* descs, const uniir_image_plan* plans,
                                 const uniir_image_batch_info* info, const float* mean3, const float* std3, float* out,
                                 void* workspace, int64_t workspace_bytes, void* stream);

/* Train-time augmentation on the device: the ten ops of BLIP's RandomAugment(2, 5) (upstream backbone/transform/randaugment.py,
 * blip_transform.py:11-40) on RGB uint8 images [n][n][3], between the flip and ToTensor.  The DRAW stays on the host
 * (uniir_amd/randaugment.py: the reference's np.random calls); the device gets one uniir_image_aug record per image: up to
 * UNIIR_AUG_MAX_SLOTS ops applied in order, each an op code and the parameters the host prepared for it.
 *   table ops, per channel, a 256-entry table from the channel's histogram (lo / hi = smallest / largest value present):
 *     AUTOCONTRAST      fp64, no fused multiply-add: scale = 255 / (hi - lo), off = ((256 - lo) % 256) * scale (the reference negates
 *                       a uint8: only lo == 0 stretches as intended), t[i] = trunc(clip(i * scale + off, 0, 255)); hi <= lo: unchanged
 *     AUTOCONTRAST_PIL  the same with off = -lo * scale (PIL.ImageOps.autocontrast); never drawn unless the caller asks
 *     EQUALIZE          integers: step = (pixels outside the last nonzero bin) / 255; t[i] = min((step / 2 + sum of the bins
 *                       below i) / step, 255); step == 0: unchanged
 *     BRIGHTNESS        t[i] = trunc(clip(float(i) * float(factor), 0, 255)), no histogram
 *   SHARPNESS           factor 1: the input.  Else d = the 3x3 filter (1 1 1 / 1 5 1 / 1 1 1) / 13 in fp32 (taps added in row-major
 *                       order, reflect-101 border, half-even, saturated); factor 0: d; else the interior [1, n-1) becomes
 *                       int32(trunc(d + float(factor) * (x - d))) & 255, the border rows and columns keep the input
 *   SHEAR_X / SHEAR_Y / TRANSLATE_X / TRANSLATE_Y / ROTATE: the forward matrix ([[1, f, 0], [0, 1, 0]], [[1, 0, 0], [f, 1, 0]],
 *                       [[1, 0, -o], [0, 1, 0]], [[1, 0, 0], [0, 1, -o]] with f, o rounded to fp32; rotation by the angle in degrees
 *                       about (n / 2, n / 2): [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]], a = cos, b = sin) is inverted
 *                       in fp64 by uniir_image_aug_plan; for destination (x, y):
 *                         X = (rint((m01 * y + m02) * 1024) + 16 + rint(m00 * x * 1024)) >> 5, Y likewise with m11, m12, m10;
 *                       source cell (X >> 5, Y >> 5), fractions (X & 31, Y & 31) / 32, four weights (32 - fy)(32 - fx) * 32 ... of sum
 *                       32768, result (sum p * w + 16384) >> 15; a source pixel outside the image counts as 128.
 * (DESIGN.md section 3 has the definition in full; tests/randaugment_ref.py restates it in numpy.)
 *
 * uniir_image_aug_plan is HOST-ONLY (no HIP call): ops / args are [count][slots] (arg = the enhance factor, the shear factor, the
 * translate offset in pixels, the angle in degrees; ignored by the other ops); it fills table[count] and the summary.  Errors:
 * null pointer, count < 0, n <= 0, slots outside [0, UNIIR_AUG_MAX_SLOTS], an unknown op code, a non-finite argument ->
 * UNIIR_EINVAL; n above 2048 or an argument above 1e6 in magnitude -> UNIIR_EUNSUPPORTED.  info->launches is 2 * slots for any
 * count >= 1 (per slot: one statistics launch -- histograms in LDS, one workgroup per image whose op needs them -- and one
 * apply launch over all pixels), info->launches_preprocess = 3 + 2 * slots + 1.
 *
 * uniir_image_augment_batch: the op kernels alone.  in_u8 / out_u8 are DEVICE uint8 [count][n][n][3] (different buffers), table the
 * DEVICE copy, info the HOST summary; workspace >= info->workspace_bytes, 256-byte aligned.  Allocates nothing, never
 * synchronises.  slots == 0 copies.
 *
 * uniir_image_preprocess_batch_aug: uniir_image_preprocess_batch with the table between the flip and ToTensor: resize to uint8, the
 * slots, then x / 255 -> (v - mean) / std -> out[out_index].  aug[i] belongs to descs[i].  workspace >= info->workspace_bytes +
 * aug_info->workspace_bytes.  With an all-Identity table the output equals uniir_image_preprocess_batch's bit for bit. */
#define UNIIR_AUG_MAX_SLOTS 4
enum {
    UNIIR_AUG_IDENTITY = 0, UNIIR_AUG_AUTOCONTRAST = 1, UNIIR_AUG_EQUALIZE = 2, UNIIR_AUG_BRIGHTNESS = 3, UNIIR_AUG_SHARPNESS = 4,
    UNIIR_AUG_SHEAR_X = 5, UNIIR_AUG_SHEAR_Y = 6, UNIIR_AUG_TRANSLATE_X = 7, UNIIR_AUG_TRANSLATE_Y = 8, UNIIR_AUG_ROTATE = 9,
    UNIIR_AUG_AUTOCONTRAST_PIL = 10, UNIIR_AUG_OPS = 11
};
typedef struct uniir_image_aug_slot {
    int32_t op, reserved;
    double p[6];                /* warps: the inverse matrix m00 m01 m02 m10 m11 m12; enhance ops: p[0] = factor */
} uniir_image_aug_slot;
typedef struct uniir_image_aug {
    uniir_image_aug_slot slot[UNIIR_AUG_MAX_SLOTS];
} uniir_image_aug;
typedef struct uniir_image_aug_info {
    int64_t workspace_bytes;    /* two uint8 [count][n][n][3] buffers + the tables, 256-byte aligned */
    int32_t count, n, slots;
    int32_t launches;           /* of uniir_image_augment_batch: the same for every count >= 1 */
    int32_t launches_preprocess;    /* of uniir_image_preprocess_batch_aug */
    int32_t reserved;
} uniir_image_aug_info;
int uniir_image_aug_plan(const int32_t* ops, const double* args, int32_t count, int32_t slots, int32_t n, uniir_image_aug* table,
                         uniir_image_aug_info* info);
int uniir_image_augment_batch(const void* in_u8, const uniir_image_aug* table, const uniir_image_aug_info* info, void* out_u8,
                              void* workspace, int64_t workspace_bytes, void* stream);
int uniir_image_preprocess_batch_aug(const void* packed_u8, const uniir_image_desc* descs, const uniir_image_plan* plans,
                                     const uniir_image_batch_info* info, const uniir_image_aug* aug,
                                     const uniir_image_aug_info* aug_info, const float* mean3, const float* std3, float* out,
                                     void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIIR_HIP_H */
