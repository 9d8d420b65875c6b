/*
 * mjv.h - C ABI of libmjv_hip.so: the MI355X (gfx950) kernels under the MJ-VIDEO reward-scoring path.
 *
 * The reference (aiming-lab/MJ-Video) has no FFI: its boundary is the Python class API
 * (scripts/model/moe_reward.py:137-297).  This library sits UNDER the Python mirror of that API
 * (mj-video_amd/modeling.py) and replaces the PyTorch/cuBLAS/flash-attn ops the reference's forward
 * reaches.  Every entry point cites the reference code it replaces (paths relative to
 * /root/reference/scripts/model).
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers borrowed from the caller (PyTorch tensors); the library
 *     allocates nothing; the caller keeps buffers alive until the stream has been synchronised;
 *   - bf16 tensors are passed as `const uint16_t*` (raw bf16 bit patterns), row-major, with an explicit
 *     leading dimension in ELEMENTS;
 *   - every call only ENQUEUES on `stream` (a hipStream_t passed as void*; 0 = null stream) and never
 *     synchronises; the library keeps no setting between calls (ABI 4: what a caller may choose - the tile kernel of a
 *     GEMM, the attention kernel - travels in the call's descriptor; there is no process-wide setter), so calls from
 *     different threads on different streams do not interact; the only shared state is the opt-in profiler (mutex);
 *     the measurement switches of earlier ABI versions live in the separate bench build (include/mjv_bench.h);
 *   - return value 0 = ok, negative = error (MJV_E_*); `mjv_last_error()` gives a thread-local message.
 *   - rounding points follow the reference's bf16 eager path (bf16 result after every torch op), with ONE stated exception:
 *     attention's score_round_mode 2 keeps the scores in fp32 up to the softmax, as the reference's flash-attention path does
 *     on a GPU (modeling_intern_vit.py:229-244, modeling_internlm2.py:437-561).  Modes 0 / 1 are the eager rounding points;
 *     the Python model's DEFAULT is mode 2 (model.attention_scores = "flash"; "eager" selects 0 / 1; DESIGN 4 "Attention,
 *     round 4" holds the fixtures' verdict on the two).
 *
 * ABI 5 adds the MX-fp8 operand format for the GEMMs (BASELINE configs[4]; opt-in, the default path
 * is bf16 as before): the `*_format` / `*_scales` fields at the END of the GEMM descriptor - all zero = bf16 everywhere -,
 * mjv_quantize_mxfp8, mjv_layernorm_mxfp8, mjv_rmsnorm_mxfp8.
 * ABI 6 adds, at the END of the attention descriptor (all zero = ABI 5): suffix queries (cu_seqlens_q) and a shared key / value
 * prefix (prefix_k / prefix_v) for causal launches - the two pieces of work a scorer can leave out of the language tower - and
 * lets MJV_EPI_ROPE_QKV run with rope_group 0 (a k | v projection without q heads).
 * ABI 7 adds what the Phi-3-mini language tower of BASELINE configs[4] needs beyond the InternLM2 one: head_dim 96 in
 * mjv_attention_bf16 and mjv_rope_heads_bf16 (rotary embedding in place on a [q | k | v] projection).
 * ABI 7, additive (MJV_ABI_VERSION stays 7: nothing existing changes): mjv_attention_ctx_bf16 with its plan / workspace queries -
 * causal attention of few own rows per sequence over long key / value contexts that many sequences share (the caption pass of
 * model.score_captions).
 * ABI 7, additive (MJV_ABI_VERSION stays 7, no new symbol): one field at the END of mjv_attn_ctx_desc, ctx_any_length - 0 = as
 * before (a context is a positive multiple of 64 keys), 1 = a context may end at any key, so a caller can cache the whole
 * prefix that the captions of a video share.
 * ABI 7, additive (MJV_ABI_VERSION stays 7): mjv_gemm_plan - the launches mjv_gemm_bf16 makes for a descriptor, readable without
 * a GPU and for any number of compute units.
 * ABI 7, additive (MJV_ABI_VERSION stays 7; mjv_attn_ctx_desc is untouched): mjv_attn_ctx_segments with mjv_attention_ctx_seg_plan /
 * _seg_workspace_bytes / _seg_bf16 - a context of the caption pass may be the concatenation of several row ranges that live in
 * different tensors, and contexts may share ranges (a video that grows frame by frame, one video under several instructions).
 * ABI 7, additive (MJV_ABI_VERSION stays 7): mjv_attn_readout_desc with mjv_attention_readout_plan / mjv_attention_readout_bf16 -
 * the softmax mass of a few query rows per bin of key positions (which frames the reward rows attend to), fp32.
 */
#ifndef MJV_H_
#define MJV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJV_ABI_VERSION 7

enum {
  MJV_OK = 0,
  MJV_E_ARG = -1,     /* bad argument (shape/alignment/null) */
  MJV_E_LAUNCH = -2,  /* HIP launch error */
  MJV_E_UNSUPPORTED = -3
};

typedef uint16_t mjv_bf16;

/* ---------------------------------------------------------------------------------------------
 * MXFP8 operand format (OCP Microscaling v1.0 "MXFP8 E4M3": 32-element blocks along K with one shared power-of-two
 * scale; the format gfx950's v_mfma_scale_f32_16x16x128_f8f6f4 consumes).  The reference has no fp8 path (its README
 * names only the 2B bf16 checkpoint; BASELINE configs[4] asks for an fp8 MFMA weight path): this is a definition, pinned by
 * oracle/ref_fp8.py, not a restatement.
 *   elements : uint8 OCP e4m3fn, row-major [rows][ld] (K contiguous), K % 128 == 0, ld % 16 == 0
 *   scales   : uint8 e8m0 (value 2^(b - 127)), one per (row, 32-element block).  For a block of bf16 values with largest
 *              magnitude amax (bf16 bits u = E:8 | m:7):  b = max(1, E - 8 + (m > 0x60));  the smallest power of two with
 *              amax / 2^(b-127) <= 448, so no element saturates;  element = e4m3_rne(x / 2^(b-127)).
 *   scale layout ("lane layout" of the MFMA's scale operand): byte offset of (row, block kb of K-tile kt = k / 128)
 *              = ((kt * groups + row / 64) * 256) + (row % 16) * 16 + kb * 4 + (row / 16) % 4,   groups = ceil(rows / 64);
 *              i.e. per K-tile and 64-row group one 256-byte record whose dword [row % 16][kb] holds the four 16-row
 *              fragments' bytes - the dword a lane hands to the MFMA with op_sel = fragment.  mjv_mxfp8_scale_bytes().
 * ------------------------------------------------------------------------------------------- */
enum mjv_format { MJV_FMT_BF16 = 0, MJV_FMT_MXFP8 = 1 };
int64_t mjv_mxfp8_scale_bytes(int64_t rows, int64_t cols);
/* bf16 [rows][ldx] -> MXFP8 elements [rows][ldy] + scales (weights once at load; tests).  cols % 128 == 0. */
int mjv_quantize_mxfp8(const uint16_t* x, int64_t ldx, uint8_t* y, int64_t ldy, uint8_t* scales, int32_t rows, int32_t cols,
                       void* stream);

int mjv_abi_version(void);
const char* mjv_last_error(void);
/* name of the device architecture the code object was built for ("gfx950") */
const char* mjv_arch(void);

/* ---------------------------------------------------------------------------------------------
 * GEMM:  C[M,N] = epilogue( A[M,K] @ W[N,K]^T )      (torch.nn.Linear layout: W is [out, in])
 * replaces every nn.Linear / Conv2d-as-GEMM on the path:
 *   internvl2/modeling_intern_vit.py:145-147,164 (patch embed), :196,208 (qkv, proj), :256-257 (fc1, fc2)
 *   internvl2/modeling_internvl_chat.py:135-140 (mlp1)
 *   internvl2/modeling_internlm2.py:301-307 (wqkv, wo), :256-258 (w1, w3, w2)
 *   moe_reward.py:24-26 (gating hidden layers)
 * Requirements: K % 64 == 0, N % 8 == 0, lda/ldw/ldc/ldr % 8 == 0, 16-byte aligned base pointers (A, W, C, res; bias and
 * scale: 8-byte aligned) - checked for every kernel family before anything is launched (MJV_E_ARG).
 * ------------------------------------------------------------------------------------------- */
enum mjv_epilogue {
  MJV_EPI_BIAS = 0,       /* C = bf16(acc + bias)                       bias may be NULL            */
  MJV_EPI_BIAS_GELU = 1,  /* C = bf16(gelu_erf(bf16(acc + bias)))       (F.gelu on the bf16 Linear)  */
  MJV_EPI_BIAS_RELU = 2,  /* C = bf16(max(acc + bias, 0))                                           */
  MJV_EPI_SCALE_RES = 3,  /* v = bf16(acc + bias); if scale: v = bf16(v * scale[n]); C = bf16(res + v) */
  MJV_EPI_SILU_MUL = 4,   /* W rows interleaved [16 x w1 | 16 x w3]...; C[M,N/2] =
                             bf16( bf16(silu(bf16(acc_w1))) * bf16(acc_w3) )   (modeling_internlm2.py:262) */
  MJV_EPI_ROPE_QKV = 5    /* InternLM2 wqkv (modeling_internlm2.py:359-381): columns are kv groups of (rope_group + 2) heads
                             of 128 = [q heads of the group | k | v].  v = bf16(acc) goes to C (its own columns, the other
                             columns of C are left untouched); the q and k heads get the rotary embedding on the bf16 Linear
                             output, out = bf16(bf16(x cos) + bf16(rotate_half(x) sin)) with cos / sin rows taken at
                             rope_pos[m], and go de-interleaved to rope_q [M][heads * 128] / rope_k [M][kv_heads * 128].
                             Needs N % ((rope_group + 2) * 128) == 0, no bias. */
};

typedef struct mjv_gemm_desc {
  const mjv_bf16* A; int64_t lda;   /* activations [M][lda] */
  const mjv_bf16* W; int64_t ldw;   /* weights     [N][ldw] */
  mjv_bf16* C; int64_t ldc;         /* output rows            */
  int32_t M, N, K;
  int32_t epilogue;                 /* enum mjv_epilogue */
  const mjv_bf16* bias;             /* [N] or NULL */
  const mjv_bf16* scale;            /* [N] or NULL (LayerScale ls1/ls2, modeling_intern_vit.py:291,293) */
  const mjv_bf16* res; int64_t ldr; /* residual rows or NULL */
  int32_t res_mod, res_off;         /* res_mod > 0: residual row = res_off + (m % res_mod)   (pos-emb add) */
  int32_t out_group, out_pad;       /* out_group > 0: out row = (m / out_group) * (out_group + out_pad) + out_pad
                                       + m % out_group   (skip the CLS slot of every tile)               */
  const int32_t* out_rows;          /* optional explicit output row per m (splice into <IMG_CONTEXT> rows,
                                       modeling_internvl_chat.py:176-179); overrides out_group            */
  void* workspace;                  /* optional scratch (device, 16-B aligned) private to this stream while the call is in
                                       flight; lets under-filled launches split K (fp32 partial tiles, summed in a fixed
                                       order: results stay deterministic).  NULL: never split.  mjv_gemm_workspace_bytes() */
  int64_t workspace_bytes;
  int32_t tile;                     /* 0 = automatic (256x256 8-wave kernel for M >= 512 and N >= 256; else the 64x32 skinny
                                       kernel up to 128 rows, 128x128 above); 64 / 128 / 256 force one kernel - every choice
                                       computes the same roundings, only the fp32 summation order differs (the parity tests
                                       run every case on all three) */
  /* MJV_EPI_ROPE_QKV only */
  const mjv_bf16 *rope_cos, *rope_sin;   /* [positions][128] tables (bf16, modeling_internlm2.py:147-180) */
  const int32_t* rope_pos;               /* [M] position of every row (device) */
  mjv_bf16 *rope_q, *rope_k;             /* outputs */
  int64_t rope_ldq, rope_ldk;
  int32_t rope_group;                    /* q heads per kv head; 0 (ABI 6) = columns are [k | v] pairs only, rope_q unused */
  /* ---- ABI 5: operand / output formats (enum mjv_format; all zero = bf16 everywhere, the ABI-4 behaviour) ----
   * a_format == w_format == MJV_FMT_MXFP8: A and W point to e4m3 bytes (lda / ldw in BYTES = elements), a_scales / w_scales
   * to their scale records (layout above; groups = ceil(M / 64) and ceil(N / 64)); K % 128 == 0; the product of the
   * dequantised operands is accumulated in fp32 by v_mfma_scale_f32_16x16x128_f8f6f4 and the epilogue is the bf16 one.
   * Epilogues: BIAS, BIAS_GELU, BIAS_RELU, SCALE_RES, SILU_MUL (plain output rows only; no ROPE_QKV).
   * c_format == MJV_FMT_MXFP8 (BIAS, BIAS_GELU, BIAS_RELU, SILU_MUL): the epilogue's bf16 result is block-quantised on
   * the way out - C points to e4m3 bytes (ldc in bytes), c_scales to its scale records (groups = ceil(M / 64)); output
   * width (N, or N / 2 for SILU_MUL) % 128 == 0.  Bit-identical to the bf16 output followed by mjv_quantize_mxfp8. */
  int32_t a_format, w_format, c_format;
  const uint8_t *a_scales, *w_scales;
  uint8_t* c_scales;
  /* ---- ABI 5: a norm folded into this GEMM (north_star "RMSNorm / LayerNorm -> GEMM fusion"; bf16 operands) ----
   * The Linear's value before its bf16 rounding becomes   row_scale[m] * acc - row_shift[m] * col_shift[n] + bias_f32[n]
   * (row_shift / col_shift / bias_f32 all NULL: row_scale[m] * acc + bias[n]).  With A = the UN-normalised rows x and
   * W' = W * gain (folded once), row_scale = rstd, row_shift = mean * rstd, col_shift[n] = sum_k W'[n][k],
   * bias_f32 = bias + W beta this is Linear(LayerNorm(x)) (modeling_intern_vit.py:291-293) / Linear(RMSNorm(x))
   * (modeling_internlm2.py:138-143,653,669) without the normalised rows ever reaching HBM; mjv_row_stats_bf16 writes the two
   * row vectors.  Rounding points DIFFER from the reference's (no bf16 rounding of the normalised rows, the gain rounded into
   * W'): opt-in, behind model.norm_fusion, judged by the fixtures (DESIGN "Norm fusion, round 4").
   * fp32 vectors, 16-byte aligned; row vectors readable up to ceil(M / 256) * 256 entries, column vectors up to
   * ceil(N / 256) * 256 (the 256-tile kernel fetches whole tiles of them by LDS-DMA).  Not with MJV_EPI_SCALE_RES.  The
   * 256-tile kernel instantiates BIAS / BIAS_GELU with a folded LayerNorm and SILU_MUL / ROPE_QKV with a folded RMSNorm (the
   * model's four call sites); every other combination runs on the small-tile kernels or returns MJV_E_UNSUPPORTED. */
  const float *row_scale, *row_shift, *col_shift, *bias_f32;
} mjv_gemm_desc;

/* a workspace of this size is enough for every problem shape (256 partial 256x256 fp32 tiles = 64 MiB) */
int64_t mjv_gemm_workspace_bytes(void);

int mjv_gemm_bf16(const mjv_gemm_desc* d, void* stream);

/* ABI 7, additive.  Writes the launches mjv_gemm_bf16 would make for *d (bf16 or MXFP8 operands; the descriptor is checked as
 * there, nothing it points to is read) on a device with `cus` compute units (cus <= 0: the current device).  Touches no device
 * memory, launches nothing.  Returns the number of int32 written (or needed, when out == NULL), or a negative error code.
 *   out[0 .. 3]          {n_launches (1 or 2), gm (group-M of the 256-tile order), nt_store (1 = streaming output stores), 0}
 *   out[4 + 8 i .. + 7]  launch i, in stream order; the launches' rows partition [0, M), a first of two has rows % 256 == 0:
 *     [0] family           64 = 64 x 32 skinny kernel, 128 = 128 x 128, 256 = 256 x 256 (bf16 and MXFP8), 2 = tile code 2
 *     [1] epilogue         the one this launch runs (MJV_EPI_BIAS where rows of a ROPE_QKV problem take the fallback, see [7])
 *     [2] row0, [3] rows
 *     [4] split            K slices per tile through the workspace (1 = none; > 1: the slice kernel and its finish kernel)
 *     [5] grid             workgroups of the main kernel
 *     [6] persistent       1 = the persistent 256-tile kernel (grid == cus workgroups walk the tiles)
 *     [7] rope_split_after 1 = the launch stores the un-rotated Linear where the fused epilogue puts its result (v heads to C,
 *                            q / k heads to rope_q / rope_k; the other columns of C untouched) and the rotary step follows in
 *                            place on its rows of rope_q / rope_k (profiler tag rope_split) */
int64_t mjv_gemm_plan(const mjv_gemm_desc* d, int32_t cus, int32_t* out, int64_t out_ints);

/* ---------------------------------------------------------------------------------------------
 * Flash-style attention over packed variable-length sequences (no N x N scores in HBM).
 *   non-causal D=64 : internvl2/modeling_intern_vit.py:210-227 (_naive_attn) / :229-244 (_flash_attn)
 *   causal GQA D=128: internvl2/modeling_internlm2.py:383-411 (eager) / :437-561 (flash varlen)
 * Q/K/V/O are addressed as base + row * ld + head * head_stride (elements); K/V head = q_head / kv_group.
 * Alignment: Q, K, V, O 16-byte aligned; ldq / ldk / ldv / ldo and the four head strides multiples of 8 elements (every
 * kernel moves 16-byte pieces of a row; O included since round 4).
 * score rounding: mode 0: s = bf16(acc * scale)   [(q*scale) @ k^T with scale a power of two]
 *                 mode 1: s = bf16(bf16(acc) * scale)   [matmul, then / sqrt(D) in bf16]
 *                 mode 2: s = acc * scale in fp32, never rounded   [the reference's flash-attention numerics, the path it takes on
 *                         a GPU: modeling_intern_vit.py:229-244, modeling_internlm2.py:437-561; kernel 0 / 6 / 7 only]
 * ------------------------------------------------------------------------------------------- */
typedef struct mjv_attn_desc {
  const mjv_bf16 *Q, *K, *V;
  mjv_bf16* O;
  int64_t ldq, ldk, ldv, ldo;
  int32_t q_head_stride, k_head_stride, v_head_stride, o_head_stride;
  const int32_t* cu_seqlens;  /* [n_seqs + 1] packed row offsets (device) */
  int32_t n_seqs, max_seqlen;
  int32_t n_heads, kv_group;
  int32_t head_dim;           /* 64, 128, or (ABI 7; kernel 0 / 7 only) 96 - Phi-3-mini's heads: dense 192-byte K / V rows in LDS */
  int32_t causal;
  float scale;
  int32_t score_round_mode;
  int32_t kernel;             /* 0 = automatic (round 3: the two-sub-block pipelined kernel); 4 = the register-staged round-1
                                 kernel for every shape;
                                 5 = the round-2 choice (its LDS-DMA form up to 4096 keys); 6 / 7 = the round-3 kernel with two /
                                 four waves (128 / 256 queries at head_dim 64; 128 at 128) per workgroup (automatic = four;
                                 bit-identical results).  6 exists at head_dim 64 only: at 128 a workgroup stages 64 KiB of
                                 K / V, two fit a CU, and a two-wave block would run one wave per SIMD - MJV_E_UNSUPPORTED.
                                 Every accepted choice gives correct results: the tests A/B them.  Other values: MJV_E_ARG */
  /* ---- ABI 6 (all zero = the ABI-5 behaviour): what a SCORER may leave out of a causal tower (kernel 0 / 6 / 7, causal only;
   * otherwise MJV_E_UNSUPPORTED).  The reward heads read two late rows per sample (moe_reward.py:226-243) and every prompt
   * starts with the same system tokens (conversation.py:354-365, eval_genai_mjvideo.py:132-137):
   *   cu_seqlens_q / max_seqlen_q : the queries of sequence s are only its LAST cu_seqlens_q[s+1] - cu_seqlens_q[s] positions,
   *       packed at those rows of Q and O (cu_seqlens still describes the K / V rows); local query i sits at key position
   *       prefix_len + keys(s) - queries(s) + i.  max_seqlen_q >= the longest query count.
   *   prefix_k / prefix_v / prefix_len : prefix_len keys SHARED by every sequence precede its own: rows of prefix_k / prefix_v
   *       [prefix_len][ldk / ldv] with K's / V's head strides (a cache of the constant prompt prefix's keys / values);
   *       prefix_len % 64 == 0.  Key j < prefix_len comes from the prefix rows, key j >= prefix_len from row j - prefix_len
   *       of the sequence.  Same arithmetic, same key-tile boundaries as one launch over the concatenated rows. */
  const int32_t* cu_seqlens_q;
  int32_t max_seqlen_q;
  int32_t prefix_len;
  const mjv_bf16 *prefix_k, *prefix_v;
} mjv_attn_desc;

int mjv_attention_bf16(const mjv_attn_desc* d, void* stream);
/* max_seqlen MUST be >= the longest sequence of cu_seqlens: query rows beyond it are not computed (their O rows are left
 * untouched). */

/* ---------------------------------------------------------------------------------------------
 * ABI 7, additive - caption-pass attention: every sequence has a few OWN rows (1 - 200) and a long CONTEXT of keys / values
 * (2 000 - 28 000) that it shares with other sequences of the launch (a video's system + frame tokens under M captions).
 * Keys of sequence s = [rows cu_context[c] .. cu_context[c + 1] of ctx_k / ctx_v, c = context_index[s] | its own rows of K / V],
 * causal: local query i sits at key position context_len + own_rows - queries + i.  head_dim 128, GQA, score_round_mode 1 / 2
 * with the rounding points of mjv_attention_bf16 (scores as there, P rounded to bf16 before P V, fp32 accumulation); any other
 * head_dim and non-causal launches: MJV_E_UNSUPPORTED.
 *   Q / K / V / O : the own rows, addressed as in mjv_attn_desc - cu_seqlens: K / V rows; cu_seqlens_q, optional: the queries are
 *       the LAST cu_seqlens_q[s + 1] - cu_seqlens_q[s] own rows, packed at those rows of Q / O.
 *   ctx_k / ctx_v : every context's rows in one packed buffer each, with leading dimensions and head strides of their own;
 *       a context's length is a positive multiple of 64, or (ctx_any_length = 1) any positive length: a context of `len` keys
       then has ceil(len / 64) key tiles, its last piece ends at `len` and masks the keys behind it as an own part does; rows
       behind a context's length are NEVER READ (they need not exist).  For lengths that are multiples of 64 the plan, the
       workspace and every bit of the result are those of ctx_any_length = 0.  Or ctx_k_list / ctx_v_list (end of the struct): one base pointer per
 *       context, no packed buffer.
 *   cu_seqlens / cu_seqlens_q / context_index / cu_context are HOST arrays, read during the call only: every shape is checked
 *       on the host before anything is launched.  What the kernels read is the PLAN, a device copy of the int32 array
 *       mjv_attention_ctx_plan() derives from exactly these arrays (n_heads, kv_group and head_dim included): the caller builds
 *       it once per batch, uploads it, and hands it to every layer's call.  A plan from other index arrays is the caller's error
 *       (the entry can check its size only).
 *   How the work is laid out: the context part has no mask, so the queries of all sequences of a context and the kv_group
 *       q-heads of a kv head are stacked into tiles of 128 rows that stage a 64-key K / V tile once; a context's keys are cut
 *       into pieces (a function of that context's own query count and length, so a sequence's bits do not depend on sequences
 *       of other contexts) that run as workgroups of their own and leave fp32 (offset, row sum, O) partials in `workspace`; the
 *       causal part over the own rows is one more partial; a second launch on the same stream merges a row's partials in a
 *       fixed order and writes bf16.  No atomics, no flags: equal bits run to run.  The library allocates nothing.
 * ------------------------------------------------------------------------------------------- */
typedef struct mjv_attn_ctx_desc {
  const mjv_bf16 *Q, *K, *V;
  mjv_bf16* O;
  int64_t ldq, ldk, ldv, ldo;
  int32_t q_head_stride, k_head_stride, v_head_stride, o_head_stride;
  const mjv_bf16 *ctx_k, *ctx_v;
  int64_t ld_ctx_k, ld_ctx_v;
  int32_t ctx_k_head_stride, ctx_v_head_stride;
  const int32_t* cu_seqlens;     /* HOST [n_seqs + 1] own K / V row offsets, cu_seqlens[0] = 0 */
  const int32_t* cu_seqlens_q;   /* HOST [n_seqs + 1] or NULL (queries = all own rows) */
  const int32_t* context_index;  /* HOST [n_seqs] */
  const int32_t* cu_context;     /* HOST [n_contexts + 1] row offsets into ctx_k / ctx_v */
  int32_t n_seqs, n_contexts;
  int32_t n_heads, kv_group;
  int32_t head_dim;              /* 128 */
  int32_t causal;                /* 1 */
  float scale;
  int32_t score_round_mode;      /* 1 or 2 */
  const int32_t* plan;           /* DEVICE copy of mjv_attention_ctx_plan's output for these index arrays */
  int64_t plan_ints;
  void* workspace;               /* DEVICE, 16-byte aligned, private to this stream while the call is in flight */
  int64_t workspace_bytes;       /* >= mjv_attention_ctx_workspace_bytes(d) */
  /* Contexts where they lie (both NULL = the packed buffers above; one without the other: MJV_E_ARG).  DEVICE arrays
   * [n_contexts] of device pointers: context c's rows start at ctx_k_list[c] / ctx_v_list[c] (16-byte aligned, at least
   * cu_context[c + 1] - cu_context[c] rows), every context with the leading dimensions ld_ctx_k / ld_ctx_v and the head strides
   * ctx_*_head_stride.  cu_context then only gives the lengths, ctx_k / ctx_v are ignored.  The plan is the same for both
   * addressing modes (a context tile's entry carries its context number), and so are the cut points, the workspace, the merge
   * and every bit of the result.  The entry cannot read the arrays: what they hold is the caller's to check. */
  const mjv_bf16* const* ctx_k_list;
  const mjv_bf16* const* ctx_v_list;
  /* 0 = every context is a positive multiple of 64 keys (anything else: MJV_E_ARG); 1 = any positive length.  Other values:
   * MJV_E_ARG.  In the packed buffers a context's rows start at cu_context[c] as before; a listed context tensor holds at least
   * cu_context[c + 1] - cu_context[c] rows. */
  int32_t ctx_any_length;
} mjv_attn_ctx_desc;

/* Reads the index arrays and sizes of `d` only (no device pointer).  plan_host == NULL: returns the number of int32 the plan
 * takes; otherwise writes it (plan_ints = capacity) and returns the number written.  Negative = MJV_E_*. */
int64_t mjv_attention_ctx_plan(const mjv_attn_ctx_desc* d, int32_t* plan_host, int64_t plan_ints);
/* bytes of fp32 partials the launch described by `d` (index arrays and sizes only) needs; negative = MJV_E_* */
int64_t mjv_attention_ctx_workspace_bytes(const mjv_attn_ctx_desc* d);
int mjv_attention_ctx_bf16(const mjv_attn_ctx_desc* d, void* stream);

/* ABI 7, additive - SEGMENTED contexts.  The three entries above are the three below with seg == NULL, int for int and bit for
 * bit.  With segments the keys of context c are, in key order, the first use_len[u] rows of tensor use_tensor[u] for
 * u = cu_use[c] .. cu_use[c + 1] - 1: ctx_k_list / ctx_v_list then hold one base pointer per TENSOR (n_tensors entries, every
 * tensor with the leading dimensions / head strides of the descriptor and at least the rows its longest use reads), and two
 * contexts may name the same tensor - a parent's rows are read where they lie by every context grown or branched from it.
 * Checked on the host before any launch (MJV_E_ARG, the message names the use or the context):
 *   - segments need the pointer lists: seg != NULL with packed ctx_k / ctx_v is refused (the launch entry; the plan and workspace
 *     queries read no pointer);
 *   - every context has at least one use, cu_use[0] == 0, cu_use[n_contexts] == n_uses;
 *   - cu_context[c + 1] - cu_context[c] (which still gives a context's length) equals the sum of its use_len;
 *   - ctx_any_length must be 1 unless every use_len is a multiple of 64;  use_len > 0;  0 <= use_tensor < n_tensors;
 *   - head_dim != 128 stays MJV_E_UNSUPPORTED with the message it has.
 * Plan: a context's key tiles are the sum over its uses of ceil(use_len / 64); the number of pieces wanted follows from the
 * context's query count and that total as for a plain context, and every use is cut into pieces of the resulting chunk - a
 * piece never straddles two uses, a use's last piece ends at use_len and masks the keys behind it (rows behind use_len are
 * NEVER READ).  A tile's parts stay contiguous and in key order, then the own part: the merge is the plain one.  A part's
 * first / end key are relative to its tensor and its fourth int is the tensor's list entry.  Where a context is cut depends on
 * its own query count and use lengths alone.  A context of exactly one use has the plain plan of that context except for that
 * fourth int; where the use boundaries fall on the plain plan's piece boundaries the result has the plain launch's bits. */
typedef struct mjv_attn_ctx_segments {
  const int32_t* cu_use;      /* HOST [n_contexts + 1]: context c = uses cu_use[c] .. cu_use[c+1]-1, in key order; >= 1 use each */
  const int32_t* use_tensor;  /* HOST [n_uses]: entry of ctx_k_list / ctx_v_list this use reads (two contexts may name the same one) */
  const int32_t* use_len;     /* HOST [n_uses]: the first use_len keys of that tensor, > 0; rows behind are never read */
  int32_t n_uses, n_tensors;  /* n_tensors = entries of ctx_k_list / ctx_v_list */
} mjv_attn_ctx_segments;
int64_t mjv_attention_ctx_seg_plan(const mjv_attn_ctx_desc* d, const mjv_attn_ctx_segments* seg, int32_t* plan_host, int64_t plan_ints);
int64_t mjv_attention_ctx_seg_workspace_bytes(const mjv_attn_ctx_desc* d, const mjv_attn_ctx_segments* seg);
int mjv_attention_ctx_seg_bf16(const mjv_attn_ctx_desc* d, const mjv_attn_ctx_segments* seg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7, additive - attention READOUT: for a few query rows (the two rows per sample the reward heads read, moe_reward.py:226-243),
 * per head, the softmax mass that falls into caller-stated bins of key positions (a frame's image tokens, the prompt text, the
 * caption).  A compact form of `output_attentions`, which the reference declares and hard-wires to False (moe_reward.py:207): no
 * [N, N] matrix, no values, nothing but `mass` is written.
 *   mass[q][h][b] = sum over keys j of bin b of  exp(s_j - m) / sum_i exp(s_i - m),   s = the scores of mjv_attention_bf16 under
 *       score_round_mode 1 / 2 (mode 0: MJV_E_ARG), m = their maximum; fp32 throughout, the probabilities are NOT rounded to bf16
 *       (a readout, not an operand).  Bins b >= the query's bin count are written as 0 up to ld_mass.
 *   Q : n_queries rows x n_heads heads of ALREADY ROTATED queries, row q at Q + q * ldq, head h at + h * q_head_stride.
 *       head_dim 128 or 96 (anything else: MJV_E_UNSUPPORTED, the message names the value).
 *   keys : the keys of query q are, in key order, rows range_row0[r] .. + range_rows[r] of tensor range_tensor[r] for
 *       r = cu_range[q] .. cu_range[q + 1] - 1; tensor t starts at k_list[t] (DEVICE table of n_tensors device pointers, 16-byte
 *       aligned rows), every tensor with the leading dimension ldk and the head stride k_head_stride (kv head = h / kv_group) - so
 *       a tensor may be a column range of wider rows.  The host states EXACTLY the keys a query sees (the caller cuts the last
 *       range at the query's own position): the kernel has no mask and never reads a row outside a stated range.
 *   bins : query q has cu_bin[q + 1] - cu_bin[q] - 1 bins (1 to 128) with the edges bin_edge[cu_bin[q] ..]: ascending key positions
 *       (equal neighbours = an empty bin, mass 0), the first 0, the last the query's key count.
 *   cu_range / range_* / cu_bin / bin_edge are HOST arrays, read during the call only; everything is checked on the host before
 *       any launch (MJV_E_ARG, the message names the query or range).  What the kernel reads is the PLAN, a device copy of the
 *       int32 image mjv_attention_readout_plan() makes of exactly these arrays: built once per batch, handed to every layer's call -
 *       only Q and k_list change between layers.
 *   One workgroup per (query, kv head pair of q-heads), two passes over the keys (the maximum; then the same scores again, summed
 *       per bin), partial sums merged in a fixed order: no atomics, no flags, equal bits run to run, and a query's bits do not
 *       depend on the other queries of the launch.  Profiler tags attn_readout_d128 / attn_readout_d96.
 * ------------------------------------------------------------------------------------------- */
typedef struct mjv_attn_readout_desc {
  const mjv_bf16* Q;
  int64_t ldq;
  int32_t q_head_stride;
  int32_t n_queries, n_heads, kv_group;
  int32_t head_dim;              /* 128 or 96 */
  float scale;
  int32_t score_round_mode;      /* 1 or 2 */
  const mjv_bf16* const* k_list; /* DEVICE [n_tensors] device pointers */
  int32_t n_tensors;
  int32_t k_head_stride;
  int64_t ldk;
  const int32_t* cu_range;       /* HOST [n_queries + 1], cu_range[0] = 0 */
  const int32_t* range_tensor;   /* HOST [n_ranges] */
  const int32_t* range_row0;     /* HOST [n_ranges] */
  const int32_t* range_rows;     /* HOST [n_ranges], > 0 */
  const int32_t* cu_bin;         /* HOST [n_queries + 1] offsets into bin_edge, cu_bin[0] = 0 (a query owns bins + 1 edges) */
  const int32_t* bin_edge;       /* HOST */
  float* mass;                   /* DEVICE fp32 [n_queries][n_heads][ld_mass] */
  int64_t ld_mass;               /* >= every query's bin count */
  const int32_t* plan;           /* DEVICE copy of mjv_attention_readout_plan's output for these index arrays */
  int64_t plan_ints;
} mjv_attn_readout_desc;

/* Reads the HOST arrays and sizes of `d` only (no device pointer; callable without a GPU).  plan_host == NULL: returns the number
 * of int32 the plan takes; otherwise writes it (plan_ints = capacity) and returns the number written.  Negative = MJV_E_*. */
int64_t mjv_attention_readout_plan(const mjv_attn_readout_desc* d, int32_t* plan_host, int64_t plan_ints);
int mjv_attention_readout_bf16(const mjv_attn_readout_desc* d, void* stream);

/* LayerNorm over the last dim, fp32 statistics, bf16 out (nn.LayerNorm on bf16:
 * modeling_intern_vit.py:291,293; modeling_internvl_chat.py:136).
 * gather_grid > 0 selects the pixel-shuffle gather of modeling_internvl_chat.py:228-242,255-260:
 * output row (tile, a2, b2) is the concatenation of the 4 source rows
 * (2a2,2b2) (2a2,2b2+1) (2a2+1,2b2) (2a2+1,2b2+1) of a [tile][1 + grid*grid][dim/4] buffer (CLS skipped).
 * All the norms below move 16-byte pieces of a row: dim % 8 == 0, dim <= 4096, ldx / ldy % 8 == 0 and x, y, gamma / beta / w
 * 16-byte aligned (MJV_E_ARG otherwise, before anything is launched). */
int mjv_layernorm_bf16(const mjv_bf16* x, int64_t ldx, mjv_bf16* y, int64_t ldy, const mjv_bf16* gamma,
                       const mjv_bf16* beta, int32_t rows, int32_t dim, float eps, int32_t gather_grid,
                       void* stream);

/* InternLM2RMSNorm (modeling_internlm2.py:138-143): y = w * bf16(x * rsqrt(mean(x^2) + eps)).
 * row_index (optional, device) gathers input rows: y[i] = norm(x[row_index[i]]). */
int mjv_rmsnorm_bf16(const mjv_bf16* x, int64_t ldx, mjv_bf16* y, int64_t ldy, const mjv_bf16* w,
                     const int32_t* row_index, int32_t rows, int32_t dim, float eps, void* stream);

/* the same two norms with an MXFP8 output (elements y [rows][ldy] bytes + scale records): bf16(norm(x)) exactly as above,
 * then block-quantised - what the fp8 FFN GEMMs (fc1, w1|w3) read.  dim % 128 == 0.  No gathers. */
int mjv_layernorm_mxfp8(const mjv_bf16* x, int64_t ldx, uint8_t* y, int64_t ldy, uint8_t* y_scales, const mjv_bf16* gamma,
                        const mjv_bf16* beta, int32_t rows, int32_t dim, float eps, void* stream);
int mjv_rmsnorm_mxfp8(const mjv_bf16* x, int64_t ldx, uint8_t* y, int64_t ldy, uint8_t* y_scales, const mjv_bf16* w,
                      int32_t rows, int32_t dim, float eps, void* stream);

/* Row statistics of a norm that is folded into the consuming GEMM (mjv_gemm_desc.row_scale): one pass over x,
 * rstd[m] = rsqrt(var + eps) with var = mean((x - mean)^2) (LayerNorm) or mean(x^2) (mean_rstd == NULL: RMSNorm),
 * mean_rstd[m] = mean * rstd.  8 bytes written per row instead of the normalised row. */
int mjv_row_stats_bf16(const mjv_bf16* x, int64_t ldx, float* rstd, float* mean_rstd, int32_t rows, int32_t dim, float eps,
                       void* stream);

/* GQA de-interleave + rotary embedding (modeling_internlm2.py:361-381,233-247):
 * qkv [rows][kv_heads * (group + 2) * 128] -> q [rows][kv_heads*group*128], k [rows][kv_heads*128], both rotated
 * with bf16 cos/sin tables [max_pos][128]; V stays in place (read strided by the attention kernel). */
int mjv_rope_split_bf16(const mjv_bf16* qkv, int64_t ldqkv, mjv_bf16* q, int64_t ldq, mjv_bf16* k, int64_t ldk,
                        const mjv_bf16* cos_tab, const mjv_bf16* sin_tab, const int32_t* positions,
                        int32_t rows, int32_t kv_heads, int32_t group, void* stream);

/* ABI 7 - rotary embedding in place on `n_heads` consecutive heads of every row (head h at x + row * ldx + h * head_stride): the
 * language tower of BASELINE configs[4] (InternVL2-4B = InternViT + Phi-3-mini; the reference cannot build it -
 * internvl2/modeling_internvl_chat.py:125-130 - so this restates transformers/models/phi3/modeling_phi3.py, the module the
 * upstream checkpoint's code is generated from): apply_rotary_pos_emb on qkv_proj's [q heads | k heads | v heads] columns, one
 * launch over the q + k heads.  x' = bf16(bf16(x cos) + bf16(rotate_half(x) sin)) on the first rot_dim elements of a head;
 * cos / sin [positions][rot_dim] bf16 tables that already carry the LongRoPE attention factor (Phi3RotaryEmbedding.forward).
 * rot_dim % 16 == 0, head_stride % 8 == 0, 16-byte aligned pointers. */
int mjv_rope_heads_bf16(mjv_bf16* x, int64_t ldx, int32_t head_stride, int32_t n_heads, int32_t rot_dim, const mjv_bf16* cos_tab,
                        const mjv_bf16* sin_tab, const int32_t* positions, int32_t rows, void* stream);

/* im2col for the patch-embedding conv (modeling_intern_vit.py:145-147,164): pixels [tiles][3][S][S] ->
 * patches [tiles * (S/P)^2][ldp], column = c*P*P + i*P + j, zero-padded to ldp. */
int mjv_patchify_bf16(const mjv_bf16* pixels, mjv_bf16* patches, int64_t ldp, int32_t tiles, int32_t image_size,
                      int32_t patch, void* stream);

/* CLS row of every tile: x[tile * tokens_per_tile] = bf16(cls + pos0)   (modeling_intern_vit.py:166-173) */
int mjv_cls_rows_bf16(mjv_bf16* x, int64_t ldx, const mjv_bf16* cls, const mjv_bf16* pos0, int32_t tiles,
                      int32_t tokens_per_tile, int32_t dim, void* stream);

/* tok_embeddings gather (modeling_internvl_chat.py:163): x[t] = table[ids[t]] unless ids[t] == skip_id
 * (those rows are written by the projector GEMM through out_rows). */
int mjv_embed_gather_bf16(const int32_t* ids, const mjv_bf16* table, int64_t ldt, mjv_bf16* x, int64_t ldx,
                          int32_t rows, int32_t dim, int32_t skip_id, int32_t vocab, void* stream);

/* Reward / gating heads (moe_reward.py:226-285).  hr / hg = post-final-norm reward rows h_r and gating rows h_g
 * ([B][hidden] each, row stride ldh).  ga/gc = outputs of the last hidden layer (post-ReLU) of the aspect / criteria
 * gating MLPs.  Outputs follow CustomOutput (moe_reward.py:287-297). */
typedef struct mjv_heads_desc {
  const mjv_bf16* hr; const mjv_bf16* hg; int64_t ldh; int32_t hidden;
  const mjv_bf16* ga; const mjv_bf16* gc; int64_t ldg; int32_t gate_hidden;
  const mjv_bf16* w_reg;      /* [n_obj][hidden]  regression_layer.weight */
  const mjv_bf16* w_transform;/* [n_obj][n_obj]   reward_transform_matrix */
  const mjv_bf16* wa; const mjv_bf16* ba;  /* aspect_gating last layer   [n_asp][gate_hidden], [n_asp] */
  const mjv_bf16* wc; const mjv_bf16* bc;  /* criteria_gating last layer [n_obj][gate_hidden], [n_obj] */
  const mjv_bf16* ls_a; const mjv_bf16* ls_c; /* logit_scale[0] of each net */
  float temperature;
  int32_t batch, n_obj, n_asp;
  const int32_t* group_offsets; /* [n_asp + 1] into group_index */
  const int32_t* group_index;   /* [n_obj] criteria ids in aspect2criteria dict order */
  mjv_bf16* rewards;            /* [B][n_obj] */
  mjv_bf16* criteria_gating;    /* [B][n_obj] pre-softmax */
  mjv_bf16* aspect_gating;      /* [B][n_asp] */
  mjv_bf16* aspect_weights;     /* [B][n_obj] concatenated in dict order */
  mjv_bf16* weighted_last;      /* [B] last aspect's bf16 weighted sum (moe_reward.py:273,294) */
  float* aspect_scores;         /* [B][n_asp] */
  float* score;                 /* [B] */
  float* packed34;              /* optional [B][1 + n_asp + n_obj] = (score, aspect_scores, rewards) for the
                                   RCCL all-gather of SURVEY.md §8(e); may be NULL */
} mjv_heads_desc;

int mjv_reward_heads_bf16(const mjv_heads_desc* d, void* stream);

/* Frame preprocessing of load_video on the GPU (scripts/data_processor/data.py:56-64,81-117,158-179):
 * decoded uint8 RGB frames [n_frames][height][width][3] -> Pillow-bit-exact bicubic resize to out_w x out_h (two passes,
 * uint8 intermediate `tmp` [n_frames][height][out_w][3]) -> crop into tile_size^2 tiles (row-major grid) ->
 * ((u8/255) - mean) / std in fp32 -> bf16, written to out[(frame * tiles_per_frame + tile_offset + tile)][3][S][S].
 * xbounds/ybounds = (first tap, tap count) per output column / row, xcoef/ycoef = 22-bit fixed-point taps
 * [out][kx|ky], computed on the host exactly as Pillow does (mj-video_amd/video.py: pil_resample_coeffs).
 * mean / stdv are HOST pointers to 3 floats. */
int mjv_resize_normalize_u8(const uint8_t* frames, int32_t n_frames, int32_t height, int32_t width, int32_t out_w,
                            int32_t out_h, const int32_t* xbounds, const int32_t* xcoef, int32_t kx,
                            const int32_t* ybounds, const int32_t* ycoef, int32_t ky, uint8_t* tmp, mjv_bf16* out,
                            int32_t tile_size, int32_t tiles_per_frame, int32_t tile_offset, const float* mean,
                            const float* stdv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Opt-in profiler: when enabled, every launch is bracketed by hipEvents recorded on ITS stream.
 * mjv_prof_collect synchronises those events and accumulates per-kernel-tag time; used by bench.py
 * for the roofline line (kernel average launch duration measured on the launch stream).
 * ------------------------------------------------------------------------------------------- */
int mjv_prof_enable(int32_t on);
/* record only launches with this tag (NULL or "" = every tag): lets a timed region carry events for one kernel only */
int mjv_prof_filter(const char* tag);
int mjv_prof_reset(void);
int mjv_prof_collect(void);
/* number of distinct tags seen; tag i: name, launches, total ms, total algorithmic flops, total algorithmic bytes */
int mjv_prof_count(void);
int mjv_prof_get(int32_t i, const char** name, int64_t* launches, double* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* MJV_H_ */
