/*
 * stllm_hip.h — C ABI of libstllm_hip.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * ST-LLM video-token hot path (EVA-CLIP-g ViT -> Q-Former -> projector -> Vicuna-7B prefill).
 *
 * The reference (TencentARC/ST-LLM) has NO native/FFI layer for this path:
 * the arithmetic is torch.nn ops dispatched to vendor BLAS/DNN kernels.  Each entry point below
 * therefore cites the reference torch call site(s) it replaces (paths relative to the reference
 * root) rather than an existing FFI symbol.  The Python binding a maintainer would add is the
 * ctypes stub in st-llm_amd/hip.py (shown in INTEGRATION.md).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch types.  All data pointers are DEVICE pointers
 *     owned by the caller (torch tensors in the shipped host code); nothing is allocated inside.
 *   - every call takes the hipStream_t to launch on (void* here so the header needs no HIP include).
 *   - return 0 on success, negative stllm_status on error; stllm_last_error() gives the message
 *     (thread-local).  Kernels are launched asynchronously; launch errors are reported, execution
 *     errors surface at the caller's next synchronisation as usual.
 *   - "T" below is the compute dtype selected by `dtype`: bf16 / fp16 (MFMA 32x32x16, fp32
 *     accumulate) or fp32 (exact-fp32 MFMA 32x32x2 — the "verify" numerics mode).
 *   - the residual stream / normalisation inputs are always fp32 (SURVEY.md §7 hard-part 1).
 *   - matrices are row-major; weights are [N, K] (out_features, in_features) exactly as
 *     torch.nn.Linear stores them, possibly row-permuted by the packers in st-llm_amd/pack.py.
 */
#ifndef STLLM_HIP_H
#define STLLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* STLLM_BF16X3 (ABI >= 5; stllm_gemm and the whole-stack entry points only): the "split" verify mode — fp32 activations and outputs, every GEMM
 * run as THREE bf16 matrix-core products (A_hi W_hi + A_hi W_lo + A_lo W_hi, x = hi + lo in bf16) in one bf16 GEMM with K' = 3 K; the
 * fp32 accuracy class (~2^-16 relative per product) at 3x the bf16 FLOPs instead of the 16x of the exact fp32 MFMA.  See stllm_gemm. */
typedef enum { STLLM_BF16 = 0, STLLM_F16 = 1, STLLM_F32 = 2, STLLM_BF16X3 = 3 } stllm_dtype;

typedef enum {
  STLLM_OK = 0,
  STLLM_ERR_BAD_SHAPE = -1,   /* size/stride/alignment constraint violated */
  STLLM_ERR_BAD_DTYPE = -2,
  STLLM_ERR_HIP = -3,         /* hip runtime error at launch */
  STLLM_ERR_UNSUPPORTED = -4
} stllm_status;

/* GEMM epilogues (fused into the producing kernel) */
typedef enum {
  STLLM_EPI_STORE = 0,   /* out = act(acc + bias), out dtype T or f32                              */
  STLLM_EPI_RESID = 1,   /* out_f32 = resid_f32 + acc + bias        (in place when out == resid)   */
  STLLM_EPI_SWIGLU = 2,  /* out[:, j] = silu(gate_j) * up_j; W rows packed [32 gate | 32 up] x N/64 */
  STLLM_EPI_ROPE = 3,    /* fused QKV: rotate-half RoPE on columns < rope_cols (packed layout)     */
  STLLM_EPI_PATCH = 4    /* patch-embed: out_f32[n*257+1+p] = acc + bias + pos_embed[1+p]          */
} stllm_epilogue;

typedef enum { STLLM_ACT_NONE = 0, STLLM_ACT_GELU = 1, STLLM_ACT_RELU = 2 } stllm_act;

/*
 * MEMORY REGIONS — what every entry point below promises about the bytes it touches (tests/test_poison_*.py and the NaN / guard cases of the kernel
 * tests hold the library to it; every buffer a caller passes may come straight from an allocator that does not clear memory):
 *   never read        an operand given as rows with a leading dimension, [rows, ld], is read at the columns [0, width) of its LOGICAL rows only:
 *                     never the columns [width, ld), never a row in front of, between (2-level rows: only row (m / rows_per_batch, m % rows_per_batch))
 *                     or behind the logical rows, never a row at or behind a length bound (Skv, kv_len[b], sfx_len[b], P) unless the entry point's own
 *                     paragraph lists it under "read, weightless".  NaN or any other bit pattern there cannot reach an output.  A tile that overhangs
 *                     M re-reads the LAST logical row instead of the row behind it.
 *   read, weightless  loaded, but multiplied by an exact zero weight or masked: the VALUE cannot matter provided it is FINITE (0 x NaN = NaN).  The caller
 *                     must have written something finite there.  Only stllm_attention / stllm_attention_offset have such a region (their paragraphs).
 *   never written     an output [rows, ldo] is written at the columns [0, width) of its logical rows and NOWHERE else: not the columns [width, ldo), not
 *                     a row in front of / between / behind them, not a row whose index is >= M inside an overhanging tile.  Inputs are never written
 *                     (RESID in place writes `resid` as its output).  Every logical output element IS written (no "left as it was"), except where a
 *                     paragraph says so (free slots of stllm_kv_append_rows).
 *   workspace         "no initialisation needed" means exactly that: every byte that is read was written earlier in the same call.  The contents after
 *                     the call are undefined.  The one exception is stllm_gemm_args.workspace (flags: zero at allocation, kept consistent by the kernels).
 * Entry points without a paragraph of their own (the element-wise, gather and training ops) follow the three rules with no exception.
 */
const char* stllm_last_error(void);
int stllm_abi_version(void);
/* HOST utility (no GPU involved): n values of the deterministic synthetic-weight stream (stllm_amd/synth.py: random-init benchmarks,
 * parity fixtures) for element indices start .. start + n - 1 of the tensor whose (name, seed) hash to `key`; bit-identical to the
 * torch recipe that fills device tensors. */
int stllm_synth_normal_f32(float* out, int64_t n, int64_t start, uint32_t key, float scale, float mean);
/* name of the kernel template instantiation chosen by the last stllm_gemm call on this thread (for profiling) */
const char* stllm_last_kernel(void);

/*
 * C[M,N] = epilogue(A[M,K] @ W[N,K]^T)  on MFMA, LDS-tiled (128-byte K panels, XOR-swizzled).
 * Replaces every nn.Linear / F.linear on the path:
 *   eva_vit.py:124 (qkv), :146 (proj), :55-59 (fc1/fc2); Qformer.py:186-198 (query/key/value),
 *   :286 (attention output dense), :359 (intermediate), :372 (output); st_llm.py:368 (llama_proj),
 *   :475 (down/up_proj), :38-42 (mvm_decoder.head), :122 (lm_head); HF LlamaAttention q/k/v/o_proj
 *   and LlamaMLP gate/up/down_proj (spec: modeling_llama_mem.py:163-166, 138-144).
 * Constraints: K*sizeof(T) % 128 == 0; N % 128 == 0; lda/ldw*sizeof(T) % 16 == 0; A, W 16-byte aligned.
 * A: T[M,lda]   W: T[N,ldw]   bias: f32[N] or NULL
 * STORE : out = T or f32 (out_is_f32) [M,ldo]; act = stllm_act
 * RESID : resid/out f32 [M,ldo]
 * SWIGLU: out T[M,ldo], N/2 columns
 * ROPE  : out T[M,ldo]; rope_cos/rope_sin f32[rope_seq, 64]; row m is position m % rope_seq;
 *         head_dim fixed at 128; columns >= rope_cols are stored unrotated
 * PATCH : A is ignored — the A operand is gathered from `frames` f32 [n_frames,3,224,224]
 *         (implicit GEMM, eva_vit.py:196-204); M = n_frames*256; K = 588 padded (W zero-padded to
 *         ldw); out_f32 = x[n_frames*257, ldo]; `aux` = pos_embed f32[257,N].
 * dtype STLLM_BF16X3: A is f32 [M,lda]; W is bf16 [N, ldw >= 3 K] = stllm_split3_rows(weight, side 1) — (hi | lo | hi) along K;
 *         every output is f32 (STORE / SWIGLU / ROPE write f32 [M,ldo]; act = exact erf GELU / ReLU); K % 64 == 0; PATCH and a_norm_*
 *         are rejected.  Needs split_ws (below).  Internally: split A -> bf16 [M, 3 K] (hi | hi | lo), ONE bf16 GEMM with K' = 3 K and
 *         fp32 output on the kernels above, then the activation / SwiGLU / RoPE as an fp32 row pass.
 * Memory regions.  Never read: A columns [K, lda), A rows >= M (a tile overhanging M re-reads row M - 1) and, with a_rows_per_batch, the rows between the
 *         row groups; W columns [K, ldw) (PATCH: up to the packer's zero-padded K); resid columns [N, ldr) and rows >= M; bias / rope tables behind N /
 *         rope_seq rows; frames behind n_frames.  a_norm_x: columns [K, a_norm_ldx) and rows >= M.  Read, weightless: nothing.  Never written: out columns
 *         [N', ldo) (N' = N, N / 2 for SWIGLU, 3 N' for STLLM_SPLIT_OUT), rows >= M, the rows between o_rows_per_batch groups; PATCH writes rows
 *         n * 257 + 1 .. + 256 only (the CLS rows n * 257 are stllm_vit_cls_rows').  workspace: flags must be zero at allocation; the partial slabs and
 *         split_ws need no initialisation.  Holds for every kernel family (64 x 64 / 128 x 128 tiles, stream-K, phased, one-wave w4, t1, W-direct, GEMV).
 */
typedef struct {
  int dtype;          /* stllm_dtype */
  int epilogue;       /* stllm_epilogue */
  int act;            /* stllm_act (STORE only) */
  int out_is_f32;     /* STORE only */
  const void* A; int64_t lda;
  const void* W; int64_t ldw;
  const float* bias;
  void* out; int64_t ldo;
  const float* resid; int64_t ldr;
  const float* aux0;  /* ROPE: cos table; PATCH: pos_embed */
  const float* aux1;  /* ROPE: sin table */
  const float* frames;/* PATCH */
  int rope_seq; int rope_cols;
  int M, N, K;
  /* optional 2-level row indexing (0 = flat): logical row m lives at
   *   (m / rows_per_batch) * batch_stride + (m % rows_per_batch) * ld      [elements]
   * used for the Q-Former's query / text row groups inside a [N, 32+Lt, C] buffer
   * (Qformer.py:430-462 slices hidden states by query_length). */
  int a_rows_per_batch; int64_t a_batch_stride;
  int o_rows_per_batch; int64_t o_batch_stride;
  /* optional scratch for the phased / stream-K kernels (large problems): >= stllm_gemm_workspace_bytes() bytes of device
   * memory, 16-byte aligned, private to the launch stream (launches on one stream may share it).  NULL => the
   * small-tile kernel is used for every shape.  Contents need no initialisation beyond one memset at allocation. */
  void* workspace; int64_t workspace_bytes;
  /* optional, ABI version >= 2 (decode regime: M <= 8, 16-bit dtypes, every epilogue but PATCH): the A operand is not read
   * from memory but computed on the fly as  RMSNorm(x) * gamma  cast to `dtype` — Llama's input_layernorm /
   * post_attention_layernorm (modeling_llama_mem.py:61-78) fused into the projection that follows it in the one-token step.
   * a_norm_x: fp32 rows [M, K], row stride a_norm_ldx elements; a_norm_gamma: fp32 [K].  A / lda are ignored (may be NULL / 0).
   * Outside the decode regime the call is rejected (STLLM_ERR_UNSUPPORTED): run stllm_rmsnorm first. */
  const float* a_norm_x; int64_t a_norm_ldx; const float* a_norm_gamma; float a_norm_eps;
  /* ABI version >= 5, dtype STLLM_BF16X3 only: >= stllm_gemm_split_ws_bytes(M, N, K, epilogue) bytes of device memory, 16-byte aligned, private
   * to the launch stream, no initialisation (the split A operand and, for SWIGLU, the fp32 gate/up columns).  (ABI 4's fold_* fields —
   * LayerNorm folded into the GEMMs, measured slower than the LayerNorm kernels — were removed with their kernels in ABI 5.) */
  void* split_ws; int64_t split_ws_bytes;
  /* dtype STLLM_BF16X3 only — chaining two split GEMMs without an fp32 round trip between them:
   *   STLLM_SPLIT_A_PRESPLIT: A is ALREADY the split image, bf16 [M, lda >= 3 K] = (hi | hi | lo) — written by stllm_layernorm / stllm_rmsnorm called with
   *     dtype STLLM_BF16X3, by stllm_split3_rows, or by a previous GEMM with STLLM_SPLIT_OUT;
   *   STLLM_SPLIT_OUT (STORE and SWIGLU epilogues): `out` receives the split image of the result, bf16 [M, ldo >= 3 N'] (N' = N, or N / 2 for SWIGLU), after the
   *     activation — the A operand of the next GEMM — instead of the fp32 tensor.  The values are bit-identical to splitting the fp32 result afterwards. */
  int split_flags;
  /* optional, ABI version >= 7 (16-bit dtypes; STORE without activation, SWIGLU, ROPE): a FRAGMENT-MAJOR copy of W — [N / 32][K / 16][64 lanes][8 elements],
   * lane l of fragment (nb, ks) = W[32 nb + (l & 31)][16 ks + 8 (l >> 5) .. + 7], i.e. one contiguous KiB per v_mfma_f32_32x32x16 operand
   * (st-llm_amd/pack.py: frag32).  When present (N % 256 == 0, K % 256 == 0) prefill-sized problems may run on the W-direct kernel (csrc/gemm_wd.inc):
   * W fragments go straight into registers, only A is staged through the LDS.  W itself must still be valid (other shapes / kernels read it).
   * Replaces nothing in the reference: a layout of the nn.Linear weight of modeling_llama_mem.py:130-144, 172-248. */
  const void* w_frag;
} stllm_gemm_args;
enum { STLLM_SPLIT_A_PRESPLIT = 1, STLLM_SPLIT_OUT = 2 };
int64_t stllm_gemm_split_ws_bytes(int M, int N, int K, int epilogue, int split_flags);
/* x f32 [M, K] (row stride ldx; rows_per_batch / batch_stride: the 2-level row indexing of stllm_gemm_args, 0 = flat) ->
 * out bf16 [M, ldo >= 3 K]: hi = bf16(x), lo = bf16(x - hi), laid out (hi | hi | lo) along K for weight_side == 0 (the A operand) and
 * (hi | lo | hi) for weight_side != 0 (the weight: packed once).  K % 4 == 0. */
int stllm_split3_rows(const float* x, int64_t ldx, int rows_per_batch, int64_t batch_stride, void* out, int64_t ldo, int M, int K,
                      int weight_side, void* stream);
int64_t stllm_gemm_workspace_bytes(void);
/* Synchronises `stream` and returns 0 when no GEMM launch that used `workspace` ever gave up waiting for a peer workgroup
 * (the split-K exchanges poll with a bound instead of hanging the GPU when not all workgroups are resident, e.g. on a
 * GPU shared with another process), non-zero otherwise (sticky; stllm_last_error() explains). */
int stllm_gemm_workspace_status(const void* workspace, void* stream);
/* Host-only introspection of the phased kernel's schedule for an M x N x K problem (no GPU needed; used by the CPU tests):
 * plan5 = { data-parallel rounds q, remainder tiles r, K slices per remainder tile s, slice groups per XCD cap, estimated us }
 * for tile_rows = 192 | 256; heavy = 0 plain 16-bit output, 1 fp32 output / residual, 2 GELU.  T = q * 256 + r tiles of
 * tile_rows x 256; the s workgroups of a remainder tile sit on one XCD (s <= 32, 8 * cap >= r, cap = 32 / s). */
int stllm_gemm_plan(int M, int N, int K, int heavy, int tile_rows, int* plan5);
/* The same for the one-wave-per-SIMD kernel (st-llm_amd/csrc/gemm_w4.inc): shape = 32 (192 x 128 tile) | 42 (256 x 128) | 34 (192 x 256) |
 * 44 (256 x 256) | 22 (128 x 128, two workgroups per CU: T = q * 512 + r).  heavy bit 3 (| 8): the epilogue is STORE / RESID, so a last tile row of <= 32 rows is computed outside the tile
 * grid ("thin tail": ViT fc1's 4112 rows = 16 tile rows + 16 rows) and does not count as tiles. */
int stllm_gemm_w4_plan(int M, int N, int K, int heavy, int shape, int* plan5);
/* tuning / test hooks.  Option state is PER THREAD (thread-local, like the error string): the first stllm_* call of a host thread reads the
 * STLLM_GEMM_SK / _DEBUG / _GEMV / _P8 / _W4, STLLM_GEMV_MFMA, STLLM_ATTN_DMA, STLLM_ATTN_BWD_VALU, STLLM_NORM_FAST environment variables once,
 * stllm_set_option() changes the calling thread's copy only — two host threads driving different streams / devices never race on it.
 * Per-device launch state (dynamic-LDS opt-in, occupancy answers) is kept per device ordinal.
 * The fused-RMSNorm operand (a_norm_*) exists in the GEMV kernels only: "gemm_gemv" = 0 and forced tile kernels do not apply to it.
 *   "gemm_p8"    = -1 auto (cost model) | 0 off | 1 always (cost model picks the tile height) | 3 / 4 always, 192 / 256-row tile:
 *                  the phased 192|256 x 256 kernel (st-llm_amd/csrc/gemm_p8.inc; 16-bit dtypes, needs `workspace`)
 *   "gemm_w4"    = -1 auto = 2 | 0 off | 1 always (cost model picks the tile) | 2 where its plan beats the other kernels' estimates (from 1024 rows on also
 *                  plans whose K-split hides behind >= 1 whole round; below 1024 rows exchange-free plans of ONE partial round only) | 32 / 42 / 34 / 24 / 43 / 33 always,
 *                  192 x 128 / 256 x 128 / 192 x 256 / 128 x 256 / 256 x 192 / 192 x 192 tile (44 = 256 x 256 was retired in round 3: unsupported, falls back) | 22 (round 5, never chosen
 *                  automatically): the 128 x 128 tile as TWO workgroups per CU (two waves per SIMD, 80 KiB of LDS each, 512 persistent workgroups, exchange-free plans):
 *                  the one-wave-per-SIMD kernel (st-llm_amd/csrc/gemm_w4.inc; 16-bit dtypes, needs `workspace`)
 *   "gemm_gemv"  = -1 on (M <= 16) | 0 off | 1 only M <= 4 | 2 = -1: the skinny kernels of the decode regime (st-llm_amd/csrc/gemv.hip):
 *                  the 5 beams of demo.py's beam search, small serving batches (5-row step 6.99 -> 4.34 ms on MI355X)
 *   "gemv_mfma"  = -1 matrix-core GEMV (v_mfma_f32_16x16x32) from M = 3, the VALU kernel (v_dot2c) below | 0 never (M > 8 then runs on the
 *                  tile kernels) | 1 from M = 1
 *   "attn_dma"   = 1 (default) attention at head_dim 128 (Llama prefill) and 88 (ViT) staged by LDS-DMA, V through the transposing LDS read |
 *                  0 register-staged kernels | 10 nw + ks (nw x ks <= 12, ks in 1 / 2 / 4): force the head_dim-128 kernel's work split — nw query tiles per
 *                  workgroup x ks key-split waves per tile (tools/attn_bench.py --audit)
 *   "attn_decode_single" = 1 (default) one-workgroup-per-head decode attention for Skv <= 1536 | 0 always the split-KV pair
 *   "gemm_sk"    = -1 auto | 0 off | 1 (128x128) | 2 (128x256) | 3 (256x256): stream-K tile of the older kernels
 *   "gemm_debug" = ablation bits of the 128x128 kernels; bit 16 = in-kernel timeline of the phased kernel (tools/gemm_harness.cpp)
 *   "attn_bwd_valu" = 0 (default) MFMA attention backward for 16-bit operands | 1 the VALU twins
 *   "norm_fast"  = 1 (default) one row per wave | 2: two rows per wave for >= 2048 short rows (bit-identical results, same speed: an A/B switch)
 *   "gemm_w4_odd" = 1 (default) the 192-column tiles (43 = 256 x 192, 33 = 192 x 192; 16-bit STORE epilogues) take part in the automatic
 *                  choice | 0 the round-2 choice (A/B inside one process: bench.py --ab)
 *   "gemm_w4_wide" = 1 (default) a 16-bit GEMM of at most 640 rows whose 128 x 256 tiles make ONE round of 192..256 tiles (the Llama prefill qkv
 *                  GEMM at 385..640 rows: 5 x 48 = 240 tiles at S = 576) runs on the one-wave kernel's 128 x 256 tile (code 24) | 0 on the 128 x 128 kernel */
int stllm_set_option(const char* key, int value);
int stllm_gemm(const stllm_gemm_args* args, void* stream);

/*
 * W8A16 skinny GEMM of the decode regime (st-llm_amd/csrc/gemv.hip), ABI version >= 7 (additive):
 *   C[M,N] = epilogue(scale[n] * (A[M,K] @ Wq[N,K]^T) + bias[n])
 * A: bf16 / fp16 [M,lda]; Wq: int8 [N,ldw] (ldw in BYTES = elements), |q| <= 127, packed like the 16-bit weight it was quantised from
 * (st-llm_amd/pack.py: quant8_rows after llama_qkv / llama_gate_up / linear); scale: f32 [N], one per output row of Wq.
 * The accumulation is fp32 over the exact products a * q (|q| <= 127 is exact in bf16 and fp16); scale is applied once per output column in
 * the epilogue, before bias / residual / SwiGLU / RoPE.  Wq and scale are read-only.
 * Epilogues: STORE (dtype or f32 out, no activation), RESID, SWIGLU, ROPE — the meaning, the (c, c + 32) column pairs, the 2-level row
 * indexing and the strided output rows of stllm_gemm.  a_norm_*: the fused RMSNorm operand of stllm_gemm_args, M <= 2 only (the VALU kernel).
 * Kernels: M <= 2 (option "gemv_mfma" = 0: M <= 8) the VALU kernel (v_dot2c on pairs converted in registers; the staged rows of A,
 * 1 / 2 / 4 / 6 / 8 x K x 2 bytes, must fit 150 KiB of LDS); 3 <= M <= 16 ("gemv_mfma" = 1: from M = 1) the matrix-core kernel (K % 64 == 0).
 * Constraints: 1 <= M <= 16; N % 64 == 0; K % 16 == 0; Wq 16-byte aligned, ldw % 16 == 0; A / out / resid as for stllm_gemm.
 * M > 8 (or M >= 3 with the default options) runs on the matrix-core kernel only, which needs K % 64 == 0: K % 64 == 16 / 32 / 48 is served for M <= 8.
 * A shape or option combination no kernel covers returns STLLM_ERR_UNSUPPORTED (stllm_last_error() says which): nothing else runs in its place.
 * Launches are seen by stllm_gemm_profile; stllm_last_kernel() names gemv_w8_kernel<...> / gemv_w8_mfma_kernel<...>.
 * Stands in for the nn.Linear calls of the one-token step (modeling_llama_mem.py:130-144, 163-166) when the weights are held in 8 bits —
 * the `device_8bit` / low-resource knob of demo.py:41, which the reference carries without an implementation.
 * Memory regions: those of stllm_gemm.  Never read: A columns [K, lda) and rows >= M (the staged / fragment rows past M re-read row M - 1), Wq bytes
 * [K, ldw) of a row, resid columns [N, ldr).  Never written: out columns [N', ldo), rows >= M, the rows between strided output rows.
 */
typedef struct {
  int dtype;          /* STLLM_BF16 | STLLM_F16: A and the 16-bit outputs */
  int epilogue;       /* STORE | RESID | SWIGLU | ROPE */
  int out_is_f32;     /* STORE only */
  int M, N, K;
  const void* A; int64_t lda;            /* elements; ignored with a_norm_x */
  const void* Wq; int64_t ldw;           /* int8 rows, stride in bytes */
  const float* scale;                    /* f32 [N] */
  const float* bias;                     /* f32 [N] or NULL */
  void* out; int64_t ldo;
  const float* resid; int64_t ldr;
  const float* rope_cos; const float* rope_sin; int rope_seq; int rope_cols;
  int a_rows_per_batch; int64_t a_batch_stride;
  int o_rows_per_batch; int64_t o_batch_stride;
  const float* a_norm_x; int64_t a_norm_ldx; const float* a_norm_gamma; float a_norm_eps;
} stllm_gemv_w8_args;
int stllm_gemv_w8(const stllm_gemv_w8_args* args, void* stream);

/*
 * W4A16 skinny GEMM of the decode regime (st-llm_amd/csrc/gemv.hip), ABI version >= 7 (additive):
 *   C[M,N] = epilogue(sum_g scale[n,g] * (A[M, 128 g : 128 g + 128] @ q[n, 128 g : 128 g + 128]^T) + bias[n])
 * A: bf16 / fp16 [M,lda]; Wq: uint8 [N,ldw] (ldw in BYTES, >= K / 2), two 4-bit weights per byte, stored nibble u = q + 8 in [1, 15] (|q| <= 7),
 * rows packed like the 16-bit weight they were quantised from (st-llm_amd/pack.py: quant4_groups after llama_qkv / llama_gate_up / linear).
 * Nibble placement: dword d of a row holds elements 8 d .. 8 d + 7; element 2 t at bits [4 t, 4 t + 4), element 2 t + 1 at bits [16 + 4 t, 16 + 4 t + 4).
 * scale: f32 [N, ld_scale], one per output row and group of 128 K elements (ld_scale >= K / 128, in floats).
 * The accumulation is fp32 over exact products (q, or the exact offset form 136 + q whose offset is removed in fp32); the scale multiplies the finished
 * sum of its group, before bias / residual / SwiGLU / RoPE.  Wq and scale are read-only.
 * Epilogues, 2-level row indexing, strided output rows and a_norm_* (M <= 2): those of stllm_gemv_w8.
 * Kernels: M <= 2 (option "gemv_mfma" = 0: M <= 8) the VALU kernel (the staged rows of A, 1 / 2 / 4 / 6 / 8 x K x 2 bytes, must fit 150 KiB of LDS);
 * 3 <= M <= 16 ("gemv_mfma" = 1: from M = 1) the matrix-core kernel.
 * Constraints: 1 <= M <= 16; N % 64 == 0; K % 128 == 0; Wq 16-byte aligned, ldw % 16 == 0; A / out / resid as for stllm_gemm.
 * A shape or option combination no kernel covers returns STLLM_ERR_UNSUPPORTED (stllm_last_error() says which): nothing else runs in its place.
 * Launches are seen by stllm_gemm_profile; stllm_last_kernel() names gemv_q4_kernel<...> / gemv_q4_mfma_kernel<...>.
 * Memory regions: those of stllm_gemv_w8; Wq bytes [K / 2, ldw) of a row and scale columns [K / 128, ld_scale) are never read.
 */
typedef struct {
  int dtype;          /* STLLM_BF16 | STLLM_F16: A and the 16-bit outputs */
  int epilogue;       /* STORE | RESID | SWIGLU | ROPE */
  int out_is_f32;     /* STORE only */
  int M, N, K;
  const void* A; int64_t lda;            /* elements; ignored with a_norm_x */
  const void* Wq; int64_t ldw;           /* packed nibbles, row stride in bytes */
  const float* scale; int64_t ld_scale;  /* f32 [N, K / 128], row stride in floats */
  const float* bias;                     /* f32 [N] or NULL */
  void* out; int64_t ldo;
  const float* resid; int64_t ldr;
  const float* rope_cos; const float* rope_sin; int rope_seq; int rope_cols;
  int a_rows_per_batch; int64_t a_batch_stride;
  int o_rows_per_batch; int64_t o_batch_stride;
  const float* a_norm_x; int64_t a_norm_ldx; const float* a_norm_gamma; float a_norm_eps;
} stllm_gemv_q4_args;
int stllm_gemv_q4(const stllm_gemv_q4_args* args, void* stream);

/* HIP-event timing of stllm_gemm launches on their launch stream, per calling thread (bench.py's roofline leg; also sees the launches of
 * the whole-stack entry points below).  mode 0 off | 1 every launch | 2 only launches whose kernel symbol — learned per (dtype, epilogue,
 * act, M, N, K) while mode 1 was on — equals target_symbol | 3 every 7th of those (a sample: the event records sit between the kernels on
 * the stream and cost the measured step ~3 us per timed launch; bench.py's timed region uses 3).  Every call starts a new, empty session.  _read synchronises record i's end
 * event and returns its kernel symbol (stllm_last_kernel naming), duration, algorithmic FLOPs (2 M N K) and shape. */
int stllm_gemm_profile(int mode, const char* target_symbol);
int stllm_gemm_profile_count(void);
int stllm_gemm_profile_read(int i, char* symbol, int symbol_cap, float* ms, double* flops, int* mnk3 /* M, N, K or NULL */);

/* =========================================================================================================================
 * Whole-stack entry points: one host call issues every launch of a layer stack, through the entry points of this header
 * with the arguments the per-op host code passes (bit-identical results; ~540 host round trips per step become a handful).
 * All weight pointers are device pointers to tensors packed as for stllm_gemm (st-llm_amd/pack.py); ld_* = row stride in elements.
 * ========================================================================================================================= */

/* one EVA ViT block (eva_vit.py:157-180: norm1, attn.qkv + (q_bias, 0, v_bias), attn.proj, norm2, mlp.fc1, mlp.fc2) */
typedef struct {
  const float* n1w; const float* n1b; float e1;
  const void* wqkv; int64_t ld_qkv; const float* bqkv;     /* [3 dim, dim], bias f32 [3 dim] = (q_bias, 0, v_bias) (eva_vit.py:120-124) */
  const void* wproj; int64_t ld_proj; const float* bproj;
  const float* n2w; const float* n2b; float e2;
  const void* wfc1; int64_t ld_fc1; const float* bfc1;     /* [hidden, dim] */
  const void* wfc2; int64_t ld_fc2; const float* bfc2;     /* [dim, hidden] */
} stllm_vit_block_weights;
typedef struct {
  int dtype; int n_seq; int seq_len; int num_heads; int dim; int hidden;
  float* x; int64_t ldx;                       /* fp32 residual stream [n_seq * seq_len, dim], updated in place */
  void* scratch; int64_t scratch_bytes;        /* >= stllm_vit_blocks_scratch_bytes(...), 256-byte aligned, no initialisation */
  void* workspace; int64_t workspace_bytes;    /* the stllm_gemm workspace of the launch stream */
} stllm_vit_blocks_args;
int64_t stllm_vit_blocks_scratch_bytes(int dtype, int n_seq, int seq_len, int dim, int hidden);
/* VisionTransformer.forward_features' block loop (eva_vit.py:336-339; Block.forward :173-180) for n_blocks consecutive blocks */
int stllm_vit_blocks(const stllm_vit_blocks_args* args, const stllm_vit_block_weights* blocks, int n_blocks, void* stream);

/* one HF LlamaDecoderLayer (spec modeling_llama_mem.py:61-316): RMSNorm weights, fused [q | k | v] rows in the packed RoPE layout,
 * o_proj, packed [32 gate | 32 up] rows, down_proj; kv_cache: NULL or this layer's [B, cache_max_len, 3 hidden] cache buffer */
typedef struct {
  const float* ln1; const void* wqkv; int64_t ld_qkv; const void* wo; int64_t ld_o;
  const float* ln2; const void* wgu; int64_t ld_gu; const void* wdown; int64_t ld_down;
  void* kv_cache;
  const void* wqkv_frag; const void* wgu_frag;   /* ABI >= 7: NULL or the fragment-major copies of wqkv / wgu (stllm_gemm_args.w_frag) */
} stllm_llama_layer_weights;
typedef struct {
  int dtype; int B; int S; int n_heads; int hidden; int inter; float eps;
  float* x; int64_t ldx;                       /* fp32 residual stream [B * S, hidden], updated in place */
  const float* rope_cos; const float* rope_sin;/* f32 [S, 64] */
  const int32_t* kv_len;                       /* int32 [B] valid lengths of right-padded sequences, or NULL */
  int64_t cache_max_len;                       /* 0: no KV cache */
  void* scratch; int64_t scratch_bytes;        /* >= stllm_llama_layers_scratch_bytes(...) */
  void* workspace; int64_t workspace_bytes;
} stllm_llama_layers_args;
int64_t stllm_llama_layers_scratch_bytes(int dtype, int B, int S, int hidden, int inter);
/* the decoder-layer loop of the PREFILL (st_llm.py:56-92 -> HF LlamaModel.forward, use_cache False or filling a fresh cache) */
int stllm_llama_layers(const stllm_llama_layers_args* args, const stllm_llama_layer_weights* layers, int n_layers, void* stream);
/* the decoder-layer loop for S NEW positions pos0 .. pos0 + S - 1 behind pos0 positions already in the KV cache (LlamaModel.extend; additive to ABI 7):
 * as stllm_llama_layers with a cache (args->cache_max_len >= pos0 + S, args->kv_len NULL, args->rope_cos / rope_sin pointing at position pos0's table row),
 * but layer l's fused QKV rows go to rows [pos0, pos0 + S) of every batch entry's block of layers[l].kv_cache and the attention is stllm_attention_offset
 * (Sq = S, Skv = pos0 + S, q_off = pos0) with `attn_workspace` (>= stllm_attention_offset_workspace_bytes(B, n_heads, S, pos0 + S), or NULL: tile kernels only).
 * Scratch as for stllm_llama_layers.  bf16 / fp16 / fp32.  The same launches, in the same order, as the per-op path: bit-identical. */
int stllm_llama_layers_extend(const stllm_llama_layers_args* args, const stllm_llama_layer_weights* layers, int n_layers, int pos0,
                              void* attn_workspace, int64_t attn_workspace_bytes, void* stream);
/* ---- LoRA adapters on q_proj / v_proj (peft 0.8.1 Linear, eval: y = W x + (lora_alpha / r) B (A x); the reference builds them at st_llm.py:165-177).  Additive to
 * ABI 7: new symbols only, no existing struct changes.
 *
 * stllm_lora_down: out[M, n_pad] = x[M, K] · A[n, K]^T in T (fp32 accumulation), columns [n, n_pad) written as zeros.  A = [lora_A(q_proj) ; lora_A(v_proj)]
 * (n = 2 r).  K is split over workgroups and reduced in a fixed order (no atomics): two calls on the same input give the same bits.  1 <= M, n <= n_pad <= 128,
 * n_pad % 32 == 0, K a whole number of 128-byte panels, rows 16-byte aligned; x and out may be column ranges of ONE row buffer (ldx == ldo).
 * workspace: >= stllm_lora_down_workspace_bytes(dtype, M, K, n_pad) bytes (0 for tall problems). */
int64_t stllm_lora_down_workspace_bytes(int dtype, int M, int K, int n_pad);
int stllm_lora_down(int dtype, const void* x, int64_t ldx, const void* A, int64_t lda, void* out, int64_t ldo, int M, int K, int n, int n_pad,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* adapter of one decoder layer: A [2 r, hidden] in T (q rows, then v rows); wqkv_ext [3 hidden, hidden + P] in T = the layer's packed wqkv with P extra columns:
 * q rows (in the packed RoPE head order) [s B_q | 0], k rows 0, v rows [0 (r columns) | s B_v | 0], s = lora_alpha / r; P = 2 r rounded up to the GEMMs' K
 * granularity (64 columns in 16 bits, 32 in fp32), the same for every layer of a call. */
typedef struct {
  const void* A; int64_t ld_a;
  const void* wqkv_ext; int64_t ld_ext;
  int r; int P;
} stllm_llama_lora_layer;
int64_t stllm_llama_layers_lora_scratch_bytes(int dtype, int B, int S, int hidden, int inter, int P);
/* stllm_llama_layers with active adapters — still ONE call per prefill: per layer RMSNorm -> stllm_lora_down -> ONE QKV GEMM over K = hidden + P (the low-rank
 * term joins the fp32 accumulator BEFORE the RoPE epilogue; layers[l].wqkv / wqkv_frag are not read) -> the rest of the base layer.  bf16 / fp16 / fp32. */
int stllm_llama_layers_lora(const stllm_llama_layers_args* args, const stllm_llama_layer_weights* layers, const stllm_llama_lora_layer* lora_layers, int n_layers, void* stream);
/* ONE decoder layer of a SEQUENCE-PARALLEL prefill in two parts (ABI >= 7, round 6; st-llm_amd/models/llama.py: LlamaModel.prefill_sp — no reference counterpart, the
 * reference has no sequence parallelism: SURVEY.md 2b): this rank owns the positions [s0, s1) of one sequence (args->B == 1, args->S == s1 - s0 rows in x,
 * args->rope_cos / rope_sin pointing at position s0's table row), `qkv` is the fused buffer [s1, 3 * hidden] (compute dtype) whose rows [0, s0) hold the earlier
 * members' K | V (their q columns zero).
 *   part 0: RMSNorm(x) -> fused QKV GEMM + RoPE at positions s0 .. -> rows [s0, s1) of `qkv`            (the caller then ships / receives K | V rows)
 *   part 1: causal attention of the s1 query rows over the s1 keys, rows [s0, s1) -> o_proj + residual -> RMSNorm -> gate/up + SiLU(gate) * up -> down + residual
 * The same launches, in the same order, as the per-op path: bit-identical.  Scratch: stllm_llama_layer_sp_scratch_bytes(dtype, s0, s1, hidden, inter). */
int64_t stllm_llama_layer_sp_scratch_bytes(int dtype, int s0, int s1, int hidden, int inter);
int stllm_llama_layer_sp(const stllm_llama_layers_args* args, const stllm_llama_layer_weights* layer, void* qkv, int s0, int s1, int part, void* stream);

/* BertSelfOutput / BertOutput (Qformer.py:281-289, 384-400): LayerNorm(dense(x) + input) */
typedef struct {
  const void* w; int64_t ldw; const float* b;  /* dense [hidden, in], bias f32 [hidden] */
  const float* g; const float* beta; float eps;/* LayerNorm weight / bias f32 [hidden] */
} stllm_bert_output_weights;
/* one Q-Former BertLayer (Qformer.py:367-484): fused self-attention [q | k | v] rows, attention.output, on the layers with cross-attention
 * (has_cross: layer_num % cross_attention_freq == 0) crossattention.self.query + crossattention.output — the cross K / V projections of ALL
 * layers live in ONE weight (stllm_qformer_layers_args.ckv_w; ckv_index = this layer's [k | v] column block in its output) —, the query
 * rows' FFN (intermediate_query / output_query) and, with text rows, the text FFN (intermediate / output; ft_w1 NULL otherwise) */
typedef struct {
  const void* wqkv; int64_t ld_qkv; const float* bqkv;
  stllm_bert_output_weights attn_out;
  int has_cross; int ckv_index;
  const void* cq_w; int64_t ld_cq; const float* cq_b;
  stllm_bert_output_weights cross_out;
  const void* fq_w1; int64_t ld_fq1; const float* fq_b1; stllm_bert_output_weights fq_out;
  const void* ft_w1; int64_t ld_ft1; const float* ft_b1; stllm_bert_output_weights ft_out;
} stllm_qformer_layer_weights;
typedef struct {
  int dtype; int n_seq; int n_query; int n_text; int n_heads; int hidden; int inter; int enc_len; int enc_dim; int n_cross;
  float* hq32; void* hq16;                     /* query rows [n_seq * n_query, hidden]: fp32 post-LN stream + its compute-dtype copy, both updated in place */
  float* ht32; void* ht16;                     /* text rows [n_seq * n_text, hidden] likewise (NULL when n_text == 0) */
  const void* enc16; int64_t ld_enc;           /* ln_vision'd image tokens, compute dtype [n_seq * enc_len, enc_dim] */
  const void* ckv_w; int64_t ld_ckv; const float* ckv_b;   /* [n_cross * 2 hidden, enc_dim]: (key | value) rows of the cross layers in layer order */
  const int32_t* kv_len;                       /* int32 [n_seq] = n_query + valid text tokens (right-padded text), or NULL */
  void* scratch; int64_t scratch_bytes;        /* >= stllm_qformer_layers_scratch_bytes(...), 256-byte aligned, no initialisation */
  void* workspace; int64_t workspace_bytes;    /* the stllm_gemm workspace of the launch stream */
} stllm_qformer_layers_args;
int64_t stllm_qformer_layers_scratch_bytes(int dtype, int n_seq, int n_query, int n_text, int hidden, int inter, int enc_len, int enc_dim, int n_cross);
/* BertEncoder.forward's layer loop (Qformer.py:495-589; BertLayer.forward :402-484) on the embedded rows: self-attention over [queries | text],
 * cross-attention of the query rows against the image tokens on the has_cross layers, the two FFNs.  STLLM_BF16X3: fp32 activations, every
 * Linear split inside its GEMM (no pre-split images: the rows are too few for the split passes to matter). */
int stllm_qformer_layers(const stllm_qformer_layers_args* args, const stllm_qformer_layer_weights* layers, int n_layers, void* stream);

/*
 * Decode attention: ONE query row per (batch, head) against Skv cached keys (the one-token step of generate(), SURVEY §8f
 * rank 1; HF LlamaAttention with past_key_values, spec modeling_llama_mem.py:172-248).  HBM-bound: the keys are split over
 * several workgroups per head and the partial softmax states are merged by a second launch.  head_dim 128, bf16 / fp16.
 * q: element (b, h, d) at q[b*q_bs + h*128 + d];  k, v: (b, s, h, d) at k[b*k_bs + s*k_rs + h*128 + d];  out like q.
 * workspace: >= stllm_attention_decode_workspace_bytes(B, H, Skv) bytes, 16-byte aligned, no initialisation needed.
 * Memory regions.  Never read: K / V rows at or behind Skv of every batch row (the cache rows the step has not reached are uninitialised), the columns
 * of a row outside head h's 128, q / k / v behind H * 128 columns.  Read, weightless: nothing (a key that is not loaded contributes through a `live`
 * predicate, not through a zero weight).  Never written: out behind H * 128 columns of a row, rows other than b * o_bs.  Every workspace record the merge
 * reads was written by the partial pass of the same call.
 */
int64_t stllm_attention_decode_workspace_bytes(int B, int H, int Skv);
int stllm_attention_decode(int dtype, const void* q, int64_t q_bs, const void* k, int64_t k_bs, int64_t k_rs,
                           const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs, int B, int H, int Skv,
                           int D, float scale, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Ragged decode attention (additive to ABI 7): stllm_attention_decode for a KV cache whose batch rows have DIFFERENT lengths.
 * kv_len: int32 [B] in device memory; row b attends keys [0, min(kv_len[b], max_kv)); max_kv is the host-known upper bound of the lengths, from which the
 * schedule (single pass | split-KV pair, "attn_decode_single") and the grid are chosen exactly as stllm_attention_decode chooses them from Skv.  A row with
 * kv_len[b] <= 0 (a free slot of the batch) gets zeros, never NaN.  Row b's output is bit-identical to stllm_attention_decode on that row alone with
 * Skv = kv_len[b] whenever that call takes the same schedule: same key-to-lane assignment, and in the split pair the split count and keys per split of its
 * own length, merged in the same order.  bf16 / fp16 at head_dim 128 only: anything else returns STLLM_ERR_UNSUPPORTED (fp32: stllm_attention with kv_len).
 * Addressing as for stllm_attention_decode; workspace: >= stllm_attention_decode_ragged_workspace_bytes(B, H, max_kv) bytes, 16-byte aligned.
 * Memory regions.  Never read: K / V rows at or behind min(kv_len[b], max_kv) of batch row b; q, K and V of a row with kv_len[b] <= 0 altogether (a free
 * slot's query is whatever the scratch held).  Read, weightless: nothing.  Written: every out row b at columns [0, H * 128), zeros for a free slot whatever
 * the buffer held before; nothing else.  Workspace: the surplus split workgroups of a short row (split index >= that row's split count) exit without
 * writing, and the merge reads exactly the records its row's own split count names — an unwritten record is never read.
 */
int64_t stllm_attention_decode_ragged_workspace_bytes(int B, int H, int max_kv);
int stllm_attention_decode_ragged(int dtype, const void* q, int64_t q_bs, const void* k, int64_t k_bs, int64_t k_rs,
                                  const void* v, int64_t v_bs, int64_t v_rs, void* out, int64_t o_bs, int B, int H,
                                  const int32_t* kv_len, int max_kv, int D, float scale, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/*
 * Shared-prefix attention (additive to ABI 7): B = G * R query rows in G contiguous groups of R.  Query (b, i) sees ALL P keys of prefix row b / R
 * (kp / vp: G rows, read-only) and suffix key j of its own row b (ks / vs: B rows) iff j < min(sfx_len[b], max_sfx) — with `causal` also j <= sfx_q_off + i.
 * sfx_len: int32 [B] in device memory, or NULL (every row holds max_sfx keys).  The prefix and the suffix buffers have independent (batch, row) strides, in
 * elements; q, out: element (b, i, h, d) at b*bs + i*rs + h*128 + d.  Neither buffer is read at or behind those bounds (the rows there may be uninitialised).
 *   bf16 / fp16, Sq == 1 (the decode step): a partial pass — prefix workgroups that load each K / V tile once for all R rows of a group (matrix cores) plus
 *     suffix workgroups in the same launch — and a merge in a fixed order: two launches, deterministic.
 *   bf16 / fp16, Sq > 1: the key-split tile kernels of stllm_attention_offset, once over the prefix (batch G, R * Sq query rows) and once per row over the
 *     suffix, then the same merge.  Needs the query rows of a group at one row stride (q_bs == Sq * q_rs) when R > 1.
 *   fp32: one vector kernel (the verify mode), any Sq.
 * head_dim 128 only; anything unsupported returns STLLM_ERR_UNSUPPORTED (stllm_last_error() says what): nothing else runs in its place.
 * workspace: >= stllm_attention_shared_workspace_bytes(B, G, H, Sq, P, max_sfx) bytes, 16-byte aligned, no initialisation needed (unused in fp32).
 * Memory regions.  Never read: prefix rows at or behind P, suffix rows at or behind min(sfx_len[b], max_sfx) of row b — in the Sq > 1 suffix pass the tile
 * kernel runs with LIVE loads (rows behind the length are replaced by zeros in the LDS instead of being loaded).  Read, weightless: nothing.  Pad query rows
 * (Sq > 1, i >= the row's own new tokens) are read and their output rows are written with don't-care (finite-or-not) values: the caller ignores them.
 * Never written: kp / vp / ks / vs; out behind H * 128 columns.  Workspace records: written by the partial pass before the merge reads them.
 */
int64_t stllm_attention_shared_workspace_bytes(int B, int G, int H, int Sq, int P, int max_sfx);
int stllm_attention_shared(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* kp, int64_t kp_bs, int64_t kp_rs,
                           const void* vp, int64_t vp_bs, int64_t vp_rs, int P, const void* ks, int64_t ks_bs, int64_t ks_rs,
                           const void* vs, int64_t vs_bs, int64_t vs_rs, const int32_t* sfx_len, int max_sfx, int sfx_q_off,
                           void* out, int64_t o_bs, int64_t o_rs, int B, int G, int H, int Sq, int D, float scale, int causal,
                           void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Ragged KV-cache append (additive to ABI 7): for every batch row b the [k | v] columns (with_q != 0: [q | k | v]) of the dense fused row
 * src[b*ld_src .. + 3*hidden) are copied to cache[b*batch_stride + pos[b]*row_stride + the same columns].  pos: int32 [B] in device memory; a position
 * outside [0, max_len) marks a free slot: nothing is written for that row.  All strides in elements of `dtype` (bf16 / fp16 / fp32).  16-byte vector
 * copies: pointers, hidden * esize and every stride * esize must be multiples of 16 bytes.  The QKV GEMV writes rows at ONE stride only, so a ragged
 * decode step lets it write a dense [B, 3*hidden] scratch and scatters from there.
 * Memory regions.  Never read: src row b of a free slot; the q columns of src unless with_q.  Never written: any cache row other than (b, pos[b]), the q
 * columns of that row unless with_q, anything at all for a free slot (the one place where a logical output row is deliberately left as it was).
 */
int stllm_kv_append_rows(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                         const int32_t* pos, int B, int hidden, int max_len, int with_q, void* stream);

/*
 * Frame preprocessing in front of the path — replaces the CPU transform chain of Chat.__init__ / upload_video
 * (stllm/conversation/conversation.py:190-198, 276-279; stllm/test/video_transforms.py:54-60, 94-124, 367-407):
 *   GroupScale(224, BICUBIC) -> GroupCenterCrop(224) -> Stack -> ToTorchFormatTensor -> GroupNormalize(CLIP mean / std)
 * frames: uint8 RGB [n, H, W, 3] (frame n at frames + n * frame_stride_bytes);  out: f32 [n, 3, 224, 224].
 * Bit-identical to torchvision 0.15.1 + Pillow on the CPU: short side -> 224 with Pillow's antialiased bicubic (22-bit
 * fixed-point coefficients, horizontal then vertical pass, uint8 in between), centre crop with round-half-even offsets,
 * x / 255, (x - mean) / std in fp32.  Down-scaling up to ~31x.  `workspace`: >= stllm_preprocess_workspace_bytes(n, H, W)
 * bytes of device memory, 16-byte aligned, no initialisation needed (coefficient tables + the uint8 image between the passes).
 */
int64_t stllm_preprocess_workspace_bytes(int n_frames, int H, int W);   /* -1: unsupported geometry */
int stllm_preprocess_frames(const uint8_t* frames, int64_t frame_stride_bytes, int n_frames, int H, int W, float* out,
                            void* workspace, int64_t workspace_bytes, void* stream);

/*
 * LayerNorm over the last dim of x f32[M,D] (ldx), fp32 statistics (two-pass), affine.
 * Writes out_t T[M,D] (ldo_t) and/or out_f32 [M,D] (ldo_f); either may be NULL.
 * dtype STLLM_BF16X3 (ABI >= 5): out_t is the split image bf16 [M, ldo_t >= 3 D] = (hi | hi | lo) of the fp32 result — the A operand of a bf16x3 GEMM
 * called with STLLM_SPLIT_A_PRESPLIT (same for stllm_rmsnorm).
 * Replaces nn.LayerNorm at eva_vit.py:157,163 (eps 1e-6), blip2.py:103-109 (ln_vision, eps 1e-5),
 * Qformer.py:65,106,282,288,368,374 (eps 1e-12), st_llm.py:39 (mvm_decoder.norm).
 * D % 4 == 0, D <= 8192.
 * Memory regions (stllm_layernorm and stllm_rmsnorm).  Never read: x columns [D, ldx), rows >= M.  Never written: out_t columns [D, ldo_t) ([3 D, ldo_t)
 * for STLLM_BF16X3), out_f32 columns [D, ldo_f), rows >= M of either.
 */
int stllm_layernorm(int dtype, const float* x, int64_t ldx, const float* gamma, const float* beta,
                    float eps, void* out_t, int64_t ldo_t, float* out_f32, int64_t ldo_f,
                    int M, int D, void* stream);

/* RMSNorm (HF LlamaRMSNorm, spec modeling_llama_mem.py:61-78): out = w * x * rsqrt(mean(x^2)+eps). */
int stllm_rmsnorm(int dtype, const float* x, int64_t ldx, const float* gamma, float eps,
                  void* out_t, int64_t ldo_t, float* out_f32, int64_t ldo_f, int M, int D, void* stream);

/*
 * Fused softmax(scale * Q K^T + mask) V, FlashAttention-style (online softmax, LDS-tiled K/V,
 * MFMA 32x32x16; fp32 dtype uses an exact-fp32 vector kernel).  Never materialises S.
 * Replaces eva_vit.py:128-145 (ViT, 16 heads x 88), Qformer.py:205-268 (self: 12x64, cross),
 * HF LlamaAttention softmax(QK^T/sqrt(128) + causal/pad mask) V (spec modeling_llama_mem.py:172-248).
 * q: T, element (b, s, h, d) at q[b*q_bs + s*q_rs + h*D + d]; same for k, v (Skv rows) and out.
 * kv_len: int32[B] or NULL — keys >= kv_len[b] are masked (right-padding / Q-Former text mask,
 *         Qformer.py:785-801 with -10000 == exact 0 after fp32 softmax).
 * causal: key j visible to query i iff j <= i (Sq == Skv).
 * D in {64, 88, 128}; all strides multiples of 8 elements; pointers 16-byte aligned.
 * Memory regions.  Never read: q rows >= Sq and K / V rows >= Skv of a batch entry (the part of a key tile that overhangs Skv is never loaded: the
 * register-staged kernels put zeros into the LDS there, the LDS-DMA kernels a second copy of row Skv - 1, its scores masked), columns behind H * D.  READ, WEIGHTLESS, MUST BE FINITE: the K / V rows in [kv_len[b], Skv).  The tile kernels load whole key tiles up to Skv
 * and mask the SCORES; a masked probability is an exact 0, and 0 x NaN in V would reach the output — so the caller must have written finite values there
 * (the prefill does: they are the projections of the pad positions).  Memory that may be uninitialised behind a length belongs behind Skv, or to
 * stllm_attention_decode_ragged / stllm_attention_shared, which bound their loads by the length.  (The fp32 one-wave-per-row vector kernel bounds its key loop by
 * kv_len; the fp32 matrix-core kernel loads up to Skv like the 16-bit ones: callers must not rely on which kernel runs.)  Query rows at or behind kv_len[b] of a causal call are ordinary rows: read, and their
 * outputs written (they attend the valid keys).  Never written: out behind H * D columns of a row, rows >= Sq of a batch entry.
 * After a call that launched, stllm_last_kernel() names the kernel family and every parameter the dispatcher chose, e.g. "attn_dma_kernel<bf16_t,4,128,512> nw=2
 * q_lds=1 merge_par=1" (nw: query tiles per workgroup after clipping to the tiles there are), "attn_dma88_kernel<f16_t>", "attn_resident_kernel<bf16_t,96,288>",
 * "attn_mfma_kernel<bf16_t,96,1>", "attn_mfma_f32_kernel<128,3>", "attn_f32_kernel"; the string lives until the calling thread's next library call.
 */
int stllm_attention(int dtype, const void* q, int64_t q_bs, int64_t q_rs,
                    const void* k, int64_t k_bs, int64_t k_rs,
                    const void* v, int64_t v_bs, int64_t v_rs,
                    void* out, int64_t o_bs, int64_t o_rs,
                    int B, int H, int Sq, int Skv, int D, float scale, int causal,
                    const int32_t* kv_len, void* stream);

/*
 * stllm_attention with a QUERY OFFSET (additive to ABI 7): query row i (0 <= i < Sq) sits at position q_off + i; with `causal`, key j is visible iff
 * j <= q_off + i.  Needs q_off >= 0 and q_off + Sq <= Skv; q_off = 0 with Sq == Skv is stllm_attention's causal case.  Operand addressing, dtypes and kv_len
 * as for stllm_attention.  The shape this exists for is a short suffix behind a long KV cache (Sq new rows, Skv = q_off + Sq cached keys): in bf16 / fp16 at
 * head_dim 128 such shapes run a key-split kernel pair — the keys of one (batch, head, query chunk) are split over several workgroups that leave fp32
 * partial softmax states in `workspace`, a second launch merges them in a fixed order (deterministic) —, everything else the register-staged tile kernels.
 * workspace: NULL (tile kernels only) or >= stllm_attention_offset_workspace_bytes(B, H, Sq, Skv) bytes, 16-byte aligned, no initialisation needed.
 * stllm_set_option("attn_ksplit", 0 / 1 / -1): never / wherever eligible / by the measured rule (default).  stllm_last_kernel() names the kernel that ran.
 * Memory regions: those of stllm_attention — K / V rows >= Skv = q_off + Sq never read (the cache rows behind the new suffix are uninitialised), rows in
 * [kv_len[b], Skv) read, weightless, must be finite (extend(lengths=) writes the pad rows of a short suffix before the attention runs).  The key-split
 * workspace needs no initialisation: every partial state the merge reads was written by the first launch of the same call.
 */
int64_t stllm_attention_offset_workspace_bytes(int B, int H, int Sq, int Skv);
int stllm_attention_offset(int dtype, const void* q, int64_t q_bs, int64_t q_rs,
                           const void* k, int64_t k_bs, int64_t k_rs,
                           const void* v, int64_t v_bs, int64_t v_rs,
                           void* out, int64_t o_bs, int64_t o_rs,
                           int B, int H, int Sq, int Skv, int D, float scale, int causal,
                           const int32_t* kv_len, int q_off, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * stllm_attention_offset with a query offset and a length PER BATCH ROW (additive to ABI 7; always causal): a block of up to Sq new query rows per batch
 * row, each batch row behind its own number of cached positions (LlamaModel.extend on a ragged cache).  q_off, kv_len: int32 [B] in device memory.  Batch
 * row b holds q_off[b] cached positions and n_b = kv_len[b] - q_off[b] new ones; max_kv is the host-known upper bound of kv_len.  The kernels clamp
 * kv_len[b] to [0, max_kv], q_off[b] to [0, kv_len[b]] and n_b to [0, Sq].  Query row i < n_b of row b sits at position q_off[b] + i and sees key j iff
 * j <= q_off[b] + i.  Operand addressing and stride rules are those of stllm_attention_offset (q typically from a dense [B * Sq, 3 * hidden] scratch, K / V
 * from the cache's own rows).
 *   bf16 / fp16 at head_dim 128: the register-staged tile kernel or the key-split pair of stllm_attention_offset — the plan (key ranges, waves per workgroup,
 *     grid) is the same pure function, evaluated at (B, H, Sq, max_kv); which of the two runs follows a rule measured on ragged rows (up to 512 (batch, head,
 *     query tile) triples and at least 160 keys: the pair), "attn_ksplit" forces it as it does there and stllm_last_kernel() names what ran.  A key range
 *     that begins behind a row's visible end leaves the empty record the merge weighs with 0.
 *   fp32 at head_dim 128, max_kv <= 2048: the one-wave-per-row vector kernel.
 *   anything else returns STLLM_ERR_UNSUPPORTED (stllm_last_error() says what): nothing else runs in its place.
 * With q_off[b] = P and kv_len[b] = P + Sq for every b the output is bit-identical to stllm_attention_offset(q_off = P, Skv = P + Sq, kv_len = NULL) under
 * the same FORCED "attn_ksplit" setting (0 / 1; 16-bit) — left to the rule (-1), the two entries follow rules of their own and may choose different
 * schedules; the same call twice gives the same bits (fixed merge order).
 * workspace: NULL (tile kernel only) or >= stllm_attention_offset_ragged_workspace_bytes(B, H, Sq, max_kv) bytes, 16-byte aligned, no initialisation needed.
 * Memory regions.  Never read: K / V rows at or behind kv_len[b] of batch row b (uninitialised cache memory: the tile kernel runs with LIVE loads, zeros in
 * the LDS instead of a load, not only masked scores); K / V of a row with n_b = 0 altogether.  Read, weightless: nothing.  Pad query rows (i >= n_b) may be
 * read, whatever they hold (NaN included), and influence no other row.  Written: every out row (b, i < Sq) at columns [0, H * 128) — pad rows as exact zeros,
 * never NaN; nothing else.  Workspace: every record the merge reads was written by the partial pass of the same call.
 */
int64_t stllm_attention_offset_ragged_workspace_bytes(int B, int H, int Sq, int max_kv);
int stllm_attention_offset_ragged(int dtype, const void* q, int64_t q_bs, int64_t q_rs,
                                  const void* k, int64_t k_bs, int64_t k_rs,
                                  const void* v, int64_t v_bs, int64_t v_rs,
                                  void* out, int64_t o_bs, int64_t o_rs,
                                  int B, int H, int Sq, int max_kv, int D, float scale,
                                  const int32_t* q_off, const int32_t* kv_len, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Ragged KV-cache append of token BLOCKS (additive to ABI 7): stllm_kv_append_rows for S dense rows per batch row.  For every b and every
 * i < min(n[b], S) with 0 <= pos0[b] + i < max_len the [k | v] columns of the dense fused row src[(b*S + i)*ld_src .. + 3*hidden) are copied to
 * cache[b*batch_stride + (pos0[b] + i)*row_stride + the same columns].  pos0, n: int32 [B] in device memory.  Dtypes, strides and alignment as for
 * stllm_kv_append_rows; B * S <= 65535.
 * Memory regions.  Never read: the q columns of src, the pad rows i >= n[b], every row of a batch row with n[b] <= 0.  Never written: the q columns of the
 * cache, any cache row other than (b, pos0[b] + i) for i < n[b], anything at all for a batch row with n[b] <= 0 or behind max_len.
 */
int stllm_kv_append_spans(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                          const int32_t* pos0, const int32_t* n, int B, int S, int hidden, int max_len, void* stream);

/*
 * stllm_attention_offset_ragged on a PACKED query buffer (additive to ABI 7; always causal): R segments, the step of a serving loop that carries one token for
 * every running request and a whole prompt for a newly admitted one (LlamaModel.step_segments).  q and out hold T packed rows (row strides q_rs / o_rs, no
 * batch stride); K / V are the rows of a cache of n_slots rows (k_bs / v_bs between cache rows).  slot, row0, q_off, kv_len: int32 [R] in device memory:
 *   slot[r]    cache row of segment r (K / V base = slot[r] * k_bs)
 *   row0[r]    first packed row of the segment (q / out base = row0[r] * q_rs / o_rs)
 *   q_off[r]   cached positions in front of the segment
 *   kv_len[r]  q_off[r] + n_r, n_r the segment's new rows; clamped as stllm_attention_offset_ragged clamps them (kv_len to [0, max_kv], q_off to
 *              [0, kv_len], n_r to [0, max_n])
 * Query row i < n_r of segment r is packed row row0[r] + i, sits at position q_off[r] + i and sees key j of cache row slot[r] iff j <= q_off[r] + i.
 * max_n bounds n_r and sizes the query-tile grid, max_kv bounds kv_len.  The host keeps slots distinct and in range and the segments' packed rows disjoint;
 * on top of that the kernels guard the tables: a segment with slot[r] outside [0, n_slots), row0[r] < 0 or row0[r] + n_r > T does nothing at all.
 * Coverage, dispatch rule, "attn_ksplit" forcing, workspace size and stllm_last_kernel() are those of stllm_attention_offset_ragged, the plan evaluated at
 * (R, H, max_n, max_kv); anything else returns STLLM_ERR_UNSUPPORTED.  With slot[r] = r, row0[r] = r * Sq, every n_r = Sq = max_n and T = R * Sq the output
 * is bit-identical to stllm_attention_offset_ragged(B = R) under the same forced "attn_ksplit" (0 / 1); the same call twice gives the same bits.
 * Memory regions.  Never read: K / V at or behind kv_len[r]; every cache row not named by a live segment; packed q rows that belong to no live segment's
 * [row0[r], row0[r] + n_r) — a pad lane of a query tile loads zeros, not the neighbouring segment's row —, rows at or behind T among them.  Written: exactly
 * the packed out rows row0[r] + i, i < n_r, of live segments, at columns [0, H * 128); no pad row, no zero row, nothing else.  Workspace: every record the
 * merge reads was written by the partial pass of the same call (pad rows leave no record and the merge reads none).
 */
int64_t stllm_attention_segments_workspace_bytes(int R, int H, int max_n, int max_kv);
int stllm_attention_segments(int dtype, const void* q, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs, const void* v, int64_t v_bs,
                             int64_t v_rs, void* out, int64_t o_rs, int R, int H, int D, int T, int n_slots, int max_n, int max_kv, float scale,
                             const int32_t* slot, const int32_t* row0, const int32_t* q_off, const int32_t* kv_len, void* workspace,
                             int64_t workspace_bytes, void* stream);

/*
 * stllm_kv_append_spans for a PACKED source (additive to ABI 7).  slot, row0, pos0, n: int32 [R] in device memory.  For every segment r and every
 * i < n[r] (n[r] <= max_n, which sizes the grid) with 0 <= pos0[r] + i < max_len the [k | v] columns of the packed fused row src[(row0[r] + i)*ld_src ..
 * + 3*hidden) are copied to cache[slot[r]*batch_stride + (pos0[r] + i)*row_stride + the same columns], 16 bytes per lane.  A segment with slot[r] outside
 * [0, n_slots), row0[r] < 0 or row0[r] + n[r] > T writes nothing.  Dtypes, strides and alignment as for stllm_kv_append_rows; R, max_n <= 65535.  With
 * slot[r] = r and row0[r] = r * S the result is bit-identical to stllm_kv_append_spans.
 * Memory regions.  Never read: the q columns of src, packed rows outside the live segments.  Never written: the q columns of the cache, any cache row not
 * named by a segment, any position other than pos0[r] + i, i < n[r], of a named one, anything behind max_len.
 */
int stllm_kv_append_segments(int dtype, const void* src, int64_t ld_src, void* cache, int64_t batch_stride, int64_t row_stride,
                             const int32_t* slot, const int32_t* row0, const int32_t* pos0, const int32_t* n, int R, int T, int n_slots,
                             int max_n, int hidden, int max_len, void* stream);

/*
 * In-place re-order of the cache rows of beam groups (additive to ABI 7): what beam search's `past.index_select(0, beam_idx)` does to one
 * layer buffer, for the rows and positions that can differ only.  The `rows` cache rows come in groups of nb consecutive rows, group g = rows
 * [g*nb, (g+1)*nb).  src: int32 [rows], lo / hi: int32 [rows / nb], all in device memory.  For every group g, every row r of it with src[r] != r and every
 * position p in [max(lo[g], 0), min(hi[g], capacity)) (positions of the buffer itself: local ones for a cache with a base) the [k | v] columns of
 * cache[r*batch_stride + p*row_stride ..] receive what the same columns of cache[src[r]*batch_stride + p*row_stride ..] held BEFORE the call.  src may be
 * any mapping inside a group (a fan-out, a cycle, a mix).  A src[r] outside its own group is taken as r, so a bad table cannot reach another group's rows.
 * max_span: the host-known bound of the CLAMPED range's length, min(hi[g], capacity) - max(lo[g], 0) (hi[g] - lo[g] bounds it); it sizes the grid, which
 * counts from the clamped start: positions at or behind max(lo[g], 0) + max_span are not moved.
 * Schedule: one thread owns one 16-byte cell (position, column piece) of a group; it loads the cell from all nb rows, then stores the rows whose source
 * differs.  No other thread touches that cell in any row of the group: no scratch buffer, no second launch, no barrier, no atomics — the same call on
 * the same bytes gives the same bytes.  nb <= 16 (the cells live in registers); anything else returns STLLM_ERR_UNSUPPORTED and writes nothing.
 * Dtypes (it moves bytes), strides and alignment as for stllm_kv_append_rows; rows % nb == 0, rows / nb <= 65535.
 * Memory regions.  Never read: the q columns; positions outside [lo[g], hi[g]); every row of a group with hi[g] <= lo[g] or whose src is the identity.
 * (A group that moves anything reads the range of ALL its nb rows, also rows that are nobody's source: bytes are moved, never interpreted.)  Never
 * written: the q columns, positions outside the range, rows with src[r] == r, rows whose src[r] lies outside their own group, groups with hi[g] <= lo[g].
 */
int stllm_kv_reorder_rows(int dtype, void* cache, int64_t batch_stride, int64_t row_stride, const int32_t* src, const int32_t* lo, const int32_t* hi,
                          int rows, int nb, int hidden, int capacity, int max_span, void* stream);

/*
 * stllm_attention_segments on a SHARED BASE (additive to ABI 7; always causal): the R segments of a packed query buffer all sit behind the same
 * P prefix keys — ONE row of a base buffer (kp / vp, row strides kp_rs / vp_rs) that is only read — and each reads its own suffix keys in row slot[r] of the
 * slot buffers (ks / vs, (slot, row) strides).  The four int32 [R] device tables are those of stllm_attention_segments in SUFFIX-LOCAL positions:
 *   slot[r], row0[r]   as there
 *   sfx_off[r]         suffix positions held before this step (0: a fresh admission)
 *   sfx_len[r]         the suffix end after the append: n_r = sfx_len[r] - sfx_off[r] new rows; clamped as there (sfx_len to [0, max_sfx], sfx_off to
 *                      [0, sfx_len], n_r to [0, max_n])
 * Query row i < n_r of segment r is packed row row0[r] + i; it sees all P prefix keys and the suffix keys j <= sfx_off[r] + i of slot row slot[r].
 * The table guard is stllm_attention_segments': a segment with slot[r] outside [0, n_slots), row0[r] < 0, row0[r] + n_r > T or n_r <= 0 does nothing at all.
 * bf16 / fp16 at head_dim 128: three launches, no atomics, flags or polling — the prefix as one non-causal problem of T query rows and P keys planned at
 * (1, H, T, P), the suffixes per segment planned at (R, H, max_n, max_sfx), both leaving (O, m, l) records in the workspace, and a merge that folds a row's
 * prefix records, then its suffix records, ascending.  With slot[r] = r, row0[r] = r * n, every sfx_off[r] = off and n_r = n the output is bit-identical to
 * stllm_attention_shared(B = R, G = 1, Sq = n, causal = 1, sfx_q_off = off) on the same buffers.  fp32 at head_dim 128: one vector kernel (no workspace).
 * Anything else returns STLLM_ERR_UNSUPPORTED.  stllm_last_kernel() is "attn_segments_shared".
 * workspace: >= stllm_attention_segments_shared_workspace_bytes(R, H, T, P, max_n, max_sfx) bytes (a pure function of the two plans; -1 for an empty
 * problem), 16-byte aligned, no initialisation needed (unused in fp32).
 * Memory regions.  Never read: base rows at or behind P; suffix K / V at or behind sfx_len[r]; slot rows named by no live segment; packed q rows at or behind
 * T.  (The prefix pass reads all T packed q rows, whichever segment owns them.)  Written: exactly the packed out rows row0[r] + i, i < n_r, of live
 * segments, at columns [0, H * 128).  Every record the merge reads was written by the two passes of the same call.
 */
int64_t stllm_attention_segments_shared_workspace_bytes(int R, int H, int T, int P, int max_n, int max_sfx);
int stllm_attention_segments_shared(int dtype, const void* q, int64_t q_rs, const void* kp, int64_t kp_rs, const void* vp, int64_t vp_rs, int P,
                                    const void* ks, int64_t ks_bs, int64_t ks_rs, const void* vs, int64_t vs_bs, int64_t vs_rs, void* out,
                                    int64_t o_rs, int R, int H, int D, int T, int n_slots, int max_n, int max_sfx, float scale,
                                    const int32_t* slot, const int32_t* row0, const int32_t* sfx_off, const int32_t* sfx_len, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/*
 * Row gather (token-block assembly, dynamic masking, residual-index selection, embedding lookup):
 *   dst[i, :] = scale * ((idx_a[i] >= 0 ? src_a[idx_a[i], :] : src_b[-idx_a[i]-1, :]) + (add ? add[idx_add[i], :] : 0))
 * all f32, D % 4 == 0.  The same kernel re-orders tokens between the BT-Adapter's spatial '(b t) p' and temporal
 * 'b (p t)' layouts and averages branches (eva_btadapter.py:179-196, 261-310).  Replaces torch.cat / index / embed_tokens glue at st_llm.py:391-404,
 * 416-431, 473-476, 491, 509, 524-530 and conversation.py:288-293, 336-337.
 */
int stllm_gather_rows(const float* src_a, int64_t ld_a, const float* src_b, int64_t ld_b,
                      const int32_t* idx_a, const float* add, int64_t ld_add, const int32_t* idx_add,
                      float* dst, int64_t ld_dst, int n_rows, int D, float scale, void* stream);

/* out[b, j] = mean_t x[b, t, j]  (x f32 [B,T,J] contiguous) — st_llm.py:468,471; conversation.py:282,287 */
int stllm_mean_t(const float* x, float* out, int B, int T, int64_t J, void* stream);

/* x[n*257, :] = cls_token + pos_embed[0]  for every frame — eva_vit.py:328-331 (CLS row) */
int stllm_vit_cls_rows(const float* cls, const float* pos, float* x, int64_t ldx, int n_frames, int D,
                       void* stream);

/* MVM loss pieces (st_llm.py:89-91): out[i] = 2 - 2 * <a_i/|a_i|, b_i/|b_i|>, rows gathered by index */
int stllm_cosine_rows(const float* a, int64_t lda, const int32_t* idx_a, const float* b, int64_t ldb,
                      const int32_t* idx_b, float* out, int n_rows, int D, void* stream);

/* shifted-label cross entropy rows (st_llm.py:127-135): loss[i] = logsumexp(logits[i]) - logits[i,labels[i]];
 * labels[i] < 0 (ignore_index) -> 0.  The caller averages over the valid rows. */
int stllm_cross_entropy_rows(const float* logits, int64_t ldl, const int32_t* labels, float* loss,
                             int n_rows, int V, void* stream);

/* out T[M,D] = cast(x f32[M,D]) — the .to(dtype)/type_as casts at st_llm.py:453,474 and the autocast
 * boundary of blip2.py:36-44, when a GEMM consumes rows of the fp32 stream without a norm in between. */
int stllm_cast_rows(int dtype, const float* x, int64_t ldx, void* out, int64_t ldo, int M, int D, void* stream);

/*
 * Token selection on the device (generation.py, selection="device"): what HF's logits processors, warpers and `argmax` / `multinomial` / `topk`
 * do to one row of next-token logits, in ONE launch with one workgroup per row.  The row is staged once into the LDS as fp32 (columns >= V of the
 * padded row are never read) and every later pass reads the LDS only; all reductions run in a fixed order, so a launch is bit-reproducible.
 * V * 4 bytes (+ n_prev * 4 when a penalty applies) must fit the 160 KiB of LDS less 4 KiB of scratch: otherwise STLLM_ERR_UNSUPPORTED, nothing
 * else runs in its place.  Rows that are all -inf or hold a NaN are outside the contract.
 *
 * Per row r, s = logits[r, :V]:
 *   1. penalty != 1: for every DISTINCT id in prev[r, :n_prev] (ids outside [0, V) are ignored): s[id] = s[id] < 0 ? s[id] * penalty : s[id] / penalty,
 *      once per id, from the original score (IEEE fp32 multiply / divide)                              — RepetitionPenaltyLogitsProcessor
 *   2. suppress_eos (cur_len < min_length) and 0 <= eos_id < V: s[eos_id] = -inf                      — MinLengthLogitsProcessor
 *   3. sample == 0: token = lowest index of max(s).
 *      sample != 0: s /= temperature; e_i = exp(s_i - max); token i is KEPT iff sum_{j: e_j <= e_i} e_j > (1 - top_p) * sum_j e_j, or i is the argmax
 *      (TopPLogitsWarper, min_tokens_to_keep = 1; a tie group at the threshold is kept whole; top_p >= 1 keeps every e_i > 0); with Z_kept the sum
 *      over the kept ids, token = the smallest kept id whose inclusive prefix sum over the kept ids, in id order, exceeds u[r] * Z_kept
 *      (u[r] in [0, 1), a device float the caller draws); the last kept id if rounding runs past the end.
 *   4. unfinished (nullable, int32 [rows], in / out): a row at 0 emits pad_id and nothing else; a row that emits eos_id is set to 0.
 *   5. out[r * out_stride] = token (int32).  aux (nullable, float [rows, 4]): max, log sum exp(s - max), the threshold e-value (0 when greedy),
 *      Z_kept / Z_all (1 when greedy); rows finished on entry leave their aux untouched.
 */
typedef struct stllm_select_args {
  const float* logits;       /* [rows, ldl] fp32 */
  int64_t ldl;               /* row stride in floats (>= V; any alignment) */
  int rows, V;
  const int32_t* prev;       /* [rows, ld_prev] int32 ids generated so far; may be NULL when n_prev == 0 */
  int64_t ld_prev;
  int n_prev;
  float penalty;             /* 1: none */
  int suppress_eos;
  int eos_id;                /* < 0: none */
  int pad_id;
  int sample;                /* 0 greedy, 1 top-p sampling */
  float temperature;         /* > 0 */
  float top_p;
  const float* u;            /* [rows], sample only */
  int32_t* unfinished;       /* nullable */
  int32_t* out;
  int64_t out_stride;        /* in elements */
  float* aux;                /* nullable, [rows, 4] */
} stllm_select_args;
int stllm_select_tokens(const stllm_select_args* args, void* stream);

/*
 * Beam-search candidates: per row r (= prompt * num_beams + beam), lp = s - max - log sum exp(s - max) (log_softmax), then steps 1 and 2 above applied
 * TO lp (HF's order in beam search), score = lp + beam_score[r]; the k best (1 <= k <= 32, k <= V) ordered by (score descending, token ascending):
 * cand_score fp32 [rows, k], cand_token int32 [rows, k].  The host merges the num_beams * k candidates of a prompt by (score descending,
 * beam * V + token ascending): the first 2 * num_beams of that union are what a top-k over num_beams * V scores returns.  Same staging, LDS limit
 * and error behaviour as stllm_select_tokens.
 */
typedef struct stllm_beam_args {
  const float* logits;
  int64_t ldl;
  int rows, V;
  const int32_t* prev;
  int64_t ld_prev;
  int n_prev;
  float penalty;
  int suppress_eos;
  int eos_id;
  const float* beam_score;   /* [rows] */
  int k;
  float* cand_score;         /* [rows, k] */
  int32_t* cand_token;       /* [rows, k] */
} stllm_beam_args;
int stllm_beam_candidates(const stllm_beam_args* args, void* stream);

/*
 * Token selection with per-slot state (serving.Engine(state="device")): stllm_select_tokens for the slots of a continuous batch, each
 * with its own step count, history, EOS suppression, token budget and stop-sequence match.  ONE launch, one workgroup per slot; staging, reductions, LDS
 * limit and error behaviour are stllm_select_tokens' (the row body is the same device function).  (V + ld_ids) * 4 bytes must fit the LDS limit above —
 * a whole history, whatever the slots hold in this step: otherwise STLLM_ERR_UNSUPPORTED.
 *
 * src[s] is the row of `logits` that belongs to slot s in this step; src[s] < 0 or >= rows: the slot is NOT SERVED — nothing of it is read (not its
 * state, ids, u) and nothing is written.  state[s] = (live, n_gen, max_new, pending), in / out.
 *   A served slot with live == 0: pending = pad_id; nothing else is read or written (its ids, u and aux are untouched).
 *   A served slot with live != 0, c = n_gen clamped to [0, ld_ids - 1]:
 *     token = steps 1 - 3 of stllm_select_tokens on logits[src[s], :V] with prev = ids[s, :c], n_prev = c, suppress_eos = (eos_id >= 0 && n_gen < min_length)
 *             and u[s];
 *     ids[s, c] = token, n_gen = c + 1, pending = token;
 *     live = 0 iff token == eos_id, or c + 1 >= max_new, or ids[s, :c + 1] ends in stops[j, :stop_len[j]] for some j with 0 < stop_len[j] <= c + 1
 *             (and stop_len[j] <= ld_stop); otherwise live = 1.
 *     aux[s] (nullable, float [n_slots, 4]) as stllm_select_tokens writes it.
 * Token and aux of a live served slot are bit-identical to a stllm_select_tokens launch of that row alone with that slot's n_prev, suppress_eos and u.
 * Never read: logits columns >= V and rows that no src names; ids[s, j] for j >= n_gen (they may hold anything); stops[j, i] for i >= stop_len[j];
 * u unless sample.  Never written: logits, src, u, stops, stop_len; ids other than ids[s, c]; anything of a slot that is not served.  Two slots may
 * name the same row: rows are only read.
 */
typedef struct stllm_select_slots_args {
  const float* logits;       /* [rows, ldl] fp32 */
  int64_t ldl;               /* row stride in floats (>= V; any alignment) */
  int rows, V;
  int n_slots;
  const int32_t* src;        /* [n_slots] logits row of the slot in this step; outside [0, rows): not served */
  int32_t* state;            /* [n_slots, 4] (live, n_gen, max_new, pending), in / out */
  int32_t* ids;              /* [n_slots, ld_ids] generated history, in / out */
  int64_t ld_ids;            /* >= 1 */
  float penalty;             /* 1: none */
  int min_length;
  int eos_id;                /* < 0: none */
  int pad_id;
  int sample;                /* 0 greedy, 1 top-p sampling */
  float temperature;         /* > 0 */
  float top_p;
  const float* u;            /* [n_slots], sample only */
  const int32_t* stops;      /* [n_stop, ld_stop]; may be NULL when n_stop == 0 */
  int64_t ld_stop;
  const int32_t* stop_len;   /* [n_stop] */
  int n_stop;
  float* aux;                /* nullable, [n_slots, 4] */
} stllm_select_slots_args;
int stllm_select_slots(const stllm_select_slots_args* args, void* stream);

/*
 * Beam-search candidates with per-row state (serving.Engine(num_beams > 1, state="device"); additive to ABI 7): stllm_beam_candidates for
 * the beam rows of a continuous batch, each request at its own step.  ONE launch, one workgroup per candidate row; staging, reductions and error behaviour
 * are stllm_beam_candidates' (the row body is the same kernel template).  (V + ld_prev) * 4 bytes must fit the LDS limit of stllm_select_tokens — a whole
 * history, whatever the rows hold in this step: otherwise STLLM_ERR_UNSUPPORTED.
 *
 * src[r] is the row of `logits` that candidate row r reads in this step; src[r] < 0 or >= n_logits_rows: the row is NOT SERVED — nothing of it is read
 * (not its n_prev, prev, beam_score) and nothing is written.  Several rows may name the same logits row (the admission step: all beams of a request start
 * from the prompt's one row); rows are only read.  A served row r, c = n_prev[r] clamped to [0, ld_prev]:
 *   cand_score[r, :k], cand_token[r, :k] = what stllm_beam_candidates gives for logits row src[r] with prev = prev[r, :c], n_prev = c,
 *   suppress_eos = (eos_id >= 0 && n_prev[r] < min_length) and beam_score[r] — bit for bit a stllm_beam_candidates launch of that row alone.
 * Never read: logits columns >= V and rows that no src names; prev[r, j] for j >= n_prev[r] (they may hold anything).  Never written: logits, src, prev,
 * n_prev, beam_score; cand_score / cand_token of a row that is not served.
 */
typedef struct stllm_beam_rows_args {
  const float* logits;       /* [n_logits_rows, ldl] fp32 */
  int64_t ldl;               /* row stride in floats (>= V; any alignment) */
  int n_logits_rows, V;
  int rows;                  /* candidate rows */
  const int32_t* src;        /* [rows] logits row of the candidate row in this step; outside [0, n_logits_rows): not served */
  const int32_t* prev;       /* [rows, ld_prev] int32 ids generated so far; may be NULL when ld_prev == 0 */
  int64_t ld_prev;
  const int32_t* n_prev;     /* [rows] */
  float penalty;             /* 1: none */
  int min_length;
  int eos_id;                /* < 0: none */
  const float* beam_score;   /* [rows] */
  int k;
  float* cand_score;         /* [rows, k] */
  int32_t* cand_token;       /* [rows, k] */
} stllm_beam_rows_args;
int stllm_beam_candidates_rows(const stllm_beam_rows_args* args, void* stream);

/* =========================================================================================================================
 * Backward / optimizer entry points.  The reference has no such code of its own: the gradients come
 * from torch.autograd over st_llm.py:116-146 (shifted CE + loss_mvm) driven by HF Trainer + DeepSpeed (train_hf.py,
 * stllm_trainer.py:317, config/(model)_stllm_qa.yaml: freeze_LLM False, bf16, AdamW lr 2e-5).  Each entry point below is the
 * transpose (vector-Jacobian product) of one forward entry point above, with the same pointer / stride / stream conventions;
 * GEMM-shaped gradients reuse stllm_gemm on operands re-laid-out by stllm_transpose:
 *      y = x W^T :   dx = gemm(A = dy,   W = W^T [K, N])          dW = gemm(A = dy^T [N, Mp], W = x^T [K, Mp])  (fp32 out)
 * ========================================================================================================================= */

/* dst[c, r] = src[r, c] for r < rows, 0 for rows <= r < rows_padded (zero K-padding for the GEMM).  dtype sizes 2 or 4. */
int stllm_transpose(int dtype, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols, int rows_padded,
                    void* stream);

/* scratch of the two norm-backward entry points and of stllm_colsum: per-row statistics + column partial sums */
int64_t stllm_norm_bwd_workspace_bytes(int rows, int cols);

/* Transpose of stllm_rmsnorm (modeling_llama_mem.py:61-78): with r = rsqrt(mean(x^2) + eps), xh = x r, g = gamma * dy:
 *   dx (+)= r * (g - xh * mean(g * xh))      dgamma[c] = sum_rows dy * xh       (dy: T_dy [rows, cols], T_dy any dtype code)
 * accumulate != 0 adds into dx (the fp32 residual-stream gradient), else overwrites.  Deterministic (no atomics). */
int stllm_rmsnorm_bwd(int dy_dtype, const float* x, int64_t ldx, const float* gamma, float eps, const void* dy, int64_t lddy,
                      float* dx, int64_t lddx, int accumulate, float* dgamma, void* workspace, int64_t workspace_bytes, int rows,
                      int cols, void* stream);

/* Transpose of stllm_layernorm (st_llm.py:39 mvm_decoder.norm): xh = (x - mu) r;
 *   dx (+)= r * (g - mean(g) - xh * mean(g * xh))      dgamma = sum dy * xh      dbeta = sum dy */
int stllm_layernorm_bwd(int dy_dtype, const float* x, int64_t ldx, const float* gamma, float eps, const void* dy, int64_t lddy,
                        float* dx, int64_t lddx, int accumulate, float* dgamma, float* dbeta, void* workspace,
                        int64_t workspace_bytes, int rows, int cols, void* stream);

/* SiLU(gate) * up on RAW gate/up activations in the packed [32 gate | 32 up] column groups of the SWIGLU epilogue
 * (modeling_llama_mem.py:143-144).  Training keeps the raw activations (STORE epilogue) so the backward needs no
 * recomputation:  gu T[rows, 2*inter] -> out T[rows, inter]. */
int stllm_swiglu(int dtype, const void* gu, int64_t ldgu, void* out, int64_t ldo, int rows, int inter, void* stream);

/* d gate = dg * up * s * (1 + gate * (1 - s)),  d up = dg * gate * s,  s = sigmoid(gate); output in the packed layout of gu. */
int stllm_swiglu_bwd(int dtype, const void* gu, int64_t ldgu, const void* dg, int64_t lddg, void* dgu, int64_t lddgu, int rows,
                     int inter, void* stream);

/* Transpose of the ROPE epilogue's rotation, in place on the first rope_cols columns of d T[rows, cols] (packed head layout,
 * position = row % rope_seq; cos/sin as for stllm_gemm):  dx1 = dy1 c + dy2 s,  dx2 = dy2 c - dy1 s. */
int stllm_rope_bwd(int dtype, void* d, int64_t ld, const float* cos_t, const float* sin_t, int rows, int cols, int rope_seq,
                   int rope_cols, void* stream);

/* Gradients of stllm_attention: dq, dk, dv from q, k, v, the forward output o and its gradient dO; same element addressing as
 * stllm_attention for all eight operands; masks as in the forward (causal needs Sq == Skv).  D % 8 == 0, D <= 128.
 * bf16 / f16 run on MFMA kernels (the Llama prefill, the Q-Former's 64-wide self- and cross-attention heads, EVA's 88-wide heads padded
 * to 96 in LDS), fp32 on fp32-FMA kernels (also for 16-bit operands with STLLM_ATTN_BWD_VALU=1 in the environment).
 * workspace: stllm_attention_bwd_workspace_bytes(B, H, Sq) (log-sum-exp and dO.o per query row), no initialisation needed: every word the second
 * launch reads was written by the first launch of the same call.
 * Memory regions.  Never read: q / o / dO rows >= Sq and K / V rows >= Skv of a batch entry (a tile overhanging the end is filled with zeros in the
 * LDS / registers, not loaded), columns behind H * D of any operand, and dq / dk / dv themselves (outputs only: the caller may pass uninitialised
 * memory).  READ, WEIGHTLESS, MUST BE FINITE: the K / V rows in [kv_len[b], Skv) — the kernels load whole key tiles up to Skv and zero the
 * PROBABILITY, and dP = dO V^T of such a row is multiplied by that exact 0: a NaN or Inf there would reach dq, dk and dv.  Query rows at or behind
 * kv_len[b] are ordinary rows (read; they attend the valid keys).  Written: EVERY element of dq inside [B, Sq, H * D] and of dk and dv inside
 * [B, Skv, H * D] — also the rows nobody attends: dk and dv rows at or behind kv_len[b] are written as exact 0, so a GEMM may read the whole
 * block afterwards.  kv_len[b] <= 0: no key is visible, dq, dk and dv of that batch row are written as 0 (zeros, never NaN, as in the decode
 * kernels).  Never written: columns behind H * D of a row, rows >= Sq (dq) / >= Skv (dk, dv) of a batch entry. */
int64_t stllm_attention_bwd_workspace_bytes(int B, int H, int Sq);
int stllm_attention_bwd(int dtype, const void* q, int64_t q_bs, int64_t q_rs, const void* k, int64_t k_bs, int64_t k_rs,
                        const void* v, int64_t v_bs, int64_t v_rs, const void* o, int64_t o_bs, int64_t o_rs,
                        const void* dO, int64_t do_bs, int64_t do_rs, void* dq, int64_t dq_bs, int64_t dq_rs,
                        void* dk, int64_t dk_bs, int64_t dk_rs, void* dv, int64_t dv_bs, int64_t dv_rs,
                        int B, int H, int Sq, int Skv, int D, float scale, int causal, const int32_t* kv_len,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Transpose of stllm_cross_entropy_rows summed with weight `scale` (st_llm.py:127-135; scale = 1 / #valid rows):
 * dlogits[i, c] = scale * (softmax(logits[i, :vocab])[c] - [c == labels[i]]) for labels[i] >= 0, else 0; columns
 * vocab .. cols_padded-1 (lm_head padding) are written as 0.  dlogits: T[rows, cols_padded]. */
int stllm_cross_entropy_bwd(int dtype, const float* logits, int64_t ldl, const int32_t* labels, float scale, void* dlogits,
                            int64_t lddl, int rows, int vocab, int cols_padded, void* stream);

/* Transpose of stllm_gather_rows: (idx[i] >= 0 ? dst_a[idx[i]] : dst_b[-idx[i]-1]) += scale * src[i]  (fp32 atomics; rows that
 * are hit more than once — repeated token ids — make the summation order, not the set of summands, run-dependent). */
int stllm_scatter_add_rows(const float* src, int64_t ld_src, const int32_t* idx, float* dst_a, int64_t ld_a, float* dst_b,
                           int64_t ld_b, int n_rows, int D, float scale, void* stream);

/* d/da of  scale * sum_i stllm_cosine_rows(a, b)[i]  (st_llm.py:89-91; b is the detached target):
 * da[i] = -2 scale / |a_i| * (b_i/|b_i| - cos_i * a_i/|a_i|),  rows gathered by index as in the forward. */
int stllm_cosine_rows_bwd(const float* a, int64_t lda, const int32_t* idx_a, const float* b, int64_t ldb, const int32_t* idx_b,
                          float scale, float* da, int64_t ldda, int n_rows, int D, void* stream);

/* out[c] = sum_rows x[r, c]  (bias gradients); workspace: stllm_norm_bwd_workspace_bytes(rows, cols).  Deterministic. */
int stllm_colsum(int dtype, const void* x, int64_t ldx, float* out, int rows, int cols, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* dx = dy * (y > 0)  — the ReLU between down_proj and up_proj (st_llm.py:473-475); cols % 8 == 0. */
int stllm_relu_bwd(int dtype, const void* dy, int64_t lddy, const void* y, int64_t ldy, void* dx, int64_t lddx, int rows, int cols,
                   void* stream);

/* exact-erf GELU (nn.GELU(), eva_vit.py:45; Qformer.py:347 ACT2FN["gelu"]) on RAW pre-activations and its derivative: training keeps the
 * pre-activations (STORE epilogue) because the fused GELU epilogue of the forward does not.  cols % 8 == 0. */
int stllm_gelu(int dtype, const void* x, int64_t ldx, void* out, int64_t ldo, int rows, int cols, void* stream);
int stllm_gelu_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int rows, int cols,
                   void* stream);

/* x[r, :] *= scale[idx ? idx[r] : r / rows_per_group], in place (T [rows, cols], cols % 8 == 0): timm's drop_path as called by the
 * BT-Adapter blocks in train mode (eva_vit.py:30-38, eva_btadapter.py:274-280, 303) — per-sample keep mask / keep_prob — and, being
 * linear and diagonal, its own backward. */
int stllm_scale_rows(int dtype, void* x, int64_t ldx, const float* scale, const int32_t* idx, int rows_per_group, int rows, int cols,
                     void* stream);

/* Transpose of stllm_mean_t up to the 1/T factor: dst[b, t, j] += scale * src[b, j]  (f32, J % 4 == 0). */
int stllm_bcast_add_t(float* dst, const float* src, int B, int T, int64_t J, float scale, void* stream);

/* torch.optim.AdamW step on flat fp32 state (what HF Trainer instantiates for the reference's runs):
 *   g' = grad_scale * g;  p *= 1 - lr * weight_decay;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps);   p16 (optional, dtype code p16_dtype) = cast(p). */
int stllm_adamw(float* p, const float* g, float* m, float* v, void* p16, int p16_dtype, int64_t n, float lr, float beta1,
                float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* out[0] += sum x^2  (gradient-norm clipping, torch.nn.utils.clip_grad_norm_); the caller zeroes out[0]. */
int stllm_sumsq(const float* x, int64_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STLLM_HIP_H */
