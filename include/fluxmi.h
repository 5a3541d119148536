/* fluxmi.h -- C ABI of libfluxmi.so, the MI355X (gfx950) implementation of the Flux denoise hot path
 * of aredden/flux-fp8-api.
 *
 * The reference has no FFI of its own: its only operator-swap mechanism is Python module replacement
 * (float8_quantize.py:320-392 swaps nn.Linear -> F8Linear / the external cublas_ops.CublasLinear).
 * This header is therefore the boundary a maintainer binds from the reference's Python operator
 * classes (ctypes stub in INTEGRATION.md).  Each entry point cites the reference code it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers, sizes, a hipStream_t passed as void* (0 = null stream)
 *   - every function returns 0 on success; non-zero -> call fluxmi_last_error() (thread-local string)
 *   - nothing throws across the ABI; no allocation and no host synchronisation inside any op call, fluxmi_engine_forward or
 *     fluxmi_engine_run_block (all are hipGraph-capturable).  Allocation happens in fluxmi_engine_create (constants, pinned
 *     staging, events) and fluxmi_engine_prepare (workspace + the step-ahead modulation table) only.  fluxmi_engine_denoise
 *     allocates nothing and never waits on the stream; its only host waits are (a) on the event of the PREVIOUS request's schedule
 *     upload before the pinned staging buffer is rewritten (complete long before, in practice never blocks) and (b) one
 *     hipStreamSynchronize the first time a shape is seen, immediately before the hipGraph capture
 *   - multi-GPU: the library holds no communicator.  The path shards by batch with no data-path collective, so the
 *     three small exchanges (embeddings + noise broadcast, per-layer amax MAX during calibration, latent gather) are made by the
 *     host with torch.distributed over RCCL (flux-fp8-api_amd/fluxmi/dist.py); the engine exposes the one hook they need that
 *     lies INSIDE a forward pass: fluxmi_engine_set_amax_exchange
 *   - caller owns every buffer passed in; row strides ("ld") are in ELEMENTS of that buffer
 *   - tensors are bf16 (uint16 storage) unless stated; fp8 tensors are OCP e4m3fn / e5m2 bytes
 *   - an engine handle is not re-entrant: the host wrapper serialises calls per engine
 */
#ifndef FLUXMI_H
#define FLUXMI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FLUXMI_ABI_VERSION 5

/* fp8 format codes (torch.float8_e4m3fn / torch.float8_e5m2, float8_quantize.py:39,43) */
#define FLUXMI_E4M3 0
#define FLUXMI_E5M2 1

/* GEMM epilogues: what happens to h = bf16(acc * sa * sb + bias) */
enum {
  FLUXMI_EPI_BF16 = 0,       /* C(bf16) = h                                   float8_quantize.py:284-292 */
  FLUXMI_EPI_GELU_QUANT = 1, /* C(fp8)  = q(bf16(gelu_tanh(h)), q_scale)      flux_model.py:301,335 + float8_quantize.py:274-276 */
  FLUXMI_EPI_GATE_RESID = 2, /* C(bf16) = bf16(resid + bf16(gate[n] * h))     flux_model.py:387-396,484 */
  FLUXMI_EPI_SPLIT = 3,      /* n < split_n: C(bf16) = h ; else C2(fp8) = q(gelu) at column c2_col0 + n - split_n
                                                                              flux_model.py:471-480 */
  FLUXMI_EPI_QUANT = 4,      /* C(fp8)  = q(h, q_scale) */
  FLUXMI_EPI_SILU_QUANT = 5  /* C(fp8)  = q(bf16(silu(h)), q_scale)           flux_model.py:154-155 */
};

/* one problem of a (grouped) linear: out[M,N] = epilogue(A[M,K] . W[N,K]^T)
 *
 * Strides and alignment.  lda, ldc, ldr count ELEMENTS of their buffer (fp8: bytes; bf16: 2 bytes each; ldc of a quantising epilogue:
 * bytes), ldc2 and c2_col0 count bytes of the fp8 output C2, split_n counts columns of N.  Operands and outputs may be views of wider
 * buffers (lda > K, ldc > N, ldr != ldc, resid == C); nothing outside rows [0, M) x the view's columns is written.
 *   - A, W: 16-byte aligned, and a row of A (lda elements) a multiple of 16 bytes -- every kernel fetches them in 16-byte pieces.  The
 *     one-wave-per-SIMD and persistent kernels address A through a buffer descriptor of M * lda elements from A: a view's last row is
 *     followed by up to lda - K elements that lie inside the descriptor and may be FETCHED (never used), so they must be readable.
 *   - C, C2, bias, gate, resid: 16-byte aligned; rows of C, C2 and resid (ldc, ldc2, ldr) multiples of 16 bytes; c2_col0 and split_n
 *     multiples of 16 (a tile config also needs split_n to be a multiple of its N tile).  The tiled and split-K kernels load and store these as
 *     8- and 16-byte vectors.  The generic kernel (tile_cfg 100, and every N that is not a multiple of 64) touches them one element at
 *     a time: there they need only their element's alignment.
 * fluxmi_gemm_grouped refuses a group that violates this, by field name, before it launches anything.  Groups with M == 0 are allowed
 * anywhere in a launch: they get no tile and none of their pointers is followed. */
typedef struct fluxmi_gemm_group {
  const void* A;          /* activations [M,K]: fp8 bytes (F8Linear) or bf16 (nn.Linear) */
  const void* W;          /* weight [N,K] row-major = F8Linear.float8_data / nn.Linear.weight */
  const void* bias;       /* bf16 [N] or NULL */
  const float* sa_recip;  /* device scalar F8Linear.input_scale_reciprocal (NULL = 1) */
  const float* sb_recip;  /* device scalar F8Linear.scale_reciprocal       (NULL = 1) */
  void* C;                /* primary output */
  void* C2;               /* secondary output (FLUXMI_EPI_SPLIT) */
  const void* gate;       /* bf16 [N] */
  const void* resid;      /* bf16 [M, ldr] (may alias C) */
  const float* q_scale;   /* device scalar: input_scale of the consuming F8Linear */
  long long lda, ldc, ldc2, ldr;
  int M;
  int m_tile_start;       /* internal, filled by the launcher */
  int split_n, c2_col0;
  /* Optional fused attention-layout outputs (FLUXMI_EPI_BF16 / FLUXMI_EPI_SPLIT, 256x256 LDS-epilogue tile configs 13 and 16 only;
   * all NULL / 0 = off).  The N columns are [q | k | v | ...] with heads*128 columns each (the qkv Linear of a DoubleStreamBlock,
   * or the first 3*hidden columns of SingleStreamBlock.linear1).  V columns are written TRANSPOSED into vt_out
   * [heads*128][vt_ld] (key position = tok0 + row, key order inside every 16-key group bit2<->bit3 swapped = the k-slot order of
   * the attention kernel's PV MFMA; positions tok0+M .. tok0+vt_rows-1 are zero filled) instead of into C; K columns are
   * RMS-normalised (k_norm), rotated (pe) and written to k_out [heads][k_rows][128] instead of into C (tile configs 13, 16 and the
   * persistent config 18, which does it at a fraction of the cost: csrc/gemm_persist.hip).
   * Replaces the V / K halves of fluxmi_qkv_rope.                       flux_model.py:351-354,158-176,60-65,380-382 */
  void* vt_out;
  void* k_out;
  const void* pe;         /* (cos, sin) bf16 [k_rows][64][2] of this batch element */
  const void* k_norm;     /* bf16 [128] */
  long long vt_ld;
  int k_rows, tok0, vt_rows, kv_col0, heads;
  int k_f16;              /* k_out holds fp16 instead of bf16 (exact for bf16 values in fp16's range: fluxmi_attention's folded QK^T) */
  /* Optional 64 KiB table for the quantising epilogues (FLUXMI_EPI_GELU_QUANT and the mlp columns of FLUXMI_EPI_SPLIT, tile config
   * 13): q_lut[b] = the fp8 byte the epilogue would compute for the bf16 GEMM output with bit pattern b -- bf16 -> GELU -> bf16 ->
   * x input_scale -> bf16 -> clamp -> fp8 is a pure function of those 16 bits once the scale is frozen.  Built by
   * fluxmi_build_quant_lut from the same helpers; measured over all 65536 inputs (profiles/r06_qlut_vs_computed.txt) the table equals the
   * oracle's torch chain on every finite input outside a 4-pattern fp32-tanh cliff, and the epilogue the kernels COMPUTE when no table is
   * given differs from the table on ONE pattern (hipcc contracts the GELU polynomial differently per kernel) -- the table is the default
   * and the more faithful of the two; latents of a qlut = 0 run drift from the default's like two fp8 runs do.  It replaces ~25 VALU
   * instructions per element by one LDS gather while the matrix pipe is idle.  NULL = compute (tile configs 2, 13, 16; the persistent
   * config 18 has no computed quantising epilogue).                       flux_model.py:301,480 + float8_quantize.py:217-218,274-276 */
  const void* q_lut;
  /* Optional copy of W in the ROW-PAIR layout [N/2][K_bytes/64][2][64] (fluxmi_pair_rows): the 64-byte K-steps of rows 2r and 2r+1 share one
   * 128-byte line.  The tiled kernels fetch an operand one 64-byte K-step at a time, i.e. HALF an L2 line per row and step -- each line crosses the
   * L2 -> CU path twice per tile; with the weight stored in row pairs every line of W is fetched once (profiles/r04_gemm_persist.txt section 9: the
   * K loop of the persistent kernel 62.4 K -> 56.5 K cycles per tile).  Same values, same results; NULL = read W.  Honoured by tile configs 18
   * (all groups of a launch with or all without) and 16; the engine keeps such a copy of the weights those launches read (+8 GB at Flux-dev). */
  const void* W_pairs;
  /* ACTIVATIONS in the row-pair layout (ABI 5, round 6).  a_pairs != 0: A (fp8, dense rows: lda == K, M % 2 == 0) is stored as
   * [M/2][K/64][2][64] like W_pairs -- the 64-byte K-steps of rows 2r and 2r + 1 share one 128-byte line, so every L2 line of the A panel
   * crosses to the CU once per tile instead of twice (in-step, timing-only ablation of the persistent kernel alone: -1.3 % per step,
   * profiles/r06_act_pairs.txt).  c8_pairs != 0: the fp8 output of the QUANTISING epilogues (C for FLUXMI_EPI_GELU_QUANT / _QUANT /
   * _SILU_QUANT, C2 for FLUXMI_EPI_SPLIT) is written in that layout over rows of ldc (ldc2) bytes: byte (m, col) of the row-major buffer
   * lives at (m / 2) * 2 * ld + (m % 2) * 64 + (col / 64) * 128 + col % 64 (ld % 64 == 0; col = the column inside the FULL row, i.e.
   * c2_col0 + n - split_n for SPLIT) -- the next F8Linear reads it with a_pairs.  Same values, same results; honoured by tile configs 2,
   * 13, 16, 17, 18 (every group of a launch with the same flags); the generic and split-K kernels refuse a flagged group.  The engine
   * keeps its fp8 activation buffers this way in fused mode (fluxmi_tuning_t.a_pairs). */
  int a_pairs;
  int c8_pairs;
} fluxmi_gemm_group_t;

const char* fluxmi_last_error(void);
int fluxmi_abi_version(void);

/* ---- kernel-selection knobs (ABI 3; attn_split: ABI 4; a_pairs: ABI 5) --------------------------------------------------------------------------------------------
 * The reference has no counterpart (its only switches are the ModelSpec flags of util.py:40-77); these choose between kernels /
 * fusion levels.  What each VALUE promises about the model's output -- bit-identical to the defaults, or within a stated rel-L2 of them
 * (another summation order or rounding grid: split-K, the attention arithmetic knobs, the one-wave-per-row LayerNorm), or excluded (timing
 * builds) -- is the table of tests/knob_contract.py, which the test suite checks against fluxmi_set_tuning and runs at model level.  They
 * are resolved ONCE: the first call that needs a knob parses the FLUXMI_*
 * environment variables named below into this struct (csrc/tuning.cpp -- the only getenv site of the library);
 * fluxmi_set_tuning replaces it at run time (A/B probes, tests).  An engine re-captures its step graph when the struct changed
 * since the capture, and fluxmi_engine_create logs it once under FLUXMI_LOG=1. */
typedef struct fluxmi_tuning {
  int struct_size;       /* sizeof(fluxmi_tuning_t): filled by fluxmi_get_tuning, checked by fluxmi_set_tuning */
  int gemm_cfg;          /* FLUXMI_GEMM_CFG     -1 = cost model (default), else force this tile config (2, 13, 15..21; nothing else is
                                                 accepted) on the launches it runs -- shape, split column, fused K / V^T outputs, operand
                                                 format and epilogue (17: fp8 x e5m2 gate*y+x or bf16 plain / gate*y+x; 20, 21: fp8 x e5m2
                                                 gate*y+x) -- every other launch keeps the cost model.  Turns split-K, the 128x128 peel, the
                                                 persistent kernel and the lower tiles off */
  int gemm_splitk;       /* FLUXMI_GEMM_SPLITK   1: small-M bf16 launches split K over several workgroups per tile */
  int gemm_hybrid;       /* FLUXMI_GEMM_HYBRID   1: peel the thin groups of a grouped launch into a 128x128 launch */
  int gemm_esel;         /* FLUXMI_GEMM_ESEL     1: one kernel instantiation per hot epilogue (0 = run-time switch, A/B) */
  int gemm_persist;      /* FLUXMI_GEMM_PERSIST  1: multi-round fp8 launches on the persistent kernel (tile config 18); 2 = its timing build (probes) */
  int attn_var;          /* FLUXMI_ATTN_VAR      bit 1: exact instead of deferred running max (other bits); bit 0 selects nothing */
  int attn_abl;          /* FLUXMI_ATTN_ABL      ablation bits of the 8-wave kernel (probes): bit 1 drops a barrier (timing only, results
                                                 undefined), bit 3 stores the fp8 output as 4-byte words (the same bytes; also taken for
                                                 rows that are not 16-byte aligned); bits 0 and 2 select nothing */
  float attn_defer_log2; /* FLUXMI_ATTN_THR      rescale threshold of the deferred running max, log2; [0, 16], default 8 */
  int attn_f16k;         /* FLUXMI_ATTN_F16K     1: the engine stores K as fp16 and runs the folded attention arithmetic */
  int fuse_kv;           /* FLUXMI_FUSE_KV       0 / 1 / 2 (default): K, V^T by the relayout kernel / V^T from the qkv GEMM epilogue / both */
  int qlut;              /* FLUXMI_QLUT          1: table-driven GELU -> fp8 epilogues */
  int ln_variant;        /* FLUXMI_LN_V          2 = streaming LayerNorm kernel (default; hidden <= 3072), 3 = the same at two workgroups
                                                 per CU (same bits), 1 = one wave per row (mean / variance in another order; the fused step
                                                 then keeps plain activation rows, as it does at hidden > 3072) */
  int roctx;             /* FLUXMI_ROCTX         1: roctx ranges around the phases of a denoise call */
  int prefetch;          /* FLUXMI_PREFETCH      1: launches with idle CUs (attention, the 216-tile GEMMs) carry extra workgroups that read the
                                                 weights of the following launches into the memory-side cache (engine, fused mode); 2: a double
                                                 block's attention also pulls in mlp.2, 3: a single block's attention also the next block's linear1
                                                 (in-step -0.1 .. -0.7 % by lease for 2 and 3, +0.3 % once: inside the noise, default stays 1) */
  int w_pairs;           /* FLUXMI_W_PAIRS       1: the engine keeps a row-pair copy of the F8Linear weights its persistent GEMM launches read
                                                 (fluxmi_gemm_group_t.W_pairs: every L2 line of W fetched once per tile instead of twice) */
  int log;               /* FLUXMI_LOG           1: print the struct to stderr when it is resolved / set / an engine is created */
  int gemm_tile192;      /* FLUXMI_GEMM_TILE192  1 (default): gate*y+x launches of the one-wave-per-SIMD kernel (K >= 8192) whose 256-row tiles fill less
                                                 than one round of the CUs run on 192 x 256 tiles (tile config 17; same bits, 36 % more tiles of
                                                 three quarters the work: Flux-dev 768^2 mlp.2 / linear2, 132 -> 180 tiles); round 6: also 224-row
                                                 (config 20: 1024^2 linear2, 216 -> 252 tiles) and 160-row tiles (config 21: 768^2, 216 tiles), the
                                                 four waves side by side along N; 2 = config 17 only (A/B), 0 = 256-row tiles only */
  int attn_split;        /* FLUXMI_ATTN_SPLIT    1 (default): attention launches whose last round of workgroups is THIN (at most 8 of an XCD's
                                                 32 CUs busy: 264 tasks on 256 CUs at Flux-dev 768^2) run that round's tasks as pieces of
                                                 their key range and merge the partial softmax states (fp32 log-sum-exp in a fixed order:
                                                 deterministic); see fluxmi_attention_plan.  2 = wherever such a plan exists (fuller last
                                                 rounds: measured not to pay, Flux-dev 1024^2 +3.4 % per step), 0 = one workgroup per task */
  int a_pairs;           /* FLUXMI_A_PAIRS       1 (default): in fused mode the engine keeps its fp8 ACTIVATION buffers (LayerNorm / attention /
                                                 GELU outputs = the A operands of the block linears) in the row-pair layout
                                                 (fluxmi_gemm_group_t.a_pairs / c8_pairs) -- same bits, fewer L2 lines.  Only where every
                                                 producer takes it: even L and Lt, the streaming LayerNorm (ln_variant >= 2, hidden <= 3072),
                                                 3 x hidden % 256 == 0, mlp_hidden % 128 == 0 */
} fluxmi_tuning_t;
int fluxmi_get_tuning(fluxmi_tuning_t* out);
int fluxmi_set_tuning(const fluxmi_tuning_t* in); /* validates every field (non-zero + fluxmi_last_error on a bad value) */

/* Probes (tools/): a device buffer of [workgroup][tile < 8][8] uint64 that the timing build of the persistent GEMM (tile config 19)
 * fills with {tile start, K loop end, epilogue end} shader-clock stamps, the 100 MHz real-time counter and four phase stamps of the
 * table epilogue; NULL switches it off.
 * fluxmi_clock_sample writes {XCC id, s_memtime, s_memrealtime} of one wave per XCD to out[0..23] (24 uint64) on `stream`: two samples
 * around a timed region, paired by XCC id, give the average shader clock the chip sustained over it (bench.py). */
int fluxmi_gemm_debug_buffer(void* dev_u64);
int fluxmi_clock_sample(void* out24_dev_u64, void* stream);

/* ---- F8Linear / Linear ------------------------------------------------------------------------- */
/* Grouped linear.  is_fp8=1: A is `act_fmt` fp8, W is e4m3fn (torch._scaled_mm, float8_quantize.py:284-292);
 * is_fp8=0: A, W bf16 (F.linear).  tile_cfg: -1 auto (cost model + split of a thin last round, what the engine uses);
 * 13 = 256x256 ping-pong LDS ring (K*bytes % 64 == 0); 16 = 256x256 with one wave per SIMD (K*bytes % 256 == 0), 17 = the same kernel on 192x256 tiles
 * (fp8 x e5m2 or bf16 operands, plain bf16 or gate*y+x epilogue: launches with a thin single round of 256-row tiles); 2 = 128x128 and 15 = 128x64
 * double-buffered tiles (K*bytes % 128 == 0); 100 = generic any-shape kernel (scalar fma: <= 1 bf16 ulp of the others on bf16 operands).  The
 * tiled configs compute the same bits for fp8 AND, since round 6, for bf16 operands (one K association: test_bf16_tile_configs_are_bit_identical).  (Other numbers
 * named kernel generations that were removed: they are rejected.)  18 = config 13 as a PERSISTENT kernel (one workgroup per CU walks the tiles;
 * fp8 x e5m2, N % 256 == 0, K % 256 == 0, K >= 512; the auto dispatch takes it for launches of more than 256 tiles), 19 = its timing build.
 * 113 + S (S = 2..32, S <= K-steps): config 13 with SPLIT-K -- S workgroups per tile, each over its own K range, fp32 partial tiles in a 256 MiB
 * scratch summed in ascending K order by a second pass that applies the epilogue (FLUXMI_EPI_BF16 / FLUXMI_EPI_GATE_RESID only).  The scratch
 * belongs to the (device, stream) pair of the launch: allocated, under a lock, by the first EAGER split-K launch on that stream -- a first use
 * under stream capture is refused -- so launches on different streams never share partial tiles; a fluxmi_engine owns one of its own (its step
 * graph is captured on a private stream).  The auto dispatch uses split-K for bf16 launches of <= 128 tiles with >= 192 K-steps (M <= 512:
 * Flux-schnell at 256x256, the text encoders): deterministic, <= 1 bf16 ulp of fp64 like the others, but not bit-identical to the unsplit
 * kernels (the fp32 sum is associated differently) -- i.e. the bits of a bf16 auto-dispatched GEMM called through THIS entry depend on how many
 * rows share the launch.  A fluxmi_engine announces its batch to the dispatcher, which then takes the slice count of ONE sample's groups, so a
 * sample's bits do not follow the batch it rides in (round 6; test_a_sample_does_not_depend_on_its_batch).  Other callers that need
 * batch-invariant bits launch a fixed number of rows (the native text encoders run one prompt per launch; the engine's modulation-table GEMM
 * blocks the choice) or set fluxmi_tuning_t.gemm_splitk = 0. */
int fluxmi_gemm_grouped(const fluxmi_gemm_group_t* groups, int n_groups, int N, int K, int is_fp8, int act_fmt,
                        int epilogue, int tile_cfg, void* stream);
/* The launches fluxmi_gemm_grouped(tile_cfg = -1) would issue for these groups under the process-wide tuning, WITHOUT issuing them: host
 * arithmetic only, works without a GPU (added within ABI 5: no struct or existing entry point changed).  Of a group it reads M, the layout
 * fields and whether its pointers are NULL, never through them; any n_groups >= 1 (launches carry at most 16 groups each).  `batch`: what an
 * engine would announce for its bf16 launches (1 = none): the decisions of ONE sample's share of the groups are replayed on all of them.
 * plan[0 .. *plan_len) receives one record per launch, in launch order:
 *     kind, cfg, S, n, g_0 .. g_(n-1)
 * kind 0 = tile config `cfg` (csrc/gemm_cfg.h), 1 = the generic kernel (cfg = -1), 2 = split-K with S slices on 256x256 tiles (cfg = -1);
 * S = 0 unless kind 2; g_i = indices into `groups`, in the order the launch carries them.  Every group appears in exactly one record.
 * When plan_cap is too small the call fails with *plan_len set to the length needed (n_groups + 4 x launches <= 5 x n_groups). */
int fluxmi_gemm_plan(const fluxmi_gemm_group_t* groups, int n_groups, int N, int K, int is_fp8, int act_fmt, int epilogue, int batch,
                     int* plan, int plan_cap, int* plan_len);
/* single-problem convenience form of fluxmi_gemm_grouped (F8Linear.forward after quantisation) */
int fluxmi_f8_gemm(const void* a_fp8, const void* w_e4m3, const float* sa_recip, const float* sb_recip, const void* bias,
                   void* out, int M, int N, int K, int act_fmt, int epilogue, const void* gate, const void* resid,
                   const float* q_scale, int tile_cfg, void* stream);
/* skinny linear (M = batch <= 8): out[b,n] = bf16((x_q[b,:].W[n,:]) * sa*sb + bias), optional SiLU on x first
 * (Modulation.forward flux_model.py:251-257, MLPEmbedder flux_model.py:154-155, LastLayer.adaLN flux_model.py:495-500) */
int fluxmi_gemv(const void* x, long long ldx, const void* W, const void* bias, const float* in_scale, const float* sa_recip,
                const float* sb_recip, void* out, long long ld_out, int B, int N, int K, int w_fp8, int act_fmt, int pre_silu,
                void* stream);

/* ---- quantisation state machine (F8Linear) ------------------------------------------------------- */
/* q = fp8(clamp(bf16(x*scale)))                                                float8_quantize.py:217-218,274-276 */
int fluxmi_quantize_act(const void* x, void* q, const float* scale, int rows, int cols, long long ld_in, long long ld_out,
                        int fmt, void* stream);
/* *amax = max(*amax, max|x|)  (caller zeroes *amax first)                      float8_quantize.py:227
 * An inf element gives inf; a NaN element is SKIPPED (fmaxf drops it), where torch.max would return NaN: the maximum is taken over the
 * other elements, and a tensor of NaNs alone leaves *amax as it was (tests/test_quant_kernels_gpu.py pins this). */
int fluxmi_amax(const void* x, float* amax, int rows, int cols, long long ld, void* stream);
/* one call of F8Linear.quantize_input's scale logic for trial `trial_index`     float8_quantize.py:220-246 */
int fluxmi_calib_update(const float* amax, float* trials, float* scale, float* scale_recip, int trial_index, int num_trials,
                        float max_val, void* stream);
/* F8Linear.quantize_weight: amax -> scale -> e4m3 data + reciprocal             float8_quantize.py:195-207 */
int fluxmi_quantize_weight(const void* w_bf16, void* q, float* amax_tmp, float* scale, float* scale_recip, int N, int K, int fmt,
                           void* stream);
/* LoRA fuse into an fp8 weight: W' = requant(bf16(dequant(W) + scale * B@A))     lora_loading.py:509-577,615-631,686-687 */
int fluxmi_lora_fuse_f8(void* w_fp8, float* w_scale, float* w_scale_recip, const float* lora_B, const float* lora_A, int N, int K,
                        int R, int n_chunks, float lora_scale, float* work_f32, float* amax_tmp, void* stream);
int fluxmi_dequant(const void* q, float* out, const float* scale_recip, long long n, int fmt, void* stream);

/* ---- block elementwise ----------------------------------------------------------------------------- */
/* y = (1+scale)*LayerNorm(x)+shift (+fp8 quantise); rows [B][L], rows l<split use set 0   flux_model.py:367-368,389,469-470,501 */
int fluxmi_ln_modulate(const void* x, long long ldx, void* out, long long ldo, const void* shift0, const void* scale0,
                       const void* shift1, const void* scale1, long long mod_bstride, const float* q_scale0,
                       const float* q_scale1, int B, int L, int split, int H, int out_fp8, int fmt, void* stream);
/* the same with out_pairs: != 0 stores the fp8 output in the row-pair layout of fluxmi_pair_rows over the B * L rows (needs fp8 output,
 * ldo == H, H % 64 == 0, H <= 3072, B * L even and fluxmi_tuning_t.ln_variant >= 2; refused otherwise); 0 is fluxmi_ln_modulate */
int fluxmi_ln_modulate_pairs(const void* x, long long ldx, void* out, long long ldo, const void* shift0, const void* scale0,
                             const void* shift1, const void* scale1, long long mod_bstride, const float* q_scale0,
                             const float* q_scale1, int B, int L, int split, int H, int out_fp8, int fmt, int out_pairs, void* stream);
/* mode 0: GELU(tanh), 1: SiLU (bf16 -> bf16)                                     flux_model.py:301,139 */
int fluxmi_act(const void* x, void* y, int rows, int cols, long long ld_in, long long ld_out, int mode, void* stream);
/* out = x + gate[b] * y                                                           flux_model.py:387-396,484 */
int fluxmi_gate_residual(const void* x, const void* y, const void* gate, void* out, int B, int L, int H, long long ldx,
                         long long ldy, long long ldo, long long gate_bstride, void* stream);
int fluxmi_add(const void* a, const void* b, void* z, long long n, void* stream);
/* z[r, :] = a[r, :] + b[r % nb, :] over dense rows of `cols` bf16 (cols % 8 == 0, nb >= 1) */
int fluxmi_add_bcast(const void* a, const void* b, void* z, long long rows, int nb, int cols, void* stream);

/* lut[b] for every bf16 bit pattern b: the fp8 byte of  to_fp8_saturated(act(bf16 b), *scale)  (act: 0 none, 1 gelu-tanh, 2 silu),
 * rounded at the same points as the fused epilogues.  65536 bytes.                      float8_quantize.py:217-218 */
int fluxmi_build_quant_lut(const float* scale, int fmt, int act, void* lut, void* stream);
/* rows x row_bytes (row-major, rows % 2 == 0, row_bytes % 64 == 0) -> the row-pair layout of fluxmi_gemm_group_t.W_pairs; out != in */
int fluxmi_pair_rows(const void* in, void* out, int rows, long long row_bytes, void* stream);
/* the inverse: the row-pair layout back to plain rows (ABI 5; tests, fluxmi_engine_copy_buffer) */
int fluxmi_unpair_rows(const void* in, void* out, int rows, long long row_bytes, void* stream);

/* ---- attention path --------------------------------------------------------------------------------- */
/* pe[rows, pairs, (cos,sin)] from position ids                                    flux_model.py:49-57,82-92 */
int fluxmi_rope_table(const void* ids, const float* omega, const int* axis, void* pe, long long rows, int n_axes, int pairs,
                      void* stream);
/* qkv split + QKNorm + RoPE + head-major relayout (V transposed); Q may be NULL      flux_model.py:351-354,158-176,60-65,380-382
 * k_f16 != 0: K is stored as fp16 instead of bf16 (same bytes per element; the normalised + rotated bf16 values are exact in fp16
 * unless |k| < 6.1e-5).  That is the operand format of the attention kernel's folded schedule, see fluxmi_attention. */
int fluxmi_qkv_rope(const void* qkv, long long ld, const void* pe, const void* q_scale0, const void* k_scale0,
                    const void* q_scale1, const void* k_scale1, void* Q, void* K, void* VT, int B, int L, int Lp, int H, int split,
                    int k_f16, void* stream);
/* softmax(QK^T/sqrt(128))V -> [B,L,H*128] (bf16, or fp8 with the consumer's input scale)   flux_model.py:41-45
 * k_f16 != 0: K holds fp16 (fluxmi_qkv_rope(k_f16 = 1)).  The kernel then multiplies Q by 128^-0.5 * log2(e) while it builds its
 * fragments (fp16, 2^-11 relative rounding), runs QK^T on the f16 MFMA and starts every score accumulator from minus the running
 * maximum, so a score costs one exp2 instead of fma + exp2 (+4.7 % at L = 4608).  Q and V^T are bf16 either way.  Knobs
 * (fluxmi_tuning_t): attn_defer_log2 = log2 of the deferred-rescale threshold (default 8), attn_var bit 1 = exact running max,
 * attn_split = the balanced grid of fluxmi_attention_plan (fp16-K calls). */
int fluxmi_attention(const void* Q, const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                     const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16,
                     void* stream);

/* The launch plan of the kernel above for ONE SAMPLE's H heads of L keys on a 256-CU part (host arithmetic only, no GPU needed; tests + bench
 * notes).  Since round 6 the plan is per sample and a batch is launched sample by sample when it is on: B only has to be >= 1 and the pieces a
 * (head, row block) is cut into -- hence its bits -- do not depend on the batch (test_attention_is_batch_invariant_at_thin_last_rounds).
 * The kernel runs one workgroup of 256 query rows per (head, row block) -- a TASK -- and one workgroup per CU at a time, so 264 tasks take two
 * rounds for 1.03 rounds of work.  Under fluxmi_tuning_t.attn_split (fp16-K calls only) every XCD runs full_per_x of its n_per_x tasks whole
 * and the remaining ones as `npieces` PIECES of their key range, launched longest first, so that every CU ends up with the same number of key
 * tiles: a THIN last round (at most 8 of an XCD's 32 CUs) is folded into the full round in front of it (768^2: 33 tasks over 32 bins), a
 * single partial round (fewer than 32 tasks per XCD) is spread over all CUs, a fuller last round is binned on its own.  A piece writes its
 * softmax state (O, m, l; fp32) to a scratch slot and the piece that arrives last at the task's counter merges them in piece order -- the
 * result does not depend on the arrival order.  Returns 0 when the launch runs one workgroup per task, 1 when a plan exists and
 * attn_split = 1 takes it (a thin last round behind at least one full one), 2 when only attn_split = 2 does (fuller last rounds and single
 * partial rounds: measured not to pay).
 * pieces[i] (i < npieces <= 64), in launch order: bits 0-7 index of the binned task, 8-15 piece index within the task, 16-23 pieces of
 * the task, 24-31 canonical index of the task's first piece (= its scratch slot), 32-47 first key tile, 48-63 key tiles. */
int fluxmi_attention_plan(int B, int L, int H, int* n_per_x, int* full_per_x, int* npieces, unsigned long long* pieces);
/* Probes (tools/attn_timeline.py): a device buffer of [workgroups][8] uint64 that every attention workgroup fills with {blockIdx, XCC id | HW_ID << 8,
 * start, end, Q fragments built, prologue tiles landed, step loop done, drain done} (100 MHz real-time counter): which CU ran which task / piece
 * when, and where a workgroup's time outside its key tiles goes.  NULL switches it off. */
int fluxmi_attention_debug_buffer(void* dev_u64);

/* The same with Q taken RAW from the qkv GEMM output (q at column 0 of `qkv`, row stride ld_qkv): QKNorm (qn_scale0 for rows
 * < split, qn_scale1 otherwise) + RoPE (pe) are applied while the query fragments are loaded, so Q never round-trips through HBM.
 * Pair with fluxmi_qkv_rope(..., Q = NULL, ...) which then produces K and V^T only.     flux_model.py:41-45,60-65,158-176 */
int fluxmi_attention_rawq(const void* qkv, long long ld_qkv, const void* pe, const void* qn_scale0, const void* qn_scale1, const void* K,
                          const void* VT, void* out, long long ld_out, int col_off, int out_fp8, const float* q_scale0,
                          const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16, void* stream);

/* Token-group masks (regional prompts, key-masked padding): the two entries above plus `groups`, a DEVICE table [B, L] of one 32-bit
 * descriptor per token of the joint sequence, and `out_pairs` (fp8 output rows in the row-pair layout of fluxmi_gemm_group_t.a_pairs).
 *   descriptor = g | P << 16:  g (bits 0-3) the token's KEY GROUP, P (bits 16-31) the groups its QUERY admits; bits 4-15 are zero.
 *   Query i attends key j iff bit g_j of P_i is set: F.scaled_dot_product_attention(q, k, v, attn_mask=allowed).
 * Every query must admit its own group (no empty softmax row); the CALLER checks that (FLUXMI_ATTN_DESC and ops.attention do; the table is
 * device data and this call does not read it back).  groups = NULL is the dense call.  A table that admits everything gives the dense
 * result bit for bit.  The mask costs two more QK^T MFMAs per 64-key tile (one-hot group code x permission row; csrc/attention2.hip) and
 * L <= 12096 (the keys' group codes are staged in LDS).  Masked launches take no balanced-grid plan: one workgroup per task under every
 * attn_split.  Scores of admitted keys must stay above -1024 + 126 in the exp2 domain (|q . k| / sqrt(128) < ~620: the masked rows' running
 * maximum starts from that floor, see the kernel). */
#define FLUXMI_ATTN_DESC(group, perm) ((unsigned)(group) | ((unsigned)(perm) << 16))
int fluxmi_attention_grouped(const void* Q, const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                             const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16,
                             const unsigned* groups, int out_pairs, void* stream);
int fluxmi_attention_rawq_grouped(const void* qkv, long long ld_qkv, const void* pe, const void* qn_scale0, const void* qn_scale1,
                                  const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                                  const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16,
                                  const unsigned* groups, int out_pairs, void* stream);

/* ---- VAE pieces (NHWC bf16) -------------------------------------------------------------------- */
/* 3x3 patch matrix: x [B, Hi, Wi, C] -> col [B*H*W, 9*C], column (dy*3+dx)*C + c, (H, W) = the OUTPUT grid.  `upsample`:
 *   1  stride 1 / pad 1 (Hi = H);   2  nearest 2x upsample folded into the gather (Hi = H/2; Upsample.forward);
 *  -2  stride 2 with zero pad on the right/bottom only (Hi = 2H; Downsample.forward).
 * The convolution is then fluxmi_gemm_grouped(is_fp8=0) with the weight reordered to [Cout][dy][dx][Cin].
 *                                                                            modules/autoencoder.py:65-72,95-120,228,259 */
int fluxmi_im2col3x3(const void* x, void* col, int B, int H, int W, int C, int upsample, void* stream);
/* The same convolution WITHOUT the patch matrix (ABI 5, round 6): out [B*H*W, Cout] = conv3x3(x) (+ bias) (+ resid when given: out = resid +
 * gate * y with gate [Cout] bf16, normally ones) -- the 128x128 bf16 tile kernel gathers each 128-byte K-step (64 channels of one tap) from the
 * NHWC input inside its LDS-DMA address computation and pads through a zero page; w2 [Cout][3][3][C] bf16.  Same K order, same MFMAs as the GEMM
 * on fluxmi_im2col3x3's matrix: identical bits (tests/test_ops_gpu.py::test_conv3x3_implicit_equals_im2col_gemm).  Needs C %% 64 == 0 and
 * Cout %% 128 == 0 (FLUX VAE: every 3x3 convolution except conv_in / conv_out).  `upsample` as above; (H, W) = the OUTPUT grid. */
int fluxmi_conv3x3(const void* x, const void* w2, const void* bias, const void* gate, const void* resid, void* out, int B, int H, int W, int C,
                   int Cout, int upsample, void* stream);
/* GroupNorm(32 groups, affine) in fp32 + optional swish, rounded to bf16 once; x, y [B, P, C]; work: float[(B*ceil(P/512)+B)*64] (ABI 5: was ceil(P/4096)).
 *                                                                                modules/autoencoder.py:19-20,28-30,62-70,256 */
int fluxmi_groupnorm(const void* x, const void* gamma, const void* beta, void* y, float* work, int B, int P, int C, int swish, float eps,
                     void* stream);
/* P[r,:] = softmax(scale * S[r,:]) (fp32 inside), bf16 [rows, cols], row stride ld            modules/autoencoder.py:47 */
int fluxmi_softmax_rows(const void* S, void* P, int rows, int cols, long long ld, float scale, void* stream);

/* ---- text-conditioning encoder pieces (bf16) ------------------------------------------------------------
 * The reference runs transformers' T5EncoderModel / CLIPTextModel (modules/conditioner.py:74-117, flux_emphasis.py:420-429); their
 * Linear layers map to fluxmi_gemm_grouped(is_fp8=0), the rest to the three entry points below. */
/* mode 0: T5LayerNorm  y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))  (bias ignored);  mode 1: LayerNorm  y = bf16((x - mean) * rstd * w + b).
 * x, y [rows, D] bf16 with row strides ldx, ldy; fp32 statistics. */
int fluxmi_row_norm(const void* x, const void* weight, const void* bias, void* y, int rows, int D, long long ldx, long long ldy, float eps, int mode,
                    void* stream);
/* mode 0: in [rows, 2F] = [a | b] -> out [rows, F] = bf16(bf16(gelu_new(a)) * b)   (T5 v1.1 gated FF: wi_0 / wi_1 fused into one GEMM)
 * mode 1: in [rows, F] -> out = bf16(a * sigmoid(1.702 a))                          (CLIP quick_gelu) */
int fluxmi_act_mul(const void* in, void* out, int rows, int F, long long ld_in, long long ld_out, int mode, void* stream);
/* Self-attention with head_dim 64 for one sequence: q, k [Lp, ld_qk] (head h at columns h*64..), vt [H*64, ld_vt] = V transposed
 * (row h*64+d, column = key; keys >= L are ignored), out [Lp, ld_out] (rows < L written).  logits = scale * q.k
 * + rel_bias[h][key - query + bias_ld/2] (fp32 [H, bias_ld], NULL = none; T5's bucketed relative-position bias) with keys > query
 * masked when causal (CLIP); fp32 softmax, P rounded to bf16, out = P V + v_bias (bf16 [H*64] or NULL).  Lp %% 32 == 0. */
int fluxmi_text_attention(const void* q, const void* k, long long ld_qk, const void* vt, long long ld_vt, void* out, long long ld_out,
                          const float* rel_bias, int bias_ld, const void* v_bias, float scale, int causal, int L, int Lp, int H, void* stream);
/* fluxmi_text_attention's kernel over B sequences in one launch (B images of a vision encoder), non-causal, no position bias, at a padded head
 * width head_dim = 64 or 96: head h at columns h*head_dim.. of q / k / out and rows h*head_dim.. of vt.  A head narrower than head_dim (SigLIP-so400m:
 * 72 in 96) is zero-padded by the caller in q, k, vt and v_bias; the padded output columns then come out zero.  Sequence b is at
 * q + b*bs_qk, k + b*bs_qk, vt + b*bs_vt, out + b*bs_out (element strides); q / k / vt hold Lp rows (columns) of finite values per sequence,
 * keys >= L are ignored, out rows < L are written.  Lp %% 32 == 0; ld_qk, bs_qk %% 8 == 0; ld_vt, bs_vt, ld_out, bs_out %% 4 == 0. */
int fluxmi_vision_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                            void* out, long long ld_out, long long bs_out, const void* v_bias, float scale, int head_dim, int L, int Lp, int H, int B,
                            void* stream);
/* Streaming attention of the autoencoder's mid block: ONE head of width D = 64 or 512, non-causal, B images in one launch, no [P, P] matrix.
 *   q, k   bf16 [B][Pp][D], row stride ld_qk, batch stride bs_qk (both: two column windows of one fused projection output are fine)
 *   vt     bf16 [B][D][Pp] = V transposed (row = channel, column = key), row stride ld_vt, batch stride bs_vt
 *   out    bf16 [B][P][D], row stride ld_out, batch stride bs_out; rows >= P and everything outside the addressed window are not written
 *   v_bias bf16 [D] or NULL
 * Pp is a multiple of 64 that is >= P (P rounded up to 64).  Rows >= P of q and k and columns >= P of vt may hold arbitrary FINITE values; no
 * output depends on them.  Arithmetic, with c = fp32(log2 e / sqrt D) and the keys walked in tiles of FLUXMI_VAE_ATTN_KEY_TILE:
 *   s_ij = fp32 MFMA sum of the bf16 products q_i . k_j;   t_ij = s_ij * c in fp32
 *   per tile: m' = max(m, max_j t_ij), exact;  O and l are multiplied by exp2(m - m') in fp32 when the maximum grew;
 *             p_ij = exp2(t_ij - m') in fp32;  l += sum_j p_ij in fp32;  O += bf16(p) V on the matrix pipe with fp32 accumulation
 *   out = bf16(O / l + v_bias[d])  -- the only rounding of the output
 * P is rounded to bf16 once, after its tile's maximum is final; there is no deferred maximum.  Keys >= P have weight exactly 0.  A sample's
 * bits depend on that sample alone, and results are deterministic (no atomics, fixed summation order).
 * Returns non-zero before any launch for: D other than 64 / 512; P < 1; Pp %% 64 != 0 or Pp < P; B outside 1..65535; a stride that is no
 * multiple of 8 (or too short for its operand); a pointer that is not 16-byte aligned.  All stride arithmetic is 64-bit. */
#define FLUXMI_VAE_ATTN_KEY_TILE 64
int fluxmi_vae_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                         void* out, long long ld_out, long long bs_out, const void* v_bias, int D, int P, int Pp, int B, void* stream);
/* The 3x3 convolution of RRDBNet (ESRGAN family; modules/upscaler.py): stride 1, zero pad 1, NHWC bf16, reading and writing CHANNEL WINDOWS
 * of strided pixel buffers, so a residual dense block is five launches on one [B, H, W, nf + 4 gc] buffer with no concatenation copy.
 *   x      bf16 [B][Hi][Wi] pixels, pixel stride ldx elements; channels [0, Cin) of each pixel are read.  (H, W) is the OUTPUT grid:
 *          upsample 1: Hi = H, Wi = W;  upsample 2: Hi = H/2, Wi = W/2, the nearest 2x upsample folded into the gather (output pixel
 *          (y, x) of the upsampled image is input pixel (y/2, x/2); the zero pad surrounds the UPSAMPLED image) -- fluxmi_conv3x3's convention
 *   w2     bf16 [Cout32][3][3][Cin], Cout32 = Cout rounded up to 32; the caller zero-pads rows >= Cout
 *   bias   bf16 [Cout32] or NULL
 *   out    bf16 [B][H][W] pixels, pixel stride ldo; channels [0, Cout) at `out` are written and NOTHING else is (the caller points `out`
 *          at the first channel of the window)
 *   r1, r2 optional bf16 residuals, channels [0, Cout) of [B][H][W] pixels with pixel strides ldr1, ldr2 (r2 needs r1)
 * Arithmetic, all fp32 until the store:
 *   acc = MFMA (v_mfma_f32_32x32x16_bf16) sum of the bf16 products over input-channel chunks of 64, then (dy, dx), then 16-channel steps
 *   y = acc + bias;   act = 1: y = y < 0 ? slope * y : y;   r1: y = a1 * y + r1;   r2: y = a2 * y + r2;   out = bf16(y)
 * Each scale-and-add is TWO operations (a rounded product, then a rounded sum), not an fma.  The store is the only bf16 rounding.
 * One workgroup computes a FLUXMI_CONV_DENSE_TILE x FLUXMI_CONV_DENSE_TILE pixel tile of one image.
 * Aliasing: `out` may lie in the same buffer as x iff its channel window does not meet [0, Cin); r1 and r2 may alias x; `out` overlaps
 * neither residual.  Deterministic (no atomics, fixed summation order); a sample's bits depend on that sample alone.  All address
 * arithmetic is 64-bit.
 * Returns non-zero before any launch (text in fluxmi_last_error) for: Cin not a multiple of 16 in 16..256; Cout outside 1..64; upsample
 * other than 1 / 2, or 2 with odd H or W; act other than 0 / 1; B, H or W < 1; B or ceil(H / tile) above 65535 (the launch grid);
 * a stride that is no multiple of 8 or shorter than its channels; a pointer that is not 16-byte aligned; r2 without r1; out == r1 or r2. */
#define FLUXMI_CONV_DENSE_TILE 16
int fluxmi_conv3x3_dense(const void* x, long long ldx, int Cin, const void* w2, const void* bias, void* out, long long ldo, int Cout,
                         const void* r1, long long ldr1, float a1, const void* r2, long long ldr2, float a2, float slope, int act,
                         int upsample, int B, int H, int W, void* stream);
/* Patch rows of a stride-`patch` "valid" convolution: pix bf16 [B, C, H, W] (NCHW, contiguous) -> out bf16 [B*grid*grid, Kp], row
 * (b, gy, gx), column c*patch*patch + ky*patch + kx (the order of a Conv2d weight [N, C, patch, patch] flattened), columns >= C*patch*patch
 * zero.  Pixels past grid*patch are not read.  Kp %% 8 == 0; grid*patch <= H, W.  SigLIP-so400m: C 3, patch 14, grid 27, Kp 640. */
int fluxmi_patchify(const void* pix, void* out, int B, int C, int H, int W, int patch, int grid, int Kp, void* stream);

/* ---- control-map preprocessors (csrc/preprocess.hip): photo -> edge map / luma / blurred image ---------------------------------------
 * Images are uint8 [B][H][W][C], channels adjacent, with a ROW stride `ld` and an IMAGE stride `bs` in bytes (ld >= W * C; bs >= H * ld
 * when B > 1), so an operand may be a window of a larger buffer: nothing outside the W * C bytes of a row is read or written.  Pointers
 * need no alignment; 4-byte accesses are used on rows whose address is a multiple of 4.  B, H <= 65535, W <= 2^24.  A sample's bits depend
 * on that sample alone, and every function here is deterministic.
 *
 * Canny.  Everything is integer arithmetic and the text below IS the definition: the kernels match it bit for bit.  It follows the steps
 * and constants of the widely used open-source implementation (3 x 3 Sobel, the channel of largest magnitude, 22.5-degree sectors by the
 * fixed-point tan 13573 / 2^15, hysteresis over 8-neighbours), but parity with an OpenCV binary is NOT pinned: none is available to the tests.
 *
 * fluxmi_canny_classify: rgb [B][H][W][3] -> state [B][H][W] in {0, 1 (weak), 2 (strong)}, one launch.
 *   per channel c, with p(y, x) read at indices clamped to the image (the border is replicated):
 *     dx = (p(y-1,x+1) + 2 p(y,x+1) + p(y+1,x+1)) - (p(y-1,x-1) + 2 p(y,x-1) + p(y+1,x-1))          rows [-1 0 1; -2 0 2; -1 0 1]
 *     dy = (p(y+1,x-1) + 2 p(y+1,x) + p(y+1,x+1)) - (p(y-1,x-1) + 2 p(y-1,x) + p(y-1,x+1))          its transpose
 *     m  = |dx| + |dy|   (l2 = 0)      or      dx dx + dy dy   (l2 = 1; low and high are then squared here, saturating at 2^31 - 1)
 *   the pixel takes (dx, dy, m) of the channel with the largest m; a later channel replaces an earlier one only when strictly greater.
 *   The magnitude of a position outside the image is 0.  lo = min(low, high), hi = max(low, high), both >= 0.
 *   m <= lo: state 0.  Otherwise non-maximum suppression, with x = |dx|, y = |dy| << 15, t22 = x * 13573, t67 = t22 + (x << 16):
 *     y < t22:   kept iff m >  m(y, x-1)  and m >= m(y, x+1)
 *     y > t67:   kept iff m >  m(y-1, x)  and m >= m(y+1, x)
 *     otherwise: s = -1 if dx and dy have opposite signs, else +1;  kept iff m > m(y-1, x-s) and m > m(y+1, x+s)
 *   not kept: state 0;  kept: state 2 if m > hi, else 1.
 *   Example: a vertical step of height h between columns c - 1 and c gives dx = 4 h, dy = 0 in both columns; the tie keeps the LEFT one
 *   (m > left, m >= right), so the edge is the single column c - 1 (likewise the upper row of a horizontal step), and h <= lo / 4 gives none.
 *   One workgroup owns a FLUXMI_CANNY_TILE x FLUXMI_CANNY_TILE pixel tile; its 2-pixel input halo is staged in LDS once and every magnitude
 *   of the tile + 1 is computed once.
 * fluxmi_canny_hysteresis_round: one round on a state map of values 0 / 1 / 2, in place.  Each workgroup loads its FLUXMI_CANNY_TILE^2 tile
 *   and a 1-pixel halo (0 outside the image), promotes 1 -> 2 wherever one of the 8 neighbours is 2 until the tile stops changing, stores
 *   the promoted pixels of its own tile and sets *changed_flag = 1 (device int; never cleared here) if it promoted any.  A halo pixel may be
 *   read before or after its owner's store of the same round; the update is monotone, so repeated rounds reach the one closure -- the set
 *   of weak pixels 8-connected to a strong one -- whatever the interleaving.  No workgroup waits on another.
 * fluxmi_canny_hysteresis: rounds until one changes nothing, then edges [B][H][W] = 255 where state == 2, else 0.  Rounds are launched in
 *   groups of FLUXMI_CANNY_ROUND_GROUP, each with its own zeroed slot of `flags` (that many device ints); the group's flags are read back
 *   (this call synchronises the stream) and *rounds_out = the rounds up to and including the first that changed nothing (those launched
 *   behind it in its group did nothing).  Every other round promotes a pixel, so H * W + 1 rounds suffice: beyond that an error is
 *   returned.  `state` is modified (it ends as the closure).  rounds_out may be NULL.
 * fluxmi_canny = classify into `work`, then fluxmi_canny_hysteresis.  work: 16-byte aligned, FLUXMI_CANNY_WORK_BYTES(B, H, W) bytes. */
#define FLUXMI_CANNY_TILE 32
#define FLUXMI_CANNY_ROUND_GROUP 4
#define FLUXMI_CANNY_WORK_BYTES(B, H, W) ((long long)(B) * (H) * (((long long)(W) + 3) & ~3LL) + 4 * FLUXMI_CANNY_ROUND_GROUP)
int fluxmi_canny_classify(const void* rgb, long long ld, long long bs, void* state, long long state_ld, long long state_bs, int B, int H, int W,
                          int low, int high, int l2, void* stream);
int fluxmi_canny_hysteresis_round(void* state, long long state_ld, long long state_bs, int B, int H, int W, int* changed_flag, void* stream);
int fluxmi_canny_hysteresis(void* state, long long state_ld, long long state_bs, void* edges, long long edges_ld, long long edges_bs, int* flags,
                            int B, int H, int W, int* rounds_out, void* stream);
int fluxmi_canny(const void* rgb, long long ld, long long bs, void* edges, long long edges_ld, long long edges_bs, void* work,
                 long long work_bytes, int B, int H, int W, int low, int high, int l2, int* rounds_out, void* stream);
/* gray [B][H][W] = (19595 R + 38470 G + 7471 B + 32768) >> 16 of rgb [B][H][W][3]: PIL's convert("L"), bit for bit. */
int fluxmi_rgb_to_gray(const void* rgb, long long ld, long long bs, void* gray, long long gray_ld, long long gray_bs, int B, int H, int W,
                       void* stream);
/* Separable Gaussian blur of src [B][H][W][C], C in {1, 3}, into dst (not src): radius r = ceil(3 sigma) (sigma as fp32, the product in
 * fp64), 1 <= r <= FLUXMI_BLUR_MAX_RADIUS; taps w[i] = exp(-i^2 / (2 sigma^2)), i = -r .. r, divided by their sum in fp64 and rounded to
 * fp32 once (handed to both passes as fp32 kernel-argument data).  Indices are clamped to the image (the border is replicated).
 *   t(y, x, c)   = sum_i w[i] src(y, x + i, c)      horizontal pass, fp32: acc = fma(w[i], value, acc) from 0, i ascending; NOT rounded to uint8
 *   dst(y, x, c) = sum_i w[i] t(y + i, x, c)        vertical pass, the same way; then rint (to nearest, ties to even) and clamp to 0..255
 * work: 16-byte aligned, FLUXMI_BLUR_WORK_BYTES(B, H, W, C) bytes (the fp32 intermediate). */
#define FLUXMI_BLUR_MAX_RADIUS 64
#define FLUXMI_BLUR_WORK_BYTES(B, H, W, C) ((long long)(B) * (H) * ((((long long)(W) * (C)) + 3) & ~3LL) * 4)
int fluxmi_gaussian_blur(const void* src, long long ld, long long bs, void* dst, long long dst_ld, long long dst_bs, void* work,
                         long long work_bytes, int B, int H, int W, int C, float sigma, void* stream);

/* ---- baseline JPEG encoder (csrc/jpeg.hip, csrc/jpeg_host.cpp): device pixels -> the bytes of a JFIF file --------------------------------
 * A baseline sequential (SOF0) Huffman-coded JPEG of rgb uint8 [B][H][W][3] (row stride ld, image stride bs, in bytes, as above).  Everything
 * is integer arithmetic and the text below IS the definition: the kernels and tests/jpeg_ref.py match it byte for byte.  It is libjpeg's
 * integer pipeline at its defaults (the "islow" DCT, the Annex K tables), so a stream decodes to what that library's own stream decodes to;
 * tests/test_jpeg_cpu.py pins byte equality of the entropy-coded segment with Pillow on libjpeg-turbo.
 *   Input.   A batch is ONE image of B * H rows: image b's row r is row b * H + r.  W <= 65535 and B * H <= 65535, any H, W >= 1.
 *   Colour.  Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16        (>> is arithmetic)
 *            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   Subsampling.  FLUXMI_JPEG_420: 16 x 16 MCUs, blocks Y00 Y01 Y10 Y11 Cb Cr, chroma sample (i, j) = (a + b + c + d + bias) >> 2 of the
 *            2 x 2 box at (2i, 2j), bias = 1 for even j and 2 for odd j.  FLUXMI_JPEG_444: 8 x 8 MCUs, blocks Y Cb Cr.
 *   Edges.   MCUs run left to right, top to bottom over ceil(W / m) x ceil(B H / m) MCUs (m = 16 or 8).  A sample right of the image repeats
 *            the last column, a sample below it the last row -- of ITS OWN plane: below a 4:2:0 image the last CHROMA row repeats (the box
 *            of rows B H - 2 and B H - 1 when B H is even), which is how libjpeg pads.  A Y block of a 4:2:0 MCU that holds no image pixel
 *            at all (block column >= ceil(W / 8) or block row >= ceil(B H / 8)) is libjpeg's dummy block: no AC levels, and the DC LEVEL
 *            of the block before it in the MCU (which may itself be a dummy block).
 *   DCT.     Samples - 128, then the accurate integer forward DCT: rows, then columns, each the 12-multiply butterfly with 13-bit
 *            constants (2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172); the row pass keeps 2 extra bits (outputs 0 and
 *            4 shifted left by 2, the others descaled by 11 bits), the column pass removes them (by 2 and by 15 bits); descale(x, n) =
 *            (x + (1 << (n - 1))) >> n.  The result is the DCT scaled by 8.
 *   Quantisation.  Annex K.1's tables, entry t -> clamp((t s + 50) / 100, 1, 255) with s = 5000 / quality below 50 and 200 - 2 quality
 *            from 50 (quality 1..100, integer division).  Level of coefficient c: sign(c) ((|c| + 4 t) / (8 t)).
 *   Entropy coding.  Annex K.3's four Huffman tables, canonical codes; per block the DC difference against the previous block of the same
 *            component (category + magnitude bits, a negative value v as v - 1 in `category` bits), then (run, size) symbols for the
 *            non-zero AC levels in zigzag order, ZRL (0xF0) for every 16 zeros of a run, EOB unless level 63 is non-zero; bits most
 *            significant first, a byte 0xFF followed by 0x00.
 *   Restarts.  restart = R in 1..65535: a DRI segment; after every R MCUs (but the last) the stream is padded with 1-bits to a byte, RSTm
 *            with m = k mod 8 for the k-th marker follows, and the DC predictions restart at 0.  R = 0: no DRI, no markers; the device then
 *            codes the whole image as one interval in one workgroup -- correct and slow.  FLUXMI_JPEG_RESTART_420 / _444 (24 blocks per
 *            interval either way) are what fluxmi.ops picks when not told: ~2.5 bytes per interval, 0.1 - 0.6 % of a quality-99 file.
 *   Header.  SOI, APP0 (JFIF 1.01, aspect 1:1), DQT 0, DQT 1, SOF0, DHT (DC 0, AC 0, DC 1, AC 1), DRI when R > 0, SOS; EOI ends the file.
 * Three launches and no host wait: (1) one workgroup per 16 x 16 pixels converts, downsamples, transforms and quantises into int16 levels,
 * zigzag order, MCU by MCU; (2) one workgroup per interval codes its blocks, one wave per block (a ballot gives the non-zero mask, each
 * lane its run, code and length, a wave prefix sum the bit positions), assembles the bits in LDS, stuffs them and writes them to the
 * interval's own slot of `work` -- FLUXMI_JPEG_SLOT_BYTES_PER_BLOCK bytes per block, twice the worst case of 1660 bits, so no slot can
 * overflow -- and records the byte count; (3) a prefix sum of the counts, then each slot is copied behind the header with its marker.
 * An interval's bytes are written by its own workgroup alone: the same input gives the same bytes, run to run.
 * fluxmi_jpeg_workspace_bytes: *work_bytes = the size of `work` (256-byte aligned), *out_cap = a size of `out` no stream can exceed.
 * fluxmi_jpeg_encode: asynchronous.  Writes the file to out[0 .. n) and n (int64) to *n_bytes_dev, a DEVICE address.  No byte at or beyond
 *   out + out_cap is written whatever n is; n > out_cap means the file did not fit and `out` holds a truncated stream.  An out_cap below the
 *   header + EOI is refused here.
 * fluxmi_jpeg_finish: the one small read-back: *n_bytes = *n_bytes_dev after synchronising `stream`; n > out_cap is an error.
 * fluxmi_jpeg_header: host only: the header bytes (SOI .. SOS) of such a file into buf[0 .. cap), *n_bytes = their count. */
#define FLUXMI_JPEG_420 0
#define FLUXMI_JPEG_444 1
#define FLUXMI_JPEG_RESTART_420 4
#define FLUXMI_JPEG_RESTART_444 8
#define FLUXMI_JPEG_SLOT_BYTES_PER_BLOCK 416
int fluxmi_jpeg_workspace_bytes(int B, int H, int W, int subsampling, int restart, long long* work_bytes, long long* out_cap);
int fluxmi_jpeg_encode(const void* rgb, long long ld, long long bs, int B, int H, int W, int quality, int subsampling, int restart, void* work,
                       void* out, long long out_cap, void* n_bytes_dev, void* stream);
int fluxmi_jpeg_finish(const void* n_bytes_dev, long long out_cap, long long* n_bytes, void* stream);
int fluxmi_jpeg_header(int B, int H, int W, int quality, int subsampling, int restart, void* buf, long long cap, long long* n_bytes);

/* ---- depth estimator pieces (csrc/depth.hip; modules/depth.py: Depth Anything = a DINOv2 tower + a DPT decoder) -----------------------
 * The tower runs on the vision-encoder entry points above, the decoder's stride-1 convolutions on fluxmi_conv3x3 / fluxmi_conv3x3_dense; what
 * those do not cover is here.  Maps are NHWC bf16: [B][H][W] pixels addressed densely with ONE pixel stride `ld` in elements (ld >= C,
 * ld %% 8 == 0, 16-byte aligned pointers), so an operand may be a channel window of a wider buffer; channels outside [0, C) of a pixel are
 * neither read nor written.  Every function is deterministic (no atomics, fixed order), a sample's bits depend on that sample alone, and
 * all address arithmetic is 64-bit.
 *
 * fluxmi_unary: y[r][c] = bf16(f(x[r][c])) for rows of `cols` bf16 values with row strides ld_in, ld_out (>= cols), f in fp32, ONE rounding:
 *   FLUXMI_UNARY_GELU_ERF  0.5 x (1 + erf(x * 0.70710678118654752440f))   (torch's exact GELU; fluxmi_act's mode 0 is the tanh form)
 *   FLUXMI_UNARY_RELU      x > 0 ? x : 0                                   (a NaN gives 0)
 *   Any cols >= 1: full groups of 8 columns move as 16 bytes when both pointers are 16-byte aligned and both strides multiples of 8, the
 *   tail (and everything otherwise) element by element.  y may be x.
 * fluxmi_resize_bilinear: x [B][Hi][Wi] -> out [B][Ho][Wo], C channels (C %% 8 == 0), align_corners=True, any sizes >= 1.  Per axis, as
 *   torch computes it:  scale = fp32(in - 1) / fp32(out - 1) (0 when out == 1);  src = scale * fp32(o), in fp32;  i0 = (int)src, clamped to
 *   in - 1;  i1 = i0 + 1 unless i0 == in - 1, then i0;  l = src - i0;  h = 1 - l.  With a, b = x(y0, x0), x(y0, x1) and c, d = x(y1, x0), x(y1, x1):
 *     top = hx * a + lx * b;   bot = hx * c + lx * d;   v = hy * top + ly * bot        each product and sum rounded to fp32 (no fma contraction
 *   is relied on: the gate of tests/test_depth_gpu.py covers either);  out = bf16(v).  Equal sizes give scale 1 and l = 0: out == x exactly.
 *   With `add` ([B][Ho][Wo] pixels, stride add_ld; NULL = none):  out = bf16(fp32(bf16(v)) + add)  -- torch's bf16 tensor sum.  out != x.
 * fluxmi_patchify_rect: fluxmi_patchify for a grid_h x grid_w grid: row (b, gy, gx), column c*patch*patch + ky*patch + kx, zero past C*patch*patch
 *   (one gather kernel serves both, csrc/text.hip: fluxmi_patchify is the grid_h = grid_w case).
 * fluxmi_im2col3x3_s2: x [B, Hi, Wi, C] dense -> col [B*Ho*Wo, 9*C], Ho = (Hi - 1) / 2 + 1, Wo likewise, column (dy*3+dx)*C + c = input pixel
 *   (2 yo + dy - 1, 2 xo + dx - 1), zero outside the image: the patch matrix of Conv2d(kernel 3, stride 2, padding 1) at odd and even sizes
 *   (fluxmi_im2col3x3's -2 mode pads right / bottom only and needs even sizes; the same kernel, csrc/vae.hip, at stride 2 and pad 1).  The
 *   convolution is then the bf16 GEMM.  C %% 8 == 0.
 * fluxmi_depth_head: out[p] = max(0, sum_c x[p][c] * w[c] + bias[0]) for n pixels (stride ldx), fp32: acc = fma(x_c, w_c, acc) from 0 with c
 *   ascending, then + bias, then the ReLU; out fp32 [n], NOT rounded to bf16.  w bf16 [C], bias bf16 [1] or NULL, C %% 8 == 0 (the caller
 *   zero-pads).  This is the head's last 1x1 convolution + ReLU of a relative-depth model.
 * fluxmi_depth_to_map: depth fp32 [B][h][w] (row stride ld, image stride bs, in elements) -> out uint8 [B][H][W][3] (row stride out_ld, image
 *   stride out_bs, in bytes; out_ld >= 3 W), the value written to all three channels.  Half-pixel bilinear (align_corners=False), per axis as
 *   torch computes it:  scale = fp32(in) / fp32(out);  src = max(scale * (o + 0.5) - 0.5, 0);  i0, i1, l, h and the four-tap blend v as above.
 *     FLUXMI_DEPTH_MINMAX  t = (v - mn) * s, with mn / mx the minimum / maximum of THIS image's SOURCE depth (not the resized one) and
 *                          s = 255 / (mx - mn) in fp32, s = 0 for a constant image (which therefore gives 0 everywhere)
 *     FLUXMI_DEPTH_RAW     t = v
 *   byte = clamp(floor(t + 0.5), 0, 255) (a NaN gives 0).  The minimum and maximum come from two launches -- per-chunk partials of 4096
 *   elements, then one workgroup per image over the partials, each a fixed tree -- into `work` (fp32, 4-byte aligned,
 *   FLUXMI_DEPTH_MAP_WORK_BYTES(B, h, w) bytes; unused and may be NULL for FLUXMI_DEPTH_RAW).  B, H <= 65535. */
#define FLUXMI_UNARY_GELU_ERF 0
#define FLUXMI_UNARY_RELU 1
#define FLUXMI_DEPTH_MINMAX 0
#define FLUXMI_DEPTH_RAW 1
#define FLUXMI_DEPTH_MAP_WORK_BYTES(B, h, w) ((long long)(B) * ((((long long)(h) * (w) + 4095) / 4096) + 1) * 8)
int fluxmi_unary(const void* x, void* y, long long rows, int cols, long long ld_in, long long ld_out, int kind, void* stream);
int fluxmi_resize_bilinear(const void* x, long long ldx, void* out, long long ldo, const void* add, long long add_ld, int B, int Hi, int Wi, int Ho,
                           int Wo, int C, void* stream);
int fluxmi_patchify_rect(const void* pix, void* out, int B, int C, int H, int W, int patch, int grid_h, int grid_w, int Kp, void* stream);
int fluxmi_im2col3x3_s2(const void* x, void* col, int B, int Hi, int Wi, int C, void* stream);
int fluxmi_depth_head(const void* x, long long ldx, int C, const void* w, const void* bias, float* out, long long n, void* stream);
int fluxmi_depth_to_map(const float* depth, long long ld, long long bs, void* out, long long out_ld, long long out_bs, float* work,
                        long long work_bytes, int B, int h, int w, int H, int W, int normalize, void* stream);

/* ---- step scalars -------------------------------------------------------------------------------------- */
/* timestep_embedding(t, 2*half) with host-provided frequency table                 flux_model.py:95-116 */
int fluxmi_timestep_embedding(const void* t, const float* freqs, void* out, int B, int half, float time_factor, void* stream);
/* img += dts[*step] * pred                                                          flux_pipeline.py:651 */
int fluxmi_euler(void* img, const void* pred, const float* dts, const int* step, long long n, void* stream);
/* The guided Euler update (true classifier-free guidance).  img bf16 [2B, img_rows, c_in], pred bf16 [2B, pred_rows, c_out]: sample b is the
 * prompt branch, sample B + b the negative branch of the same image.  For every predicted element (rows [0, pred_rows), channels
 * [0, c_out) of a sample), with c = pred[b], u = pred[B + b], x = img[b], s = *scale, dt = dts[*step] (step NULL: dts[0]):
 *   d = bf16(c - u);  m = bf16(s * d);  p = bf16(u + m);  x' = bf16(x + bf16(dt * p));  img[b] = img[B + b] = x'
 * i.e. the torch expression x + dt * (u + s * (c - u)) on bf16 tensors.  x is read from the prompt half only, so the halves are
 * bit-identical afterwards.  pred_rows < img_rows (Kontext reference rows) or c_out < c_in (Fill / Depth / Canny conditioning channels),
 * not both: those rows / channels are neither read nor written.  dts, step, scale are DEVICE pointers; c_in, c_out multiples of 8. */
int fluxmi_cfg_euler(void* img, const void* pred, const float* dts, const int* step, const float* scale, int B, long long img_rows,
                     long long pred_rows, int c_in, int c_out, void* stream);
/* The masked-latent (inpainting) update: the Euler step, then the blend with the init latent re-noised to the NEXT time.  img, pred, dts,
 * step, B, img_rows, pred_rows, c_in, c_out as for fluxmi_cfg_euler; scale == NULL: the unguided update on img [B, ...] / pred [B, ...], else
 * the guided one on [2B, ...] (x read from the prompt half, x' written to both).  x0, noise, mask: dense bf16 [B, pred_rows, c_out];
 * tnext, one_minus_tnext (and thr): DEVICE fp32 tables indexed by *step like dts.  Per predicted element, one bf16 rounding per operation:
 *   x1 = x + dt * v                (guided: v = u + s * (c - u))
 *   p  = tnext * noise + one_minus_tnext * x0
 *   x' = (1 - m) * p + m * x1      (m = 1: regenerate, m = 0: keep)
 * i.e. those torch expressions on bf16 tensors.  thr == NULL: m = mask (a linear blend).  Else (differential diffusion) m = 1 where
 * float(mask) > thr[*step], compared in fp32, and 0 elsewhere.  Reference rows and conditioning channels are neither read nor written. */
int fluxmi_blend_euler(void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts, const float* tnext,
                       const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B, long long img_rows,
                       long long pred_rows, int c_in, int c_out, void* stream);
/* The table-driven solver update (higher-order samplers): one linear update whose coefficients are DEVICE tables indexed
 * by *step like dts (step NULL: row 0), so the caller's tables decide which solver runs.  img, pred, step, scale, B, img_rows, pred_rows, c_in,
 * c_out as for fluxmi_blend_euler (scale == NULL: unguided on [B, ...]; else guided on [2B, ...], x read from the prompt half, x' written to
 * both).  xs: bf16 [B, pred_rows, c_out], a saved iterate; hist: fp32 [2][B, pred_rows, c_out], two history slots; coef: fp32 [n][8] =
 * {cx, cs, c0, c1, c2, ga, gb, 0}; ctl: int32 [n][4] = {save_xs, w_slot, h1_slot, h2_slot}, a slot is -1, 0 or 1.  Per predicted element:
 *   v   = pred                          (guided: fluxmi_cfg_euler's bf16 chain d, m, p)
 *   g   = ga * x + gb * v               fp32
 *   acc = cx * x + cs * xs + c0 * g + c1 * hist[h1_slot] + c2 * hist[h2_slot]      fp32, left to right
 *   x1  = bf16(acc)
 * Every product and every sum is rounded to fp32 on its own (no fma).  A term whose coefficient is exactly 0.0f or whose slot is -1 is
 * skipped and its buffer never read (it may hold anything); the sum starts at the first term present.  x0 != NULL (with noise, mask, tnext,
 * one_minus_tnext, optionally thr: fluxmi_blend_euler's operands): its blend then runs on x1, same roundings, same differential compare.
 * After all reads of the element: save_xs stores the pre-update x to xs, w_slot >= 0 stores g to hist[w_slot] (which may be a slot just
 * read), x' goes to img.  Reference rows and conditioning channels are neither read nor written; 16-byte accesses. */
int fluxmi_solver_step(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0, const void* noise,
                       const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step, const float* scale,
                       int B, long long img_rows, long long pred_rows, int c_in, int c_out, void* stream);
/* Counter-based Gaussian noise (stochastic samplers): Philox4x32-10 with the published constants, then Box-Muller.
 * ids: DEVICE uint32 [B][4] = {key_lo, key_hi, c2, c3} per image.  Element e of an image belongs to Philox block q = e / 4: counter
 * (q, eval, c2, c3), key (key_lo, key_hi) -> words w0..w3 -> four normals,
 *   u = ((w_even >> 9) + 0.5f) * 2^-23 in (0, 1),  t = (w_odd >> 8) * 2^-24 in [0, 1)     (both exact in fp32)
 *   r = sqrtf(-2.f * logf(u)),  (s, c) = sincospif(2.f * t),  z = r*c, r*s from (w0, w1), then r*c, r*s from (w2, w3)
 * so a value is a pure function of (ids[b], eval, e): no state, no dependence on B or on the launch.  out: [B][n_per_image], raw = 1 the
 * uint32 words, raw = 0 the fp32 normals; n_per_image %% 8 == 0.  The device function is the one fluxmi_solver_step_noise draws from. */
int fluxmi_philox_normal(void* out, const unsigned* ids, int B, long long n_per_image, unsigned eval, int raw, void* stream);
/* fluxmi_solver_step with the stochastic samplers' noise term: column 7 of the row is cn, and after the c2 term
 *   acc = acc + (cn * z)                (product and sum each rounded to fp32; then x1 = bf16(acc), then the blend if set)
 * z = the normal fluxmi_philox_normal gives element e of image b's dense [pred_rows, c_out] block for ids[b] at eval = *step + *eval_offset
 * (eval_offset: DEVICE int, NULL = 0; step NULL = 0).  ids: DEVICE uint32 [B][4], per IMAGE: a guided call draws once per image and writes
 * x' to both halves as before.  cn == 0.0f: the term is skipped like every absent term, ids is not read and nothing is generated -- the
 * result is fluxmi_solver_step's bit for bit.  Everything else, refusals included, as for fluxmi_solver_step; NULL ids is refused. */
int fluxmi_solver_step_noise(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0,
                             const void* noise, const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step,
                             const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out, const unsigned* ids,
                             const int* eval_offset, void* stream);

/* ---- FlowEdit: inversion-free text-guided editing of an init image (Kulikov et al. 2024, Algorithm 1) --------------
 * img / pred: bf16 [2B, rows, C]; sample b is the SOURCE branch of image b, sample B + b its TARGET branch.  z (the edit state) and x0 (the
 * init image's latent tokens, never modified): bf16, dense [B, rows, C].  ids: DEVICE uint32 [B][4] per image, as for fluxmi_philox_normal.
 * Coupling at time t and draw index ev, with n = bf16(the normal fluxmi_philox_normal gives element e of image b for ids[b] at eval = ev):
 *   zs = bf16( bf16((1 - t) * x0) + bf16(t * n) )  -> img[b]          zt = bf16( bf16(z + zs) - x0 )  -> img[B + b]
 * one bf16 rounding per operation, t and 1 - t fp32 (one_minus_t is the caller's: subtracted in double).  fluxmi_flowedit_couple is the
 * coupling alone at HOST scalars; z is only read.
 * fluxmi_flowedit_step: the update after an evaluation, then the next coupling.  coef: DEVICE fp32 [n][4] = {w, dt, tn, 1 - tn}, ctl: DEVICE
 * int32 [n][2] = {first, apply}; row j = *step (step: DEVICE int, NULL = 0), vs = pred[b], vt = pred[B + b]:
 *   d   = bf16(vt - vs)
 *   acc = (first ? 0 : acc) + w * float(d)            fp32, the product and the sum each rounded (never fused)
 *   apply:  D = bf16(acc);  m = bf16(dt * D);  z' = bf16(float(z) + float(m)), stored to z;        else acc is stored
 *   then the coupling at t = tn with ev = *step + 1 + *eval_offset (eval_offset: DEVICE int, NULL = 0) on z' (z without apply).
 * acc: fp32, dense [B, rows, C]: stored by a row without apply, read by a row without first.  A row with first AND apply (one evaluation per
 * step) neither reads nor writes it and acc may be NULL; NULL acc with any other row is refused (this entry then reads *step and the row
 * back, which synchronises the stream: the engine, which knows its program, does not).  pred and x0 are never written; every read of an
 * element precedes its writes; 16-byte accesses, one thread per 8 elements (two Philox blocks).
 * Refused: c_in != c_out or pred_rows != img_rows (v1 steps the whole stream: no Kontext rows, no conditioning channels), NULL ids,
 * c_out %% 8 != 0, more than 2^31 - 1 vectors. */
int fluxmi_flowedit_couple(void* img, const void* z, const void* x0, float t, float one_minus_t, const unsigned* ids, unsigned eval, int B,
                           long long img_rows, long long pred_rows, int c_in, int c_out, void* stream);
int fluxmi_flowedit_step(void* img, const void* pred, void* z, float* acc, const void* x0, const float* coef, const int* ctl, const int* step,
                         const unsigned* ids, const int* eval_offset, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                         void* stream);

/* ---- tiled generation: a canvas stepped from overlapping windows (MultiDiffusion, Bar-Tal et al. 2023) -------------
 * canvas x: bf16, dense [N, Hc, Wc, C], the token grid of the packed latent, row-major.  img / pred: bf16 [S, h * w, C], S = N * ny * nx, or
 * [2S, ...] when guided (the negative branches behind the prompt branches).  Sample s = (n * ny + a) * nx + b is window (a, b) of image n; its
 * token i * w + j is canvas token (row0[a] + i, col0[b] + j).  Windows sit on a Cartesian grid, so placement and blend weights are separable.
 * DEVICE tables: row0 int32 [ny], col0 int32 [nx], Ny fp32 [ny][Hc], Nx fp32 [nx][Wc]; the weight tables are normalised per canvas position
 * by the caller (fluxmi/windows.py) and zero outside their window.  A window (a, b) COVERS canvas token (r, c) when row0[a] <= r < row0[a] + h
 * and col0[b] <= c < col0[b] + w.  fluxmi_window_step, per canvas element, with dt = dts[*step] (dts: DEVICE fp32; step: DEVICE int, NULL = 0):
 *   v_k  = pred[s_k]                                                                unguided (scale == NULL)
 *          d = bf16(c - u); m = bf16(s * d); p = bf16(u + m)  (fluxmi_cfg_euler's chain) on c = pred[s_k], u = pred[S + s_k], s = *scale (DEVICE)
 *   wgt  = Ny[a][r] * Nx[b][c]                                                       fp32, rounded
 *   num  = sum over the covering windows, ascending (a, b), of wgt * v_k             fp32, the product and the sum each rounded (never fused)
 *   vbar = bf16(num)
 *   x'   = bf16(float(x) + float(bf16(dt * vbar)))                                   (fluxmi_euler's last operation)
 *   canvas <- x';  img[s_k] (and img[S + s_k] when guided) <- x' for every covering window
 * fluxmi_window_gather is the last line alone with x' = x: it fills the stream from the canvas before the first evaluation (guided != 0: both
 * halves); the canvas is only read.  pred and the tables are never written; every read of a vector precedes its writes; 16-byte accesses, one
 * thread per 8 channels of one canvas token; a stream element maps to exactly one canvas token.  No LDS, no atomics.
 * Refused: C %% 8 != 0, a window that leaves the canvas (h > Hc, w > Wc, row0[a] outside [0, Hc - h], col0[b] outside [0, Wc - w]), a canvas row
 * or column that no window covers, NULL tables, more than 2^31 - 1 vectors in the canvas or in the stream.  The placement rules speak of the
 * tables' contents: these entries read row0 / col0 back, which synchronises the stream (the engine, which is given host tables, does not). */
int fluxmi_window_gather(const void* canvas, void* img, const int* row0, const int* col0, int N, int Hc, int Wc, int h, int w, int ny, int nx,
                         int C, int guided, void* stream);
int fluxmi_window_step(void* canvas, void* img, const void* pred, const float* dts, const int* step, const float* scale, const int* row0,
                       const int* col0, const float* Ny, const float* Nx, int N, int Hc, int Wc, int h, int w, int ny, int nx, int C,
                       void* stream);

/* ---- guidance shaping of true classifier-free guidance: CFG rescale, APG, CFG-Zero*  ------------------------------
 * Operands as for fluxmi_cfg_euler: pred bf16, dense [2B][N], N = pred_rows * c_out, N %% 8 == 0; sample b is c (the prompt branch), sample
 * B + b is u (the negative branch).  r: fp32, dense [B][N], APG's running difference (NULL: no r; its sums are 0, it is never touched and mu
 * counts as 0).  params: DEVICE float[8] = {s, phi, eta, rho, mu, mode, zero_init, 0}; mode 0 = CFG, 1 = APG, 2 = CFG-Zero*.
 *
 * moments: grid (ceil(N / 16384), B); workgroup g of image b owns elements [16384 g, 16384 (g + 1)) (fluxmi_fb_metric's rule) and writes the
 * nine fp32 sums  Sc, Su, Sr, cc, uu, rr, cu, cr, ur  (plain sums, then sums of products) over them to part[b][g][9].  256 threads, 16-byte
 * loads; a thread adds its vectors in ascending order (at most 64 adds per sum), then a fixed 8-level tree over the 256 threads (wave64
 * butterfly, (w0 + w1) + (w2 + w3) through LDS); every product and every sum is rounded on its own; no atomics.  An image's partials depend
 * on its own N elements only: the same bits alone, in any batch, at every launch.
 *
 * combine: grid (ceil(N / 16384), B).  Every workgroup of image b adds part[b][0..] in fp64 in ascending g, evaluates in fp64
 *   CFG:        alpha = s,  beta = 1 - s,  gamma = 0
 *   CFG-Zero*:  s* = cu / uu (1 if uu == 0);  alpha = s,  beta = s* (1 - s),  gamma = 0                    [ = s* u + s (c - s* u) ]
 *   APG:        p = c + (s - 1)(d_perp + eta d_par),  d = c - u + mu r  projected on c:
 *               dd = cc + uu + mu^2 rr - 2 cu + 2 mu cr - 2 mu ur;  dc = cc - cu + mu cr
 *               tau = min(1, rho / sqrt(dd)) if rho > 0 and dd > 0, else 1;  k = tau dc / cc (0 if cc == 0)
 *               alpha = 1 + (s - 1)(tau + (eta - 1) k);  beta = -(s - 1) tau;  gamma = (s - 1) tau mu
 *   rescale (phi > 0, on whichever coefficients resulted):
 *               mean_p = (alpha Sc + beta Su + gamma Sr) / N
 *               E[p^2] = (alpha^2 cc + beta^2 uu + gamma^2 rr + 2 alpha beta cu + 2 alpha gamma cr + 2 beta gamma ur) / N
 *               var_p = E[p^2] - mean_p^2;  var_c = max(0, cc / N - (Sc / N)^2)
 *               f = phi sqrt(var_c / var_p) + (1 - phi)  (1 if var_p <= 0);  alpha, beta, gamma *= f
 *   zero-init:  *step + *step_offset < zero_init (step, step_offset: DEVICE ints, NULL = 0):  alpha = beta = gamma = 0
 * and casts alpha, beta, gamma to fp32: all workgroups of an image hold the same bits.  Workgroup 0 writes coef_out[b] = {alpha, beta,
 * gamma, f} (fp32 [B][4], may be NULL; f as computed, zero-init or not).  Then per element, in fp32, every product and sum rounded on its
 * own (no fma):
 *   v = bf16((alpha c + beta u) + gamma r)  -> pred[b] AND pred[B + b]
 *   mu != 0:  r' = (c - u) + mu r  -> r, stored behind all reads of the element           (mu == 0: r is neither read nor written)
 * A term whose coefficient is exactly 0.0f is skipped and its buffer not read (fluxmi_solver_step's rule); the sum starts at the first term
 * present, 0 when none.  With v in both halves every guided update kernel (fluxmi_cfg_euler, guided fluxmi_blend_euler / _solver_step) computes
 * d = bf16(v - v) = 0, m = 0, p = v and steps with v as it is, for every finite scale.  part: float [B][ceil(N / 16384)][9]. */
int fluxmi_guidance_moments(const void* pred, const float* r, float* part, int B, long long N, void* stream);
int fluxmi_guidance_combine(void* pred, float* r, const float* part, const float* params, const int* step, const int* step_offset,
                            float* coef_out, int B, long long N, void* stream);

/* ---- latent preview -------------------------------------------------------------------
 * The denoised estimate of ONE model evaluation, projected to RGB at latent resolution (csrc/preview.hip).  x: bf16 [B (2B guided), img_rows,
 * c_in], the model input of the evaluation -- only the leading pred_rows rows of each sample and the leading c_out = 64 channels of a row are
 * read (Kontext's reference rows and Fill / Depth / Canny's conditioning channels trail them).  pred: bf16, dense [B (2B guided), pred_rows,
 * 64]; scale != NULL (DEVICE fp32 scalar) is the guided form: sample b is c (the prompt branch), sample B + b is u, and only the B prompt
 * samples produce images.  ts: DEVICE fp32 table, step: DEVICE int (NULL = 0); t = ts[*step].  proj: DEVICE float [51] = M[16][3], then
 * bias[3].  ctl: DEVICE int [2] = {every, eval_offset} (NULL = {1, 0}).  out: uint8 [FLUXMI_PREVIEW_SLOTS][B][2 h][2 w][3].
 *
 * For image b, token r = ty * w + tx of the h x w token grid (h * w == pred_rows), sub-pixel sub = py * 2 + px and latent channel c in 0..15
 * the packed column is c * 4 + sub (FluxPipeline.unpack's layout).  In fp32, every operation rounded once, fma = one fused multiply-add:
 *   v    = pred                                  plain
 *   v    = fma(s, c - u, u)                      guided: the subtraction rounded on its own, s = *scale
 *   x0_c = fma(-t, v, x)
 *   a_k  = bias_k;  a_k = fma(M[c][k], x0_c, a_k)  for c = 0, 1, .., 15 in this order            (k = 0, 1, 2)
 *   q    = rint(fma(0.5, a_k, 0.5) * 255)        the product rounded on its own, rint = round half to even
 *   out[slot][b][2 ty + py][2 tx + px][k] = uint8(q > 0 ? (q < 255 ? q : 255) : 0)               NaN -> 0
 * With g = eval_offset + *step the launch writes nothing unless every > 0 and g % every == 0, and then writes slot
 * (g / every) % FLUXMI_PREVIEW_SLOTS; every other slot keeps its bytes.  every and eval_offset are device data: one captured graph serves
 * every cadence and every slice of a request.  One thread per token, sixteen (guided: twenty-four) 16-byte loads -- the token's 128 contiguous
 * bytes of x and of pred -- and twelve byte stores; no LDS, no atomics.  An image's bytes depend on its own tokens only.
 * Refused: c_out != 64, h * w != pred_rows, img_rows < pred_rows, c_in < 64 or no multiple of 8, x / pred not 16-byte aligned. */
#define FLUXMI_PREVIEW_DEPTH 2                          /* evaluations the host loop of a hooked denoise call may be ahead of the GPU */
#define FLUXMI_PREVIEW_SLOTS (FLUXMI_PREVIEW_DEPTH + 1) /* slots of the preview ring (fluxmi_engine_set_preview has the argument) */
int fluxmi_latent_preview(const void* x, const void* pred, const float* ts, const int* step, const float* scale, const float* proj,
                          const int* ctl, void* out, int B, long long img_rows, long long pred_rows, int c_in, int c_out, int h, int w,
                          void* stream);

/* ---- first-block step cache: the streaming passes --------------------------------------
 * B samples of n bf16 elements each (n = cached rows x hidden, n %% 8 == 0).  The `x` side is the residual stream: the pointer is the first
 * cached row of sample 0, x_bstride the batch stride in elements; every other tensor is dense [B, n].  16-byte accesses; workgroup c of a
 * sample owns its elements [c * 16384, (c + 1) * 16384).
 *   snapshot: dst = x                                              (h0, before double block 0)
 *   metric:   r = bf16(x - h0)  (fp32 subtract, one rounding; r may be h0's buffer);  num_b = sum |r - r_ref|, den_b = sum |r_ref| in fp32,
 *             ratio[b] = num_b / den_b (+inf when den_b == 0), numden[2b], numden[2b + 1] = num_b, den_b (numden may be NULL).  Two stages, no
 *             atomics: per-workgroup partials into `part` (float [B][ceil(n / 16384)][2], scratch), then one workgroup per sample adds them
 *             in a fixed order.  A sample's three numbers depend on its own n elements only: same bits alone, in any batch, at every launch.
 *   commit:   r_ref = r, h1 = x                                    (a miss, before the remaining blocks run)
 *   store:    R = bf16(x - h1)                                     (a miss, after the last single block)
 *   apply:    x = bf16(h1 + R); h1 strided like x (h1_bstride) and allowed to be x itself  (a hit) */
int fluxmi_fb_snapshot(const void* x, long long x_bstride, void* dst, int B, long long n, void* stream);
int fluxmi_fb_metric(const void* x, long long x_bstride, const void* h0, void* r, const void* r_ref, float* part, float* ratio, float* numden,
                     int B, long long n, void* stream);
int fluxmi_fb_commit(const void* x, long long x_bstride, const void* r, void* r_ref, void* h1, int B, long long n, void* stream);
int fluxmi_fb_store(const void* x, long long x_bstride, const void* h1, void* R, int B, long long n, void* stream);
int fluxmi_fb_apply(void* x, long long x_bstride, const void* h1, long long h1_bstride, const void* R, int B, long long n, void* stream);

/* ---- ControlNet residual hand-over ---------------------------------------------------
 *   x[b, j] = bf16(x[b, j] + bf16(r[b, j] * *scale))     for b < B, j < n
 * i.e. the torch expression x + r * s on bf16 tensors with s a Python float (diffusers' FluxControlNetModel scales its block samples by
 * conditioning_scale, FluxTransformer2DModel adds them to the image stream).  x, r: bf16 with batch strides x_bstride / r_bstride in elements
 * (>= n); scale: DEVICE fp32 scalar, used as it is -- never rounded to bf16 -- so one captured graph serves every scale.  Any n; 16-byte
 * accesses when both pointers are 16-byte aligned and both strides are multiples of 8, element accesses otherwise (same arithmetic). */
int fluxmi_add_scaled(void* x, long long x_bstride, const void* r, long long r_bstride, const float* scale, int B, long long n, void* stream);

/* ---- whole-model engine ------------------------------------------------------------------------------- */
typedef struct fluxmi_linear {
  const void* weight;      /* fp8 float8_data [N,K] (kind 1) or bf16 weight [N,K] (kind 0) */
  const void* bias;        /* bf16 [N] or NULL */
  float* w_scale_recip;    /* F8Linear.scale_reciprocal        (device scalar) */
  float* in_scale;         /* F8Linear.input_scale             (device scalar) */
  float* in_scale_recip;   /* F8Linear.input_scale_reciprocal  (device scalar) */
  float* amax_trials;      /* F8Linear.input_amax_trials [num_trials] (device) */
  int kind;                /* 0 = nn.Linear (bf16), 1 = F8Linear */
  int N, K;
  int in_fmt;              /* FLUXMI_E5M2 / FLUXMI_E4M3 */
} fluxmi_linear_t;

typedef struct fluxmi_model_desc {
  int hidden, heads, mlp_hidden, depth, depth_single, in_channels, vec_in, ctx_in, guidance_embed;
  int axes_dim[3];
  int theta;
  int num_trials;
} fluxmi_model_desc_t;

/* Layer order in `linears` (count = fluxmi_engine_num_linears(desc)):
 *   img_in, time_in.in, time_in.out, vector_in.in, vector_in.out, [guidance_in.in, guidance_in.out], txt_in,
 *   per double block i: img_mod.lin, img_attn.qkv, img_attn.proj, img_mlp.0, img_mlp.2,
 *                       txt_mod.lin, txt_attn.qkv, txt_attn.proj, txt_mlp.0, txt_mlp.2
 *   per single block i: modulation.lin, linear1, linear2
 *   final_layer.adaLN_modulation.1, final_layer.linear
 * `norm_scales`: bf16 [128] pointers, per double block: img q, img k, txt q, txt k; per single block: q, k.
 * Channels: C_in = desc->in_channels is img_in's K, the width of the image stream; C_out = final_layer.linear's N is what the model predicts.
 * create requires C_out <= C_in, both multiples of 8.  C_out < C_in (FLUX.1 Fill [dev]: 384 / 64, Depth / Canny [dev]: 128 / 64): the trailing
 * C_in - C_out channels of every image row are step-invariant conditioning that img_in reads and the Euler update never writes. */
typedef struct fluxmi_engine fluxmi_engine_t;
int fluxmi_engine_num_linears(const fluxmi_model_desc_t* desc);
int fluxmi_engine_create(const fluxmi_model_desc_t* desc, const fluxmi_linear_t* linears, int n_linears,
                         const void* const* norm_scales, int n_norm_scales, fluxmi_engine_t** out);
int fluxmi_engine_destroy(fluxmi_engine_t* e);
/* constant tables computed by the host with the reference's own expressions: timestep frequencies
 * exp(-ln(1e4)*i/128) (flux_model.py:106-110), RoPE omega per pair and the id axis each pair uses (flux_model.py:50-51,84-90) */
int fluxmi_engine_set_tables(fluxmi_engine_t* e, const float* freqs128, const float* omega64, const int* axis64);
/* re-read weight pointers / kinds after a LoRA fuse or dtype swap (float8_quantize.py:209-212).  MANDATORY after ANY write to a weight
 * the engine was created / last re-bound with, even an in-place one that keeps the pointer: the engine SNAPSHOTS weights -- its GEMMs read a
 * row-pair copy of the block linears' fp8 weights (fluxmi_tuning_t.w_pairs, rebuilt on the first launch after a rebind), the 64 KiB
 * quantising-epilogue tables and the captured step graph are derived from the scales.  A write without a rebind is silently ignored.
 * The copies are made only while the device has at least twice their size + 4 GiB free (else the GEMMs read the caller's weights: same
 * results) and are freed when w_pairs is switched off.  A rebind that changes which linears are bf16 may drop the workspace: call
 * fluxmi_engine_prepare again before the next forward (the host wrapper does, per call). */
int fluxmi_engine_rebind(fluxmi_engine_t* e, const fluxmi_linear_t* linears, int n_linears);
/* per-request setup: (re)allocates the workspace for (B, Li, Lt), builds the RoPE table from the position ids
 * (step-invariant: flux_model.py:701-702) */
int fluxmi_engine_prepare(fluxmi_engine_t* e, int B, int Li, int Lt, const void* img_ids, const void* txt_ids, void* stream);
/* FLUX.1 Kontext (reference-image editing): the same setup for an image stream of Li predicted + Lc reference rows per sample.
 * img_ids: [B, Li+Lc, 3], the reference rows last in each sample (their axis 0 = 1).  fluxmi_engine_prepare == this with Lc = 0.  After a
 * prepare with Lc > 0, fluxmi_engine_forward / fluxmi_engine_denoise take img as [B, Li+Lc, in_channels]; forward writes pred as
 * [B, Li, in_channels] (the reference rows run through every block, only the leading Li rows are predicted); denoise steps rows [0, Li) of
 * each sample in place and leaves the reference rows bit-for-bit as they were.  The split (Li, Lc) is part of the workspace key: another
 * split of the same Li+Lc re-allocates and re-captures the step graph.  Lc > 0 is refused on a model with C_in != C_out (see create). */
int fluxmi_engine_prepare_cond(fluxmi_engine_t* e, int B, int Li, int Lc, int Lt, const void* img_ids, const void* txt_ids, void* stream);
/* one Flux.forward (flux_model.py:672-716).  mode 0 = calibrating/unfused (advances the F8Linear trial state
 * machine exactly like the reference's first 13 calls), 1 = frozen/fused.  img: bf16 [B, Li(+Lc), C_in], the conditioning channels (if any)
 * behind the noisy ones of every row; pred: bf16 [B, Li, C_out]. */
int fluxmi_engine_forward(fluxmi_engine_t* e, const void* img, const void* txt, const void* y, const void* timesteps,
                          const void* guidance, void* pred, int mode, int trial_index, void* stream);
/* the denoise loop (flux_pipeline.py:619-651): timesteps_host[n_steps+1]; img bf16 [B, Li(+Lc), C_in] updated in place: channels
 * [0, C_out) of the predicted rows are stepped, the conditioning channels [C_out, C_in) (and Kontext's reference rows) stay bit for bit.
 * Steps with trial_index <= num_trials run unfused; the remainder replays ONE captured hipGraph per step. */
int fluxmi_engine_denoise(fluxmi_engine_t* e, void* img, const void* txt, const void* y, float guidance,
                          const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream);
/* The same loop with true classifier-free guidance (a negative prompt).  The engine has been prepared for a batch of 2B whose halves
 * carry the same position ids; img is the caller's B samples [B, Li(+Lc), C_in], stepped in place exactly as above; txt [2B, Lt, ctx] and
 * y [2B, vec] hold the prompt branch first, then the negative branch of the same images.  img is copied into both halves of the engine's
 * stream, every step is ONE forward on the 2B samples followed by fluxmi_cfg_euler with scale = cfg_scale (any value; 1 reproduces the
 * prompt branch up to the roundings of the formula), in the calibrating and in the graph-replayed steps alike.  One trial per step, as in
 * a whole-batch calibration.  cfg_scale is device data of the captured graph: another scale replays the same graph; a plain and a guided
 * request of the same prepared shape never share one (each switch re-captures).  An odd prepared batch is refused (2B <=
 * FLUXMI_ENGINE_MAX_BATCH follows from prepare).  Timing, the amax-exchange hook and use_graph as for fluxmi_engine_denoise. */
int fluxmi_engine_denoise_cfg(fluxmi_engine_t* e, void* img, const void* txt, const void* y, float guidance, float cfg_scale,
                              const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream);
/* hipEvent timing of the frozen STEPS of the last fluxmi_engine_denoise / _denoise_cfg call: the first event is recorded on the caller's stream behind
 * the step-ahead modulation table, the eager warm step and the graph capture of a new shape (none of them is inside the window), the
 * second behind the last step (the reference's only meter is tqdm's it/s, flux_pipeline.py:628-630).  A request longer than 64 steps
 * includes the table builds of its later windows.  Blocks until the second event has completed.  steps = number of steps between the
 * events (0: nothing was timed, ms = 0).
 * FLUXMI_ROCTX=1 additionally emits roctx ranges (calibrating steps / modulation table / graph replays) for rocprofv3 --marker-trace. */
int fluxmi_engine_last_timing(fluxmi_engine_t* e, float* ms, int* steps);
/* Batch-sharded calibration: F8Linear.quantize_input takes amax over the WHOLE batch (float8_quantize.py:227).
 * With a hook installed the engine keeps the per-layer running amax in the caller's device array amax_dev[n >= n_linears] and
 * calls hook(user, first, count, stream) on the host after the amax of layers [first, first+count) is enqueued on `stream` and
 * before their scale update is: the host enqueues an all-reduce(MAX) of amax_dev[first..first+count) on that stream (RCCL via
 * torch.distributed) and returns 0.  Calibrating steps only; never called from the captured graph.  hook = NULL uninstalls. */
typedef int (*fluxmi_amax_hook_t)(void* user, int first, int count, void* stream);
int fluxmi_engine_set_amax_exchange(fluxmi_engine_t* e, float* amax_dev, int n, fluxmi_amax_hook_t hook, void* user);
/* introspection for tests / bench; workspace_bytes = every device byte the engine owns beside the caller's weights: the per-shape workspace,
 * the step-ahead modulation table and the row-pair weight copies (fluxmi_gemm_group_t.W_pairs; 8 GB at Flux-dev, 0 with fluxmi_tuning_t.w_pairs = 0) */
int fluxmi_engine_workspace_bytes(fluxmi_engine_t* e, long long* bytes);
int fluxmi_engine_get_buffer(fluxmi_engine_t* e, const char* name, void** ptr, long long* bytes);
/* Teacher-forced parity hooks (tests only).  run_block: stages [stage_from, stage_to] of DoubleStreamBlock (kind 0; stages
 * 0 LN+modulate->a8, 1 qkv GEMM->qkv(+V^T), 2 K relayout, 3 attention->attn8, 4 proj+gate+resid->x, 5 LN+modulate->a8,
 * 6 mlp.0+GELU->h8, 7 mlp.2+gate+resid->x; flux_model.py:356-400) or SingleStreamBlock (kind 1; 0 LN+modulate->a8,
 * 1 linear1->qkv(+V^T)|cat8[:,H:], 2 K relayout, 3 attention->cat8[:,:H], 4 linear2+gate+resid->x; flux_model.py:467-485) `index`
 * on the engine's own workspace: the residual stream is buffer "x" ([B, Lt+Li, H], txt rows first), the modulation vectors are read
 * from buffer "mod" (per batch row: double block i at [i*12H, +12H) = img shift1|scale1|gate1|shift2|scale2|gate2 then txt, single
 * block i at depth*12H + i*3H = shift|scale|gate, LastLayer.adaLN at depth*12H + single*3H = shift|scale).  kind 2 = LastLayer (index 0;
 * stages 0 LN+modulate of the img rows of x -> "fin", 1 bf16 Linear -> buffer "pred_s" [B, Li, C_out = out_channels]; flux_model.py:499-503).
 * mode 1 = fused kernels, 2 = unfused with frozen scales.
 * copy_buffer: device-to-device copy between a named workspace buffer and a caller buffer (to_engine != 0 writes the workspace).  The fp8
 * activation buffers "a8", "attn8", "h8", "cat8" are exchanged as PLAIN rows.  Inside the engine each one is in the layout of its last
 * writer -- row pairs after a fused step or stage (fluxmi_tuning_t.a_pairs, even L and Lt), plain rows after an unfused / calibrating one --
 * and the copy converts from (reading) or into (writing) that layout; offset / bytes must then cover whole pairs of rows.  A buffer written
 * here is read correctly by a stage that runs in the mode of that last writer (teacher forcing in mode 1 or 2). */
int fluxmi_engine_run_block(fluxmi_engine_t* e, int kind, int index, int mode, int stage_from, int stage_to, void* stream);
int fluxmi_engine_copy_buffer(fluxmi_engine_t* e, const char* name, long long offset, void* dev_ptr, long long bytes, int to_engine,
                              void* stream);

/* First-block step caching (off by default).  set_step_cache applies to the following fluxmi_engine_denoise /
 * _denoise_cfg calls: threshold <= 0 = off (those calls launch exactly what they launch without this entry point), negative / NaN refused,
 * max_consecutive_hits 0 = unbounded, negative refused.  On: every FROZEN step runs embedders + double block 0 ("head"), measures per sample
 *   ratio_b = sum |r - r_ref| / sum |r_ref|,  r = bf16(h1 - h0) on the rows the final layer reads, r_ref = the r of the last full step,
 * and the host reads the B ratios (one event wait per step).  HIT iff a full step has run in this call, every ratio_b < threshold and fewer
 * than max_consecutive_hits hits precede it in a row: x = bf16(h1 + R) on those rows, final layer, update ("skip").  Otherwise MISS: r_ref = r,
 * the remaining blocks run, R = bf16(x - h1) is stored, final layer, update ("body").  One decision per pass (all samples, both branches of a
 * guided request).  head / body / skip are three captured graphs sharing the plain step's device-side step counter; use_graph = 0 runs the
 * same pieces eagerly.  Calibrating steps never touch the cache.  The cache buffers ("fb_h0" = h0, overwritten by r; "fb_h1"; "fb_rref";
 * "fb_R"; all bf16 [B, Lpred, hidden]; "fb_ratio" = float ratio[B] | (num, den)[B]) are allocated at the first cached call of a prepared shape
 * and are readable through fluxmi_engine_copy_buffer.
 * step_cache_log: the frozen steps of the last denoise call, cached or not (a plain call: *n = 0): *n = their number, *batch = B of that pass, ratios[i * B + b]
 * and hit[i] for the first min(*n, cap) of them; a step with no reference yet (the first) logs +inf.  ratios / hit may be NULL with cap = 0. */
int fluxmi_engine_set_step_cache(fluxmi_engine_t* e, float threshold, int max_consecutive_hits);
/* Token-group attention mask (fluxmi_attention_grouped) for every attention launch of the PREPARED shape: `table` = [B, L] descriptors on
 * the device, L = Lt + Li in the order of the joint sequence (text rows, image rows, reference rows).  The engine copies them into its own
 * buffer (counted in fluxmi_engine_workspace_bytes) and checks on the host that every token admits its own group.  NULL turns masking off.
 * Masked versus dense is a kind of step graph like guided versus plain: a change re-captures; the table's CONTENTS are device data, so
 * one set of graphs serves every layout of a prepared shape.  A prepare that re-allocates the workspace clears the table.  Call it after
 * fluxmi_engine_prepare* and before forward / denoise. */
int fluxmi_engine_set_attn_groups(fluxmi_engine_t* e, const unsigned* table, void* stream);
int fluxmi_engine_step_cache_log(fluxmi_engine_t* e, int* n, int* batch, float* ratios, unsigned char* hit, int cap);
/* Masked-latent inpainting (and differential diffusion) for the following fluxmi_engine_denoise / _denoise_cfg calls on the PREPARED shape:
 * every update of those calls -- calibrating, graph-replayed, both tails of a step-cached step, guided -- is fluxmi_blend_euler instead of
 * the Euler / guided Euler kernel (as many launches per step as without a mask), with tnext[i] = (float)timesteps[i + 1] and
 * one_minus_tnext[i] = (float)(1.0 - timesteps[i + 1]) built from the call's schedule.  x0, noise, mask: device bf16 [batch, Li, C_out] for the
 * caller's `batch` images (the prepared B of a plain call, B / 2 of a guided one: checked by the denoise call), copied into the engine's own
 * buffers "inp_x0", "inp_noise", "inp_mask" (allocated at the first masked call of a prepared shape, dropped with the workspace, counted
 * in fluxmi_engine_workspace_bytes), so the caller's tensors are free again when this returns and a captured graph never holds their
 * pointers.  thresholds_host == NULL: the linear blend with the mask as given.  Else differential diffusion: n_thresholds doubles, one per
 * step of the denoise call -- a call with another n_steps is refused -- and step i blends with (float(mask) > (float)thresholds_host[i]).
 * x0 == NULL switches the feature off (the other arguments are ignored); a prepare that re-allocates the workspace does too.  Blend on / off
 * and differential on / off are kinds of step graph like guided versus plain: requests of different kinds alternating on one shape re-capture,
 * never replay each other's graph.  A request without a mask allocates and launches nothing of this.  Call it after fluxmi_engine_prepare*. */
int fluxmi_engine_set_inpaint(fluxmi_engine_t* e, const void* x0, const void* noise, const void* mask, int batch, const double* thresholds_host,
                              int n_thresholds, void* stream);
/* A solver program (higher-order samplers) for the following fluxmi_engine_denoise / _denoise_cfg calls on the PREPARED
 * shape: every update of those calls -- calibrating, graph-replayed, guided, with the inpainting state set -- is fluxmi_solver_step on the
 * tables given here instead of the (guided / blend) Euler kernel.  coef_host: n x 8 doubles, ctl_host: n x 4 ints, the rows of
 * fluxmi_solver_step (cast to fp32 here), n <= 1024.  An engine "step" is then one EVALUATION of the model: timesteps_host[j] is the model
 * time of evaluation j and timesteps_host[j + 1] the time of the iterate it produces (what the blend's tnext table reads); the dts table is
 * unused, and a denoise call whose n_steps != n is refused, as is one with step caching on.  The tables are device data carried through the
 * pinned schedule staging like dts: solver on / off is a kind of step graph like guided versus plain, and ONE graph serves every solver and
 * every schedule of a length.  The buffers "sol_xs" and "sol_hist" are allocated at the first solver call of a prepared shape, dropped
 * with the workspace and counted in fluxmi_engine_workspace_bytes.  coef_host == NULL switches the feature off; a prepare that re-allocates
 * the workspace does too.  A request without a solver allocates nothing and launches exactly what it launched before. */
int fluxmi_engine_set_solver(fluxmi_engine_t* e, const double* coef_host, const int* ctl_host, int n);
/* The noise of a stochastic solver program (column 7, cn, non-zero in some row): valid only after such a fluxmi_engine_set_solver, for the
 * denoise calls that program serves.  ids_host: batch x 4 uint32 = {key_lo, key_hi, c2, c3} per image (fluxmi_philox_normal); batch = the
 * caller's images -- the prepared batch, half of it for a guided call; the denoise call checks it, like fluxmi_engine_set_inpaint's.
 * eval_offset >= 0: evaluation j of the call draws at eval = j + eval_offset, so a request cut into several denoise calls draws what the
 * uncut one draws.  Every update of the call is then fluxmi_solver_step_noise.  ids and the offset are device data ("sol_ids": uint32
 * [prepared batch][4], then the offset) staged with the call's schedule like the coefficient tables: solver-with-noise is a kind of step graph
 * of its own, and ONE graph serves every seed and every offset.  "sol_ids" is allocated at the first such call of a prepared shape, counted
 * in fluxmi_engine_workspace_bytes and dropped with the workspace.  fluxmi_engine_set_solver (a new program, or NULL) and a prepare that
 * re-allocates the workspace switch the noise off; a denoise call whose program has a non-zero cn and no ids set is refused.  A deterministic
 * solver request and a request without a solver allocate and launch exactly what they did before. */
int fluxmi_engine_set_solver_noise(fluxmi_engine_t* e, const unsigned* ids_host, int batch, int eval_offset);
/* FlowEdit state (fluxmi_flowedit_step) for the following fluxmi_engine_denoise_edit calls on the PREPARED shape (2 x batch
 * samples: source branches first).  x0_dev: bf16 [batch, Li, C] on the device, copied into the engine-owned "fe_x0" on `stream`; coef_host:
 * n x 4 doubles, ctl_host: n x 2 ints, the rows of fluxmi_flowedit_step (cast to fp32 here), n <= 1024; ids_host: batch x 4 uint32 per image;
 * eval_offset >= 0: the call's first coupling draws at eval_offset and evaluation j's update at eval_offset + j + 1, so a request cut into
 * several calls draws what the uncut one draws.  source_guidance / target_guidance: the distilled-guidance value of each half of the batch.
 * Tables, ids and the offset are device data staged with the call's schedule; "fe_z" and -- only when some row lacks first or apply --
 * "fe_acc" are made at the first edit call of a prepared shape.  All of it is counted in fluxmi_engine_workspace_bytes and dropped with the
 * workspace.  x0_dev == NULL switches the state off; a prepare that re-allocates the workspace does too.  fluxmi_engine_denoise and
 * _denoise_cfg do not consult the state: a request without it allocates and launches exactly what it did before. */
int fluxmi_engine_set_flow_edit(fluxmi_engine_t* e, const void* x0_dev, int batch, const double* coef_host, const int* ctl_host, int n,
                                const unsigned* ids_host, int eval_offset, float source_guidance, float target_guidance, void* stream);
/* The edit loop: fluxmi_engine_denoise's loop -- calibrating steps, then frozen steps replayed from ONE captured graph -- on the 2 x batch
 * samples, with fluxmi_flowedit_step as every update.  z: bf16 [batch, Li, C], the edit state, in and out; txt [2 batch, Lt, ctx] and y
 * [2 batch, vec]: the source branches, then the target branches; timesteps_host[j], j < n_evals: the model time of evaluation j.  z is copied
 * to "fe_z", one coupling at (timesteps_host[0], eval_offset) fills the stream, and at the end "fe_z" is copied back.  Edit versus not is a
 * kind of step graph: seeds, offset, guidance pair and schedule are device data.  Refused: no state set, n_evals != its n, a batch other than
 * half the (even) prepared batch, reference rows or conditioning channels, an inpainting state, a solver program, step caching, an
 * attention-group table, an attached ControlNet, an IP-Adapter, and a step hook with every > 0 (a hook with every = 0 works: evaluation
 * counts model evaluations). */
int fluxmi_engine_denoise_edit(fluxmi_engine_t* e, void* z, const void* txt, const void* y, const double* timesteps_host, int n_evals,
                               int* trial_index_inout, int use_graph, void* stream);
/* Window state (fluxmi_window_step) for the following fluxmi_engine_denoise_windows calls on the PREPARED shape: S =
 * n_images * ny * nx samples (2S for a guided call) of Li = h * w rows with ONE set of window-local position ids, so that every window looks
 * like a stand-alone image to the model.  row0_host [ny], col0_host [nx], Ny_host [ny][Hc], Nx_host [nx][Wc]: the tables of
 * fluxmi_window_step on the HOST, checked here (placement rules, finite weights) and copied into the engine-owned "win_tab" on `stream`; the
 * call returns behind one stream synchronisation.  "win_x" (the canvas, bf16 [n_images, Hc, Wc, C]) is made with it.  Both are counted in
 * fluxmi_engine_workspace_bytes and dropped with the workspace.  Refused: S > the prepared batch (or > 32, one pass), h * w != Li.
 * row0_host == NULL switches the state off; a prepare that re-allocates the workspace does too.  fluxmi_engine_denoise and _denoise_cfg do
 * not consult the state: a request without windows allocates and launches exactly what it did before. */
int fluxmi_engine_set_windows(fluxmi_engine_t* e, int n_images, int Hc, int Wc, int h, int w, int ny, int nx, const int* row0_host,
                              const int* col0_host, const float* Ny_host, const float* Nx_host, void* stream);
/* The windowed loop: fluxmi_engine_denoise's loop -- calibrating steps, then frozen steps replayed from ONE captured graph -- on the S (guided
 * != 0: 2S) samples, with fluxmi_window_step as every update after one fluxmi_window_gather up front.  canvas: bf16 [n_images, Hc, Wc, C], in
 * and out (copied to "win_x" and back); txt [S or 2S, Lt, ctx] and y [S or 2S, vec]: one row per SAMPLE (guided: the negative branches in the
 * second half); guidance, cfg_scale, timesteps_host (n_steps + 1 times), trial_index_inout, use_graph as for fluxmi_engine_denoise_cfg.
 * Windowed versus not is a kind of step graph and the canvas geometry is part of its key; tables, scale and schedule are device data.
 * Refused: no state set, a prepared batch other than S (guided: 2S), reference rows or conditioning channels, an inpainting state, a solver
 * program, step caching, an attention-group table, an attached ControlNet, an IP-Adapter, a FlowEdit state, guidance shaping (guided), and a
 * step hook with every > 0 (a hook with every = 0 works: progress and cancellation). */
int fluxmi_engine_denoise_windows(fluxmi_engine_t* e, void* canvas, const void* txt, const void* y, float guidance, int guided, float cfg_scale,
                                  const double* timesteps_host, int n_steps, int* trial_index_inout, int use_graph, void* stream);
/* Guidance shaping (fluxmi_guidance_moments / _combine) for the following fluxmi_engine_denoise_cfg calls on the PREPARED
 * shape: every step of those calls -- calibrating, graph-replayed, both tails of a step-cached step -- launches moments and combine on
 * "pred_s" immediately in front of the update kernel the request already had (guided Euler, blend, solver, with or without noise), which
 * then steps with the shaped prediction.  params_host: the 8 floats of fluxmi_guidance_combine (finite; mode 0, 1 or 2; phi in [0, 1];
 * rho, zero_init >= 0), step_offset >= 0: evaluation j of the call counts as j + step_offset against zero_init, so a request cut into
 * several denoise calls zero-initialises what the uncut one does.  Both are device data staged with the call's schedule ("gd_params": float
 * [8] | the offset): shaped versus unshaped is a kind of step graph like guided versus plain, and ONE graph serves every mode and value.
 * The engine owns "gd_part", "gd_coef" (the last step's {alpha, beta, gamma, f} per image) and "gd_r" (fp32 [B / 2][Lpred * C_out]), made at
 * the first shaped call of a prepared shape, dropped with the workspace and counted in fluxmi_engine_workspace_bytes; EVERY set call with
 * params zeroes "gd_r" behind the next denoise call's staging, so a request starts APG's running difference at 0.  An unguided
 * fluxmi_engine_denoise call does not consult the state.  params_host == NULL switches it off; a prepare that re-allocates the workspace
 * does too.  A request without shaping allocates and launches exactly what it did before. */
int fluxmi_engine_set_guidance(fluxmi_engine_t* e, const float* params_host, int step_offset);
/* Progress, live previews and cancellation for the following fluxmi_engine_denoise / _denoise_cfg calls on the PREPARED
 * shape, until cleared.  hook(user, evaluation, n_evaluations, rgb, images, height, width) is called on the caller's thread once per model
 * evaluation of those calls, in order, AFTER the GPU has finished that evaluation: evaluation = eval_offset + the call's step index,
 * n_evaluations as given here (the whole request's, so a request cut into several denoise calls continues its numbering like
 * fluxmi_engine_set_solver_noise's eval_offset), rgb = uint8 [images][height = 2 h][width = 2 w][3] in an engine-owned pinned buffer that is
 * valid until the hook returns, or NULL at an evaluation without a preview.  images = the caller's images (the prepared batch, half of it
 * for a guided call).  h x w is the token grid of the stepped rows; proj51_host = the 51 floats of fluxmi_latent_preview.
 *   every > 0: fluxmi_latent_preview is launched in front of whatever update the evaluation has -- behind guidance shaping, in the calibrating
 *              steps, the eager warm step, the plain piece and both tails of a step-cached step alike -- and evaluation g has a preview iff
 *              g % every == 0.  Previewed versus not is a kind of step graph like guided versus plain; every, eval_offset and the factors
 *              are device data, so ONE graph serves every cadence and every slice of a request.
 *   every = 0: progress and cancellation only: nothing is allocated, captured or launched beyond events.
 *   hook = NULL clears the state (the other arguments are ignored); a prepare that re-allocates the workspace does too.  A request without
 *   the state allocates, captures and launches exactly what it did before.
 * Look-ahead: with a hook set the host loop stays at most FLUXMI_PREVIEW_DEPTH evaluations ahead of the GPU.  Before launching evaluation
 * i >= DEPTH it waits on the event recorded behind evaluation i - DEPTH and delivers every evaluation up to i - DEPTH not yet delivered; after
 * the last launch it waits for and delivers the rest.  A HOOKED DENOISE CALL IS THEREFORE SYNCHRONOUS: when it returns, every evaluation has
 * finished and been delivered (the copy of the latent back into img is still only enqueued on the caller's stream).  Delivery copies the slot
 * to the pinned buffer on a private stream and waits for that copy.  Since the delivery of evaluation k precedes the launch of k + DEPTH, at
 * most the previews of evaluations k + 1 .. k + DEPTH can be written while k's is unread: FLUXMI_PREVIEW_SLOTS = DEPTH + 1 slots suffice for
 * every cadence.  Device and pinned memory: SLOTS (pinned: 1) x images x 4 h w x 3 bytes, independent of the step count, counted in
 * fluxmi_engine_workspace_bytes.
 * Cancellation: a non-zero hook return stops the launches.  The engine waits for what was launched, copies the latent out as usual, updates
 * *trial_index_inout for the calibrating steps that ran, delivers nothing further and returns FLUXMI_CANCELLED; fluxmi_last_error names the evaluations run.
 * Cancelling at evaluation k of a call of n runs exactly min(n, k + DEPTH) of them (offsets aside).  There is no device-side abort.  The
 * engine is fully usable afterwards: the next request computes what it computes on a fresh engine.
 * Refused: on a ControlNet engine, under an attached amax-exchange hook (the host waits would stall a process group's collectives),
 * every < 0, eval_offset < 0, h * w != the prepared shape's stepped rows, a model whose C_out != 64.  The state speaks of the prepared batch:
 * the host wrapper refuses a batch that needs more than one engine pass.
 * fluxmi_engine_preview_stats is read-only, for tests: *captures = the graph captures the engine has made since it was created,
 * *evaluations_run = the evaluations the last denoise call launched (what a cancelled call ran; 0 after a call without a hook). */
#define FLUXMI_CANCELLED 3
typedef int (*fluxmi_step_hook_t)(void* user, int evaluation, int n_evaluations, const unsigned char* rgb /* NULL: no preview at this evaluation */,
                                  int images, int height, int width);
int fluxmi_engine_set_preview(fluxmi_engine_t* e, const float* proj51_host, int h, int w, int every, int eval_offset, int n_evaluations,
                              fluxmi_step_hook_t hook, void* user);
int fluxmi_engine_preview_stats(fluxmi_engine_t* e, long long* captures, int* evaluations_run);
/* Test hook: phases [phase_from, phase_to] of ONE frozen forward on the engine's own buffers, mode 1 (fused) or 2 (unfused, frozen scales):
 *   0 img_in + txt_in on the request buffers "img_s" / "txt_s" (mode 1: the cached "txt_emb" of the last denoise call) + this step's
 *     modulation vectors out of the step-ahead table the last denoise call left (step = the request's step index, written to the device-side
 *     step counter first; step < 0 keeps the counter)
 *   1 double block 0 | 2 every later block | 3 the final layer -> "pred_s".
 * The counterpart of fluxmi_engine_run_block for what that cannot reach; needs a finished fluxmi_engine_denoise call on this shape. */
int fluxmi_engine_run_phase(fluxmi_engine_t* e, int mode, int phase_from, int phase_to, int step, void* stream);

/* ---- FLUX ControlNet (diffusers' FluxControlNetModel) -----------------------------------------------------------------
 * A ControlNet is an engine of its own kind: a Flux trunk of desc->depth (= Nd >= 1) double and desc->depth_single (= Ns >= 0) single blocks
 * with its own embedders and NO final layer, plus the bf16 nn.Linear projections controlnet_x_embedder [hidden, in_channels] and one
 * [hidden, hidden] per block.  Layer order in `linears` (count = fluxmi_controlnet_num_linears(desc), host arithmetic only):
 *   the trunk's list (fluxmi_engine_create) WITHOUT its two final-layer entries, then
 *   controlnet_x_embedder, controlnet_blocks[0 .. Nd), controlnet_single_blocks[0 .. Ns)          -- all kind 0 (bf16), refused otherwise
 * norm_scales as for fluxmi_engine_create.  mode_table: bf16 [num_mode, hidden] = controlnet_mode_embedder.weight of a Union net, or NULL
 * (num_mode 0).  The handle is a fluxmi_engine_t: fluxmi_engine_set_tables, _rebind, _set_amax_exchange, _workspace_bytes, _get_buffer,
 * _copy_buffer and _destroy apply; it keeps its own workspace, step-ahead modulation table, quantising tables and row-pair weight copies.  It
 * is prepared and run only through fluxmi_engine_attach_controlnet: prepare / forward / denoise on the handle itself are refused. */
int fluxmi_controlnet_num_linears(const fluxmi_model_desc_t* desc);
int fluxmi_controlnet_create(const fluxmi_model_desc_t* desc, const fluxmi_linear_t* linears, int n_linears, const void* const* norm_scales,
                             int n_norm_scales, const void* mode_table, int num_mode, fluxmi_engine_t** out);
/* Attach `cn` to the main engine `e` for the following fluxmi_engine_forward / _denoise / _denoise_cfg calls on e's PREPARED shape (call it
 * after fluxmi_engine_prepare, like fluxmi_engine_set_inpaint); cn == NULL detaches, and so does a prepare that re-allocates e's workspace.
 * A detached engine launches exactly what it launched before this entry point existed.
 *   cond   device bf16 [batch, Li, in_channels]: the VAE-encoded, shifted, scaled and packed control image of the caller's `batch` images;
 *          batch = the prepared B, or B / 2 (a guided request: replicated to both halves).  The engine copies it: a captured graph never
 *          holds the caller's pointer.  controlnet_x_embedder(cond) is step-invariant and computed here, once per request
 *   mode   row of mode_table (a Union net: required, 0 <= mode < num_mode), -1 for a net without one (anything else is refused)
 *   scale  the conditioning scale: device data of the captured graph (any value, another scale replays the same graph)
 *   trial_index  the ControlNet's OWN calibration counter (its F8Linears' trial_index), read back with fluxmi_controlnet_trial
 * With a net attached every forward is
 *   ControlNet: x_img = bf16(img_in(img) + controlnet_x_embedder(cond)); x_txt = [mode_table[mode] ;] txt_in(txt) (the mode row's position
 *               id is txt_ids[:1], the net's text length Lt + 1); vec from its own embedders; after double block k: r_k = bf16(
 *               controlnet_blocks[k](x_img)), after single block k: r_(Nd + k) = bf16(controlnet_single_blocks[k](x_img rows))
 *   main:       after double block i  x_img = bf16(x_img + bf16(r_(i / ceil(depth / Nd)) * scale))          (fluxmi_add_scaled, one launch)
 *               after single block i  x_img rows = bf16(x_img + bf16(r_(Nd + i / ceil(depth_single / Ns)) * scale))
 * on the same img / txt / y / timestep buffers, and a denoise step is ControlNet forward, main forward, the update kernel the request
 * already had (plain, guided, blend): ONE captured graph per frozen step.  ControlNet on / off (and which net) is a kind of step graph like
 * guided or masked.  Calibration: a step is graph-replayed only when BOTH nets are frozen; while either has trials left the steps run
 * eagerly, that net in mode 0 and the other in its frozen mode.  fluxmi_engine_forward's mode / trial_index speak of the main model; the
 * ControlNet runs mode 0 while its own counter has trials left (and advances it), else fused when the main runs fused, else unfused-frozen.
 * Refused (fluxmi_last_error says which): hidden / heads / in_channels differ from e's; e predicts fewer channels than it reads (Fill, Depth /
 * Canny [dev]); Kontext reference rows (Lc > 0); a token-group attention table; step caching on (also refused by the denoise call if it is
 * switched on afterwards); a mode out of range, missing for a Union net or given to a net without a table; a net with a guidance embedder on a main model without
 * one; a net attached elsewhere.  fluxmi_engine_run_phase is refused while a net is attached.  A captured step is keyed on a process-wide unique
 * generation number of the net's workspace and weight binding, not on its address: a net created where a destroyed one lived re-captures. */
int fluxmi_engine_attach_controlnet(fluxmi_engine_t* e, fluxmi_engine_t* cn, const void* cond, int batch, int mode, float scale, int trial_index,
                                    void* stream);
int fluxmi_controlnet_trial(fluxmi_engine_t* cn, int* trial_index);

/* ---- IP-Adapter: decoupled image attention (XLabs IPDoubleStreamBlockProcessor, restated) -------------------------------
 * For every sample b < B, image row r < rows and head h < heads (head_dim 128 only):
 *   qn   = QKNorm of the raw query  qkv[b * qkv_bstride + r * ld_qkv + h * 128 + d]  with the learnable scale qn_scale (bf16 [128]): formed by
 *          the helper fluxmi_attention_rawq uses (csrc/attention_common.h, qknorm_rinv / qknorm_apply: fp32 rms over the 128 columns, eps 1e-6,
 *          bf16((x / rms) * w)), BEFORE RoPE -- attention and the adapter see the same query bits
 *   t_j  = (qn . k_ip[b, j, h]) * (128^-1/2 * log2 e),  j < Nk      fp32 products and sums
 *   p_j  = exp2(t_j - max_j t_j),  acc_d = sum_j p_j * v_ip[b, j, h, d],  o_d = bf16(acc_d * (1 / sum_j p_j))      all fp32, one rounding
 * scale == NULL (out-of-place):  out[b * o_bstride + r * ld_o + h * 128 + d] = o_d
 * scale != NULL (fused):         x = bf16(x + bf16(o_d * scale[b * scale_bstride]))  at the same address of `out` (the residual stream): bit
 *                                for bit the out-of-place form followed by fluxmi_add_scaled.  scale is DEVICE fp32, one value per sample.
 * k_ip, v_ip: bf16, row j of sample b at b * kv_bstride + j * heads * 128; rows at or beyond Nk are never read.  1 <= Nk <= 64.  Strides in
 * elements, multiples of 8, every pointer 16-byte aligned.  A sample's result depends on its own rows only; nothing outside the addressed
 * [rows, heads * 128] window of each sample is written.  VALU kernel, no MFMA: it is bound by the bytes of q and x. */
int fluxmi_ip_attention(const void* qkv, long long ld_qkv, long long qkv_bstride, const void* qn_scale, const void* k_ip, const void* v_ip,
                        long long kv_bstride, void* out, long long ld_o, long long o_bstride, const float* scale, long long scale_bstride, int B,
                        int rows, int heads, int Nk, void* stream);
/* The adapter of the following fluxmi_engine_forward / _denoise / _denoise_cfg calls on the PREPARED shape (call it after fluxmi_engine_prepare*):
 *   k_ip, v_ip   device bf16 [depth][batch][Nk][hidden]: the step-invariant keys / values of every double block (computed once per request by
 *                the caller).  Copied into an engine-owned buffer allocated here -- never inside a capture -- so a captured graph never holds
 *                the caller's pointers; counted in fluxmi_engine_workspace_bytes; re-used while it is large enough
 *   batch        must equal the prepared batch: both branches of a guided request carry their own K / V and scales
 *   scales_host  [batch][depth] floats (ip_scale per sample and block), staged as device data: one captured graph serves every scale
 * With an adapter set, every forward launches fluxmi_ip_attention (fused form) once behind each double block, on all L - Lt image-stream
 * rows (Kontext reference rows included), reading the block's raw image q that still sits in the qkv workspace; with a ControlNet attached
 * the order is block, adapter term, ControlNet residual.  Calibrating, unfused, frozen and graph-replayed steps alike.  Adapter on / off is a
 * kind of step graph (Nk and the buffer are baked in: another Nk or a re-allocated buffer re-captures; other K / V contents or scales
 * replay the same graph).  k_ip == NULL switches it off (the other arguments are ignored); so does a prepare that re-allocates the workspace.
 * A request without an adapter allocates and launches exactly what it did before.  Refused: Nk outside 1..64, batch != the prepared one,
 * a token-group attention table, step caching on (both also by the forward / denoise call if set afterwards), a ControlNet engine as the
 * target; fluxmi_engine_run_phase is refused while an adapter is set. */
int fluxmi_engine_set_ip_adapter(fluxmi_engine_t* e, const void* k_ip, const void* v_ip, int Nk, int batch, const float* scales_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLUXMI_H */
