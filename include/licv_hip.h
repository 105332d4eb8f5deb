/*
 * licv_hip.h — C-ABI of liblicv_hip.so: the MI355X (gfx950) kernels of the L-ICV hot path.
 *
 * Boundary: the reference is pure Python; its FFI for this path would be a
 * ctypes binding.  Each entry point below names the reference/HF interface whose arithmetic it
 * replaces (ref: = ForJadeForest/LICV-VQA, hf: = transformers/models).  Conventions:
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted;
 *   - the caller owns all buffers; the library allocates nothing and never synchronises;
 *   - every launch goes on the `stream` argument (a hipStream_t passed as void*);
 *   - return 0 on success, a negative LICV_E_* otherwise; licv_last_error() gives the text
 *     (thread-local, host pointer);
 *   - dtype arguments use the LICV_* enums; leading dimensions (`ld*`) are in ELEMENTS.
 */
#ifndef LICV_HIP_H
#define LICV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point is added, removed or changes its arguments; licv/_lib.py holds the same constant and refuses a
 * library that answers anything else.  1 = round 1; 2 = rounds 2-3 (fp8, split-K slices, runner, front-end, backward, image input);
 * 3-6 = round 4 (lab library split off; weight-streaming GEMM; beam scoring; decode-step fusion; backward options; RMSNorm backward
 * on split-K slices; the gradient all-reduce); 7 = sampled decoding (licv_sample_step, licv_beam_sample_step); 8 = RICE retrieval
 * (licv_topk_ip, licv_l2_normalize_rows, licv_quick_gelu); 9 = image resize on the device (licv_resize_images); still 9 with
 * the CLIP text tower's kernels (licv_clip_text_embed, licv_attn_varlen_causal, licv_layernorm_rows_fwd): they only ADD symbols - no
 * existing entry point changed, so a binding written against 9 keeps working (check_exports still asks for every declared symbol); and still 9 with
 * constrained decoding: licv_logits_process is a new symbol, and licv_beam_step accepts one new VALUE of an existing field
 * (logits_dtype = LICV_F32_LOGPROBS) that no earlier caller passes - no struct changed its layout; and still 9 with candidate ranking:
 * licv_append_attn is a new symbol with a struct of its own; and still 9 with decode steps over long histories:
 * licv_decode_attn_split_plan and licv_decode_attn_split are new symbols that take licv_decode_attn_args as it is; and still 9 with
 * the text stack on packed rows: licv_attn_fwd_ragged and licv_idefics_text_forward_packed are new symbols that take licv_attn_args and
 * licv_idefics_text_call as they are. */
#define LICV_ABI_VERSION 9

enum { LICV_BF16 = 0, LICV_F32 = 1 };
/* A value of licv_beam_step_args.logits_dtype ONLY: fp32 rows that are final log-probabilities.  licv_beam_step is the one entry
 * that accepts it; every other entry that takes a dtype (licv_beam_sample_step, licv_sample_step, licv_logits_process, ...) checks
 * for LICV_BF16 / LICV_F32 and answers LICV_E_BADARG.  A new entry that takes a dtype must do the same. */
enum { LICV_F32_LOGPROBS = 2 };
enum { LICV_OK = 0, LICV_E_BADARG = -1, LICV_E_UNSUPPORTED = -2, LICV_E_HIP = -3 };

int         licv_version(void);
const char* licv_last_error(void);

/* The one collective of the path (replaces the gradient all-reduce Lightning DDP / DeepSpeed ZeRO-2 run for the
 * reference, ref:config/trainer/ddp.yaml:5, ref:config/trainer/zero2.yaml:5): in-place sum (average != 0: mean) of n fp32 values - the
 * gradients of icv and alpha, 131 k floats - over the ranks of `nccl_comm`, an ncclComm_t of the RCCL ALREADY loaded and initialised in
 * the calling process, enqueued on `stream`.  The library opens no communicator and does not link RCCL: ncclAllReduce is looked up
 * (dlsym) at the first call; LICV_E_UNSUPPORTED when the process has no RCCL.  (The Python host keeps torch.distributed.all_reduce,
 * which owns its communicator: licv/trainer.py.) */
int licv_allreduce_small(void* nccl_comm, float* data, int64_t n, int average, void* stream);

/* ---- the hook: ref:icv_src/icv_model/icv_intervention.py:61-86 (intervention_function) ----
 * out[r,:] = (h[r,:]+v) / ||h[r,:]+v|| * ||h[r,:]||, fp32 maths, fp32 output (torch promotion of a
 * bf16/fp32 stream with the fp32 ICV).  v = alpha*icv[layer] when `alpha` != NULL (folds
 * ref:icv_src/icv_module.py:89-92), else v = icv_row as given.  `alpha` is a device pointer to one float.
 * If norm_w != NULL the RMSNorm that consumes the edited stream next (hf:idefics/modeling_idefics.py:342-350)
 * is fused: xn_out (bf16) = w * bf16(out * rsqrt(mean(out^2)+eps)).  out may alias h when h is fp32. */
int licv_inject_renorm_fwd(const void* h, int h_dtype, const float* icv_row, const float* alpha,
                           float* out, int64_t rows, int64_t hidden,
                           const void* norm_w, void* xn_out, float norm_eps, void* stream);

/* Idefics2 hook site = a residual BRANCH (`layers.N.mlp`, ref:config/lmm/idefics2-8B-base.yaml:8): the edit is applied to the
 * branch output and the stream becomes  out = residual + edit(branch)  (fp32).  norm_flavour selects the RMSNorm fused
 * on `out` (0 Idefics, 1 Mistral: single rounding on an fp32 stream). */
int licv_inject_renorm_add_fwd(const void* branch, int branch_dtype, const float* icv_row, const float* alpha,
                               const void* residual, int residual_dtype, float* out, int64_t rows, int64_t hidden,
                               const void* norm_w, void* xn_out, float norm_eps, int norm_flavour, void* stream);

/* The layer-output hook with the layer's LAST RESIDUAL ADD folded in (hf:idefics/modeling_idefics.py:760-763, `hidden_states =
 * residual + hidden_states` at the end of IdeficsDecoderLayer.forward, then ref:icv_src/icv_model/icv_intervention.py:62-84 on that
 * output): the tensor edited is h + branch in the stream's dtype (a bf16 stream rounds the sum to bf16, an fp32 stream adds in
 * fp32 — bit for bit what the down projection's residual epilogue wrote), so the down projection can leave its bf16 branch
 * through the register-direct GEMM epilogue.  Otherwise as licv_inject_renorm_fwd. */
int licv_inject_renorm_pre_fwd(const void* h, int h_dtype, const void* branch_bf16, const float* icv_row, const float* alpha,
                               float* out, int64_t rows, int64_t hidden,
                               const void* norm_w, void* xn_out, float norm_eps, void* stream);

/* backward of the hook for training (gradients reach icv and alpha only through here;
 * ref:icv_src/icv_module.py:97-98 runs the student pass with grad).  grad_h may be NULL.
 * grad_v_partial: (n_partials, hidden) fp32 workspace, fully overwritten; the caller sums over
 * dim 0.  n_partials = licv_inject_bwd_partials(rows). */
int64_t licv_inject_bwd_partials(int64_t rows);
int licv_inject_renorm_bwd(const void* h, int h_dtype, const float* icv_row, const float* alpha,
                           const float* grad_out, float* grad_h, float* grad_v_partial,
                           int64_t rows, int64_t hidden, void* stream);

/* ---- norms ----
 * Row r of the (rows x dim) problem lives at  x + (r / inner)*ld_outer + (r % inner)*dim  (same for out
 * with its own ld); inner=1, ld=dim is the dense case, inner=n_heads covers per-head q/k norms.
 * RMSNorm flavours: 0 = Idefics (hf:idefics/modeling_idefics.py:342-350: cast to bf16 THEN * weight),
 *                   1 = Mistral (hf:mistral/modeling_mistral.py:182-199: weight * cast-back).          */
int licv_rmsnorm_fwd(const void* x, int x_dtype, const void* w_bf16, void* out_bf16,
                     int64_t rows, int64_t dim, int64_t inner, int64_t ld_x, int64_t ld_out,
                     float eps, int flavour, void* stream);
/* h += branch in place (the stream's dtype: bf16 rounds the sum; hf:idefics/modeling_idefics.py:741-743, the residual add after
 * self-attention), then out_bf16 = RMSNorm(h) (the post-attention norm, :745): the o-projection's residual epilogue folded into the
 * norm that follows it.  Dense rows (ld = dim).  row_gate (rows fp32, may be NULL) and use_scale / scale reproduce the gated
 * cross-attention layer's epilogue (:789-791, :799-800): branch row -> 0 where the gate is 0, then bf16(scale * branch). */
int licv_add_rmsnorm_fwd(void* h, int h_dtype, const void* branch_bf16, const float* row_gate, int use_scale, float scale,
                         const void* w_bf16, void* out_bf16, int64_t rows, int64_t dim, float eps, int flavour, void* stream);
/* nn.LayerNorm on a bf16 tensor (hf:idefics/vision.py:286-299, perceiver.py:140-141,155-156): fp32
 * statistics, one rounding.  Input rows addressed as for RMSNorm; output row r goes to
 *   out + (r / inner)*ld_out + (r % inner)*dim + (out_group > 0 ? (r / out_group)*out_group_extra : 0)
 * which lets LN(context) and LN(latents) land directly inside the perceiver's concatenated K/V input. */
int licv_layernorm_fwd(const void* x_bf16, const void* w_bf16, const void* b_bf16, void* out_bf16,
                       int64_t rows, int64_t dim, int64_t inner, int64_t ld_x, int64_t ld_out,
                       int64_t out_group, int64_t out_group_extra, float eps, void* stream);

/* ---- rotary: hf:idefics/modeling_idefics.py:396-428 (rotate_half form, gathered by position_ids) ----
 * In place on `n_tensors` (1 or 2: q and k) head-major slices of a (rows x ld) bf16 buffer:
 * tensor t, head h, row r at x + r*ld + t*tensor_stride + h*head_dim.  cos/sin: (n_pos, head_dim) bf16. */
int licv_rotary_fwd(void* x_bf16, const void* cos_bf16, const void* sin_bf16, const int64_t* position_ids,
                    int64_t rows, int64_t n_heads, int64_t head_dim, int64_t ld, int64_t tensor_stride,
                    int n_tensors, int64_t n_pos, void* stream);
/* rotary + KV-cache append of one fused QKV projection in one launch (hooked generate, ref:inference.py:300-321 -> HF generate's
 * past_key_values): qkv is (batch * S, 3H) bf16; Q heads are rotated in place, the rotated K heads and V go to
 * cache[b, past + s, 0:H | H:2H] (cache: (batch, cache_max_len, 2H) bf16).  Same arithmetic as licv_rotary_fwd. */
int licv_rotary_kv_append(void* qkv_bf16, const void* cos_bf16, const void* sin_bf16, const int64_t* position_ids, int64_t batch, int64_t S,
                          int64_t n_heads, int64_t head_dim, int64_t n_pos, void* cache_bf16, int64_t cache_max_len, int64_t past, void* stream);

/* ---- dense layers: nn.Linear on MFMA (every F.linear under hf:idefics/ and hf:idefics2/) ----
 * C[M,N] = epilogue( A[M,K] (bf16, lda) x W[N,K]^T (bf16, ldw) ), fp32 accumulation.
 * Epilogue, in this order (each step rounds to bf16 as the unfused torch ops would):
 *   y = bf16(acc + bias[n])                      bias_bf16 may be NULL
 *   y = bf16(act(y))                             act: 0 none, 1 GELU(erf), 2 GELU(tanh), 3 ReLU
 *   swiglu != 0: columns come in (gate,up) 16-wide interleaved pairs (weights packed by
 *                licv_pack_gate_up) and y = bf16(bf16(silu(g)) * u); the output has N/2 columns
 *   row_gate (fp32 per row) != NULL: y = 0 where row_gate[m] == 0     (cross_attention_gate)
 *   scale != 0 flag `use_scale`: y = bf16(scale * y)                   (tanh(alpha) gates)
 *   residual != NULL: out = residual[m,n] + y   in the residual dtype (bf16 or fp32 stream)
 *   store to C as out_dtype (bf16 or fp32).  C may alias residual.
 * Requirements: K % 8 == 0, lda/ldw % 8 == 0, ldc % 4 == 0, 16-byte aligned base pointers. */
typedef struct {
    const void* bias_bf16;
    const float* row_gate;
    const void* residual;
    int   residual_dtype;
    int64_t ld_res;
    int   act;
    int   swiglu;
    int   use_scale;
    float scale;
    int   out_dtype;
} licv_gemm_epilogue;

int licv_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, const licv_gemm_epilogue* ep, void* stream);
/* Skinny GEMMs (M <= 256: student pass, decode steps): K is cut into `splits` ranges, each workgroup writes its fp32 partial tile
 * to its own slice of a caller-provided workspace (no atomics: bit-reproducible), a second kernel sums the slices in order and
 * applies the epilogue.  licv_gemm_splitk_plan returns splits <= 1 when the plain kernel should be used. */
int licv_gemm_splitk_plan(int64_t M, int64_t N, int64_t K, int* splits, int64_t* workspace_bytes);
/* workspace bytes licv_gemm_bf16_splitk wants for (M, N, K); 0 = the one-pass kernels serve the shape; < 0 = bad arguments.
 * (SURVEY.md §8b "licv_workspace_size": the library allocates no device memory — every buffer, this one included, is the caller's.) */
int64_t licv_workspace_size(int64_t M, int64_t N, int64_t K);
int licv_gemm_bf16_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, const licv_gemm_epilogue* e, int splits,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* The producer half alone, for a plain epilogue whose consumer is a row kernel (decode steps and the 32-token student pass of
 * ref:inference.py:300-321 / ref:icv_src/icv_module.py:97-98, where a launch costs as much as the kernel): `splits` fp32 slices of
 * A W^T are left in the workspace — slice sp of row m at workspace + sp * slice_elems + m * row_stride (floats) — and the consumer
 * (licv_add_rmsnorm_fwd_ws, licv_inject_renorm_pre_fwd_ws, licv_rotary_kv_append_ws) sums them in slice order and rounds to bf16
 * itself: bit for bit the finalize kernel's output, one launch less per projection. */
int licv_gemm_bf16_splitk_produce(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K, int splits,
                                  void* workspace, int64_t workspace_bytes, int64_t* slice_elems, int64_t* row_stride, void* stream);
/* licv_add_rmsnorm_fwd / licv_inject_renorm_pre_fwd / licv_rotary_kv_append with the bf16 operand (branch, branch, qkv) replaced by
 * the split-K slices it would have been finalized from.  Bit-identical to finalize + the plain entry point (same per-lane sums).
 * licv_rotary_kv_append_ws writes the rotated Q rows into qkv_bf16[:, 0:H] (the attention kernel's Q operand) and nothing else there. */
int licv_add_rmsnorm_fwd_ws(void* h, int h_dtype, const float* ws, int splits, int64_t slice_elems, int64_t row_stride,
                            const float* row_gate, int use_scale, float scale, const void* w_bf16, void* out_bf16,
                            int64_t rows, int64_t dim, float eps, int flavour, void* stream);
int licv_inject_renorm_pre_fwd_ws(const void* h, int h_dtype, const float* ws, int splits, int64_t slice_elems, int64_t row_stride,
                                  const float* icv_row, const float* alpha, float* out, int64_t rows, int64_t hidden,
                                  const void* norm_w, void* xn_out, float norm_eps, void* stream);
int licv_rotary_kv_append_ws(const float* ws, int splits, int64_t slice_elems, int64_t row_stride, void* qkv_bf16,
                             const void* cos_bf16, const void* sin_bf16, const int64_t* position_ids, int64_t batch, int64_t S,
                             int64_t n_heads, int64_t head_dim, int64_t n_pos, void* cache_bf16, int64_t cache_max_len, int64_t past, void* stream);

/* ---- fp8 path (BASELINE configs[4]: "fp8 weights on CDNA4 MFMA"; no reference counterpart — parity bar in DESIGN.md) ----
 * q[r,k] = e4m3(x[r,k] / scale[r]), scale[r] = amax(x[r,:]) / 448 (OCP e4m3fn, round to nearest even).  Weights are quantised
 * once with the same kernel (rows = output channels); activations per call. */
int licv_quantize_rows_fp8(const void* x, int x_dtype, void* q_fp8, float* scale, int64_t rows, int64_t dim,
                           int64_t ld_x, int64_t ld_q, void* stream);
/* The row kernels that feed an fp8 GEMM write the fp8 image of their rows themselves (exactly licv_quantize_rows_fp8 of the bf16
 * rows they produce: e4m3 bytes (rows, dim) + one fp32 scale per row) - `out_bf16` may be NULL when nothing else reads the rows.
 * Rows are contiguous (ld = dim).  rmsnorm: as licv_rmsnorm_fwd; add_rmsnorm: as licv_add_rmsnorm_fwd without gate / scale;
 * inject_renorm_add: as licv_inject_renorm_add_fwd (xn_bf16 may be NULL); layernorm: as licv_layernorm_fwd, dim % 8 == 0. */
int licv_rmsnorm_fwd_q8(const void* x, int x_dtype, const void* w_bf16, void* out_bf16, void* q_fp8, float* q_scale, int64_t rows, int64_t dim,
                        float eps, int flavour, void* stream);
int licv_add_rmsnorm_fwd_q8(void* h, int h_dtype, const void* branch_bf16, const void* w_bf16, void* out_bf16, void* q_fp8, float* q_scale,
                            int64_t rows, int64_t dim, float eps, int flavour, void* stream);
int licv_inject_renorm_add_fwd_q8(const void* branch, int branch_dtype, const float* icv_row, const float* alpha,
                                  const void* residual, int residual_dtype, float* out_f32, int64_t rows, int64_t hidden,
                                  const void* norm_w_bf16, void* xn_bf16, void* q_fp8, float* q_scale, float norm_eps, int norm_flavour, void* stream);
int licv_layernorm_fwd_q8(const void* x_bf16, const void* w_bf16, const void* b_bf16, void* out_bf16, void* q_fp8, float* q_scale,
                          int64_t rows, int64_t dim, float eps, void* stream);
/* C = epilogue( (Aq . Wq^T) * a_scale[m] * w_scale[n] ), fp32 accumulate on v_mfma_f32_16x16x32_fp8_fp8; same epilogue
 * struct as licv_gemm_bf16.  Aq (M, K) and Wq (N, K) e4m3 bytes, K >= 256, K % 64 == 0, leading dims in bytes. */
int licv_gemm_fp8(const void* Aq, int64_t lda, const float* a_scale, const void* Wq, int64_t ldw, const float* w_scale,
                  void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const licv_gemm_epilogue* e, void* stream);

/* Kernel selection override for tests and A/B timing (process-wide).  0 = automatic: for M >= 512, N >= 256, K % 64 == 0 the
 * persistent "flow" kernel (register-direct asynchronous epilogue) where the epilogue allows it — plain / bias / activation /
 * SwiGLU / bias + bf16 residual, bf16 out, N % 64 == 0 — else the lean ping-pong kernel with the staged epilogue; the general
 * 128 x 128 kernel for everything smaller (M <= 32 with long K: licv_gemm_splitk).  1 = always the 128 x 128 kernel; 2 the round-1
 * single-barrier 256 x 256 kernel; 6 the round-1 ping-pong kernel; 8 persistent ping-pong; 20 flow wherever eligible; 21 pair kernel
 * (two K stages per phase); 22 lean ping-pong everywhere (23-27: its ordering / diagnostic builds); 30-37 four-wave kernel and its
 * timing builds; 40-42 four-wave kernel on 64-deep K tiles; 50 two workgroups per CU on 128 x 256 tiles; 60 the four-wave flow64 kernel
 * wherever eligible; 70 the 128-tile mid kernel at any M; 71 the 256 x 128 tall kernel wherever it can run (129-256 rows).  All full-result variants are
 * bit-identical (tests/test_ops_gpu.py).  Values that name a kernel of the lab library (2-8, 10-13, 21, 30-37, 50: csrc/lab/, built
 * into liblicv_hip_lab.so for tests and tools only) make licv_gemm_bf16 return LICV_E_UNSUPPORTED unless that library is loaded. */
int licv_gemm_select(int which);
/* Called by liblicv_hip_lab.so when it is loaded: registers the experiments' launcher / knob / timestamp entry points (or NULLs). */
int licv_lab_register(void* launch, void* knob, void* timestamps);
/* Knobs: 0 per-XCD start stagger of the round-1 ping-pong kernel in percent (off); 1 tile-rows per XCD patch (0 = heuristic);
 * 2 = 0: never take the flow kernel in auto mode; 4 = 0: licv_gemm_splitk_plan always answers "one pass" (split-K off for every
 * caller, the native layer runner included: the batch-independence tests compare bit for bit); 5 forced split-K count of the 128-tile
 * route (0 = the plan's choice); 6 fewest 256-tiles for the 256-tile kernels; 7 in-launch reduction of the skinny kernel; 8 = 0: fp8 GEMMs off the
 * 128-deep MFMA; 9 timing-only ablation of the mid kernel (wrong results); 10 = 4: four K tiles in flight in the mid kernel; 11 non-temporal
 * weight loads (bit 0 mid, bit 1 skinny); 12 = 0: wide outputs at 129-256 rows stay on the mid kernel instead of the tall kernel.  A/B timing
 * and tests only: every setting gives the same results except knob 9. */
int licv_gemm_experiment(int knob, int value);
/* 1 if the flow kernel may be dispatched (its code objects use no scratch memory: its counted waits rely on that), else 0 */
int licv_gemm_flow_available(void);
/* timing instrumentation: when non-NULL, wave 0 of every workgroup of the default kernel stores 5 wall_clock64() stamps
 * (start, pipeline filled, main loop done, output image in LDS, end) at dev_buffer[8 * blockIdx.x ...] (int64) */
int licv_gemm_debug_timestamps(void* dev_buffer);
/* (2I x K) gate/up weights -> the 16-row interleaved layout the swiglu epilogue expects. */
int licv_pack_gate_up(const void* gate_bf16, const void* up_bf16, void* packed_bf16,
                      int64_t inter, int64_t K, void* stream);

/* ---- attention (hf eager_attention_forward, hf:idefics/modeling_idefics.py:450-470; perceiver
 * hf:idefics/perceiver.py:150-166) as a tiled online-softmax kernel ----
 * Q: (B, Sq, n_heads, hd) at q + b*q_bs + s*q_rs + h*hd;  K,V likewise with (kv_bs, kv_rs) and
 * n_kv_heads (GQA: head h reads kv head h / (n_heads/n_kv_heads)).  O: (B, Sq, n_heads*hd) dense bf16.
 * mask_mode: 0 none; 1 causal with q offset (Sk - Sq) AND key_valid[b,key] != 0 (int32, may be NULL);
 *            2 key_valid only (bidirectional key-padding mask);
 *            3 image mask: allowed iff img_mask[b, q, key / img_len] != 0 (int32 (B,Sq,n_img)).
 * Rows with no allowed key produce zeros. */
typedef struct {
    const void* q; int64_t q_bs, q_rs;
    const void* k; const void* v; int64_t kv_bs, kv_rs;
    void* o;
    int64_t B, Sq, Sk, n_heads, n_kv_heads, head_dim;
    float scale;
    int   mask_mode;
    const int32_t* key_valid;
    const int32_t* img_mask; int64_t n_img, img_len;
} licv_attn_args;

int licv_attn_fwd(const licv_attn_args* a, void* stream);
/* The same tiled kernel on PACKED rows, for right-padded batches whose padding rows are left out (mask modes 1 and 3 only): sequence b
 * is rows cu_seqlens[b] .. cu_seqlens[b+1]-1 of Q and O (row strides q_rs and n_heads*hd; q_bs and Sq are ignored).  Mode 1: K and V
 * are packed the same way (kv_rs; kv_bs and Sk ignored), every sequence is causal on its own rows (Sk_b = Sq_b), key_valid is ignored:
 * under right padding a real query never sees a padding key.  Mode 3: K and V stay (B, Sk) per batch row (kv_bs, kv_rs), img_mask is
 * packed (total, n_img).  Key tiles and query blocks keep their boundaries relative to the sequence start, so every real row gets the
 * bits licv_attn_fwd gives it in the padded batch; rows past cu_seqlens[B] are not touched.  cu_seqlens: B + 1 int32, [0] = 0,
 * ascending in steps >= 1, given twice as licv_attn_varlen_causal takes it (HOST pointer for the checks and the grid, device copy for
 * the kernel, complete on `stream` before the call; a workgroup whose device offsets leave the packed rows does nothing).  A missing
 * copy, cu_seqlens not ascending from 0, a length of 0 or another mask mode: LICV_E_BADARG, nothing launched. */
int licv_attn_fwd_ragged(const licv_attn_args* a, const int32_t* cu_seqlens_host, const int32_t* cu_seqlens_dev, void* stream);
/* tests / A-B timing: bit 0 = always the tiled kernel (never the resident-K/V variant used for short unmasked keys);
 * bit 1 = the resident variant walks its items in blockIdx order instead of grouping consecutive heads on one XCD;
 * bit 2 = the resident variant leaves its LDS read schedule to the compiler; bit 3 = so does the tiled kernel at head dim 128 */
int licv_attn_select(int mode);

/* ---- small data-movement kernels ---- */
/* hf:idefics/modeling_idefics.py:230-267 IdeficsDecoupledEmbedding (ids >= vocab -> additional table) */
int licv_embed_gather(const int64_t* ids, const void* table_bf16, const void* extra_bf16, void* out_bf16,
                      int64_t n_tokens, int64_t dim, int64_t vocab, int64_t n_extra, void* stream);
/* Conv2d(k=s=patch, no padding) as im2col: pixels (n_img,3,H,W) bf16 -> (n_img*gh*gw, ld_out) with the
 * first 3*patch*patch columns filled (channel-major, as conv weight.flatten(1)) and the rest zeroed. */
int licv_im2col_patches(const void* pix_bf16, void* out_bf16, int64_t n_img, int64_t height, int64_t width,
                        int64_t patch, int64_t ld_out, void* stream);
/* hf:idefics/vision.py:152-166 + pre_layrnorm :369: x = cat(cls, patches) + pos; emb_out = x (optional),
 * ln_out = LayerNorm(x).  patches: (n_img*n_patch, dim) bf16. */
int licv_vit_embed_ln(const void* patches_bf16, const void* cls_bf16, const void* pos_bf16,
                      const void* ln_w, const void* ln_b, void* out_bf16,
                      int64_t n_img, int64_t n_patch, int64_t dim, float eps, void* stream);
/* out[r, :] = src[r % period, :]  (latents.repeat, hf:idefics/perceiver.py:96) */
int licv_tile_rows(const void* src_bf16, void* out_bf16, int64_t rows, int64_t dim, int64_t period, void* stream);
/* out[idx[i], :] = src[i, :] (hf:idefics2/modeling_idefics2.py:789-815 inputs_merger) */
int licv_scatter_rows(const void* src_bf16, const int64_t* idx, void* out_bf16, int64_t n, int64_t dim, void* stream);
/* silu(g)*u for an un-fused (M, 2I) [gate | up] buffer (kept for tests / odd shapes). */
int licv_swiglu(const void* gu_bf16, void* out_bf16, int64_t rows, int64_t inter, void* stream);

/* ---- backward of the student pass (ref:icv_src/icv_module.py:97-98: hooked forward WITH grad; the LMM is frozen, so
 * only d loss / d hidden-state is propagated; dense-layer input grads reuse licv_gemm_bf16 on transposed weights) ---- */
/* RMSNorm backward: dx (+)= rs*(g - xhat*mean(g*xhat)); rows addressed as forward.  g = bf16(dy*w) wherever the forward multiplied
 * the weight into bf16 rows (flavour 0 = Idefics, hf:idefics/modeling_idefics.py:342-350: always; flavour 1 = Mistral,
 * hf:mistral/modeling_mistral.py:182-199: only on a bf16 stream - on the fp32 stream behind a hook the product and its gradient are
 * fp32, g = dy*w unrounded) */
int licv_rmsnorm_bwd(const void* x, int x_dtype, const void* w_bf16, const void* dy, int dy_dtype, void* dx, int dx_dtype,
                     int64_t rows, int64_t dim, int64_t inner, int64_t ld_x, int64_t ld_dy, int64_t ld_dx, float eps,
                     int accumulate, int flavour, void* stream);
/* The same with dy still in the fp32 split-K slices of the dgrad GEMM that produced it (licv_gemm_bf16_splitk_produce): dy[r, i] =
 * bf16(sum over the slices, in slice order) - bit for bit what the finalize launch writes and licv_rmsnorm_bwd reads back; rows of
 * >= 1024 elements, dy / x / dx dense (leading dimension = dim). */
int licv_rmsnorm_bwd_ws(const void* x, int x_dtype, const void* w_bf16, const float* ws, int splits, int64_t slice_elems,
                        int64_t row_stride, void* dx, int dx_dtype, int64_t rows, int64_t dim, float eps, int accumulate,
                        int flavour, void* stream);
/* SwiGLU backward on the unfused (rows, 2I) [gate | up] buffer */
int licv_swiglu_bwd(const void* gu_bf16, const void* dact_bf16, void* dgu_bf16, int64_t rows, int64_t inter, void* stream);
/* grad entering a residual branch: out = bf16(bf16(dh)*scale), rows with row_gate == 0 zeroed (row_gate may be NULL) */
int licv_branch_grad(const float* dh, void* out_bf16, int64_t rows, int64_t dim, float scale, int use_scale,
                     const float* row_gate, void* stream);
/* attention backward for short sequences (Sq*Sk <= 16384), same argument struct as the forward; dk/dv may be NULL;
 * dK/dV are written per QUERY head (n_heads*head_dim columns): with GQA reduce them with licv_head_group_sum */
int licv_attn_bwd_small(const licv_attn_args* a, const void* dout_bf16, void* dq_bf16, int64_t dq_bs, int64_t dq_rs,
                        void* dk_bf16, void* dv_bf16, int64_t dkv_bs, int64_t dkv_rs, void* stream);
/* A/B timing and tests of the backward kernels (results are bit-identical either way).  option 0 = 0: licv_attn_bwd_small keeps the
 * head's Q / K / V / dO rows in global memory (default 1: staged in LDS where they fit beside P and dS, 1024 lanes per (batch, head);
 * 2: staged on 256 lanes, timing only); option 1 = 0: licv_rmsnorm_bwd
 * on one wave per row at every row length (default 1: four waves per row from 1024 elements on). */
int licv_backward_option(int option, int value);
/* cross-entropy rows (the "hard" loss, ref:icv_src/icv_module.py:94-95,111-117; HF ForCausalLMLoss upcasts to fp32):
 * loss_rows[i] = logsumexp(logits[rows[i], :]) - logits[rows[i], labels[i]]  (may be NULL);
 * grad[(grad_rows ? grad_rows[i] : i), :] (+)= grad_coef * (softmax - onehot), bf16 (may be NULL). */
int licv_ce_rows(const void* logits, int dtype, const int64_t* rows, const int64_t* labels, int64_t n_rows, int64_t vocab,
                 int64_t ld, float* loss_rows, float grad_coef, const float* grad_coef_dev, void* grad_bf16, int64_t ld_grad,
                 const int64_t* grad_rows, int accumulate, void* stream);
/* backward of repeat_kv (GQA): out[r, g*hd + d] = sum over the `rep` query heads of group g of src[r, (g*rep+j)*hd + d] */
int licv_head_group_sum(const void* src_bf16, void* out_bf16, int64_t rows, int64_t n_groups, int64_t rep, int64_t head_dim,
                        int64_t ld_src, int64_t ld_out, void* stream);
/* d loss / d student logits for the masked-KL rows: (n_rows, ld_grad >= vocab) bf16, scaled by upstream * T^2 / n_rows
 * (times *upstream_dev when that device pointer is given: the autograd path's incoming gradient, read without a host sync;
 * licv_ce_rows' grad_coef_dev works the same way). */
int licv_kl_rows_bwd(const void* stu_logits, const void* tea_logits, int dtype, const int64_t* stu_rows, const int64_t* tea_rows,
                     int64_t n_rows, int64_t vocab, int64_t ld_stu, int64_t ld_tea, float temperature, float eps, float upstream,
                     const float* upstream_dev, void* grad_rows_bf16, int64_t ld_grad, void* stream);

/* ---- native layer runner: the Idefics language stack (32 decoder + 8 gated cross-attention layers, hooks, final norm, LM head;
 * hf:idefics/modeling_idefics.py:1052-1074,1179-1182) given the image states, in ONE call: the same kernels, order and dispatch as
 * the Python engine loop (bit-identical), issued from C++ so that launch-bound shapes (decode steps of hooked generate,
 * ref:inference.py:300-321; the 32-token student / prefill) are not paced by the interpreter.  All pointers are device pointers
 * unless marked HOST; the caller owns every buffer. ---- */
typedef struct { const void *in_ln, *qkv_w, *o_w, *post_ln, *gu_w, *down_w; } licv_idefics_dec_w;
typedef struct { const void *in_ln, *q_w, *kv_w, *o_w, *qn_w, *kn_w, *post_ln, *gu_w, *down_w; float gate_attn, gate_dense; } licv_idefics_xattn_w;
typedef struct {
    int64_t hidden, inter, n_heads, head_dim, n_layers, cross_interval;
    int64_t vocab, n_extra_vocab, vocab_total;         /* base vocabulary, additional embeddings, rows of the fused LM head */
    int64_t img_dim, img_len, rope_len;                /* width of the image states, latents per image, rows of cos/sin */
    float rms_eps;
    const void *embed, *embed_extra, *final_ln, *lm_head, *cos, *sin;
    const licv_idefics_dec_w* dec;                     /* HOST array [n_layers] */
    const licv_idefics_xattn_w* xat;                   /* HOST array [n_layers / cross_interval] */
} licv_idefics_text_weights;
typedef struct {
    const int64_t* input_ids;                          /* (B, S) */
    const int32_t* key_valid;                          /* (B, Sk) attention mask over past + new tokens */
    const int64_t* position_ids;                       /* (B*S) */
    const void* image_states;                          /* (B, Nk, img_dim) bf16 */
    const int32_t* img_mask;                           /* (B, S, n_img) */
    const float* gate;                                 /* (B*S) cross_attention_gate */
    int64_t B, S, Sk, Nk, n_img;
    const float* icv;                                  /* (n_hooked, hidden) fp32, or NULL: no intervention */
    const float* alpha;                                /* (n_hooked) fp32 folded into the hook, or NULL: icv is already scaled */
    const int32_t* hook_slot;                          /* HOST array [n_layers]: row of icv for that layer's output, -1 = not hooked */
    void* const* kv_cache;                             /* HOST array [n_layers] of (B, cache_max_len, 2*hidden) bf16, or NULL */
    int64_t cache_max_len, past;
    const int32_t* kv_rows; int64_t ld_kv_rows;        /* physical cache row of every history position, or NULL: decode steps (S == 1, licv_decode_attn) and continuation steps (S > 1, licv_append_attn) */
    const void* const* xkv_cached;                     /* HOST array [n_x] of projected+normed cross-attention K|V (B, Nk, 2*hidden), or NULL */
    void* const* xkv_out;                              /* HOST array [n_x]: project INTO these (they become next step's xkv_cached), or NULL */
    const int64_t* logits_rows; int64_t n_rows;        /* logits only for these flat rows (n_rows = 0: all B*S rows) */
    void *h16, *h32, *x, *xn, *q, *qkv, *o, *act, *xkv, *xsel;   /* scratch: (M,H) bf16, (M,H) fp32, 3 x (M,H) bf16, (M,3H), (M,H), (M,I), (B*Nk,2H), (n_rows,H) */
    void* workspace; int64_t workspace_bytes;          /* split-K scratch (licv_workspace_size) */
    void* logits; int64_t ld_logits;                   /* (rows, ld_logits >= vocab_total) bf16 */
} licv_idefics_text_call;
/* Options of the runner: 0 = fold the decoder layers' two residual adds into the row kernels that follow (licv_add_rmsnorm_fwd,
 * licv_inject_renorm_pre_fwd), so the o / down projections take the register-direct GEMM epilogue (default 1; bit-identical either
 * way, 0 is for A/B timing).  1 = where the o / down / QKV projections run split-K (M < 512), let the row kernel behind each of
 * them sum the slices (the *_ws entry points) instead of a finalize launch (default 1; bit-identical).  2 = MiB of the next
 * projection's weights a side stream reads ahead during decode steps (default 0 = off).  3 = steps with kv_rows append
 * their K | V to the rows' own cache rows (default 1); 0 = they only read the cache (candidate scoring on a shared prompt; they run
 * licv_append_attn also when S == 1), which may then hold fewer rows than B. */
int licv_runner_option(int option, int value);
int licv_idefics_text_forward(const licv_idefics_text_weights* w, const licv_idefics_text_call* c, void* stream);
/* The same forward for a RIGHT-PADDED batch (row b holds cu_seqlens[b+1] - cu_seqlens[b] real tokens, then padding) without the
 * padding rows: the call is the one licv_idefics_text_forward takes - unpacked (B, S) inputs, scratch sized for M = B*S, unpacked
 * logits, logits_rows addressing b*S + s - and kv_cache must be NULL.  One kernel gathers input_ids, position_ids, gate and the
 * img_mask rows to packed order into pack_scratch (>= total * (20 + 4*n_img) bytes, 16-byte aligned, total = cu_seqlens[B]); every
 * launch up to and including the final RMSNorm runs on `total` rows (both attentions through licv_attn_fwd_ragged); the normed rows
 * are scattered back to (B*S, hidden) with zeros at padding positions, and the LM head / logits_rows gather run as ever.  Real
 * positions get the bits of licv_idefics_text_forward wherever licv_gemm_splitk_plan answers the same split count for `total` rows as
 * for B*S (the caller's gate); padding positions get logits of exactly 0.  pack_rows = 0 (the gate is closed): every launch runs on
 * the B*S padded rows as in licv_idefics_text_forward (pack_scratch may be NULL) and only the padding rows of the final norm are
 * zeroed, so the logits of a right-padded batch are the same at EVERY position whichever way the gate went.  cu_seqlens as
 * licv_attn_fwd_ragged takes it, every length 1 .. S; otherwise LICV_E_BADARG and nothing launched. */
int licv_idefics_text_forward_packed(const licv_idefics_text_weights* w, const licv_idefics_text_call* c, const int32_t* cu_seqlens_host,
                                     const int32_t* cu_seqlens_dev, int pack_rows, void* pack_scratch, int64_t pack_scratch_bytes, void* stream);

/* ---- one decode step's self-attention block (ref:inference.py:300-321: B x num_beams rows, one new token each; hf eager attention
 * hf:idefics/modeling_idefics.py:450-470, rotary :396-428, hf:mistral/modeling_mistral.py:122-179 for GQA) in ONE launch: fused QKV rows
 * (bf16, or the fp32 split-K slices of licv_gemm_bf16_splitk_produce) -> rotary on Q / K -> K | V appended to cache[r, past] -> attention
 * of the new query over positions 0..past -> out (M, n_heads * head_dim) bf16.  cache: (rows, max_len, 2 * n_kv_heads * head_dim) bf16,
 * K then V.  kv_rows (M, ld_kv_rows) int32, optional: the physical cache row holding position p of row r's history (beam search keeps
 * the cache in place and reorders this table, see licv_beam_step); NULL = every row reads its own cache row.  The kernel keeps a
 * row's whole table in LDS: (past + 1) * 4 bytes <= 40 KiB, i.e. at most 10 240 keys, and LICV_E_BADARG beyond; a longer history goes
 * through licv_decode_attn_split below, which has no such limit. */
typedef struct {
    const float* qkv_ws; int splits; int64_t slice_elems, row_stride;   /* split-K slices of the QKV projection, or NULL */
    const void* qkv_bf16; int64_t ldq;                                   /* (M, ldq) bf16 rows [Q | K | V] when qkv_ws == NULL */
    const void* cos; const void* sin; const int64_t* position_ids; int64_t n_pos;   /* (n_pos, head_dim) bf16 tables, (M) positions */
    void* cache; int64_t max_len, past;
    const int32_t* kv_rows; int64_t ld_kv_rows;
    const int32_t* key_valid;                                            /* (M, past + 1) attention mask, or NULL */
    void* out;
    int64_t M, n_heads, n_kv_heads, head_dim;
    float scale;
} licv_decode_attn_args;
int licv_decode_attn(const licv_decode_attn_args* a, void* stream);

/* ---- the same decode step over a history of ANY length, as two launches: the key range of every (row, kv head) is cut into n_splits
 * runs of whole 64-key sweeps; every split leaves an un-normalised partial per query head (running max, running sum, head_dim fp32
 * output columns) in `workspace`, and a second launch merges them in split order (Mx = max m_s; out = bf16(sum w_s o_s / sum w_s l_s),
 * w_s = exp2(m_s - Mx), 0 where the sum is not positive).  No workgroup waits for another and there are no atomics: the result is a
 * function of the arguments alone.  Same struct, same references and per-key arithmetic, same checks as licv_decode_attn except the
 * history limit; n_splits = 1 gives licv_decode_attn's bits, and every n_splits gives its cache.  A sweep's row-table entries and
 * key_valid flags are read when the sweep is requested, masked keys fetch no K / V, and only the split that holds position `past`
 * appends the new token's K | V.
 * licv_decode_attn_split_plan: the number of splits the library would choose for M rows over Sk = past + 1 keys (into *n_splits, may be
 * NULL) and the workspace bytes for it, M * n_heads * n_splits * (head_dim + 2) * 4; a pure function of its arguments (0 and 0 splits
 * for a non-positive argument).
 * licv_decode_attn_split: n_splits <= 0 takes the plan's choice; a value above the number of 64-key sweeps is clamped to it, one above
 * LICV_DECODE_MAX_SPLITS is LICV_E_BADARG.  workspace: 16-byte aligned, at least M * n_heads * n_splits * (head_dim + 2) * 4 bytes
 * with n_splits after clamping; its content before the call does not matter and is unspecified after it. */
#define LICV_DECODE_MAX_SPLITS 32
int64_t licv_decode_attn_split_plan(int64_t M, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t Sk, int* n_splits);
int licv_decode_attn_split(const licv_decode_attn_args* a, int n_splits, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- a continuation step's self-attention block: T new tokens per row THROUGH the cache-row table, in ONE launch.  It generalises
 * licv_decode_attn (same references, same arithmetic; T = 1 with append = 1 gives its bits) and replaces, for a step of T > 1 tokens
 * behind a row table, the only forms available before it: a chain of T licv_decode_attn launches, which fetches the history T times,
 * or licv_rotary_kv_append + licv_attn_fwd on a physically gathered copy of the cache.  Row r*T + t of qkv_bf16 / position_ids / out is
 * token t of row r.  Query t of row r attends to history positions j < past, read from cache row kv_rows[r][j] (NULL: cache row r),
 * and to the new tokens u <= t of its own row at key index past + u.  key_valid (M, past + T), optional: a key with 0 is masked for
 * every query; the output of a query whose own key is masked is unspecified but finite.  append = 1: the rotated K and the V of the T
 * tokens are written to cache[r, past : past+T] (the cache then needs M rows) and nothing else changes; append = 0: the cache is
 * only read, so M rows may share the rows of a smaller cache (candidate scoring on a shared prompt).  head_dim: a multiple of 8 up
 * to 128; (past + T) * 4 bytes <= 40 KiB as for licv_decode_attn.  That limit stays: there is no split form of this entry, so candidate
 * scoring on a prompt of more than 10 240 keys is not served (licv_decode_attn_split covers decode steps, T = 1 with append, only). */
#define LICV_APPEND_MAX_T 32
typedef struct {
    const void* qkv_bf16; int64_t ldq;                                   /* (M*T, ldq) bf16 rows [Q | K | V] */
    const void* cos; const void* sin; const int64_t* position_ids; int64_t n_pos;   /* (n_pos, head_dim) bf16 tables, (M*T) positions */
    void* cache; int64_t max_len, past;                                  /* (rows, max_len, 2 * n_kv_heads * head_dim) bf16, K then V */
    const int32_t* kv_rows; int64_t ld_kv_rows;                          /* (M, ld_kv_rows >= past) int32, or NULL */
    const int32_t* key_valid;                                            /* (M, past + T) attention mask, or NULL */
    int append;                                                          /* 1: write the new K | V to cache[r, past : past+T]; 0: leave the cache alone */
    void* out;                                                           /* (M*T, n_heads * head_dim) bf16 */
    int64_t M, T, n_heads, n_kv_heads, head_dim;
    float scale;
} licv_append_attn_args;
int licv_append_attn(const licv_append_attn_args* a, void* stream);

/* ---- beam search bookkeeping of hooked generate (ref:inference.py:300-321 -> transformers GenerationMixin._beam_search, 5.x form,
 * generation/utils.py:3077-3460; ref:config/inference.yaml:26-30: 3 beams, 5 new tokens, length_penalty 0) ----
 * ONE call (two launches: a scan over vocabulary chunks, a finish per question) per decode step: log_softmax of every beam's logits,
 * top 2*nb of (nb x V) per question, running / finished set update, early-stop heuristic, and the loop condition.  State buffers are ping-ponged by the caller (in != out for the token rows). */
typedef struct {
    const void* logits; int logits_dtype;              /* rows of V logits, bf16 or fp32, row stride ld (elements) */
    /* logits_dtype = LICV_F32_LOGPROBS ("logprobs_in"): the rows are fp32 FINAL log-probabilities, as licv_logits_process leaves them
     * with normalize = 1 (hf _beam_search: log_softmax, then the logits processors, then + running score); they may hold -inf.  The
     * scan ranks x itself and the finish uses lp = x + running score; suppress_eos and all bookkeeping are unchanged.
     * licv_beam_sample_step rejects it (LICV_E_BADARG). */
    int64_t ld;
    int64_t q_stride_rows, beam_stride_rows;           /* logits row of (question b, beam k) = b*q_stride_rows + k*beam_stride_rows
                                                          (nb, 1 in the loop; 1, 0 right after the prefill: all beams share the row) */
    int64_t B, nb, V, max_len, cur, P;                 /* cur = column being written, P = prompt length, max_len = P + max_new_tokens */
    int64_t eos;                                       /* -1 = no EOS token */
    int suppress_eos;                                  /* min_new_tokens not reached: EOS scores -inf */
    float length_penalty; int early_stopping;          /* early_stopping: 1 = True, 0 = False (the reference's setting) */
    const int64_t* running_in; const int64_t* finished_in;       /* (B, nb, max_len) token rows */
    const float* run_scores_in; const float* fin_scores_in;      /* (B, nb) */
    const uint8_t* is_fin_in; const uint8_t* improve_in;         /* (B, nb), (B) */
    const int64_t* gen_len_in;                                   /* (B, nb) generated length of each finished hypothesis */
    int64_t* running_out; int64_t* finished_out; float* run_scores_out; float* fin_scores_out; uint8_t* is_fin_out; uint8_t* improve_out;
    int64_t* gen_len_out;
    int64_t* beam_src_flat;                            /* (B*nb): row b*nb + source beam of every new running beam (the KV-cache reorder) */
    int64_t* next_tokens;                              /* (B*nb): the token each new running beam just appended (next step's input_ids) */
    int32_t* flags;                                    /* [0] = 1 while the search continues (written by the last workgroup) */
    int32_t* sync;                                     /* 4 int32, zero before the first call; the kernel leaves them zero */
    /* optional: the KV-cache row table of licv_decode_attn, (B*nb, kv_ld) int32.  Row r of the new table = row (source beam of r) of
     * the old one, then entry [cur] = r: the token a beam appends next lands in its OWN physical cache row.  NULL = not maintained. */
    const int32_t* kv_rows_in; int32_t* kv_rows_out; int64_t kv_ld;
    void* scratch; int64_t scratch_bytes;              /* >= licv_beam_step_scratch_bytes(B, nb), 16-byte aligned: the scan's per-chunk partials */
} licv_beam_step_args;
int64_t licv_beam_step_scratch_bytes(int64_t B, int64_t nb);
int licv_beam_step(const licv_beam_step_args* a, void* stream);

/* ---- logits processors of hooked generate: transformers 5.x _get_logits_processor (generation/utils.py:1123-1330), in its order:
 * RepetitionPenaltyLogitsProcessor (generation/logits_process.py:306-413), NoRepeatNGramLogitsProcessor (:1073-1139),
 * NoBadWordsLogitsProcessor (:1395-1480 on SequenceBiasLogitsProcessor.__call__, :1288-1319), SuppressTokensLogitsProcessor (:1869-1906)
 * and SuppressTokensAtBeginLogitsProcessor (:1816-1866).  ONE launch per decode step turns B*nb rows of next-token logits into dense
 * fp32 rows of processed scores: out row r = b*nb + k is made from logits row b*q_stride_rows + k*beam_stride_rows and the token
 * history ids[r, :cur] (prompt and its pad tokens included; the first P entries are the prompt).
 *   normalize = 0: the processors act on the fp32 value of the logit (hf _sample, greedy and sampling without beams);
 *   normalize = 1: on its fp32 log-softmax (x - max) - log(sum exp(x - max)) (hf _beam_search; feed licv_beam_step as LICV_F32_LOGPROBS).
 * repetition_penalty t (1 = off): every DISTINCT token of the history has its score s replaced by s * t if s < 0, else s / t
 * (once, however often it occurs).  no_repeat_ngram_size n (0 = off): nothing while cur < n; else ids[i + n - 1] is banned for every
 * i <= cur - n with ids[i .. i+n-2] == ids[cur-n+1 .. cur-1] (n = 1: every token seen).  Bad words: word w is the tokens
 * bad_words[bad_offsets[w] .. bad_offsets[w+1]); a one-token word is always banned, a word of length L in its last token when
 * cur >= L and the row's last L - 1 tokens equal its first L - 1 (hf ignores a word longer than the history; the caller drops a
 * word equal to [eos] as NoBadWordsLogitsProcessor does).  suppress: always banned.  begin_suppress: banned when cur == P.  A ban
 * writes -inf and wins over the penalty; every output is ONE IEEE operation on the mode's input value.  Tokens outside [0, V) in
 * any list or history are ignored.  bad_offsets exists twice: on the device for the kernel, on the HOST for the argument check. */
typedef struct {
    const void* logits; int logits_dtype;              /* rows of V logits, bf16 or fp32, row stride ld (elements); V <= 65536 */
    int64_t ld;
    int64_t q_stride_rows, beam_stride_rows;           /* as licv_beam_step_args: (nb, 1) = dense rows, (1, 0) = a question's beams share a row */
    int64_t B, nb, V;                                  /* B*nb output rows */
    const int64_t* ids; int64_t ids_ld;                /* (B*nb, ids_ld) token history, cur <= ids_ld valid entries per row */
    int64_t cur, P;
    float* out; int64_t out_ld;                        /* (B*nb, out_ld >= V) fp32, must not overlap logits */
    int normalize;
    float repetition_penalty;                          /* > 0; 1 = off */
    int64_t no_repeat_ngram_size;                      /* >= 0; 0 = off */
    const int32_t* bad_words; int64_t bad_words_len;   /* flat tokens of all words (device) */
    const int32_t* bad_offsets;                        /* (n_bad_words + 1) device */
    const int32_t* bad_offsets_host;                   /* the same values, HOST pointer: 0 = first, strictly rising, last = bad_words_len */
    int64_t n_bad_words;
    const int32_t* suppress; int64_t n_suppress;       /* device */
    const int32_t* begin_suppress; int64_t n_begin_suppress;
} licv_logits_process_args;
int licv_logits_process(const licv_logits_process_args* a, void* stream);

/* ---- sampled decoding (do_sample=True) of hooked generate: transformers 5.x _sample (generation/utils.py:2794-2930) and the
 * do_sample branch of _beam_search (_get_top_k_continuations, :3090-3125, :3388-3420) with the warpers of _get_logits_processor
 * (:1123-1330) in hf order: min-new-tokens EOS suppression, temperature, top-k, top-p, min-p (generation/logits_process.py).
 * Randomness: Philox4x32-10 keyed by the 64-bit seed, counter (step = cur - P, question, beam, token); u = ((x >> 8) + 0.5) * 2^-24.
 * Ties: top-k keeps every score >= the k-th largest; top-p removes in ascending score order, the higher token id first among equal
 * scores, while the removed mass stays <= (1 - top_p) * total (mass = exp(score - max) in 2^-40 fixed point); min-p keeps
 * exp(score - max) >= min_p; min_tokens_to_keep = 1 without beams, 2 with. ---- */
typedef struct {
    float temperature;                                 /* > 0 (hf TemperatureLogitsWarper: scores / T in fp32) */
    int64_t top_k;                                     /* 0 = off; raised to min_tokens_to_keep (hf TopKLogitsWarper) */
    float top_p;                                       /* (0, 1]; 1 = off (hf TopPLogitsWarper) */
    float min_p;                                       /* [0, 1]; 0 = off (hf MinPLogitsWarper) */
    uint64_t seed;                                     /* Philox key */
} licv_sample_params;

/* num_beams == 1 (hf _sample with do_sample): per row the warpers on the fp32 logits, then the inverse-CDF draw over the kept tokens
 * in token-id order (the smallest id whose prefix mass exceeds u * total).  Finished rows take the pad id.  ONE launch per step. */
typedef struct {
    const void* logits; int logits_dtype;              /* (B, V) rows, bf16 or fp32, row stride ld (elements); V <= 65536 */
    int64_t ld;
    int64_t B, V;
    int64_t* ids; int64_t ids_ld;                      /* the running (B, max_len) id buffer: column cur is written */
    int64_t max_len, cur, P;                           /* cur = column being written, P = prompt length */
    uint8_t* unfinished;                               /* (B) 1 while a row generates (hf unfinished_sequences), updated in place */
    int64_t* next_tokens;                              /* (B) the tokens just written (the next step's input ids) */
    int64_t eos, pad;                                  /* eos -1 = none */
    int suppress_eos;                                  /* min_new_tokens not reached: EOS scores -inf */
    int32_t* flags;                                    /* [0] = 1 while some row generates and cur + 1 < max_len (last workgroup) */
    int32_t* sync;                                     /* 2 int32, zero before the first call; the kernel leaves them zero */
} licv_sample_step_args;
int licv_sample_step(const licv_sample_step_args* a, const licv_sample_params* p, void* stream);

/* num_beams > 1 (beam-search multinomial sampling): the warpers act on log_softmax(logits) (beam.hip's order of evaluation) / T,
 * filtered scores are -inf and the carried beam scores are these processed values (not renormalised).  2*nb continuations per
 * question are drawn without replacement from softmax(score + running score) over (nb x V) as the 2*nb largest Gumbel keys
 * score + running + (-log(-log u)) (ties: the lower flat index); the un-noised scores go on to licv_beam_step's bookkeeping, which is
 * unchanged, KV row table included.  Fewer than 2*nb candidates of non-zero probability in a question: flags[0] bit 1 (value 2) is
 * set (torch.multinomial raises there).  a->scratch: >= licv_beam_sample_scratch_bytes(B, nb), zero before the first call. */
int64_t licv_beam_sample_scratch_bytes(int64_t B, int64_t nb);
int licv_beam_sample_step(const licv_beam_step_args* a, const licv_sample_params* p, void* stream);

/* ---- device-side front-end: integer rules between the collator / processor and the first GEMM ---- */
/* Idefics image_attention_mask (B, S, n_images) int32 one-hot rows from input_ids (B, S) int64 by the incremental rule of
 * hf:idefics/processing_idefics.py:89-110 + :66-79 (ref:icv_src/icv_datamodule.py:80-124 gets it from processor.prepare_input). */
int licv_idefics_image_attention_mask(const int64_t* input_ids, int32_t* mask_out, int64_t B, int64_t S, int64_t n_images,
                                      int64_t image_token_id, int64_t eod_token_id, void* stream);
/* Idefics2: per image real flag (some pixel != 0), patch validity (n, gh*gw) int32 and NaViT position ids (n, gh*gw) int64
 * (hf:idefics2/modeling_idefics2.py:831-855, :136-170); boundaries = the module's fp32 arange(1/n_side, 1, 1/n_side);
 * pixel_attention_mask (n, H, W) bytes, may be NULL (= everything attended). */
int licv_idefics2_patch_front(const void* pixel_values_bf16, const void* pixel_attention_mask_u8, const float* boundaries,
                              int32_t* real_out, int32_t* patch_valid_out, int64_t* position_ids_out,
                              int64_t n_images, int64_t height, int64_t width, int64_t patch, int64_t n_side, void* stream);
/* Idefics2 inputs_merger (hf:idefics2/modeling_idefics2.py:789-815): the k-th <image> token (row-major) of input_ids (M) takes row k
 * of image_rows (n_image_rows, dim) in h (M, dim); rank_scratch: M int32; count_out (1 int32, optional) = number of <image> tokens. */
int licv_merge_image_rows(void* h_bf16, const int64_t* input_ids, const void* image_rows_bf16, int32_t* rank_scratch,
                          int32_t* count_out, int64_t M, int64_t dim, int64_t n_image_rows, int64_t image_token_id, void* stream);

/* Image input (ref:icv_src/icv_datamodule.py:80-124 -> processor.prepare_input -> hf:image_transforms.py rescale :118-122, normalize
 * :437; hf:idefics2 image processor's padding + pixel_attention_mask): src (n, H, W, 3) uint8 on the device -> dst (n, 3, H, W) bf16 =
 * bf16(((float)(u8 * rescale) - mean[c]) / std[c]); valid_hw (n, 2) int32 (optional): real height / width of each image inside the
 * padded H x W (pixels outside are 0, mask 0); mask (n, H, W) uint8 (optional).  mean3 / std3 are HOST pointers. */
int licv_preprocess_images(const void* src_u8, const int32_t* valid_hw, void* dst_bf16, void* mask_u8, int64_t n_images,
                           int64_t H, int64_t W, double rescale, const float* mean3, const float* std3, void* stream);

/* ---- loss + optimiser (ref:icv_src/icv_module.py:121-134, :171-209) ---- */
/* per-row KL(teacher||student) with eps inside the log, rows gathered by index; out_rows fp32 (n_rows). */
int licv_kl_rows_fwd(const void* stu_logits, const void* tea_logits, int dtype,
                     const int64_t* stu_rows, const int64_t* tea_rows, int64_t n_rows, int64_t vocab,
                     int64_t ld_stu, int64_t ld_tea, float temperature, float eps, float* out_rows, void* stream);
/* d/dT of the same per-row sum (ref:icv_src/icv_module.py:49-52: `temperature` is a Parameter, trainable with learnable_t);
 * the caller forms dL/dT = T^2 * mean(out_rows) + 2 T * mean(kl_rows).  out_rows fp32 (n_rows). */
int licv_kl_rows_dtemp(const void* stu_logits, const void* tea_logits, int dtype,
                       const int64_t* stu_rows, const int64_t* tea_rows, int64_t n_rows, int64_t vocab,
                       int64_t ld_stu, int64_t ld_tea, float temperature, float eps, float* out_rows, void* stream);
/* fused AdamW over a flat fp32 buffer; lr per element group given by a split index (alpha first). */
int licv_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_group0,
                    float lr0, float lr1, float beta1, float beta2, float eps, float weight_decay,
                    int64_t step, float grad_scale, void* stream);

/* ---- RICE retrieval (ref:icv_src/utils/mm_topk_retriver.py: CLIP features -> faiss.IndexFlatIP(dim).search(queries, k)) ----
 * Exact flat inner-product search: for each of Q query rows the k index rows (of N) with the largest fp32 inner product.
 *   - scores are fp32 products accumulated in fp32 on the fp32-input MFMA, the whole sum over D in one fixed order (no split over D);
 *     the score of a (query row, index row) pair depends on those two rows only - the same bits wherever the index row sits and
 *     whatever Q, N and the tiling are;
 *   - each output row is sorted by (score descending, index ascending): EQUAL SCORES RESOLVE TO THE LOWEST INDEX (faiss leaves ties
 *     unspecified; this library defines them).  -0 and +0 are equal.  A NaN score is LOWER THAN EVERY NUMBER (below -inf) and is
 *     returned as NaN if it has to be (rows are L2-normalised upstream, so none is expected);
 *   - the Q x N score matrix is never stored: each workgroup keeps a running top-k per query over the index tiles of its chunk and
 *     writes k (score, index) entries per (query, chunk) to the workspace, a second kernel merges the chunks in chunk order.  No
 *     atomics: results are bit-reproducible.  Workspace: Q * chunks * k * 8 bytes with chunks <= 128 (licv_topk_ip_workspace).
 * Supported: 1 <= k <= 64, k <= N, D % 4 == 0, 4 <= D <= 1024, Q >= 1, N < 2^31 - 128; ldq / ldx >= D and multiples of 4, queries /
 * index 16-byte aligned.  Anything else is LICV_E_BADARG (nothing is clamped).  out_idx (Q, k) int64 (as faiss returns them), out_score
 * (Q, k) fp32, both dense. */
int licv_topk_ip_workspace(int64_t Q, int64_t N, int64_t D, int64_t k, int64_t* bytes);
int licv_topk_ip(const float* queries, int64_t ldq, const float* index, int64_t ldx, int64_t Q, int64_t N, int64_t D, int64_t k,
                 int64_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes, void* stream);
/* features /= features.norm(dim=-1, keepdim=True) (ref:icv_src/utils/mm_topk_retriver.py, before the features go to faiss): dense
 * (rows, dim) bf16 or fp32 in, fp32 out; the norm is one fp32 value per row (rounded once from an fp64 sum of squares), the division
 * is IEEE fp32.  out may alias x when x is fp32. */
int licv_l2_normalize_rows(const void* x, int x_dtype, float* out, int64_t rows, int64_t dim, void* stream);
/* QuickGELU (hf:activations.py QuickGELUActivation, CLIP's hidden_act) in place on a (rows, dim) bf16 view with row stride ld:
 * y = bf16(x * bf16(sigmoid(bf16(1.702 x)))), each step rounded to bf16 as the unfused torch ops round.  Columns dim..ld-1 are not
 * touched. */
int licv_quick_gelu(void* x_bf16, int64_t rows, int64_t dim, int64_t ld, void* stream);

/* ---- image resize on the device, bit-equal to Pillow (Image.resize with BICUBIC / BILINEAR on 8-bit RGB), which is what transformers'
 * PIL-backed image processors call (ref:icv_src/utils/mm_topk_retriver.py -> hf CLIPImageProcessor: shortest-edge resize + centre crop;
 * ref:icv_src/icv_datamodule.py -> the Idefics / Idefics2 processors).  THE DEFINITION IS Pillow's src/libImaging/Resample.c:
 * precompute_coeffs + normalize_coeffs_8bpc give, per output index, a first source index, a tap count and `ksize` fixed-point
 * coefficients with 22 fractional bits; ImagingResampleHorizontal_8bpc then ImagingResampleVertical_8bpc apply them,
 *     byte = clip8((2^21 + sum_k pixel[xmin + k] * coef[k]) >> 22)     (int32 accumulator, arithmetic shift, clamp to 0..255),
 * the horizontal result rounded to uint8 before the vertical pass reads it, each pass only where that axis changes size.  The
 * coefficients are computed on the HOST in IEEE double (licv.frontend.resample_plan) and uploaded; the passes are integer arithmetic,
 * so the bytes equal Pillow's.
 *
 * One call resizes a ragged batch.  src: packed RGB uint8 rows (HWC), image i at byte src_offset + y * src_ld_bytes + x0_bytes + 3 x.
 * Per image a licv_resize_desc: source size h x w, resized size oh x ow, the crop (top, left, ch x cw) inside oh x ow, and its two plans
 * inside `plans` (int32): a plan for out_size outputs with `ksize` taps is xmin[out_size], count[out_size], coef[out_size * ksize] from
 * its offset (in elements); the horizontal plan is read when w != ow, the vertical when h != oh.  h == 0 or w == 0 is a missing image.
 * The crop lands at the origin of the image's H x W frame; everything outside ch x cw is 0 (mask 0).  Output: either out_u8
 * (n, H, W, 3) uint8, or out_bf16 (n, 3, H, W) = the table of licv_preprocess_images (rescale, mean3, std3: HOST pointers) applied to
 * those bytes - bit-equal to licv_preprocess_images on the resized bytes; mask_u8 (n, H, W), optional, with either.
 *
 * desc_host is a HOST pointer (every check reads it), desc_dev a device copy of the same n records that is complete on `stream` before
 * the call.  Checked before anything is launched (LICV_E_BADARG, nothing written): the crop inside oh x ow, ch <= H and cw <= W, the
 * source rows inside src_bytes, the plans inside plan_elems, ws_offset as licv_resize_images_workspace set it.  A source row too
 * long for the LDS staging (about 21 000 pixels) is LICV_E_UNSUPPORTED.  src and workspace 16-byte aligned.  Two launches: horizontal
 * pass into the uint8 workspace (only the source rows and the output columns the crop needs), then vertical + crop + normalise.
 * licv_resize_images_workspace WRITES desc_host[i].ws_offset (sum over the images with a horizontal pass of h * align16(3 cw)) and
 * returns the total in *bytes; call it before uploading the descriptors. */
typedef struct licv_resize_desc {
    int64_t src_offset, src_ld_bytes, x0_bytes;
    int64_t h, w, oh, ow;
    int64_t top, left, ch, cw;
    int64_t hplan_offset, hplan_ksize, vplan_offset, vplan_ksize;
    int64_t ws_offset;
} licv_resize_desc;
int licv_resize_images_workspace(licv_resize_desc* desc_host, int64_t n_images, int64_t* bytes);
int licv_resize_images(const void* src_u8, int64_t src_bytes, const licv_resize_desc* desc_host, const licv_resize_desc* desc_dev,
                       int64_t n_images, const int32_t* plans, int64_t plan_elems, int64_t H, int64_t W, void* out_u8, void* out_bf16,
                       void* mask_u8, double rescale, const float* mean3, const float* std3, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---- CLIP text tower on PACKED tokens (ref:icv_src/utils/mm_topk_retriver.py encode_text -> hf CLIPTextModelWithProjection).  The
 * tower is causal (hf:clip/modeling_clip.py:543-556, create_causal_mask + is_causal=True), so the state of a token never depends on
 * what follows it: the valid tokens of a right-padded batch, laid back to back (`total` rows, sequence i = rows cu_seqlens[i] ..
 * cu_seqlens[i + 1] - 1), give the padded tower's states exactly, and the GEMMs and the attention do no work on padding. ---- */
/* hf:clip/modeling_clip.py:221-256 (CLIPTextEmbeddings.forward: token_embedding(input_ids) + position_embedding(position_ids)) on
 * packed ids: out[t, :] = bf16(tok[ids[t], :] + pos[positions[t], :]), the sum in fp32 and rounded once (torch's bf16 add).  ids
 * (total) int64 and positions (total) int32 are DEVICE arrays; the position of a token inside its sequence is made on the host together
 * with cu_seqlens (licv.clip_engine.pack_text_batch), which also validates 0 <= id < vocab and 0 <= position < n_pos before the launch.
 * The kernel reads neither table outside its rows: an id or a position out of range writes a row of zeros.  dim % 8 == 0; tables and
 * out 16-byte aligned; out (total, dim) dense. */
int licv_clip_text_embed(const int64_t* ids, const int32_t* positions, const void* tok_bf16, const void* pos_bf16, void* out_bf16,
                         int64_t total, int64_t dim, int64_t vocab, int64_t n_pos, void* stream);
/* hf:clip/modeling_clip.py:259-277 (eager_attention_forward) + :280-335 (CLIPAttention.forward) under the causal mask of :543-548, over
 * a packed (total, ld_qkv) bf16 buffer of fused projections [Q | K | V], each n_heads * head_dim wide: token i of a sequence attends
 * to tokens 0 .. i of the SAME sequence and to nothing else.  out (total, n_heads * head_dim) bf16 dense; rows past `total` are not
 * touched.  cu_seqlens: n_seq + 1 int32, [0] = 0, ascending; given twice - cu_seqlens_host (HOST pointer, every check reads it) and
 * cu_seqlens_dev (a device copy, complete on `stream` before the call; a copy that disagrees with the host's cannot take the kernel
 * out of the buffers - such sequences are skipped).  head_dim must be 64 and every length 1 .. 128: the whole K and V of one
 * (sequence, head) stay in LDS, the softmax is one fp32 pass over the resident scores, key tiles above the diagonal are skipped.
 * Rounding points as licv_attn_fwd (exp2 of fp32 scores, bf16 probabilities into the PV MFMA, fp32 accumulators, bf16 output).  A row's
 * result depends on its own sequence only: the same bits alone or in any batch.  head_dim != 64, a length of 0 or above 128,
 * cu_seqlens not ascending from 0, ld_qkv < 3 * n_heads * head_dim or not a multiple of 8, scale <= 0, misaligned pointers:
 * LICV_E_BADARG, nothing launched. */
int licv_attn_varlen_causal(const void* qkv_bf16, int64_t ld_qkv, const int32_t* cu_seqlens_host, const int32_t* cu_seqlens_dev,
                            int64_t n_seq, int64_t n_heads, int64_t head_dim, float scale, void* out_bf16, void* stream);
/* hf:clip/modeling_clip.py:558-581 (final_layer_norm, then the pooled row of every sequence) with the order swapped, which LayerNorm
 * being row-wise allows: out[j, :] = LayerNorm(x[rows[j], :]) for n_rows selected rows of a (n_src_rows, ld_x) bf16 buffer, fp32
 * statistics and one rounding as licv_layernorm_fwd.  rows: DEVICE int32; an index outside [0, n_src_rows) reads nothing and writes a
 * row of zeros.  out (n_rows, dim) dense. */
int licv_layernorm_rows_fwd(const void* x_bf16, int64_t ld_x, int64_t n_src_rows, const int32_t* rows, const void* w_bf16,
                            const void* b_bf16, void* out_bf16, int64_t n_rows, int64_t dim, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LICV_HIP_H */
