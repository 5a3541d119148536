// fluxmi -- C-ABI entry points for the individual operators (include/fluxmi.h).
// Compiled with hipcc (host-only translation unit; kernels live in the .hip files).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fluxmi_internal.h"

static thread_local char g_err[1024] = "";

void fluxmi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

const char* fluxmi_last_error(void) { return g_err; }
int fluxmi_abi_version(void) { return FLUXMI_ABI_VERSION; }

// The alignment contract of fluxmi_gemm_group_t (include/fluxmi.h): every kernel fetches A and W in 16-byte pieces (LDS-DMA, uint4 loads), and
// the tiled and split-K kernels read bias / gate / resid and store C / C2 as 8- or 16-byte vectors at columns that are multiples of 8 (bf16) or
// 16 (fp8).  The generic kernel touches its outputs one element at a time: where only it can run (tile_cfg 100, or an N no tile divides) the
// outputs need no more than their element's alignment.
static int gemm_check_alignment(const fluxmi_gemm_group_t& g, int i, int N, int is_fp8, int epilogue, int tile_cfg) {
  auto al16 = [](const void* p) { return ((unsigned long long)p & 15) == 0; };
  const long long eb = is_fp8 ? 1 : 2;
  FLUXMI_REQUIRE(al16(g.A), "gemm_grouped: group %d: A=%p must be 16-byte aligned", i, g.A);
  FLUXMI_REQUIRE(al16(g.W), "gemm_grouped: group %d: W=%p must be 16-byte aligned", i, g.W);
  FLUXMI_REQUIRE(g.lda * eb % 16 == 0, "gemm_grouped: group %d: lda=%lld: a row of A must be a multiple of 16 bytes", i, g.lda);
  if (tile_cfg == 100 || N % 64 != 0) return 0;
  const bool q_out = epilogue == FLUXMI_EPI_GELU_QUANT || epilogue == FLUXMI_EPI_QUANT || epilogue == FLUXMI_EPI_SILU_QUANT;
  FLUXMI_REQUIRE(al16(g.C), "gemm_grouped: group %d: C=%p must be 16-byte aligned", i, g.C);
  FLUXMI_REQUIRE(g.ldc * (q_out ? 1 : 2) % 16 == 0, "gemm_grouped: group %d: ldc=%lld: a row of C must be a multiple of 16 bytes", i, g.ldc);
  FLUXMI_REQUIRE(al16(g.bias), "gemm_grouped: group %d: bias=%p must be 16-byte aligned", i, g.bias);
  if (epilogue == FLUXMI_EPI_GATE_RESID) {
    FLUXMI_REQUIRE(al16(g.gate), "gemm_grouped: group %d: gate=%p must be 16-byte aligned", i, g.gate);
    FLUXMI_REQUIRE(al16(g.resid), "gemm_grouped: group %d: resid=%p must be 16-byte aligned", i, g.resid);
    FLUXMI_REQUIRE(g.ldr * 2 % 16 == 0, "gemm_grouped: group %d: ldr=%lld: a row of resid must be a multiple of 16 bytes", i, g.ldr);
  }
  if (epilogue == FLUXMI_EPI_SPLIT) {
    FLUXMI_REQUIRE(al16(g.C2), "gemm_grouped: group %d: C2=%p must be 16-byte aligned", i, g.C2);
    FLUXMI_REQUIRE(g.ldc2 % 16 == 0, "gemm_grouped: group %d: ldc2=%lld: a row of C2 must be a multiple of 16 bytes", i, g.ldc2);
    FLUXMI_REQUIRE(g.c2_col0 % 16 == 0, "gemm_grouped: group %d: c2_col0=%d must be a multiple of 16", i, g.c2_col0);
    FLUXMI_REQUIRE(g.split_n % 16 == 0, "gemm_grouped: group %d: split_n=%d must be a multiple of 16", i, g.split_n);
  }
  return 0;
}

int fluxmi_gemm_grouped(const fluxmi_gemm_group_t* groups, int n_groups, int N, int K, int is_fp8, int act_fmt, int epilogue,
                        int tile_cfg, void* stream) {
  FLUXMI_REQUIRE(groups && n_groups >= 1 && n_groups <= FLUXMI_MAX_GROUPS, "gemm_grouped: n_groups=%d (1..%d)", n_groups, FLUXMI_MAX_GROUPS);
  FLUXMI_REQUIRE(N > 0 && K > 0, "gemm_grouped: bad N=%d K=%d", N, K);
  FluxmiGemmParams p;
  memset(&p, 0, sizeof(p));
  for (int i = 0; i < n_groups; ++i) {
    p.g[i] = groups[i];
    FLUXMI_REQUIRE(groups[i].M >= 0, "gemm_grouped: group %d has M=%d", i, groups[i].M);
    FLUXMI_REQUIRE(groups[i].M == 0 || (groups[i].A && groups[i].W && groups[i].C), "gemm_grouped: group %d has NULL A/W/C", i);
    if (groups[i].M > 0) FLUXMI_TRY(gemm_check_alignment(groups[i], i, N, is_fp8, epilogue, tile_cfg));  // before any launch: a refused call has done nothing
  }
  p.n_groups = n_groups; p.N = N; p.K = K; p.epi = epilogue;
  if (tile_cfg == 100) return fluxmi_launch_gemm_generic(p, is_fp8, act_fmt, (hipStream_t)stream);
  if (tile_cfg >= 115 && tile_cfg <= 113 + 32) return fluxmi_launch_gemm_splitk(p, is_fp8, act_fmt, tile_cfg - 113, (hipStream_t)stream);
  if (tile_cfg < 0) return fluxmi_gemm_dispatch(p.g, p.n_groups, N, K, is_fp8, act_fmt, epilogue, (hipStream_t)stream);
  return fluxmi_launch_gemm(p, is_fp8, act_fmt, tile_cfg, (hipStream_t)stream);
}
int fluxmi_gemm_plan(const fluxmi_gemm_group_t* groups, int n_groups, int N, int K, int is_fp8, int act_fmt, int epilogue, int batch, int* plan,
                     int plan_cap, int* plan_len) {
  return fluxmi_gemm_plan_export(groups, n_groups, N, K, is_fp8, act_fmt, epilogue, batch, plan, plan_cap, plan_len);
}

int fluxmi_f8_gemm(const void* a_fp8, const void* w_e4m3, const float* sa_recip, const float* sb_recip, const void* bias, void* out,
                   int M, int N, int K, int act_fmt, int epilogue, const void* gate, const void* resid, const float* q_scale,
                   int tile_cfg, void* stream) {
  fluxmi_gemm_group_t g;
  memset(&g, 0, sizeof(g));
  g.A = a_fp8; g.W = w_e4m3; g.bias = bias; g.sa_recip = sa_recip; g.sb_recip = sb_recip;
  g.C = out; g.gate = gate; g.resid = resid; g.q_scale = q_scale;
  g.lda = K; g.ldc = N; g.ldr = N; g.M = M;
  return fluxmi_gemm_grouped(&g, 1, N, K, 1, act_fmt, epilogue, tile_cfg, stream);
}

int fluxmi_gemv(const void* x, long long ldx, const void* W, const void* bias, const float* in_scale, const float* sa_recip,
                const float* sb_recip, void* out, long long ld_out, int B, int N, int K, int w_fp8, int act_fmt, int pre_silu,
                void* stream) {
  FluxmiGemvLayer L;
  memset(&L, 0, sizeof(L));
  L.W = W; L.bias = bias; L.in_scale = in_scale; L.sa_recip = sa_recip; L.sb_recip = sb_recip;
  L.out = out; L.x = x; L.ld_out = ld_out; L.ldx = ldx; L.N = N; L.K = K;
  L.w_fp8 = w_fp8; L.pre_silu = pre_silu; L.act_fmt = act_fmt;
  return fluxmi_launch_gemv(nullptr, &L, 1, B, 0, 0, (hipStream_t)stream);
}

int fluxmi_quantize_act(const void* x, void* q, const float* scale, int rows, int cols, long long ld_in, long long ld_out, int fmt,
                        void* stream) {
  return fluxmi_k_quantize_act(x, q, scale, rows, cols, ld_in, ld_out, fmt, (hipStream_t)stream);
}
int fluxmi_amax(const void* x, float* amax, int rows, int cols, long long ld, void* stream) {
  return fluxmi_k_amax(x, amax, rows, cols, ld, (hipStream_t)stream);
}
int fluxmi_calib_update(const float* amax, float* trials, float* scale, float* scale_recip, int trial_index, int num_trials,
                        float max_val, void* stream) {
  FLUXMI_REQUIRE(trial_index >= 0 && trial_index <= num_trials, "calib_update: trial_index %d out of range", trial_index);
  return fluxmi_k_calib_update(amax, trials, scale, scale_recip, trial_index, num_trials, max_val, (hipStream_t)stream);
}
int fluxmi_quantize_weight(const void* w_bf16, void* q, float* amax_tmp, float* scale, float* scale_recip, int N, int K, int fmt,
                           void* stream) {
  return fluxmi_k_quantize_weight(w_bf16, q, amax_tmp, scale, scale_recip, N, K, fmt, (hipStream_t)stream);
}
int fluxmi_dequant(const void* q, float* out, const float* scale_recip, long long n, int fmt, void* stream) {
  return fluxmi_k_dequant(q, out, scale_recip, n, fmt, (hipStream_t)stream);
}

// W' = requant( bf16( dequant(W) + sum_c lora_scale * B @ A_chunk_c ) ).  lora_A is [n_chunks*R, K] (already
// multiplied by alpha/rank on the host as the reference does, lora_loading.py:529-530), lora_B is [N, R].
int fluxmi_lora_fuse_f8(void* w_fp8, float* w_scale, float* w_scale_recip, const float* lora_B, const float* lora_A, int N, int K,
                        int R, int n_chunks, float lora_scale, float* work_f32, float* amax_tmp, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)N * K;
  FLUXMI_REQUIRE(n % 4 == 0 && n_chunks >= 1, "lora_fuse: bad shape N=%d K=%d chunks=%d", N, K, n_chunks);
  // delta accumulates in work_f32[n .. 2n), dequantised weight in work_f32[0 .. n)
  float* w32 = work_f32;
  float* delta = work_f32 + n;
  FLUXMI_TRY(fluxmi_k_dequant(w_fp8, w32, w_scale_recip, n, FLUXMI_E4M3, s));
  for (int c = 0; c < n_chunks; ++c)
    FLUXMI_TRY(fluxmi_k_lora_delta(lora_B, lora_A + (long long)c * R * K, delta, N, K, R, lora_scale, c > 0 ? 1 : (n_chunks > 1 ? 2 : 0), s));
  FLUXMI_TRY(fluxmi_k_axpy_f32(w32, delta, 1.0f, n, s));
  return fluxmi_k_requantize_f32(w32, w_fp8, amax_tmp, w_scale, w_scale_recip, n, FLUXMI_E4M3, s);
}

int fluxmi_ln_modulate(const void* x, long long ldx, void* out, long long ldo, const void* shift0, const void* scale0,
                       const void* shift1, const void* scale1, long long mod_bstride, const float* q_scale0, const float* q_scale1,
                       int B, int L, int split, int H, int out_fp8, int fmt, void* stream) {
  return fluxmi_k_ln_modulate(x, ldx, (long long)L * ldx, out, ldo, (long long)L * ldo, shift0, scale0, shift1, scale1, mod_bstride,
                              q_scale0, q_scale1, B, L, split, H, out_fp8, fmt, (hipStream_t)stream);
}
int fluxmi_ln_modulate_pairs(const void* x, long long ldx, void* out, long long ldo, const void* shift0, const void* scale0,
                             const void* shift1, const void* scale1, long long mod_bstride, const float* q_scale0, const float* q_scale1,
                             int B, int L, int split, int H, int out_fp8, int fmt, int out_pairs, void* stream) {
  return fluxmi_k_ln_modulate(x, ldx, (long long)L * ldx, out, ldo, (long long)L * ldo, shift0, scale0, shift1, scale1, mod_bstride,
                              q_scale0, q_scale1, B, L, split, H, out_fp8, fmt, (hipStream_t)stream, out_pairs != 0);
}
int fluxmi_act(const void* x, void* y, int rows, int cols, long long ld_in, long long ld_out, int mode, void* stream) {
  return fluxmi_k_act(x, y, rows, cols, ld_in, ld_out, mode, (hipStream_t)stream);
}
int fluxmi_gate_residual(const void* x, const void* y, const void* gate, void* out, int B, int L, int H, long long ldx, long long ldy,
                         long long ldo, long long gate_bstride, void* stream) {
  return fluxmi_k_gate_residual(x, y, gate, out, B, L, H, ldx, ldy, ldo, gate_bstride, (hipStream_t)stream);
}
int fluxmi_add(const void* a, const void* b, void* z, long long n, void* stream) {
  return fluxmi_k_add(a, b, z, n, (hipStream_t)stream);
}
int fluxmi_add_bcast(const void* a, const void* b, void* z, long long rows, int nb, int cols, void* stream) {
  return fluxmi_k_add_bcast(a, b, z, rows, nb, cols, (hipStream_t)stream);
}
int fluxmi_rope_table(const void* ids, const float* omega, const int* axis, void* pe, long long rows, int n_axes, int pairs,
                      void* stream) {
  return fluxmi_k_rope_table(ids, omega, axis, pe, rows, n_axes, pairs, (hipStream_t)stream);
}
int fluxmi_qkv_rope(const void* qkv, long long ld, const void* pe, const void* q_scale0, const void* k_scale0, const void* q_scale1,
                    const void* k_scale1, void* Q, void* K, void* VT, int B, int L, int Lp, int H, int split, int k_f16, void* stream) {
  return fluxmi_k_qkv_rope(qkv, ld, pe, q_scale0, k_scale0, q_scale1, k_scale1, Q, K, VT, B, L, Lp, H, split, k_f16, (hipStream_t)stream);
}
int fluxmi_attention(const void* Q, const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                     const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16, void* stream) {
  return fluxmi_k_attention(Q, K, VT, out, ld_out, col_off, out_fp8, q_scale0, q_scale1, split, B, L, Lp, H, fmt, (hipStream_t)stream,
                            nullptr, 0, nullptr, nullptr, nullptr, k_f16);
}
int fluxmi_im2col3x3(const void* x, void* col, int B, int H, int W, int C, int upsample, void* stream) {
  return fluxmi_k_im2col3x3(x, col, B, H, W, C, upsample, (hipStream_t)stream);
}
int fluxmi_conv3x3(const void* x, const void* w2, const void* bias, const void* gate, const void* resid, void* out, int B, int H, int W, int C,
                   int Cout, int upsample, void* stream) {
  FLUXMI_REQUIRE(x && w2 && out && B >= 1 && H >= 1 && W >= 1, "conv3x3: NULL tensor or empty grid");
  FLUXMI_REQUIRE(upsample == 1 || upsample == 2 || upsample == -2, "conv3x3: mode in {1, 2, -2}");
  FLUXMI_REQUIRE(upsample != 2 || (H % 2 == 0 && W % 2 == 0), "conv3x3: upsampled output dims must be even");
  FLUXMI_REQUIRE((long long)B * H * W < (1LL << 31), "conv3x3: more than 2^31 output pixels");
  FLUXMI_REQUIRE(!resid || gate, "conv3x3: a residual needs the gate vector (ones for a plain add)");
  FluxmiGemmParams p;
  memset(&p, 0, sizeof(p));
  FluxmiGemmGroup& g = p.g[0];
  g.A = x; g.W = w2; g.bias = bias; g.C = out; g.gate = gate; g.resid = resid;
  g.lda = C; g.ldc = Cout; g.ldr = Cout; g.M = B * H * W;
  p.n_groups = 1; p.N = Cout; p.K = 9 * C; p.epi = resid ? FLUXMI_EPI_GATE_RESID : FLUXMI_EPI_BF16;
  p.conv.zeros = fluxmi_zero_page();
  p.conv.Hi = upsample == 2 ? H / 2 : upsample == -2 ? H * 2 : H;
  p.conv.Wi = upsample == 2 ? W / 2 : upsample == -2 ? W * 2 : W;
  p.conv.C = C; p.conv.Ho = H; p.conv.Wo = W;
  p.conv.stride = upsample == -2 ? 2 : 1; p.conv.pad = upsample == -2 ? 0 : 1; p.conv.rshift = upsample == 2 ? 1 : 0;
  return fluxmi_launch_gemm_conv(p, (hipStream_t)stream);
}
int fluxmi_groupnorm(const void* x, const void* gamma, const void* beta, void* y, float* work, int B, int P, int C, int swish, float eps,
                     void* stream) {
  return fluxmi_k_groupnorm(x, gamma, beta, y, work, B, P, C, swish, eps, (hipStream_t)stream);
}
int fluxmi_softmax_rows(const void* S, void* P, int rows, int cols, long long ld, float scale, void* stream) {
  return fluxmi_k_softmax_rows(S, P, rows, cols, ld, scale, (hipStream_t)stream);
}
int fluxmi_row_norm(const void* x, const void* weight, const void* bias, void* y, int rows, int D, long long ldx, long long ldy, float eps, int mode,
                    void* stream) {
  return fluxmi_k_row_norm(x, weight, bias, y, rows, D, ldx, ldy, eps, mode, (hipStream_t)stream);
}
int fluxmi_act_mul(const void* in, void* out, int rows, int F, long long ld_in, long long ld_out, int mode, void* stream) {
  return fluxmi_k_act_mul(in, out, rows, F, ld_in, ld_out, mode, (hipStream_t)stream);
}
int fluxmi_text_attention(const void* q, const void* k, long long ld_qk, const void* vt, long long ld_vt, void* out, long long ld_out,
                          const float* rel_bias, int bias_ld, const void* v_bias, float scale, int causal, int L, int Lp, int H, void* stream) {
  return fluxmi_k_text_attention(q, k, ld_qk, vt, ld_vt, out, ld_out, rel_bias, bias_ld, v_bias, scale, causal, L, Lp, H, (hipStream_t)stream);
}
int fluxmi_vision_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                            void* out, long long ld_out, long long bs_out, const void* v_bias, float scale, int head_dim, int L, int Lp, int H, int B,
                            void* stream) {
  return fluxmi_k_vision_attention(q, k, ld_qk, bs_qk, vt, ld_vt, bs_vt, out, ld_out, bs_out, v_bias, scale, head_dim, L, Lp, H, B, (hipStream_t)stream);
}
int fluxmi_vae_attention(const void* q, const void* k, long long ld_qk, long long bs_qk, const void* vt, long long ld_vt, long long bs_vt,
                         void* out, long long ld_out, long long bs_out, const void* v_bias, int D, int P, int Pp, int B, void* stream) {
  return fluxmi_k_vae_attention(q, k, ld_qk, bs_qk, vt, ld_vt, bs_vt, out, ld_out, bs_out, v_bias, D, P, Pp, B, (hipStream_t)stream);
}
int fluxmi_conv3x3_dense(const void* x, long long ldx, int Cin, const void* w2, const void* bias, void* out, long long ldo, int Cout,
                         const void* r1, long long ldr1, float a1, const void* r2, long long ldr2, float a2, float slope, int act,
                         int upsample, int B, int H, int W, void* stream) {
  return fluxmi_k_conv3x3_dense(x, ldx, Cin, w2, bias, out, ldo, Cout, r1, ldr1, a1, r2, ldr2, a2, slope, act, upsample, B, H, W, (hipStream_t)stream);
}
int fluxmi_canny_classify(const void* rgb, long long ld, long long bs, void* state, long long state_ld, long long state_bs, int B, int H, int W,
                          int low, int high, int l2, void* stream) {
  return fluxmi_k_canny_classify(rgb, ld, bs, state, state_ld, state_bs, B, H, W, low, high, l2, (hipStream_t)stream);
}
int fluxmi_canny_hysteresis_round(void* state, long long state_ld, long long state_bs, int B, int H, int W, int* changed_flag, void* stream) {
  return fluxmi_k_canny_hysteresis_round(state, state_ld, state_bs, B, H, W, changed_flag, (hipStream_t)stream);
}
int fluxmi_canny_hysteresis(void* state, long long state_ld, long long state_bs, void* edges, long long edges_ld, long long edges_bs, int* flags,
                            int B, int H, int W, int* rounds_out, void* stream) {
  return fluxmi_k_canny_hysteresis(state, state_ld, state_bs, edges, edges_ld, edges_bs, flags, B, H, W, rounds_out, (hipStream_t)stream);
}
int fluxmi_canny(const void* rgb, long long ld, long long bs, void* edges, long long edges_ld, long long edges_bs, void* work,
                 long long work_bytes, int B, int H, int W, int low, int high, int l2, int* rounds_out, void* stream) {
  return fluxmi_k_canny(rgb, ld, bs, edges, edges_ld, edges_bs, work, work_bytes, B, H, W, low, high, l2, rounds_out, (hipStream_t)stream);
}
int fluxmi_rgb_to_gray(const void* rgb, long long ld, long long bs, void* gray, long long gray_ld, long long gray_bs, int B, int H, int W,
                       void* stream) {
  return fluxmi_k_rgb_to_gray(rgb, ld, bs, gray, gray_ld, gray_bs, B, H, W, (hipStream_t)stream);
}
int fluxmi_gaussian_blur(const void* src, long long ld, long long bs, void* dst, long long dst_ld, long long dst_bs, void* work,
                         long long work_bytes, int B, int H, int W, int C, float sigma, void* stream) {
  return fluxmi_k_gaussian_blur(src, ld, bs, dst, dst_ld, dst_bs, work, work_bytes, B, H, W, C, sigma, (hipStream_t)stream);
}
int fluxmi_patchify(const void* pix, void* out, int B, int C, int H, int W, int patch, int grid, int Kp, void* stream) {
  return fluxmi_k_patchify(pix, out, B, C, H, W, patch, grid, Kp, (hipStream_t)stream);
}
int fluxmi_unary(const void* x, void* y, long long rows, int cols, long long ld_in, long long ld_out, int kind, void* stream) {
  return fluxmi_k_unary(x, y, rows, cols, ld_in, ld_out, kind, (hipStream_t)stream);
}
int fluxmi_resize_bilinear(const void* x, long long ldx, void* out, long long ldo, const void* add, long long lda, int B, int Hi, int Wi, int Ho,
                           int Wo, int C, void* stream) {
  return fluxmi_k_resize_bilinear(x, ldx, out, ldo, add, lda, B, Hi, Wi, Ho, Wo, C, (hipStream_t)stream);
}
int fluxmi_patchify_rect(const void* pix, void* out, int B, int C, int H, int W, int patch, int grid_h, int grid_w, int Kp, void* stream) {
  return fluxmi_k_patchify_rect(pix, out, B, C, H, W, patch, grid_h, grid_w, Kp, (hipStream_t)stream);
}
int fluxmi_im2col3x3_s2(const void* x, void* col, int B, int Hi, int Wi, int C, void* stream) {
  return fluxmi_k_im2col3x3_s2(x, col, B, Hi, Wi, C, (hipStream_t)stream);
}
int fluxmi_depth_head(const void* x, long long ldx, int C, const void* w, const void* bias, float* out, long long n, void* stream) {
  return fluxmi_k_depth_head(x, ldx, C, w, bias, out, n, (hipStream_t)stream);
}
int fluxmi_depth_to_map(const float* depth, long long ld, long long bs, void* out, long long out_ld, long long out_bs, float* work,
                        long long work_bytes, int B, int h, int w, int H, int W, int normalize, void* stream) {
  return fluxmi_k_depth_to_map(depth, ld, bs, out, out_ld, out_bs, work, work_bytes, B, h, w, H, W, normalize, (hipStream_t)stream);
}
int fluxmi_build_quant_lut(const float* scale, int fmt, int act, void* lut, void* stream) {
  return fluxmi_k_build_qlut(scale, fmt, act, lut, (hipStream_t)stream);
}
int fluxmi_pair_rows(const void* in, void* out, int rows, long long row_bytes, void* stream) {
  return fluxmi_k_pair_rows(in, out, rows, row_bytes, (hipStream_t)stream);
}
int fluxmi_unpair_rows(const void* in, void* out, int rows, long long row_bytes, void* stream) {
  return fluxmi_k_unpair_rows(in, out, rows, row_bytes, (hipStream_t)stream);
}
int fluxmi_attention_debug_buffer(void* dev_u64) { return fluxmi_attn_debug_buffer(dev_u64); }

int fluxmi_attention_plan(int B, int L, int H, int* n_per_x, int* full_per_x, int* npieces, unsigned long long* pieces) {
  return fluxmi_attn_plan_export(B, L, H, n_per_x, full_per_x, npieces, pieces);
}

int fluxmi_attention_rawq(const void* qkv, long long ld_qkv, const void* pe, const void* qn_scale0, const void* qn_scale1, const void* K,
                          const void* VT, void* out, long long ld_out, int col_off, int out_fp8, const float* q_scale0,
                          const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16, void* stream) {
  return fluxmi_k_attention(nullptr, K, VT, out, ld_out, col_off, out_fp8, q_scale0, q_scale1, split, B, L, Lp, H, fmt, (hipStream_t)stream,
                            qkv, ld_qkv, pe, qn_scale0, qn_scale1, k_f16);
}
int fluxmi_attention_grouped(const void* Q, const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                             const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16,
                             const unsigned* groups, int out_pairs, void* stream) {
  return fluxmi_k_attention(Q, K, VT, out, ld_out, col_off, out_fp8, q_scale0, q_scale1, split, B, L, Lp, H, fmt, (hipStream_t)stream,
                            nullptr, 0, nullptr, nullptr, nullptr, k_f16, out_pairs, groups);
}
int fluxmi_attention_rawq_grouped(const void* qkv, long long ld_qkv, const void* pe, const void* qn_scale0, const void* qn_scale1,
                                  const void* K, const void* VT, void* out, long long ld_out, int col_off, int out_fp8,
                                  const float* q_scale0, const float* q_scale1, int split, int B, int L, int Lp, int H, int fmt, int k_f16,
                                  const unsigned* groups, int out_pairs, void* stream) {
  return fluxmi_k_attention(nullptr, K, VT, out, ld_out, col_off, out_fp8, q_scale0, q_scale1, split, B, L, Lp, H, fmt, (hipStream_t)stream,
                            qkv, ld_qkv, pe, qn_scale0, qn_scale1, k_f16, out_pairs, groups);
}
int fluxmi_timestep_embedding(const void* t, const float* freqs, void* out, int B, int half, float time_factor, void* stream) {
  return fluxmi_k_timestep_embedding(t, freqs, out, B, half, time_factor, (hipStream_t)stream);
}
int fluxmi_clock_sample(void* out2_dev_u64, void* stream) {
  FLUXMI_REQUIRE(out2_dev_u64, "clock_sample: NULL argument");
  return fluxmi_k_clock_sample((unsigned long long*)out2_dev_u64, (hipStream_t)stream);
}
int fluxmi_euler(void* img, const void* pred, const float* dts, const int* step, long long n, void* stream) {
  return fluxmi_k_euler(img, pred, dts, step, n, (hipStream_t)stream);
}
int fluxmi_cfg_euler(void* img, const void* pred, const float* dts, const int* step, const float* scale, int B, long long img_rows,
                     long long pred_rows, int c_in, int c_out, void* stream) {
  return fluxmi_k_cfg_euler(img, pred, dts, step, scale, B, img_rows, pred_rows, c_in, c_out, (hipStream_t)stream);
}
int fluxmi_blend_euler(void* img, const void* pred, const void* x0, const void* noise, const void* mask, const float* dts, const float* tnext,
                       const float* one_minus_tnext, const float* thr, const int* step, const float* scale, int B, long long img_rows,
                       long long pred_rows, int c_in, int c_out, void* stream) {
  return fluxmi_k_blend_euler(img, pred, x0, noise, mask, dts, tnext, one_minus_tnext, thr, step, scale, B, img_rows, pred_rows, c_in, c_out,
                              (hipStream_t)stream);
}
int fluxmi_solver_step(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0, const void* noise,
                       const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step, const float* scale,
                       int B, long long img_rows, long long pred_rows, int c_in, int c_out, void* stream) {
  return fluxmi_k_solver_step(img, pred, xs, hist, coef, ctl, x0, noise, mask, tnext, one_minus_tnext, thr, step, scale, B, img_rows, pred_rows,
                              c_in, c_out, (hipStream_t)stream);
}
int fluxmi_solver_step_noise(void* img, const void* pred, void* xs, float* hist, const float* coef, const int* ctl, const void* x0,
                             const void* noise, const void* mask, const float* tnext, const float* one_minus_tnext, const float* thr, const int* step,
                             const float* scale, int B, long long img_rows, long long pred_rows, int c_in, int c_out, const unsigned* ids,
                             const int* eval_offset, void* stream) {
  return fluxmi_k_solver_step_noise(img, pred, xs, hist, coef, ctl, x0, noise, mask, tnext, one_minus_tnext, thr, step, scale, B, img_rows,
                                    pred_rows, c_in, c_out, ids, eval_offset, (hipStream_t)stream);
}
int fluxmi_philox_normal(void* out, const unsigned* ids, int B, long long n_per_image, unsigned eval, int raw, void* stream) {
  return fluxmi_k_philox_normal(out, ids, B, n_per_image, eval, raw, (hipStream_t)stream);
}

int fluxmi_flowedit_couple(void* img, const void* z, const void* x0, float t, float one_minus_t, const unsigned* ids, unsigned eval, int B,
                           long long img_rows, long long pred_rows, int c_in, int c_out, void* stream) {
  return fluxmi_k_flowedit_couple(img, z, x0, t, one_minus_t, ids, eval, B, img_rows, pred_rows, c_in, c_out, (hipStream_t)stream);
}
// acc == NULL is legal only for a row with first and apply set, and which row runs is device data: this entry (tests and tools; the engine
// knows its program and calls the launcher) then reads *step and the row back -- two small synchronising copies -- before it launches
int fluxmi_flowedit_step(void* img, const void* pred, void* z, float* acc, const void* x0, const float* coef, const int* ctl, const int* step,
                         const unsigned* ids, const int* eval_offset, int B, long long img_rows, long long pred_rows, int c_in, int c_out,
                         void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!acc && ctl && ids && B > 0 && pred_rows > 0) {
    int i = 0, row[2] = {0, 0};
    if (step) FLUXMI_CHECK_HIP(hipMemcpyAsync(&i, step, 4, hipMemcpyDeviceToHost, s));
    if (step) FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
    FLUXMI_REQUIRE(i >= 0, "flowedit_step: *step = %d < 0", i);
    FLUXMI_CHECK_HIP(hipMemcpyAsync(row, ctl + 2 * (size_t)i, 8, hipMemcpyDeviceToHost, s));
    FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
    FLUXMI_REQUIRE(row[0] != 0 && row[1] != 0, "flowedit_step: NULL acc, and row %d has first = %d, apply = %d (the fp32 accumulator is "
                   "stored by a row without apply and read by a row without first)", i, row[0], row[1]);
  }
  return fluxmi_k_flowedit_step(img, pred, z, acc, x0, coef, ctl, step, ids, eval_offset, B, img_rows, pred_rows, c_in, c_out, s);
}

// The tables are device data and the placement rules speak of their contents: these entries (tests and tools; the engine is given host
// tables and calls the launchers) read row0 / col0 back -- one synchronising copy each -- before they launch
static int window_tables_ok(const char* who, const int* row0, const int* col0, int Hc, int Wc, int h, int w, int ny, int nx, hipStream_t s) {
  FLUXMI_REQUIRE(ny >= 1 && nx >= 1 && ny <= 65536 && nx <= 65536, "%s: window grid %d x %d out of range", who, ny, nx);
  std::vector<int> r((size_t)ny), c((size_t)nx);
  FLUXMI_CHECK_HIP(hipMemcpyAsync(r.data(), row0, (size_t)ny * 4, hipMemcpyDeviceToHost, s));
  FLUXMI_CHECK_HIP(hipMemcpyAsync(c.data(), col0, (size_t)nx * 4, hipMemcpyDeviceToHost, s));
  FLUXMI_CHECK_HIP(hipStreamSynchronize(s));
  return fluxmi_window_check_tables(who, r.data(), c.data(), Hc, Wc, h, w, ny, nx);
}
int fluxmi_window_gather(const void* canvas, void* img, const int* row0, const int* col0, int N, int Hc, int Wc, int h, int w, int ny, int nx,
                         int C, int guided, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(row0 && col0, "window_gather: NULL tables (row0 int32 [ny], col0 int32 [nx] on the device)");
  FLUXMI_REQUIRE(C > 0 && C % 8 == 0 && Hc >= 1 && Wc >= 1 && h >= 1 && w >= 1 && h <= Hc && w <= Wc, "window_gather: C=%d (C %% 8 == 0), "
                 "window %d x %d inside the canvas %d x %d", C, h, w, Hc, Wc);
  FLUXMI_TRY(window_tables_ok("window_gather", row0, col0, Hc, Wc, h, w, ny, nx, s));
  return fluxmi_k_window_gather(canvas, img, row0, col0, N, Hc, Wc, h, w, ny, nx, C, guided, s);
}
int fluxmi_window_step(void* canvas, void* img, const void* pred, const float* dts, const int* step, const float* scale, const int* row0,
                       const int* col0, const float* Ny, const float* Nx, int N, int Hc, int Wc, int h, int w, int ny, int nx, int C,
                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  FLUXMI_REQUIRE(row0 && col0 && Ny && Nx, "window_step: NULL tables (row0 int32 [ny], col0 int32 [nx], Ny fp32 [ny][Hc], Nx fp32 [nx][Wc] on "
                 "the device)");
  FLUXMI_REQUIRE(C > 0 && C % 8 == 0 && Hc >= 1 && Wc >= 1 && h >= 1 && w >= 1 && h <= Hc && w <= Wc, "window_step: C=%d (C %% 8 == 0), "
                 "window %d x %d inside the canvas %d x %d", C, h, w, Hc, Wc);
  FLUXMI_TRY(window_tables_ok("window_step", row0, col0, Hc, Wc, h, w, ny, nx, s));
  return fluxmi_k_window_step(canvas, img, pred, dts, step, scale, row0, col0, Ny, Nx, N, Hc, Wc, h, w, ny, nx, C, s);
}

int fluxmi_fb_snapshot(const void* x, long long x_bstride, void* dst, int B, long long n, void* stream) {
  return fluxmi_k_fb_snapshot(x, x_bstride, dst, B, n, (hipStream_t)stream);
}
int fluxmi_fb_commit(const void* x, long long x_bstride, const void* r, void* r_ref, void* h1, int B, long long n, void* stream) {
  return fluxmi_k_fb_commit(x, x_bstride, r, r_ref, h1, B, n, (hipStream_t)stream);
}
int fluxmi_fb_metric(const void* x, long long x_bstride, const void* h0, void* r, const void* r_ref, float* part, float* ratio, float* numden,
                     int B, long long n, void* stream) {
  return fluxmi_k_fb_metric(x, x_bstride, h0, r, r_ref, part, ratio, numden, B, n, (hipStream_t)stream);
}
int fluxmi_fb_store(const void* x, long long x_bstride, const void* h1, void* R, int B, long long n, void* stream) {
  return fluxmi_k_fb_store(x, x_bstride, h1, R, B, n, (hipStream_t)stream);
}
int fluxmi_fb_apply(void* x, long long x_bstride, const void* h1, long long h1_bstride, const void* R, int B, long long n, void* stream) {
  return fluxmi_k_fb_apply(x, x_bstride, h1, h1_bstride, R, B, n, (hipStream_t)stream);
}
int fluxmi_add_scaled(void* x, long long x_bstride, const void* r, long long r_bstride, const float* scale, int B, long long n, void* stream) {
  return fluxmi_k_add_scaled(x, x_bstride, r, r_bstride, scale, B, n, (hipStream_t)stream);
}
int fluxmi_guidance_moments(const void* pred, const float* r, float* part, int B, long long N, void* stream) {
  return fluxmi_k_guidance_moments(pred, r, part, B, N, (hipStream_t)stream);
}
int fluxmi_guidance_combine(void* pred, float* r, const float* part, const float* params, const int* step, const int* step_offset,
                            float* coef_out, int B, long long N, void* stream) {
  return fluxmi_k_guidance_combine(pred, r, part, params, step, step_offset, coef_out, B, N, (hipStream_t)stream);
}
int fluxmi_latent_preview(const void* x, const void* pred, const float* ts, const int* step, const float* scale, const float* proj,
                          const int* ctl, void* out, int B, long long img_rows, long long pred_rows, int c_in, int c_out, int h, int w,
                          void* stream) {
  return fluxmi_k_latent_preview(x, pred, ts, step, scale, proj, ctl, out, B, img_rows, pred_rows, c_in, c_out, h, w, (hipStream_t)stream);
}
int fluxmi_ip_attention(const void* qkv, long long ld_qkv, long long qkv_bstride, const void* qn_scale, const void* k_ip, const void* v_ip,
                        long long kv_bstride, void* out, long long ld_o, long long o_bstride, const float* scale, long long scale_bstride, int B,
                        int rows, int heads, int Nk, void* stream) {
  return fluxmi_k_ip_attention(qkv, ld_qkv, qkv_bstride, qn_scale, k_ip, v_ip, kv_bstride, out, ld_o, o_bstride, scale, scale_bstride, B, rows, heads,
                               Nk, (hipStream_t)stream);
}

}  // extern "C"
