// fluxmi -- the GEMM tile configs: ONE table.  What a config number means -- tile shape, K-step, kernel family, which launches it takes --
// is stated here and nowhere else; gemm_dispatch.cpp (predicates, planner), gemm.hip (launcher switch), gemm_w1.hip, tuning.cpp and engine.hip
// look it up.  The numbers are part of the C ABI (fluxmi_gemm_grouped(tile_cfg), fluxmi_tuning_t.gemm_cfg) and do not change; the gaps belonged to
// kernel generations that were measured slower and removed in round 3 (profiles/r01_kernel_sweep.txt, r02_gemm_ab.txt).
#pragma once
#include "../../include/fluxmi.h"

enum : int {
  GEMM_CFG_T128 = 2,             // 128x128 double-buffered, two workgroups per CU: thin launches, N % 256 != 0 (gemm.hip)
  GEMM_CFG_PP = 13,              // 256x256 ping-pong ring, 8 waves (gemm_pp.hip); also the tiling of the split-K launches
  GEMM_CFG_T128x64 = 15,         // 128x64: narrow outputs (LastLayer.linear: N = 64) (gemm.hip)
  GEMM_CFG_W1 = 16,              // 256x256, one wave per SIMD, 2 x 2 wave grid (gemm_w1.hip)
  GEMM_CFG_W1_192 = 17,          // the same kernel on 192x256 tiles
  GEMM_CFG_PERSIST = 18,         // persistent 256x256 ping-pong, one workgroup per CU walks the tiles (gemm_persist.hip)
  GEMM_CFG_PERSIST_TIMING = 19,  // its timing build: per-tile timestamps into fluxmi_gemm_debug_buffer
  GEMM_CFG_W1_224 = 20,          // one wave per SIMD, the four waves side by side along N: 224x256 tiles
  GEMM_CFG_W1_160 = 21,          // the same wave layout on 160x256 tiles
};

enum GemmFamily { GEMM_FAMILY_TILE, GEMM_FAMILY_PINGPONG, GEMM_FAMILY_ONEWAVE, GEMM_FAMILY_PERSISTENT };
// the launches a config is compiled for, beyond what its family takes
enum GemmTakes {
  GEMM_TAKES_ANY,                    // every operand format and epilogue of the family (the persistent family: fluxmi_gemm_persist_ok)
  GEMM_TAKES_F8_GATE,                // fp8 x e5m2 operands with the gate*y+x epilogue
  GEMM_TAKES_F8_GATE_OR_BF16_PLAIN,  // ... or bf16 operands with the plain / gate*y+x epilogue
};

struct GemmTileCfg {
  int id;
  int bm, bn;         // tile height, width
  int kstep;          // K bytes of a row must be a multiple of this ...
  int min_k;          // ... and at least this many
  int wgs_per_cu;     // resident workgroups per CU (the cost model's slots per round)
  GemmFamily family;  // which launcher runs it
  bool fused_kv;      // has the fused K / V^T (attention layout) epilogue
  GemmTakes takes;
  int waves_m;        // one-wave-per-SIMD family: waves along M (bm = 32 * waves_m * TM)
};

constexpr GemmTileCfg GEMM_CFGS[] = {
    // id                      bm   bn   kstep min_k wgs family                  fused  takes                             waves_m
    {GEMM_CFG_T128,            128, 128, 128,  128,  2,  GEMM_FAMILY_TILE,       false, GEMM_TAKES_ANY,                   0},
    {GEMM_CFG_PP,              256, 256, 64,   64,   1,  GEMM_FAMILY_PINGPONG,   true,  GEMM_TAKES_ANY,                   0},
    {GEMM_CFG_T128x64,         128, 64,  128,  128,  3,  GEMM_FAMILY_TILE,       false, GEMM_TAKES_ANY,                   0},
    {GEMM_CFG_W1,              256, 256, 256,  256,  1,  GEMM_FAMILY_ONEWAVE,    true,  GEMM_TAKES_ANY,                   2},
    {GEMM_CFG_W1_192,          192, 256, 256,  256,  1,  GEMM_FAMILY_ONEWAVE,    false, GEMM_TAKES_F8_GATE_OR_BF16_PLAIN, 2},
    {GEMM_CFG_PERSIST,         256, 256, 256,  512,  1,  GEMM_FAMILY_PERSISTENT, true,  GEMM_TAKES_ANY,                   0},
    {GEMM_CFG_PERSIST_TIMING,  256, 256, 256,  512,  1,  GEMM_FAMILY_PERSISTENT, true,  GEMM_TAKES_ANY,                   0},
    {GEMM_CFG_W1_224,          224, 256, 256,  256,  1,  GEMM_FAMILY_ONEWAVE,    false, GEMM_TAKES_F8_GATE,               1},
    {GEMM_CFG_W1_160,          160, 256, 256,  256,  1,  GEMM_FAMILY_ONEWAVE,    false, GEMM_TAKES_F8_GATE,               1},
};

// the row of config `id`, nullptr when there is none
constexpr const GemmTileCfg* gemm_cfg(int id) {
  for (const GemmTileCfg& c : GEMM_CFGS)
    if (c.id == id) return &c;
  return nullptr;
}
constexpr bool gemm_cfg_is(int id, GemmFamily f) { return gemm_cfg(id) && gemm_cfg(id)->family == f; }

// does operand format x epilogue fall inside what config `c` is compiled for
constexpr bool gemm_cfg_takes(const GemmTileCfg& c, int is_fp8, int act_fmt, int epi) {
  const bool f8_gate = is_fp8 && act_fmt == FLUXMI_E5M2 && epi == FLUXMI_EPI_GATE_RESID;
  const bool bf_plain = !is_fp8 && (epi == FLUXMI_EPI_BF16 || epi == FLUXMI_EPI_GATE_RESID);
  return c.takes == GEMM_TAKES_ANY || f8_gate || (c.takes == GEMM_TAKES_F8_GATE_OR_BF16_PLAIN && bf_plain);
}
