// Launch policy of the GEMMs, bf16 and MXFP8, in one place: which kernels a checked descriptor gets on a device of `cus` compute
// units, over which rows, in how many K slices, under which profiler tag.  Pure host code (C++17, no HIP header: any host compiler
// builds it into a stand-alone program); gemm.hip and gemm_fp8.hip check the descriptor and execute the plan, mjv_gemm_plan (mjv.h)
// exports it, and tests/test_gemm_plan_host.py reads it without a GPU, for partitions of 32 - 128 CUs as for the whole part.
#pragma once
#include <algorithm>
#include "mjv.h"

void mjv_set_error(const char* fmt, ...);   // capi.hip

// Measurement knobs.  The product library (default build) has none: the values below are constants, the kernel variants that
// skip work (wrong results by construction) are not compiled, and what a caller may choose - the tile kernel, for parity
// tests - travels in the call's descriptor (mjv_gemm_desc.tile).  -DMJV_BENCH (make bench -> libmjv_hip_bench.so, loaded by
// tools/gemm_bench.py and friends) turns them into process-wide settings behind mjv_bench_gemm_set() (bf16 plans only).
struct GemmTune {
  int gm = 0;               // group-M of the 256-tile order: 0 = by shape (pick_gm)
  int skinny_max_m = 128;   // problems with at most this many rows run on the 64 x 32 kernel
  int split_max = 8;        // cap on the K slices per tile
  int split_k = 1;          // split-K for under-filled 128-tile launches when the caller gives a workspace
  int variant = 0;          // 256-tile kernel variant (3: no epilogue, 4: no global stores, 6: s_memtime stamps)
  int split256_min_kt = 8;  // fewest K-tiles per slice of the K-sliced 256-tile launches
  int split256 = 1;         // under-filled problems with deep K run as K slices of 256 x 256 tiles
  int split256_min_nk = 64; // ... deep = at least this many 64-wide K-tiles (bench: 4400 + n)
  int nt = -1;              // streaming output stores: -1 = by shape, 0 / 1 = never / always
  void* stamp_buffer = nullptr;
};

// one kernel launch (a K-sliced one: the slice kernel and its finish) over rows [row0, row0 + rows) of the problem
struct GemmLaunch {
  int family;            // 64 (64 x 32 skinny), 128, 256 (bf16 and MXFP8), 2 (tile code 2: 128 x 256, two workgroups per CU)
  int epilogue;          // the epilogue this launch runs (MJV_EPI_BIAS where a ROPE_QKV problem falls back)
  int row0, rows, split; // split: K slices per tile (1 = unsliced)
  int tiles_m, tiles_n;  // of the family's tile
  int grid;              // workgroups of the main kernel
  int persistent;        // 256: gemm256p_kernel, one workgroup per CU walks the tiles
  int fuse;              // 256 unsliced: the FUSE instantiation (0 none, 1 RMSNorm, 2 LayerNorm folded in)
  int rope_split_after;  // the launch stored the un-rotated q / k heads in rope_q / rope_k: the in-place rotary step on its rows follows
  const char* tag;       // profiler tag, named like the kernel rocprofv3 reports
  double frac;           // this launch's share of the problem's flops and bytes
};
// (flops, bytes: of the whole problem - algorithmic bytes: A and W read once, the output written once)
struct GemmPlan { int n; GemmLaunch l[2]; int gm, nt_store; double flops, bytes; };

// Group-M per shape class, from sweeps on the model's shapes (tools/gemm_bench.py 2003 ... 2016, best of 6 rounds, two
// boxes): the short-K vision GEMMs prefer 5-7 (qkv +2.8 %, proj +6 %, fc1 +2.5 % over 8 - with N = 1024 and GM = 8 a group
// is exactly the 32 tiles one XCD runs at a time, and all eight XCDs then walk the same four weight panels in step), the
// K = 8192 GEMM prefers 4 (+1.6 ... +3.8 %) and so does the 16384-column w1|w3 GEMM (+1.7 %), everything between is flat
// within 1 % and keeps 8.  (Powers of two - 4, 8 - are the worst choices for the K = 1024 shapes on both main loops.)
// By K BYTES per row (bf16: 2 K, MXFP8: K): what a K-tile moves is the same 128 bytes of a row in both formats.
inline int pick_gm(int N, long k_bytes) { return k_bytes <= 2048 ? 5 : (k_bytes >= 16384 || N >= 8192) ? 4 : 8; }

inline int gemm_out_cols(const mjv_gemm_desc* d) { return d->epilogue == MJV_EPI_SILU_MUL ? d->N / 2 : d->N; }

// streaming stores for every large output (round 4, once the stores really were nt - see store16: qkv +8 %, proj +4 %,
// fc1 +3 %, every other model shape +0.3 ... +0.8 % in tools/gemm_bench.py 7001 7002; in the model, one box, two rounds:
// never 93.5 ms per step, K <= 1024 only 92.6, always 92.3 - profiles/r04_g_nt_stores.txt); small outputs, which the next
// kernel reads back from the L2, keep plain stores.  elem_bytes: 2 for a bf16 output, 1 for an MXFP8 one.
inline int gemm_nt_store(const mjv_gemm_desc* d, int elem_bytes) { return (double)d->M * gemm_out_cols(d) * (double)elem_bytes >= 32.0 * 1024 * 1024; }

// Wave quantisation: with one 256 x 256 workgroup per CU a launch runs in ceil(tiles / cus) rounds, and a last round that is
// mostly empty costs a full tile time (M = 17488, N = 2048 on 256 CUs: 552 tiles = 2.16 rounds -> 3; the 64-row tail of the
// vision tower's 65 600 rows is a 17th round of 16 tiles after fc1's 16 full ones).  When the last round is under-filled, the
// trailing m-tile rows are peeled off into a second launch on the same stream: bf16 rows as 128 x 128 tiles (2 workgroups per
// CU, quarter-size work items), on the skinny kernel, or K-sliced; MXFP8 rows K-SLICED over all CUs.  Rows are independent and
// 64-row scale groups stay whole (the result % 256 == 0).  Returns the rows of the main launch (M: nothing is peeled).
inline int gemm_peel_m_main(const mjv_gemm_desc* d, int cus, bool fp8, bool big) {
  const int tn = (d->N + 255) / 256, tiles = tn * ((d->M + 255) / 256), rem = tiles % cus;
  // format | the last round is under-filled | and the tail has somewhere to run
  const bool may = fp8 ? rem * 2 <= cus     && d->K / 128 >= 8 && d->workspace && d->tile == 0     // (its only tail form is sliced)
                       : rem * 4 <= cus * 2 && big && !d->out_rows && d->tile == 0;
  const int rows_main_tiles = (tiles - rem) / tn;   // whole m-tile rows inside the full rounds
  if (!may || tiles <= cus || rem == 0 || rows_main_tiles == 0) return d->M;
  return rows_main_tiles * 256;                      // < M: with rem > 0 the last m-tile row is never inside the full rounds
}

// K slices (1 = unsliced) of `rows` rows: the slices' fp32 accumulators go through the caller's workspace (65536 bytes per
// slice of a 128-tile, 262144 of a 256-tile) and a second, fully parallel launch sums them in slice order (deterministic).
// 128-tiles: a launch with fewer workgroups than the chip holds (peeled tail rows, batch-sized head GEMMs) is bound by each
// CU's L2->LDS fill rate (about 45 GB/s for one workgroup); splitting K engages the idle CUs.  Measured (tools/gemm_bench.py,
// MJV_BENCH_TAILS=1): the second launch costs about 5 us, so K = 1024 / 2048 tails lose 1-5 us while K = 4096 / 8192 tails
// gain 12 / 25 us (45 -> 33, 89 -> 64): nk >= 64 only.
inline int gemm_slices128(const mjv_gemm_desc* d, int rows, int cus, const GemmTune& t) {
  if (!t.split_k || !d->workspace) return 1;
  const int tiles = ((rows + 127) / 128) * ((d->N + 127) / 128), nk = d->K / 64;
  if (tiles >= 2 * cus || nk < 64) return 1;
  const int sp = std::min({(2 * cus) / tiles, t.split_max, nk / 4});
  return (sp < 2 || (long)tiles * sp * 65536L > d->workspace_bytes) ? 1 : sp;
}
// 256-tiles, bf16: under-filled problems with deep K (K >= 4096: the ~1100-row tail of the language tower's w2, and the whole
// w2 of a single-video forward) - one workgroup per CU, at most one round; the 256 kernel's main loop moves 1.4-1.6x the flops
// per CU-second of the 128 kernel's, which pays for the fp32 round trip of the slices (1104 x 2048 x 8192 in 56 us against
// 64 us on sliced 128 tiles and 141 us on unsliced 256 tiles; 2186 rows: 83 against 145 us).  At K = 2048 it is a wash or a
// loss (wqkv tail 41 -> 44 us): not used.
inline int gemm_slices256(const mjv_gemm_desc* d, int rows, int cus, const GemmTune& t) {
  if (!t.split256 || d->tile || !d->workspace || d->out_rows) return 1;
  const int tm = (rows + 255) / 256, tiles = tm * ((d->N + 255) / 256), nk = d->K / 64;
  // (a last m-tile that is mostly empty wastes its share of every slice: 138 rows x 16384 columns ran 10 % slower sliced)
  const bool filled = (long)rows * 10 >= (long)tm * 256 * 7;
  if (rows <= t.skinny_max_m || d->N < 256 || nk < t.split256_min_nk || tiles * 2 > cus || !filled) return 1;
  const int sp = std::min({cus / tiles, t.split_max, nk / t.split256_min_kt});
  return (sp < 2 || (long)tiles * sp * 262144L > d->workspace_bytes) ? 1 : sp;
}
// 256-tiles, MXFP8 (K-tiles of 128): at least two K-tiles per slice (the pipeline's prologue fills two), at most 32 slices;
// below K = 1024 two launches cost more than the idle CUs.
inline int gemm_slices256f8(const mjv_gemm_desc* d, int rows, int cus) {
  const int nk = d->K / 128;
  if (!d->workspace || nk < 8) return 1;
  const int tiles = ((rows + 255) / 256) * ((d->N + 255) / 256);
  const int sp = std::min({cus / tiles, nk / 2, 32});
  return (sp < 2 || (long)tiles * sp * 262144L > d->workspace_bytes) ? 1 : sp;
}

// Persistent form of the 256-tile bf16 kernel (one workgroup per CU walks the tiles, next tile's first K-tile prefetched under
// the epilogue), plain or with a norm folded in: when the launch has more tiles than CUs and an even number (>= 4) of
// K-tiles.  Measured per epilogue (tools/gemm_bench.py 1000 / 1009 in one process): +1.4 ... +2.1 % for the plain-bias and SiLU
// epilogues; the LayerScale / residual epilogue loses 6-24 % - its 64 residual registers on top of the persistent loop's state
// spill - and the GELU epilogue 29 % - half the table gathers in flight per vote - so those keep the one-tile kernel, and so
// does the rotary epilogue.
inline bool gemm_persistent(int epilogue, int tiles, int nk, int cus) {
  return (epilogue == MJV_EPI_BIAS || epilogue == MJV_EPI_BIAS_RELU || epilogue == MJV_EPI_SILU_MUL) && tiles > cus && nk >= 4 && (nk & 1) == 0;
}

// The folded-norm instantiations of the unsliced 256-tile kernels, where the model uses them: a LayerNorm (2: row_scale +
// row_shift) into the ViT's qkv / fc1 (bias epilogues), an RMSNorm (1: row_scale only) into wqkv / w1|w3.  The small kernels and
// the K-sliced finish take every combination (store_frags).
constexpr int gemm_fuse_of(int epilogue) {
  return (epilogue == MJV_EPI_BIAS || epilogue == MJV_EPI_BIAS_GELU) ? 2 : (epilogue == MJV_EPI_SILU_MUL || epilogue == MJV_EPI_ROPE_QKV) ? 1 : 0;
}

inline const char* gemm_tag(bool fp8, int family, bool sliced, int epilogue) {
  static const char* const tags[7][6] = {
      {"gemm64_bias", "gemm64_bias_gelu", "gemm64_bias_relu", "gemm64_scale_res", "gemm64_silu_mul", ""},
      {"gemm128_bias", "gemm128_bias_gelu", "gemm128_bias_relu", "gemm128_scale_res", "gemm128_silu_mul", ""},
      {"gemm256_bias", "gemm256_bias_gelu", "gemm256_bias_relu", "gemm256_scale_res", "gemm256_silu_mul", "gemm256_rope_qkv"},
      {"gemm256s_bias", "gemm256s_bias_gelu", "gemm256s_bias_relu", "gemm256s_scale_res", "gemm256s_silu_mul", ""},
      {"gemm2_bias", "gemm2_bias_gelu", "", "gemm2_scale_res", "", ""},
      {"gemm256f8_bias", "gemm256f8_bias_gelu", "gemm256f8_bias_relu", "gemm256f8_scale_res", "gemm256f8_silu_mul", ""},
      {"gemm256f8s_bias", "gemm256f8s_bias_gelu", "gemm256f8s_bias_relu", "gemm256f8s_scale_res", "gemm256f8s_silu_mul", ""}};
  return tags[fp8 ? 5 + sliced : family == 64 ? 0 : family == 128 ? 1 : family == 2 ? 4 : 2 + sliced][epilogue];
}

inline GemmLaunch& gemm_plan_add(GemmPlan* p, const mjv_gemm_desc* d, bool fp8, int family, int epilogue, int row0, int rows, int split) {
  const int bm = family == 2 ? 128 : family, bn = family == 64 ? 32 : family == 2 ? 256 : family;
  const int tiles_m = (rows + bm - 1) / bm, tiles_n = (d->N + bn - 1) / bn;
  return p->l[p->n++] = GemmLaunch{family, epilogue, row0, rows, split, tiles_m, tiles_n, tiles_m * tiles_n * split, 0, 0, 0,
                                   gemm_tag(fp8, family, split > 1, epilogue), (double)rows / (double)d->M};
}

// rows [row0, row0 + rows) of a bf16 problem: the family, the slices, the rotary fallback, the 256-tile form
inline int gemm_plan_rows(GemmPlan* p, const mjv_gemm_desc* d, int cus, const GemmTune& t, int row0, int rows, bool use_big) {
  int split = gemm_slices256(d, rows, cus, t);
  if (split > 1) use_big = true;
  // skinny problems (peeled tails of a few dozen rows, batch-sized head layers): the 64 x 32 kernel.  (A 64 x 128 tile of it for the
  // language tower's ~1100-row tails measured 8 % slower than 128 x 128 with split-K: 3.67 vs 3.30 ms per step, residual GEMMs.)
  const bool skinny = !use_big && (d->tile ? d->tile == 64 : rows <= t.skinny_max_m);
  if (!use_big && !skinny) split = gemm_slices128(d, rows, cus, t);
  // the rotary epilogue needs a whole 256-column tile staged in LDS: only the unsliced 256^2 kernel has it.  Rows that run
  // on the other kernels (peeled tails, small problems) store the un-rotated Linear where that epilogue puts its result (v to C,
  // q / k heads to rope_q / rope_k) and the rotary step follows in place there: one contract for C whichever kernel runs a row.
  const bool rope_fallback = d->epilogue == MJV_EPI_ROPE_QKV && (!use_big || split > 1);
  const int epi = rope_fallback ? (int)MJV_EPI_BIAS : d->epilogue;
  GemmLaunch& L = gemm_plan_add(p, d, false, use_big ? 256 : skinny ? 64 : 128, epi, row0, rows, split);
  L.rope_split_after = rope_fallback;
  if (!use_big || split > 1) return MJV_OK;
  L.fuse = d->row_scale ? (d->row_shift ? 2 : 1) : 0;
  if (L.fuse && L.fuse != gemm_fuse_of(epi)) {
    mjv_set_error("gemm: the 256-tile kernel has no instantiation for epilogue %d with %s folded in (bias / bias+GELU take a "
                  "LayerNorm: row_scale + row_shift; SiLU-mul / RoPE-qkv an RMSNorm: row_scale only)", epi,
                  L.fuse == 2 ? "row_scale + row_shift" : "row_scale");
    return MJV_E_UNSUPPORTED;
  }
  L.persistent = gemm_persistent(epi, L.grid, d->K / 64, cus);
  // (bench build: the timing variants 3 / 4 / 6 and the A/B switch 9 are forms of the plain one-tile kernel)
  if (!L.fuse && (t.variant == 3 || t.variant == 4 || t.variant == 6 || t.variant == 9)) L.persistent = 0;
  if (L.persistent) L.grid = cus;
  return MJV_OK;
}

// MJV_OK and the plan, or the error code with mjv_last_error() set
inline int mjv_gemm_plan_build(const mjv_gemm_desc* d, int cus, const GemmTune& t, GemmPlan* p) {
  *p = GemmPlan{};
  const bool fp8 = d->a_format != MJV_FMT_BF16 || d->w_format != MJV_FMT_BF16;
  const double ops = (double)d->M * d->K + (double)d->N * d->K;
  p->flops = 2.0 * d->M * (double)d->N * d->K;
  if (fp8) {   // one kernel family (256 x 256), every epilogue on plain rows; scales counted as 3 % of the e4m3 bytes
    const bool out8 = d->c_format == MJV_FMT_MXFP8;
    p->bytes = 1.03 * ops + (out8 ? 1.03 : 2.0) * (double)d->M * gemm_out_cols(d);
    p->gm = pick_gm(d->N, d->K);
    p->nt_store = gemm_nt_store(d, out8 ? 1 : 2);
    const int m_main = gemm_peel_m_main(d, cus, true, true);
    if (m_main == d->M) {   // an under-filled launch as a whole (few rows: one video per forward) is sliced like a tail
      const int tiles = ((d->M + 255) / 256) * ((d->N + 255) / 256);
      gemm_plan_add(p, d, true, 256, d->epilogue, 0, d->M, (tiles * 2 <= cus && d->tile == 0) ? gemm_slices256f8(d, d->M, cus) : 1);
    } else {
      gemm_plan_add(p, d, true, 256, d->epilogue, 0, m_main, 1);
      gemm_plan_add(p, d, true, 256, d->epilogue, m_main, d->M - m_main, gemm_slices256f8(d, d->M - m_main, cus));
    }
    return MJV_OK;
  }
  if (d->epilogue < 0 || d->epilogue > MJV_EPI_ROPE_QKV) {
    mjv_set_error("gemm: unknown epilogue %d", d->epilogue);
    return MJV_E_ARG;
  }
  p->bytes = 2.0 * (ops + (double)d->M * gemm_out_cols(d));
  p->gm = t.gm > 0 ? t.gm : pick_gm(d->N, 2L * d->K);
  p->nt_store = t.nt >= 0 ? t.nt : gemm_nt_store(d, 2);
  if (d->tile == 2) {
    // tile 2: the 128 x 256 two-workgroups-per-CU kernel (short-K Linears; every row in ONE launch: its last m-tile may be partial)
    const bool t2_ok = (d->epilogue == MJV_EPI_BIAS || d->epilogue == MJV_EPI_BIAS_GELU || d->epilogue == MJV_EPI_SCALE_RES) && !d->out_rows &&
                       d->out_group <= 0 && d->res_mod <= 0 && !d->row_scale && (uintptr_t)d->C % 16 == 0 && d->ldc % 8 == 0 &&
                       (d->epilogue != MJV_EPI_SCALE_RES || (d->ldr % 8 == 0 && (uintptr_t)d->res % 16 == 0));
    if (!t2_ok) {
      mjv_set_error("gemm: tile 2 (128 x 256, two workgroups per CU) takes bias / bias + GELU / LayerScale + residual epilogues on plain, "
                    "16-byte aligned output rows");
      return MJV_E_UNSUPPORTED;
    }
    p->gm = t.gm > 0 ? t.gm : 8;
    gemm_plan_add(p, d, false, 2, d->epilogue, 0, d->M, 1);
    return MJV_OK;
  }
  const bool big = d->tile ? d->tile == 256 : (d->M >= 512 && d->N >= 256);
  const int m_main = gemm_peel_m_main(d, cus, false, big), rc = gemm_plan_rows(p, d, cus, t, 0, m_main, big);
  return (rc || m_main == d->M) ? rc : gemm_plan_rows(p, d, cus, t, m_main, d->M - m_main, false);
}
