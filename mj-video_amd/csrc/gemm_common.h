// Device helpers shared by the GEMM sources (gemm.hip, gemm_fp8.hip) and the bench build's un-fused epilogue pass
// (rowops.hip): the table GELU, SiLU, the streaming output stores, the XCD-aware tile order, the 256-tile operand
// staging, the scheduling-fenced barrier.
#pragma once
#include "mjv_common.h"
#include "gelu_table.h"

namespace {

// exact-erf GELU on bf16 as a finite function (tools/gen_gelu_table.py): bit-identical to torch's CPU bf16 GELU.
// (one copy per translation unit that includes this header: no -fgpu-rdc)
__device__ const u16 g_gelu_table[MJV_GELU_TABLE_LEN] = MJV_GELU_TABLE_INIT;

// x given as an fp32 value that is exactly representable in bf16; tab = table in LDS or global memory.
// Branch-free on purpose (selects only): a divergent version costs ~3x more than the table read it guards.
MJV_DEV float gelu_lut(float xf, const u16* tab) {
  const unsigned u = __float_as_uint(xf);
  const unsigned mag = (u >> 16) & 0x7fffu;
  const unsigned rel = mag - MJV_GELU_LO;                       // wraps to a huge value below the table
  const unsigned sgn = (unsigned)((int)u >> 31);                // all ones for x < 0
  const bool in_tab = rel < (unsigned)MJV_GELU_R;
  const unsigned idx = in_tab ? rel + (sgn & MJV_GELU_NEG_OFF) : 0u;
  const unsigned t = tab[idx];
  const unsigned big = gelu_beyond_table(u, mag);               // beyond the table (mjv_common.h)
  const unsigned small = __float_as_uint(0.5f * xf);            // below the table: x / 2
  const unsigned other = mag < MJV_GELU_LO ? small : big;
  return __uint_as_float(in_tab ? (t << 16) : other);
}

// The split table of the 256-tile GELU epilogues: the two sign halves sit 64 KiB apart in LDS - x > 0 at byte 0, x < 0 at
// byte GELU_SPLIT_NEG - so that the gather address is the rounded value's own bit pattern, (fp32 bits >> 15) - 2 LO =
// GELU_SPLIT_NEG sign + 2 (magnitude - LO).
constexpr int GELU_SPLIT_NEG = 65536;
// general form of the table GELU on the split table (gelu_lut's logic; lds = LDS base)
MJV_DEV float gelu_lut_split(float xf, const char* lds) {
  const unsigned u = __float_as_uint(xf);
  const unsigned mag = (u >> 16) & 0x7fffu;
  const unsigned rel = mag - MJV_GELU_LO;
  const unsigned sgn = (unsigned)((int)u >> 31);
  const bool in_tab = rel < (unsigned)MJV_GELU_R;
  const unsigned t = *(const u16*)(lds + (sgn & GELU_SPLIT_NEG) + (in_tab ? rel * 2 : 0u));
  const unsigned big = gelu_beyond_table(u, mag);               // beyond the table (mjv_common.h)
  const unsigned small = __float_as_uint(0.5f * xf);
  const unsigned other = mag < MJV_GELU_LO ? small : big;
  return __uint_as_float(in_tab ? (t << 16) : other);
}

// x * rcp(1 + e^-x): v_rcp_f32 (1 ulp) instead of the 10-instruction IEEE division; the result is rounded to bf16 next, and
// e^-x is a 1-2 ulp v_exp_f32 already, so the quotient's last fp32 bit carries no information the reference shares
MJV_DEV float silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// 16-byte / 8-byte output store, streaming (nt) on request.  The nt form is inline assembly: written as `if (nt)
// __builtin_nontemporal_store(...) else plain store`, hipcc (ROCm 7.2) merges the two arms into ONE plain store and the hint is
// gone (the kernels of rounds 1-3 contained no nt store at all - found in round 4 by reading the ISA).  Counted in vmcnt like
// any store; nothing ever waits for it.
MJV_DEV void store16(u16* dst, const u32x4& val, int nt) {
  if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(val) : "memory");
  else *(u32x4*)dst = val;
}
MJV_DEV void store8(uint8_t* dst, const u32x2& val, int nt) {
  if (nt) asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(dst), "v"(val) : "memory");
  else *(u32x2*)dst = val;
}

// XCD-aware tile order: tile (tm, tn) of the b-th of nwg workgroups.  Blocks b and b+8 share an XCD (round-robin dispatch),
// so every XCD gets a contiguous range of a tile list that is itself ordered in groups of gm m-tiles x all n-tiles, n-major
// inside a group: the ~32 tiles an XCD runs concurrently then form a gm x (32/gm) patch that shares gm activation panels and
// 32/gm weight panels through that XCD's 4 MiB L2 (row-major order shares 1 + 32 panels: the whole weight matrix was
// re-fetched over the fabric once per m-tile row - rocprofv3 FETCH_SIZE 4.7 GB per w1|w3 launch for 139 MB of operands).
MJV_DEV void xcd_tile_order(const int GM, const int tiles_m, const int tiles_n, const int nwg, const int b, int& tm, int& tn) {
  const int q = nwg >> 3, r8 = nwg & 7, xcd = b & 7;
  const int t = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (b >> 3);
  const int per_group = GM * tiles_n;
  const int grp = t / per_group, in_grp = t - grp * per_group;
  const int first_m = grp * GM;
  const int gsz = min(tiles_m - first_m, GM);
  tn = in_grp / gsz;
  tm = first_m + (in_grp - tn * gsz);
}

// The 256-tile kernels' operand staging (bf16: T = u16, MXFP8: T = uint8_t; a K-tile is 128 bytes of a row either way):
// per-lane global source pointers of the two 1-KiB DMA pieces a wave issues for each of the four half-tiles (W rows 0-127,
// W rows 128-255, A rows 0-127, A rows 128-255) at k = 0: the row clamp and the chunk swizzle are loop invariant, so a stage is
// two {pointer + k offset, global_load_lds} pairs - the DMA issue sits in the load segment that has to hide under the partner
// wave's 16-MFMA segment.  (stage_half itself stays with each kernel: issued through a shared template, one m0 setup of the
// main loops came out as two instructions.)
template <class T>
struct HalfTilePtrs {
  const T* src[4][2];
};
template <class T, class Args>
MJV_DEV void init_stage_ptrs(HalfTilePtrs<T>& sp, const Args& p, int m0, int n0, int wave, int lane) {
#pragma unroll
  for (int which = 0; which < 4; ++which) {
    const bool is_w = which < 2;
    const T* base = is_w ? p.W : p.A;
    const long ld = is_w ? p.ldw : p.lda;
    const int row0 = (is_w ? n0 : m0) + (which & 1) * 128;
    const int max_row = (is_w ? p.N : p.M) - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (wave * 2 + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ (r & 7);
      int gr = row0 + r;
      gr = gr < max_row ? gr : max_row;
      sp.src[which][i] = base + (long)gr * ld + c * (16 / (int)sizeof(T));
    }
  }
}

}  // namespace

// s_barrier the compiler schedules nothing across
#define MJV_BARRIER()                      \
  do {                                     \
    __builtin_amdgcn_sched_barrier(0);     \
    __builtin_amdgcn_s_barrier();          \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)
