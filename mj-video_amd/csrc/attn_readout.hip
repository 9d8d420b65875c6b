// Attention readout (include/mjv.h, mjv_attention_readout_bf16): for a few already-rotated query rows, the softmax mass of every
// head that falls into caller-stated bins of key positions - fp32, the probabilities never rounded and never stored.
//
// Shape of the work: few queries, long keys, no values: memory-shaped.  One workgroup per (query, GT q-heads of one kv head);
// its 16 groups of 16 lanes take 16 contiguous chunks of the query's keys, a group covers one key row per step with one 16-byte
// load per lane (head_dim 96: 12 of the 16 lanes) and v_dot2_f32_bf16 products against the q chunks it keeps in registers, then
// a butterfly over the group's lanes.  Pass 1 finds the maximum score; pass 2 recomputes the same scores with the same
// instruction sequence (one function, no contraction across its roundings) and sums exp(s - m) per bin in a register, stored to
// the group's own LDS slot when the bin changes (a group meets every bin once: its keys ascend).  The 16 groups' slots are summed
// in group order, the bins in bin order: no atomics, no flags, equal bits run to run, and a query's bits depend on its own keys,
// ranges and bins alone.
#include "mjv_common.h"

namespace {
namespace ro {

constexpr int GROUPS = 16;        // lane groups per workgroup (4 waves x 4)
constexpr int MAX_BINS = 128;
constexpr int HDR = 8;            // plan header ints
constexpr int PLAN_MAGIC = 0x524f3031;   // "RO01"

// Plan (int32; the device reads a copy):
//   [0] magic  [1] n_queries  [2] n_ranges  [3] n_edges  [4] offset of the range table  [5] offset of the edges  [6] ints  [7] 0
//   query table at HDR, 4 ints per query: first range, range count, first edge, bin count
//   range table, 4 ints per range: tensor, first row, rows, key position of the range's first key within its query
//   edges: per query bin count + 1 ascending key positions
struct Args {
  const u16* Q;
  const u16* const* k_list;
  const int32_t* plan;
  float* mass;
  long ldq, ldk, ld_mass;
  int qhs, khs, n_heads, G;
  float scale;
};

template <int RM>
MJV_DEV float round_score(float a, float scale) {
  // mode 1: matmul rounded to bf16, then / sqrt(D) on the bf16 tensor; mode 2: fp32, never rounded (mjv_attention_bf16's modes).
  // __fmul_rn: the product is rounded where it stands in both passes (no fused multiply-subtract with the maximum)
  if constexpr (RM == 1) return rbf(__fmul_rn(rbf(a), scale));
  return __fmul_rn(a, scale);
}

// walks the keys [j0, j1) of one lane group in ascending order; f(j, s[GT]) sees every key's scores (equal in the group's lanes).
// UNROLL key rows are fetched before the first is used: the walk is a chain of dependent loads otherwise (one row in flight per
// group); the order in which f sees the keys, and so every sum, is that of the plain walk
constexpr int UNROLL = 8;
template <int D, int GT, int RM, class F>
MJV_DEV void walk_keys(const Args& a, const int32_t* ranges, int n_ranges, int kvh, int c, const u32x4 (&q)[GT], int j0, int j1, F&& f) {
  constexpr int CHUNKS = D / 8;
  int r = 0, r_first = 0, r_end = 0;   // range r holds key positions [r_first, r_end)
  const u16* base = nullptr;
  long row0 = 0;
  for (int jb = j0; jb < j1; jb += UNROLL) {
    // the rows' addresses first (the range table is read here), then the loads back to back: a load behind a table read would
    // wait for every load before it
    const u16* row[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = jb + u;
      row[u] = nullptr;
      if (j < j1) {                          // (equal in the group's 16 lanes)
        while (j >= r_end && r < n_ranges) {   // (the host checked: the ranges' rows sum to the key count, so j < j1 finds its range)
          const int32_t* e = ranges + 4 * r;
          r_first = e[3];
          r_end = r_first + e[2];
          row0 = e[1];
          base = a.k_list[e[0]];
          ++r;
        }
        row[u] = base + (row0 + (j - r_first)) * a.ldk + (long)kvh * a.khs + c * 8;
      }
    }
    u32x4 kc[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      kc[u] = u32x4{0u, 0u, 0u, 0u};
      if (jb + u < j1 && c < CHUNKS) kc[u] = *(const u32x4*)row[u];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int j = jb + u;
      if (j < j1) {
        float s[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            // (the pairs through scalars: __builtin_bit_cast of a vector ELEMENT expression reads element 0 whatever the index)
            const unsigned qp = q[g][i], kp = kc[u][i];
            acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, qp), __builtin_bit_cast(bf16x2, kp), acc, false);
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);   // within the 16 lanes: every lane ends with the same bits
          s[g] = round_score<RM>(acc, a.scale);
        }
        f(j, s);
      }
    }
  }
}

template <int D, int GT, int RM>
__global__ __launch_bounds__(256) void attn_readout_kernel(Args a) {
  __shared__ float slot[GROUPS][GT][MAX_BINS];   // a group's bin sums
  __shared__ float gmax[GROUPS][GT];
  __shared__ float bins[GT][MAX_BINS];
  const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
  const int hb = a.n_heads / GT;                 // workgroups per query
  const int qi = blockIdx.x / hb, h0 = (blockIdx.x % hb) * GT, kvh = h0 / a.G;
  const int32_t* plan = a.plan;
  const int32_t* qe = plan + HDR + 4 * qi;
  const int n_ranges = qe[1], nb = qe[3];
  const int32_t* ranges = plan + plan[4] + 4 * qe[0];
  const int32_t* edges = plan + plan[5] + qe[2];
  const int L = edges[nb];
  const int chunk = (L + GROUPS - 1) / GROUPS;
  const int j0 = min(L, grp * chunk), j1 = min(L, j0 + chunk);

  u32x4 q[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    q[g] = u32x4{0u, 0u, 0u, 0u};
    if (c < D / 8) q[g] = *(const u32x4*)(a.Q + (long)qi * a.ldq + (long)(h0 + g) * a.qhs + c * 8);
  }
  for (int i = tid; i < GROUPS * GT * MAX_BINS; i += 256) (&slot[0][0][0])[i] = 0.f;

  // pass 1: the maximum
  float m[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) m[g] = -INFINITY;
  walk_keys<D, GT, RM>(a, ranges, n_ranges, kvh, c, q, j0, j1, [&](int, const float (&s)[GT]) {
#pragma unroll
    for (int g = 0; g < GT; ++g) m[g] = fmaxf(m[g], s[g]);
  });
  if (c == 0) {
#pragma unroll
    for (int g = 0; g < GT; ++g) gmax[grp][g] = m[g];
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    float v = gmax[0][g];
    for (int i = 1; i < GROUPS; ++i) v = fmaxf(v, gmax[i][g]);
    m[g] = v;
  }

  // pass 2: the same scores again, exp(s - m) summed per bin
  constexpr float LOG2E = 1.4426950408889634f;
  int b = 0;            // the bin of the group's current key: edges[b] <= j < edges[b + 1]
  float acc[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) acc[g] = 0.f;
  walk_keys<D, GT, RM>(a, ranges, n_ranges, kvh, c, q, j0, j1, [&](int j, const float (&s)[GT]) {
    if (j >= edges[b + 1]) {
      if (c == 0) {
#pragma unroll
        for (int g = 0; g < GT; ++g) slot[grp][g][b] = acc[g];
      }
#pragma unroll
      for (int g = 0; g < GT; ++g) acc[g] = 0.f;
      while (j >= edges[b + 1]) ++b;   // (the last edge is L > j)
    }
#pragma unroll
    for (int g = 0; g < GT; ++g) acc[g] += __builtin_amdgcn_exp2f(__fmul_rn(s[g] - m[g], LOG2E));
  });
  if (c == 0 && j1 > j0) {
#pragma unroll
    for (int g = 0; g < GT; ++g) slot[grp][g][b] = acc[g];
  }
  __syncthreads();
  // merge: the groups in group order, then the bins in bin order
  for (int i = tid; i < GT * MAX_BINS; i += 256) {
    const int g = i / MAX_BINS, bb = i % MAX_BINS;
    float v = slot[0][g][bb];
    for (int w = 1; w < GROUPS; ++w) v += slot[w][g][bb];
    bins[g][bb] = v;
  }
  __syncthreads();
  const int ldm = (int)a.ld_mass;
  for (int i = tid; i < GT * ldm; i += 256) {
    const int g = i / ldm, bb = i % ldm;
    float out = 0.f;
    if (bb < nb) {
      float total = bins[g][0];
      for (int k = 1; k < nb; ++k) total += bins[g][k];
      out = bins[g][bb] / total;
    }
    a.mass[((long)qi * a.n_heads + h0 + g) * a.ld_mass + bb] = out;
  }
}

struct Info {
  long ints, n_ranges, n_edges, keys;
};

// every check that needs the HOST arrays and sizes only; plan != nullptr: writes the plan
int plan_build(const mjv_attn_readout_desc* d, int32_t* plan, Info* info) {
  MJV_REQUIRE(d, "attention_readout: null descriptor");
  if (d->head_dim != 128 && d->head_dim != 96) {
    mjv_set_error("attention_readout: head_dim %d is not built (128 and 96 are)", d->head_dim);
    return MJV_E_UNSUPPORTED;
  }
  MJV_REQUIRE(d->score_round_mode == 1 || d->score_round_mode == 2, "attention_readout: score_round_mode %d not in {1, 2}", d->score_round_mode);
  MJV_REQUIRE(d->n_queries > 0 && d->n_heads > 0 && d->kv_group > 0 && d->n_heads % d->kv_group == 0,
              "attention_readout: n_queries %d, n_heads %d, kv_group %d", d->n_queries, d->n_heads, d->kv_group);
  MJV_REQUIRE(d->cu_range && d->range_tensor && d->range_row0 && d->range_rows && d->cu_bin && d->bin_edge,
              "attention_readout: null index array (cu_range, range_tensor, range_row0, range_rows, cu_bin, bin_edge are HOST arrays)");
  MJV_REQUIRE(d->n_tensors > 0, "attention_readout: n_tensors %d", d->n_tensors);
  MJV_REQUIRE(d->cu_range[0] == 0 && d->cu_bin[0] == 0, "attention_readout: cu_range[0] and cu_bin[0] must be 0");
  const int nq = d->n_queries;
  long keys_all = 0;
  for (int q = 0; q < nq; ++q) {
    const long r0 = d->cu_range[q], r1 = d->cu_range[q + 1];
    MJV_REQUIRE(r1 > r0, "attention_readout: query %d has no key range", q);
    long keys = 0;
    for (long r = r0; r < r1; ++r) {
      MJV_REQUIRE(d->range_tensor[r] >= 0 && d->range_tensor[r] < d->n_tensors, "attention_readout: range %ld (query %d): range_tensor %d not in [0, %d)",
                  r, q, d->range_tensor[r], d->n_tensors);
      MJV_REQUIRE(d->range_rows[r] > 0, "attention_readout: range %ld (query %d): range_rows %d (a range holds at least one row)", r, q,
                  d->range_rows[r]);
      MJV_REQUIRE(d->range_row0[r] >= 0 && (long)d->range_row0[r] + d->range_rows[r] <= 0x7fffffffL,
                  "attention_readout: range %ld (query %d): range_row0 %d", r, q, d->range_row0[r]);
      keys += d->range_rows[r];
    }
    MJV_REQUIRE(keys <= 0x7fffffffL, "attention_readout: query %d has %ld keys", q, keys);
    const long e0 = d->cu_bin[q], e1 = d->cu_bin[q + 1];   // edges [e0, e1): bins + 1
    const long nb = e1 - e0 - 1;
    MJV_REQUIRE(nb >= 1 && nb <= ro::MAX_BINS, "attention_readout: query %d has %ld bins (1 to %d; cu_bin counts bins + 1 edges)", q, nb, ro::MAX_BINS);
    MJV_REQUIRE(d->bin_edge[e0] == 0, "attention_readout: query %d: first bin edge %d, must be 0", q, d->bin_edge[e0]);
    for (long e = e0 + 1; e < e1; ++e)
      MJV_REQUIRE(d->bin_edge[e] >= d->bin_edge[e - 1], "attention_readout: query %d: bin edges not ascending (%d after %d)", q, d->bin_edge[e],
                  d->bin_edge[e - 1]);
    MJV_REQUIRE(d->bin_edge[e1 - 1] == keys, "attention_readout: query %d: last bin edge %d differs from its key count %ld", q, d->bin_edge[e1 - 1], keys);
    keys_all += keys;
  }
  const long n_ranges = d->cu_range[nq], n_edges = d->cu_bin[nq];
  const long off_r = HDR + 4L * nq, off_e = off_r + 4 * n_ranges, ints = off_e + n_edges;
  MJV_REQUIRE(ints <= 0x7fffffffL, "attention_readout: plan of %ld ints", ints);
  info->ints = ints; info->n_ranges = n_ranges; info->n_edges = n_edges; info->keys = keys_all;
  if (!plan) return MJV_OK;
  plan[0] = PLAN_MAGIC; plan[1] = nq; plan[2] = (int32_t)n_ranges; plan[3] = (int32_t)n_edges;
  plan[4] = (int32_t)off_r; plan[5] = (int32_t)off_e; plan[6] = (int32_t)ints; plan[7] = 0;
  for (int q = 0; q < nq; ++q) {
    int32_t* qe = plan + HDR + 4 * q;
    qe[0] = d->cu_range[q]; qe[1] = d->cu_range[q + 1] - d->cu_range[q];
    qe[2] = d->cu_bin[q]; qe[3] = d->cu_bin[q + 1] - d->cu_bin[q] - 1;
    int32_t pos = 0;
    for (long r = d->cu_range[q]; r < d->cu_range[q + 1]; ++r) {
      int32_t* re = plan + off_r + 4 * r;
      re[0] = d->range_tensor[r]; re[1] = d->range_row0[r]; re[2] = d->range_rows[r]; re[3] = pos;
      pos += d->range_rows[r];
    }
  }
  for (long e = 0; e < n_edges; ++e) plan[off_e + e] = d->bin_edge[e];
  return MJV_OK;
}

template <int D, int RM>
void launch(const Args& a, int n_queries, hipStream_t s) {
  if (a.G % 2 == 0) hipLaunchKernelGGL((attn_readout_kernel<D, 2, RM>), dim3((unsigned)(n_queries * (a.n_heads / 2))), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_readout_kernel<D, 1, RM>), dim3((unsigned)(n_queries * a.n_heads)), dim3(256), 0, s, a);
}

}  // namespace ro
}  // namespace

extern "C" int64_t mjv_attention_readout_plan(const mjv_attn_readout_desc* d, int32_t* plan_host, int64_t plan_ints) {
  ro::Info info;
  const int rc = ro::plan_build(d, nullptr, &info);
  if (rc != MJV_OK) return rc;
  if (!plan_host) return info.ints;
  if (plan_ints < info.ints) {
    mjv_set_error("attention_readout_plan: the plan needs %ld ints, the buffer holds %ld", (long)info.ints, (long)plan_ints);
    return MJV_E_ARG;
  }
  const int rc2 = ro::plan_build(d, plan_host, &info);
  return rc2 != MJV_OK ? rc2 : info.ints;
}

extern "C" int mjv_attention_readout_bf16(const mjv_attn_readout_desc* d, void* stream) {
  ro::Info info;
  const int rc = ro::plan_build(d, nullptr, &info);
  if (rc != MJV_OK) return rc;
  MJV_REQUIRE(d->Q && d->k_list && d->mass, "attention_readout: null pointer (Q, k_list, mass)");
  MJV_REQUIRE(d->ldq % 8 == 0 && d->ldk % 8 == 0 && d->q_head_stride % 8 == 0 && d->k_head_stride % 8 == 0 && d->ldq > 0 && d->ldk > 0,
              "attention_readout: ldq / ldk / head strides must be multiples of 8 elements");
  MJV_REQUIRE((uintptr_t)d->Q % 16 == 0 && (uintptr_t)d->k_list % 8 == 0 && (uintptr_t)d->mass % 4 == 0, "attention_readout: misaligned pointer");
  MJV_REQUIRE(d->ld_mass >= 1 && d->ld_mass <= 0x7fffffffL / 2, "attention_readout: ld_mass %ld", (long)d->ld_mass);
  for (int q = 0; q < d->n_queries; ++q)
    MJV_REQUIRE(d->cu_bin[q + 1] - d->cu_bin[q] - 1 <= d->ld_mass, "attention_readout: query %d has %d bins, ld_mass is %ld", q,
                d->cu_bin[q + 1] - d->cu_bin[q] - 1, (long)d->ld_mass);
  MJV_REQUIRE(d->plan && d->plan_ints >= info.ints, "attention_readout: missing or short plan (%ld ints given, %ld needed: mjv_attention_readout_plan)",
              (long)(d->plan ? d->plan_ints : 0), (long)info.ints);
  ro::Args a;
  a.Q = d->Q; a.k_list = (const u16* const*)d->k_list; a.plan = d->plan; a.mass = d->mass;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ld_mass = d->ld_mass;
  a.qhs = d->q_head_stride; a.khs = d->k_head_stride; a.n_heads = d->n_heads; a.G = d->kv_group;
  a.scale = d->scale;
  hipStream_t s = (hipStream_t)stream;
  // two passes over every key row of a kv head (the kv_group q-heads of a workgroup pair share it), two flops per product
  const double n_kv = (double)d->n_heads / d->kv_group;
  const double flops = 4.0 * d->head_dim * (double)info.keys * d->n_heads;
  const double bytes = 2.0 * 2.0 * d->head_dim * (double)info.keys * n_kv * (d->kv_group % 2 == 0 ? d->kv_group / 2 : d->kv_group);
  if (d->head_dim == 128) {
    MjvProfScope ps("attn_readout_d128", s, flops, bytes);
    if (d->score_round_mode == 2) ro::launch<128, 2>(a, d->n_queries, s);
    else ro::launch<128, 1>(a, d->n_queries, s);
    return mjv_check_launch("attention_readout");
  }
  MjvProfScope ps("attn_readout_d96", s, flops, bytes);
  if (d->score_round_mode == 2) ro::launch<96, 2>(a, d->n_queries, s);
  else ro::launch<96, 1>(a, d->n_queries, s);
  return mjv_check_launch("attention_readout");
}
