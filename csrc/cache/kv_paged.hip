// Paged KV cache on gfx950 (CDNA4 / MI355X): bf16 K/V in pages of 64 tokens behind one block
// table, and the decode attention that reads them.
//
//   lsa_kvp_append          bf16 staging cells (slot[m], h, pos[m], :) -> the cell's page
//   lsa_kvp_gather          pages of [0, len) of the named slots -> the bf16 staging layer
//   lsa_attn_decode_paged   lsa_attn_decode (kernels/attention.hip, attn_body.h) over the pages
//
// Format (ops/kv_paged.py states it in torch). One layer holds kp, vp: bf16 [n_pages, n_kv, 64, hd];
// the engine holds one table: int32 [n_slots, t_max / 64]. Token t of slot s lives in page
// table[s][t / 64] at offset t % 64. Page 0 is the null page: no kernel writes it, so it stays zero;
// an entry outside [1, n_pages) counts as 0 in every kernel, so no table can address memory outside
// the pool. The kernels only read the table (plain loads); the host writes it.
//
// The attention is a copy of attn_body.h's attn_split_body (that header is a recorded input of the
// bf16 decode path's fixture and stays as it is) with one change: the K/V address of key t goes
// through the table. Lane map, chunking (chunk, k0, k1, nact), key order, online softmax, sc1
// partials, tickets and the last-arriver merge are the static kernel's, statement for statement, so
// the two agree bit for bit on equal cache contents. The launcher makes attention.hip's choice
// between the 4-wave split kernel and the 8-wave one-trip kernel.
//
// Table fetch: every lane loads the entry of its own key with a vector load, right before the K/V
// loads that need it. The KPW keys of one load instruction start at a multiple of KPW, which divides
// 64, so they lie in one page and the entry is wave-uniform - except for lanes past the chunk, which
// read the chunk's first key instead, as in the static body. Measured against it and left out
// (profiles/kv_paged.md): a scalar load per load instruction (wave id through readfirstlane, the
// entry of k0 kept for those lanes), 0.3-1.5 points slower on the batched shapes.
#include "../kernels/common.h"

#include <type_traits>

namespace {

constexpr int KVP_PAGE = 64;
constexpr int KVP_WAVES = 4;
constexpr int KVP_THR = KVP_WAVES * LSA_WAVE;
constexpr float KVP_NEG_BIG = -1e30f;
constexpr int KVP_MAX_SPLIT = 16;  // (the merge keeps one lse per split in VGPRs)
constexpr int KVP_SMALL_NW = 8, KVP_SMALL_U = 8;  // attention.hip's one-trip kernel

// a table entry as every kernel reads it: outside [1, n_pages) it is the null page
LSA_DEVICE int page_of(int e, int n_pages) { return (unsigned)e - 1u < (unsigned)(n_pages - 1) ? e : 0; }

// ------------------------------------------------------------------------------ append
// One group of hd / 8 lanes per vector (16 B per lane); item (m, h, which) = K (0) or V (1) vector
// of row m, kv-head h: lsa_kv8_append's item map.
template <int HD>
__global__ __launch_bounds__(256) void kvp_append_kernel(
    const bf16_raw* __restrict__ kst, const bf16_raw* __restrict__ vst, bf16_raw* __restrict__ kp,
    bf16_raw* __restrict__ vp, const int* __restrict__ table, const int* __restrict__ slot,
    const int* __restrict__ pos, int rows, int n_kv, int t_max, int n_slots, int n_pages) {
  constexpr int LPK = HD / 8;
  const int tid = threadIdx.x;
  const int li = tid % LPK;
  const long long item = (long long)blockIdx.x * (256 / LPK) + tid / LPK;
  const long long items = (long long)rows * n_kv * 2;
  if (item >= items) return;
  const int which = (int)(item & 1);
  const long long mh = item >> 1;
  const int m = (int)(mh / n_kv);
  const int h = (int)(mh - (long long)m * n_kv);
  const int sl = slot[m], p = pos[m];
  if (p < 0 || p >= t_max || sl < 0 || sl >= n_slots) return;  // the QKV epilogue skipped such a row too
  const int pg = page_of(table[(size_t)sl * (t_max / KVP_PAGE) + p / KVP_PAGE], n_pages);
  if (pg == 0) return;  // not reserved: nothing is written, the null page stays zero
  const size_t src = (((size_t)sl * n_kv + h) * (size_t)t_max + p) * HD + li * 8;
  const size_t dst = (((size_t)pg * n_kv + h) * KVP_PAGE + p % KVP_PAGE) * HD + li * 8;
  st16((which ? vp : kp) + dst, ld16((which ? vst : kst) + src));
}

// ------------------------------------------------------------------------------ gather
constexpr int KVP_MAX_JOBS = 256;
struct KvpJobs {
  int slot[KVP_MAX_JOBS];
  int len[KVP_MAX_JOBS];
};

// grid (key blocks, n_kv, jobs): positions [0, len) of one (slot, kv-head), hd / 8 lanes per key
template <int HD>
__global__ __launch_bounds__(256) void kvp_gather_kernel(
    const KvpJobs a, const bf16_raw* __restrict__ kp, const bf16_raw* __restrict__ vp,
    const int* __restrict__ table, bf16_raw* __restrict__ kst, bf16_raw* __restrict__ vst, int n_kv, int t_max,
    int n_pages) {
  constexpr int LPK = HD / 8;
  const int len = a.len[blockIdx.z];
  const int key = blockIdx.x * (256 / LPK) + threadIdx.x / LPK;
  if (key >= len) return;
  const int li = threadIdx.x % LPK;
  const int sl = a.slot[blockIdx.z];
  const int pg = page_of(table[(size_t)sl * (t_max / KVP_PAGE) + key / KVP_PAGE], n_pages);
  const size_t src = (((size_t)pg * n_kv + blockIdx.y) * KVP_PAGE + key % KVP_PAGE) * HD + li * 8;
  const size_t dst = (((size_t)sl * n_kv + blockIdx.y) * (size_t)t_max + key) * HD + li * 8;
  st16(kst + dst, ld16(kp + src));  // (a null entry reads the null page: zeros)
  st16(vst + dst, ld16(vp + src));
}

// ------------------------------------------------------------------------------ attention
// attn_body.h's attn_split_body with the K/V operand behind the table. U: key groups in flight per
// wave per iteration; NT: non-temporal K/V loads; SPLIT = false: nsplit == 1 guaranteed, no partial /
// merge code; NW: waves per workgroup.
template <int HD, int G, int U, int NT, bool SPLIT, int NW>
LSA_DEVICE void attn_paged_body(
    const bf16_raw* __restrict__ q, int ldq, const bf16_raw* __restrict__ kp, const bf16_raw* __restrict__ vp,
    const int* __restrict__ table, int n_pages, const int* __restrict__ slot, const int* __restrict__ pos,
    const int* __restrict__ kv_len, int n_heads, int n_kv, int t_max, float scale_log2, int nsplit, int min_chunk,
    float* __restrict__ part_o, float* __restrict__ part_lse, bf16_raw* __restrict__ out, int ldo,
    unsigned* __restrict__ counters, int split, int kvh, int row) {
  constexpr int LPK = HD / 8;          // lanes per key row (8 bf16 = 16 B per lane)
  constexpr int KPW = LSA_WAVE / LPK;  // keys per wave-instruction
  constexpr int KPI = KPW * NW;        // keys per workgroup iteration
  constexpr int NTHR = NW * LSA_WAVE;
  static_assert(KVP_PAGE % KPW == 0, "the keys of one load instruction lie in one page");

  __shared__ float s_m[NW][G];
  __shared__ float s_l[NW][G];
  __shared__ float s_o[NW][G][HD];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int grp = lane / LPK, li = lane % LPK;

  const int* lenp = kv_len ? kv_len : pos;
  const int slot_r = slot[row], len_r = lenp[row];
  asm volatile("" ::"s"(slot_r), "s"(len_r));
  const int* tb = table + (size_t)slot_r * (t_max / KVP_PAGE);  // the slot's table row
  const size_t pstride = (size_t)n_kv * KVP_PAGE * HD;          // elements per page
  const bf16_raw* kb = kp + (size_t)kvh * KVP_PAGE * HD + li * 8;
  const bf16_raw* vb = vp + (size_t)kvh * KVP_PAGE * HD + li * 8;
  int T = len_r + (kv_len ? 0 : 1);
  T = T > t_max ? t_max : T;  // never read past the table row
  int chunk = (T + nsplit - 1) / nsplit;
  chunk = chunk < min_chunk ? min_chunk : chunk;
  chunk = (chunk + KPI - 1) / KPI * KPI;
  const int k0 = split * chunk;
  const int k1 = min(T, k0 + chunk);
  // every split derives the same number of non-empty splits from T: empty ones exit at once
  // (no ticket), and a lone active split writes the final output itself (no merge)
  const int nact = (T + chunk - 1) / chunk;
  if (k0 >= k1) return;
  const size_t pbase = ((size_t)row * n_heads + (size_t)kvh * G) * nsplit + split;
  const __amdgpu_buffer_rsrc_t por = __builtin_amdgcn_make_buffer_rsrc(part_o, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t plr = __builtin_amdgcn_make_buffer_rsrc(part_lse, (short)0, 0x7fffffff, 0x00020000);
  const size_t pbase0 = pbase - split;  // split 0 of head 0 of this group
  // last-arriver merge of the nsplit partials of this (row, kv-head) group (sc1 loads)
  auto combine = [&]() {
    for (int e = tid; e < G * HD; e += NTHR) {
      const int r = e / HD, d = e - r * HD;
      const int hb = (int)(pbase0 + (size_t)r * nsplit);  // index of split 0 of head r
      float lse[KVP_MAX_SPLIT];
      float mm = -INFINITY;
#pragma unroll
      for (int sp = 0; sp < KVP_MAX_SPLIT; ++sp) {
        lse[sp] = sp < nact ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plr, (hb + sp) * 4, 0, 16))
                            : -INFINITY;
        mm = fmaxf(mm, lse[sp]);
      }
      float ws = 0.f, acc = 0.f;
#pragma unroll
      for (int sp = 0; sp < KVP_MAX_SPLIT; ++sp) {
        if (sp < nact) {
          const float wgt = __builtin_amdgcn_exp2f(lse[sp] - mm);
          ws += wgt;
          acc += wgt * __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(por, ((hb + sp) * HD + d) * 4, 0, 16));
        }
      }
      out[(size_t)row * ldo + (size_t)(kvh * G + r) * HD + d] = f2bf(acc / ws);
    }
  };
  // publish (every storing wave drained), take the ticket, merge if last
  auto arrive = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* cnt = counters + (size_t)row * n_kv + kvh;
    if (tid == 0) {
      const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = old == (unsigned)(nact - 1);
    }
    __syncthreads();
    if (!s_last) return;
    combine();
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };

  float mx[G], l[G], o[G][8];
#pragma unroll
  for (int r = 0; r < G; ++r) {
    mx[r] = KVP_NEG_BIG;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[r][j] = 0.f;
  }

  // A key past the chunk reads the chunk's first key instead (a written cell): its score is masked
  // below, and no cell at or beyond the row's length is ever touched. The key's page comes from the
  // slot's table row, one vector load per lane.
  auto load = [&](int base_, u32x4_t (&kr_)[U], u32x4_t (&vr_)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base_ + grp + u * KPI;
      const int kk = key < k1 ? key : k0;
      const int pg = page_of(tb[kk / KVP_PAGE], n_pages);
      const size_t off = (size_t)pg * pstride + (size_t)(kk % KVP_PAGE) * HD;
      if (NT) {
        kr_[u] = ld16_nt(kb + off);
        vr_[u] = ld16_nt(vb + off);
      } else {
        kr_[u] = ld16(kb + off);
        vr_[u] = ld16(vb + off);
      }
    }
  };
  u32x4_t kr[U], vr[U];
  const int first = k0 + w * KPW;
  // One-split grids: the first trip's K/V loads go out before q is requested (attn_body.h)
  if constexpr (!SPLIT) {
    if (first < k1) load(first, kr, vr);
    __builtin_amdgcn_sched_barrier(0);
  }

  float qf[G][8];
#pragma unroll
  for (int r = 0; r < G; ++r) {
    unpack8(ld16(q + (size_t)row * ldq + (size_t)(kvh * G + r) * HD + li * 8), qf[r]);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[r][j] *= scale_log2;
  }

  // loop bound is wave-uniform (the key groups of a wave shuffle only internally)
  for (int base = first; base < k1; base += KPI * U) {
    if (SPLIT || base != first) {  // (!SPLIT: the first trip was issued above)
      load(base, kr, vr);
    }
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) valid[u] = base + grp + u * KPI < k1;
    float s[G][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
#pragma unroll
      for (int r = 0; r < G; ++r) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += qf[r][j] * kf[j];
        d = group_sum<LPK>(d);  // the key's LPK lanes (DPP; common.h)
        s[r][u] = valid[u] ? d : KVP_NEG_BIG;
      }
    }
#pragma unroll
    for (int r = 0; r < G; ++r) {
      float bm = s[r][0];
#pragma unroll
      for (int u = 1; u < U; ++u) bm = fmaxf(bm, s[r][u]);
      const float mn = fmaxf(mx[r], bm);
      const float alpha = __builtin_amdgcn_exp2f(mx[r] - mn);
      mx[r] = mn;
      l[r] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[r][j] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = valid[u] ? __builtin_amdgcn_exp2f(s[r][u] - mn) : 0.f;
        l[r] += p;
        float vf[8];
        unpack8(vr[u], vf);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[r][j] += p * vf[j];
      }
    }
  }

  // merge the KPW key-groups of this wave (same li, different grp): lane ^ LPK ... ^ 32 on DPP /
  // permlane swaps (common.h lane_xor)
  auto merge_groups = [&](auto offc) {
    constexpr int OFF = decltype(offc)::value;
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const float mo = lane_xor<OFF>(mx[r]);
      const float lo = lane_xor<OFF>(l[r]);
      const float mn = fmaxf(mx[r], mo);
      const float a = __builtin_amdgcn_exp2f(mx[r] - mn), b = __builtin_amdgcn_exp2f(mo - mn);
      l[r] = l[r] * a + lo * b;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[r][j] = o[r][j] * a + lane_xor<OFF>(o[r][j]) * b;
      mx[r] = mn;
    }
  };
  static_assert(LPK == 8 || LPK == 16, "key lane groups");
  if constexpr (LPK == 8) merge_groups(std::integral_constant<int, 8>{});
  merge_groups(std::integral_constant<int, 16>{});
  merge_groups(std::integral_constant<int, 32>{});
  if (grp == 0) {
#pragma unroll
    for (int r = 0; r < G; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s_o[w][r][li * 8 + j] = o[r][j];
      if (li == 0) {
        s_m[w][r] = mx[r];
        s_l[w][r] = l[r];
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < G * HD; e += NTHR) {
    const int r = e / HD, d = e - r * HD;
    float mm = s_m[0][r];
#pragma unroll
    for (int i = 1; i < NW; ++i) mm = fmaxf(mm, s_m[i][r]);
    float ls = 0.f, os = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const float a = __builtin_amdgcn_exp2f(s_m[i][r] - mm);
      ls += s_l[i][r] * a;
      os += s_o[i][r][d] * a;
    }
    if (!SPLIT || nact == 1) {  // lone active split: final output directly, no merge
      out[(size_t)row * ldo + (size_t)(kvh * G + r) * HD + d] = f2bf(os / ls);
    } else {
      const int pi = (int)(pbase + (size_t)r * nsplit);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(os / ls), por, (pi * HD + d) * 4, 0, 16 /* sc1 */);
      if (d == 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mm + log2f(ls)), plr, pi * 4, 0, 16);
    }
  }
  if constexpr (SPLIT) {
    if (nact > 1) arrive();
  }
}

#define KVP_ATTN_PARAMS                                                                                          \
  const bf16_raw *__restrict__ q, int ldq, const bf16_raw *__restrict__ kp, const bf16_raw *__restrict__ vp,     \
      const int *__restrict__ table, int n_pages, const int *__restrict__ slot, const int *__restrict__ pos,     \
      const int *__restrict__ kv_len, int n_heads, int n_kv, int t_max, float scale_log2

// attention.hip's attn_split_kernel<HD, G, 4, 0, 1>: U 4, non-temporal loads
template <int HD, int G>
__global__ __launch_bounds__(KVP_THR) void attn_paged_split_kernel(KVP_ATTN_PARAMS, int nsplit, int min_chunk,
                                                                   float* __restrict__ part_o,
                                                                   float* __restrict__ part_lse,
                                                                   bf16_raw* __restrict__ out, int ldo,
                                                                   unsigned* __restrict__ counters) {
  attn_paged_body<HD, G, 4, 1, true, KVP_WAVES>(q, ldq, kp, vp, table, n_pages, slot, pos, kv_len, n_heads, n_kv, t_max,
                                                scale_log2, nsplit, min_chunk, part_o, part_lse, out, ldo, counters,
                                                blockIdx.x, blockIdx.y, blockIdx.z);
}

// attention.hip's attn_small_kernel: 8 waves x U 8, one split, one trip up to 256 keys
template <int HD, int G>
__global__ __launch_bounds__(KVP_SMALL_NW * LSA_WAVE) void attn_paged_small_kernel(KVP_ATTN_PARAMS,
                                                                                  bf16_raw* __restrict__ out,
                                                                                  int ldo) {
  attn_paged_body<HD, G, KVP_SMALL_U, 1, false, KVP_SMALL_NW>(q, ldq, kp, vp, table, n_pages, slot, pos, kv_len,
                                                             n_heads, n_kv, t_max, scale_log2, 1, 1, nullptr, nullptr,
                                                             out, ldo, nullptr, 0, blockIdx.y, blockIdx.z);
}

struct KvpAttnArgs {
  const bf16_raw *q, *kp, *vp;
  int ldq;
  const int *table, *slot, *pos, *kv_len;
  int n_pages, rows, n_heads, n_kv, t_max;
  float sl2;
  int nsplit, min_chunk, small_max_wgs;
  float *po, *pl;
  bf16_raw* out;
  int ldo;
  unsigned* cnt;
  hipStream_t s;
};

template <int HD, int G>
int kvp_launch(const KvpAttnArgs& a) {
  dim3 grid(a.nsplit, a.n_kv, a.rows);
  if constexpr (G <= 4) {  // (attention.hip: G 6 / 8 keep the 4-wave kernel)
    if (a.nsplit == 1 && a.rows * a.n_kv <= a.small_max_wgs) {
      attn_paged_small_kernel<HD, G><<<grid, KVP_SMALL_NW * LSA_WAVE, 0, a.s>>>(
          a.q, a.ldq, a.kp, a.vp, a.table, a.n_pages, a.slot, a.pos, a.kv_len, a.n_heads, a.n_kv, a.t_max, a.sl2,
          a.out, a.ldo);
      LSA_CHECK_LAUNCH();
      return LSA_OK;
    }
  }
  attn_paged_split_kernel<HD, G><<<grid, KVP_THR, 0, a.s>>>(
      a.q, a.ldq, a.kp, a.vp, a.table, a.n_pages, a.slot, a.pos, a.kv_len, a.n_heads, a.n_kv, a.t_max, a.sl2,
      a.nsplit, a.min_chunk, a.po, a.pl, a.out, a.ldo, a.cnt);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

template <int HD>
int kvp_dispatch(int g, const KvpAttnArgs& a) {
  switch (g) {
    case 1: return kvp_launch<HD, 1>(a);
    case 2: return kvp_launch<HD, 2>(a);
    case 3: return kvp_launch<HD, 3>(a);
    case 4: return kvp_launch<HD, 4>(a);
    case 6: return kvp_launch<HD, 6>(a);
    case 8: return kvp_launch<HD, 8>(a);
    default: return LSA_BAD_SHAPE;
  }
}

}  // namespace

// lsa_attn_decode over pages. small_max_wgs: rows * n_kv at or below which a one-split launch takes
// the 8-wave one-trip kernel (the value lsa_attn_set_small_max_wgs holds for the static kernel; 128).
// counters: rows * n_kv zero-initialised uint32 (only read when nsplit > 1; left zeroed).
extern "C" int lsa_attn_decode_paged(const void* q, int ldq, const void* kp, const void* vp, const int* table,
                                     int n_pages, const int* slot, const int* pos, const int* kv_len, int rows,
                                     int n_heads, int n_kv, int head_dim, int t_max, float scale, int nsplit,
                                     int min_chunk, int small_max_wgs, float* part_o, float* part_lse, void* out,
                                     int ldo, unsigned* counters, hipStream_t stream) {
  if (rows < 1 || n_kv < 1 || n_heads % n_kv || nsplit < 1 || nsplit > KVP_MAX_SPLIT || min_chunk < 1) return LSA_BAD_SHAPE;
  if (!q || !kp || !vp || !table || !slot || !pos || !out) return LSA_BAD_SHAPE;
  if (n_pages < 2 || t_max < KVP_PAGE || t_max % KVP_PAGE || small_max_wgs < 0) return LSA_BAD_SHAPE;
  if (nsplit > 1 && (!counters || !part_o || !part_lse)) return LSA_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return LSA_BAD_SHAPE;
  KvpAttnArgs a;
  a.q = static_cast<const bf16_raw*>(q);
  a.kp = static_cast<const bf16_raw*>(kp);
  a.vp = static_cast<const bf16_raw*>(vp);
  a.ldq = ldq;
  a.table = table;
  a.slot = slot;
  a.pos = pos;
  a.kv_len = kv_len;
  a.n_pages = n_pages;
  a.rows = rows;
  a.n_heads = n_heads;
  a.n_kv = n_kv;
  a.t_max = t_max;
  a.sl2 = scale * 1.4426950408889634f;
  a.nsplit = nsplit;
  a.min_chunk = min_chunk;
  a.small_max_wgs = small_max_wgs;
  a.po = part_o;
  a.pl = part_lse;
  a.out = static_cast<bf16_raw*>(out);
  a.ldo = ldo;
  a.cnt = counters;
  a.s = stream;
  const int g = n_heads / n_kv;
  return head_dim == 128 ? kvp_dispatch<128>(g, a) : kvp_dispatch<64>(g, a);
}

// Copy the K and V vectors that the QKV epilogue wrote into the bf16 staging layer at
// (slot[m], h, pos[m], :) into their pages. A row with pos outside [0, t_max), a slot outside
// [0, n_slots) or a null table entry writes nothing. Rows of one launch name distinct cells.
extern "C" int lsa_kvp_append(const void* k_stage, const void* v_stage, void* kp, void* vp, const int* table,
                              const int* slot, const int* pos, int rows, int n_slots, int n_kv, int head_dim,
                              int t_max, int n_pages, hipStream_t stream) {
  if (rows < 1 || n_slots < 1 || n_kv < 1 || n_pages < 2 || t_max < KVP_PAGE || t_max % KVP_PAGE) return LSA_BAD_SHAPE;
  if (!k_stage || !v_stage || !kp || !vp || !table || !slot || !pos) return LSA_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return LSA_BAD_SHAPE;
  const long long items = (long long)rows * n_kv * 2;
  const int per = 256 / (head_dim / 8);
  const long long grid = (items + per - 1) / per;
  if (grid >= (1ll << 31)) return LSA_BAD_SHAPE;
  const bf16_raw* kst = static_cast<const bf16_raw*>(k_stage);
  const bf16_raw* vst = static_cast<const bf16_raw*>(v_stage);
  bf16_raw* k = static_cast<bf16_raw*>(kp);
  bf16_raw* v = static_cast<bf16_raw*>(vp);
  if (head_dim == 128)
    kvp_append_kernel<128><<<(unsigned)grid, 256, 0, stream>>>(kst, vst, k, v, table, slot, pos, rows, n_kv, t_max, n_slots, n_pages);
  else
    kvp_append_kernel<64><<<(unsigned)grid, 256, 0, stream>>>(kst, vst, k, v, table, slot, pos, rows, n_kv, t_max, n_slots, n_pages);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// jobs: host array of n_jobs x [slot, len], read before the call returns. Positions [0, len) of every
// kv-head of each named slot are copied from their pages into the staging layer (zeros where the
// table entry is null); nothing else is written. Refused before any launch: a slot outside
// [0, n_slots), len outside [0, t_max]. len == 0 is a no-op.
extern "C" int lsa_kvp_gather(const void* kp, const void* vp, const int* table, void* k_stage, void* v_stage,
                              const int* jobs, int n_jobs, int n_slots, int n_kv, int head_dim, int t_max,
                              int n_pages, hipStream_t stream) {
  if (n_jobs < 0 || n_slots < 1 || n_kv < 1 || n_pages < 2 || t_max < KVP_PAGE || t_max % KVP_PAGE) return LSA_BAD_SHAPE;
  if (!k_stage || !v_stage || !kp || !vp || !table || (n_jobs > 0 && !jobs)) return LSA_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return LSA_BAD_SHAPE;
  for (int j = 0; j < n_jobs; ++j)
    if (jobs[2 * j] < 0 || jobs[2 * j] >= n_slots || jobs[2 * j + 1] < 0 || jobs[2 * j + 1] > t_max) return LSA_BAD_SHAPE;
  const int per = 256 / (head_dim / 8);
  const bf16_raw* k = static_cast<const bf16_raw*>(kp);
  const bf16_raw* v = static_cast<const bf16_raw*>(vp);
  bf16_raw* kst = static_cast<bf16_raw*>(k_stage);
  bf16_raw* vst = static_cast<bf16_raw*>(v_stage);
  int j = 0;
  while (j < n_jobs) {
    KvpJobs a = {};
    int n = 0, maxlen = 0;
    for (; j < n_jobs && n < KVP_MAX_JOBS; ++j) {
      if (jobs[2 * j + 1] == 0) continue;
      a.slot[n] = jobs[2 * j];
      a.len[n] = jobs[2 * j + 1];
      maxlen = a.len[n] > maxlen ? a.len[n] : maxlen;
      ++n;
    }
    if (n == 0) continue;
    dim3 grid((maxlen + per - 1) / per, n_kv, n);
    if (head_dim == 128)
      kvp_gather_kernel<128><<<grid, 256, 0, stream>>>(a, k, v, table, kst, vst, n_kv, t_max, n_pages);
    else
      kvp_gather_kernel<64><<<grid, 256, 0, stream>>>(a, k, v, table, kst, vst, n_kv, t_max, n_pages);
    LSA_CHECK_LAUNCH();
  }
  return LSA_OK;
}
