// FP8 KV cache on gfx950 (CDNA4 / MI355X): OCP e4m3fn K/V codes with one power-of-two fp32 scale
// per cached vector, and the split-KV decode attention that reads them.
//
//   lsa_kv8_append        bf16 staging cells (slot[m], h, pos[m], :) -> codes + scales, same cell
//   lsa_kv8_dequant       codes + scales of [0, len) of the named slots -> the bf16 staging layer
//   lsa_attn_decode_kv8   lsa_attn_decode (kernels/attention.hip, attn_body.h) over k8 / v8 / ks / vs
//   lsa_attn_kv8_kpi      keys per workgroup iteration of the kernel a shape launches (chunk edges)
//
// Format (ops/kv8.py states it in torch). One layer holds k8, v8: uint8 [slots, n_kv, t_max, hd] and
// ks, vs: fp32 [slots, n_kv, t_max]. For a vector x of hd finite bf16 values: a = max |x_d|;
// a == 0 -> s = 1, else E = the fp32 exponent field of a, clamped to >= 8 (s and 1/s stay fp32
// normals), s = 2^(E - 127 - 7); code_d = e4m3_rne(fp32(x_d) * (1 / s)). |x_d / s| < 256, so no code
// saturates and the NaN code never appears; the multiply by a power of two is exact, the
// conversion is the only rounding. Dequantisation is bf16(code_d * s).
//
// The attention is attn_body.h's flash-decoding with the K/V operand changed: row m attends keys
// [0, pos + 1) (or [0, kv_len[m])) clamped to t_max; one workgroup streams one chunk for the whole
// GQA group with non-temporal loads; scores are scale * ks[t] * (q . code_t), outputs
// sum p_t * vs[t] * code_t / sum p_t, fp32 in the exp2 domain; codes are converted in registers
// (v_cvt_pk_f32_fp8) and each key's scale is applied once to the dot product / to p, never per
// element. nsplit > 1: sc1 partials, an arrival ticket per (row, kv-head), last-arriver merge in
// split order, counters left zeroed (graph-replay safe); empty splits exit; a lone split writes
// the output directly. A lane loads 8 codes (8 bytes) per key, HD / 8 lanes per key: the bf16
// kernel's lane map. Measured and left out (profiles/kv8.md): 16 codes per lane (16-byte loads;
// +0.6 % at 512 x 2048, -5 % at 512 x 143, and 256 VGPRs from G = 3 up), and attention.hip's 8-wave
// one-trip kernel for rows * n_kv <= 128 with one split (5.44 us against this kernel's 4.71 us at
// 1 x 128 keys of the 7B shape, with K/V resident in the Infinity Cache: not compared on cold K/V).
#include "../kernels/common.h"

#include <type_traits>

namespace {

constexpr int KV8_WAVES = 4;
constexpr int KV8_THR = KV8_WAVES * LSA_WAVE;
constexpr float KV8_NEG_BIG = -1e30f;
constexpr int KV8_MAX_SPLIT = 16;  // (the merge keeps one lse per split in VGPRs)

template <int W>
LSA_DEVICE float group_max(float v) {
  static_assert(W == 8 || W == 16, "DPP row groups");
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  if constexpr (W == 16) v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}

// 4 e4m3 codes of one dword -> fp32
LSA_DEVICE void cvt4(unsigned w, float* f) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}
// 4 fp32 -> one dword of e4m3 codes (round to nearest even)
LSA_DEVICE unsigned pack4(const float* y) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  return (unsigned)w;
}

constexpr int CPL = 8;  // codes per lane per load
LSA_DEVICE u32x2_t ld_codes_nt(const unsigned char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
}
LSA_DEVICE void unpack_codes(u32x2_t v, float* f) {
  cvt4(v[0], f);
  cvt4(v[1], f + 4);
}

// ------------------------------------------------------------------------------ append
// One group of hd / 8 lanes per vector (16 B of bf16 in, 8 B of codes out per lane); item
// (m, h, which) = K (0) or V (1) vector of row m, kv-head h.
template <int HD>
__global__ __launch_bounds__(256) void kv8_append_kernel(
    const bf16_raw* __restrict__ kst, const bf16_raw* __restrict__ vst, unsigned char* __restrict__ k8,
    unsigned char* __restrict__ v8, float* __restrict__ ks, float* __restrict__ vs,
    const int* __restrict__ slot, const int* __restrict__ pos, int rows, int n_kv, int t_max, int n_slots) {
  constexpr int LPK = HD / 8;
  const int tid = threadIdx.x;
  const int li = tid % LPK;
  const long long item = (long long)blockIdx.x * (256 / LPK) + tid / LPK;
  const long long items = (long long)rows * n_kv * 2;
  bool ok = item < items;
  int m = 0, h = 0, which = 0, sl = 0, p = 0;
  if (ok) {
    which = (int)(item & 1);
    const long long mh = item >> 1;
    m = (int)(mh / n_kv);
    h = (int)(mh - (long long)m * n_kv);
    sl = slot[m];
    p = pos[m];
    ok = p >= 0 && p < t_max && sl >= 0 && sl < n_slots;  // the QKV epilogue skipped such a row too
  }
  const size_t cell = ok ? ((size_t)sl * n_kv + h) * (size_t)t_max + p : 0;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = 0.f;
  if (ok) unpack8(ld16((which ? vst : kst) + cell * HD + li * 8), x);
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(x[j]));
  a = group_max<LPK>(a);
  int e = (int)(__float_as_uint(a) >> 23);
  e = (e < 8 ? 8 : e) - 7;
  if (a == 0.f) e = 127;
  const float s = __uint_as_float((unsigned)e << 23);
  const float inv = __uint_as_float((unsigned)(254 - e) << 23);
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = x[j] * inv;
  u32x2_t c;
  c[0] = pack4(y);
  c[1] = pack4(y + 4);
  if (ok) {
    *reinterpret_cast<u32x2_t*>((which ? v8 : k8) + cell * HD + li * 8) = c;
    if (li == 0) (which ? vs : ks)[cell] = s;
  }
}

// ------------------------------------------------------------------------------ dequant
constexpr int KV8_DQ_MAX_JOBS = 256;
struct Kv8DqArgs {
  int slot[KV8_DQ_MAX_JOBS];
  int len[KV8_DQ_MAX_JOBS];
};

// grid (key blocks, n_kv, jobs): positions [0, len) of one (slot, kv-head), hd / 8 lanes per key
template <int HD>
__global__ __launch_bounds__(256) void kv8_dequant_kernel(
    const Kv8DqArgs a, const unsigned char* __restrict__ k8, const unsigned char* __restrict__ v8,
    const float* __restrict__ ks, const float* __restrict__ vs, bf16_raw* __restrict__ kst,
    bf16_raw* __restrict__ vst, int n_kv, int t_max) {
  constexpr int LPK = HD / 8;
  const int len = a.len[blockIdx.z];
  const int key = blockIdx.x * (256 / LPK) + threadIdx.x / LPK;
  if (key >= len) return;
  const int li = threadIdx.x % LPK;
  const size_t cell = ((size_t)a.slot[blockIdx.z] * n_kv + blockIdx.y) * (size_t)t_max + key;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const u32x2_t c = *reinterpret_cast<const u32x2_t*>((which ? v8 : k8) + cell * HD + li * 8);
    const float s = (which ? vs : ks)[cell];
    float f[8];
    cvt4(c[0], f);
    cvt4(c[1], f + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= s;
    st16((which ? vst : kst) + cell * HD + li * 8, pack8(f));
  }
}

// ------------------------------------------------------------------------------ attention
// attn_body.h's attn_split_body over codes + scales. U: key groups in flight per wave per
// iteration; NW: waves per workgroup.
template <int HD, int G, int U, int NW>
LSA_DEVICE void attn_kv8_body(
    const bf16_raw* __restrict__ q, int ldq, const unsigned char* __restrict__ k8,
    const unsigned char* __restrict__ v8, const float* __restrict__ ks, const float* __restrict__ vs,
    const int* __restrict__ slot, const int* __restrict__ pos, const int* __restrict__ kv_len, int n_heads,
    int n_kv, int t_max, float scale_log2, int nsplit, int min_chunk, float* __restrict__ part_o,
    float* __restrict__ part_lse, bf16_raw* __restrict__ out, int ldo, unsigned* __restrict__ counters,
    int split, int kvh, int row) {
  constexpr int LPK = HD / CPL;        // lanes per key row
  constexpr int KPW = LSA_WAVE / LPK;  // keys per wave-instruction
  constexpr int KPI = KPW * NW;        // keys per workgroup iteration
  constexpr int NTHR = NW * LSA_WAVE;
  using codes_t = u32x2_t;

  __shared__ float s_m[NW][G];
  __shared__ float s_l[NW][G];
  __shared__ float s_o[NW][G][HD];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int grp = lane / LPK, li = lane % LPK;

  const int* lenp = kv_len ? kv_len : pos;
  const int slot_r = slot[row], len_r = lenp[row];
  asm volatile("" ::"s"(slot_r), "s"(len_r));
  const size_t sbase = ((size_t)slot_r * n_kv + kvh) * (size_t)t_max;  // the (slot, kv-head)'s first key
  const unsigned char* kb = k8 + sbase * HD + li * CPL;
  const unsigned char* vb = v8 + sbase * HD + li * CPL;
  const float* ksb = ks + sbase;
  const float* vsb = vs + sbase;
  int T = len_r + (kv_len ? 0 : 1);
  T = T > t_max ? t_max : T;  // never read past the static cache
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
      float lse[KV8_MAX_SPLIT];
      float mm = -INFINITY;
#pragma unroll
      for (int sp = 0; sp < KV8_MAX_SPLIT; ++sp) {
        lse[sp] = sp < nact ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plr, (hb + sp) * 4, 0, 16))
                            : -INFINITY;
        mm = fmaxf(mm, lse[sp]);
      }
      float ws = 0.f, acc = 0.f;
#pragma unroll
      for (int sp = 0; sp < KV8_MAX_SPLIT; ++sp) {
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

  float mx[G], l[G], o[G][CPL];
#pragma unroll
  for (int r = 0; r < G; ++r) {
    mx[r] = KV8_NEG_BIG;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) o[r][j] = 0.f;
  }

  // a key past the chunk reads the chunk's first key instead (a written cell): its score is
  // masked below, and no cell at or beyond the row's length is ever touched
  auto load = [&](int base_, codes_t (&kr_)[U], codes_t (&vr_)[U], float (&ksr_)[U], float (&vsr_)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base_ + grp + u * KPI;
      const int kk = key < k1 ? key : k0;
      kr_[u] = ld_codes_nt(kb + (size_t)kk * HD);
      vr_[u] = ld_codes_nt(vb + (size_t)kk * HD);
      ksr_[u] = __builtin_nontemporal_load(ksb + kk);
      vsr_[u] = __builtin_nontemporal_load(vsb + kk);
    }
  };
  codes_t kr[U], vr[U];
  float ksr[U], vsr[U];
  float qf[G][CPL];
#pragma unroll
  for (int r = 0; r < G; ++r) {
    unpack8(ld16(q + (size_t)row * ldq + (size_t)(kvh * G + r) * HD + li * CPL), qf[r]);
#pragma unroll
    for (int j = 0; j < CPL; ++j) qf[r][j] *= scale_log2;
  }

  // loop bound is wave-uniform (the key groups of a wave shuffle only internally)
  for (int base = k0 + w * KPW; base < k1; base += KPI * U) {
    load(base, kr, vr, ksr, vsr);
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) valid[u] = base + grp + u * KPI < k1;
    float s[G][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[CPL];
      unpack_codes(kr[u], kf);
#pragma unroll
      for (int r = 0; r < G; ++r) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) d += qf[r][j] * kf[j];
        d = group_sum<LPK>(d) * ksr[u];  // the key's scale, once per key
        s[r][u] = valid[u] ? d : KV8_NEG_BIG;
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
      for (int j = 0; j < CPL; ++j) o[r][j] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = valid[u] ? __builtin_amdgcn_exp2f(s[r][u] - mn) : 0.f;
        l[r] += p;
        const float pv = p * vsr[u];
        float vf[CPL];
        unpack_codes(vr[u], vf);
#pragma unroll
        for (int j = 0; j < CPL; ++j) o[r][j] += pv * vf[j];
      }
    }
  }

  // merge the KPW key-groups of this wave (same li, different grp) on DPP / permlane swaps
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
      for (int j = 0; j < CPL; ++j) o[r][j] = o[r][j] * a + lane_xor<OFF>(o[r][j]) * b;
      mx[r] = mn;
    }
  };
  static_assert(CPL == 8 && (LPK == 8 || LPK == 16), "key lane groups");
  if constexpr (LPK == 8) merge_groups(std::integral_constant<int, 8>{});
  merge_groups(std::integral_constant<int, 16>{});
  merge_groups(std::integral_constant<int, 32>{});
  if (grp == 0) {
#pragma unroll
    for (int r = 0; r < G; ++r) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) s_o[w][r][li * CPL + j] = o[r][j];
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
    if (nact == 1) {  // lone active split: final output directly, no merge
      out[(size_t)row * ldo + (size_t)(kvh * G + r) * HD + d] = f2bf(os / ls);
    } else {
      const int pi = (int)(pbase + (size_t)r * nsplit);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(os / ls), por, (pi * HD + d) * 4, 0, 16 /* sc1 */);
      if (d == 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mm + log2f(ls)), plr, pi * 4, 0, 16);
    }
  }
  if (nact > 1) arrive();
}

#define KV8_ATTN_PARAMS                                                                                        \
  const bf16_raw *__restrict__ q, int ldq, const unsigned char *__restrict__ k8,                               \
      const unsigned char *__restrict__ v8, const float *__restrict__ ks, const float *__restrict__ vs,        \
      const int *__restrict__ slot, const int *__restrict__ pos, const int *__restrict__ kv_len, int n_heads,  \
      int n_kv, int t_max, float scale_log2

template <int HD, int G>
__global__ __launch_bounds__(KV8_THR) void attn_kv8_split_kernel(KV8_ATTN_PARAMS, int nsplit, int min_chunk,
                                                                 float* __restrict__ part_o,
                                                                 float* __restrict__ part_lse,
                                                                 bf16_raw* __restrict__ out, int ldo,
                                                                 unsigned* __restrict__ counters) {
  attn_kv8_body<HD, G, 4, KV8_WAVES>(q, ldq, k8, v8, ks, vs, slot, pos, kv_len, n_heads, n_kv, t_max, scale_log2,
                                     nsplit, min_chunk, part_o, part_lse, out, ldo, counters, blockIdx.x, blockIdx.y,
                                     blockIdx.z);
}

struct Kv8AttnArgs {
  const bf16_raw* q;
  int ldq;
  const unsigned char *k8, *v8;
  const float *ks, *vs;
  const int *slot, *pos, *kv_len;
  int rows, n_heads, n_kv, t_max;
  float sl2;
  int nsplit, min_chunk;
  float *po, *pl;
  bf16_raw* out;
  int ldo;
  unsigned* cnt;
  hipStream_t s;
};

template <int HD, int G>
int kv8_launch(const Kv8AttnArgs& a) {
  dim3 grid(a.nsplit, a.n_kv, a.rows);
  attn_kv8_split_kernel<HD, G><<<grid, KV8_THR, 0, a.s>>>(
      a.q, a.ldq, a.k8, a.v8, a.ks, a.vs, a.slot, a.pos, a.kv_len, a.n_heads, a.n_kv, a.t_max, a.sl2, a.nsplit,
      a.min_chunk, a.po, a.pl, a.out, a.ldo, a.cnt);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

template <int HD>
int kv8_dispatch(int g, const Kv8AttnArgs& a) {
  switch (g) {
    case 1: return kv8_launch<HD, 1>(a);
    case 2: return kv8_launch<HD, 2>(a);
    case 3: return kv8_launch<HD, 3>(a);
    case 4: return kv8_launch<HD, 4>(a);
    case 6: return kv8_launch<HD, 6>(a);
    case 8: return kv8_launch<HD, 8>(a);
    default: return LSA_UNSUPPORTED;
  }
}

}  // namespace

// Keys per workgroup iteration of lsa_attn_decode_kv8 for a head size (split chunks are rounded up
// to it); -1 where no kernel is built.
extern "C" int lsa_attn_kv8_kpi(int head_dim) {
  if (head_dim != 128 && head_dim != 64) return -1;
  return (LSA_WAVE / (head_dim / CPL)) * KV8_WAVES;
}

extern "C" int lsa_attn_decode_kv8(const void* q, int ldq, const void* k8, const void* v8, const float* ks,
                                   const float* vs, const int* slot, const int* pos, const int* kv_len, int rows,
                                   int n_heads, int n_kv, int head_dim, int t_max, float scale, int nsplit,
                                   int min_chunk, float* part_o, float* part_lse, void* out, int ldo,
                                   unsigned* counters, hipStream_t stream) {
  // counters: rows * n_kv zero-initialised uint32 (only read when nsplit > 1; left zeroed)
  if (rows < 1 || n_kv < 1 || n_heads % n_kv || nsplit < 1 || nsplit > KV8_MAX_SPLIT || min_chunk < 1 || t_max < 1)
    return LSA_BAD_SHAPE;
  if (nsplit > 1 && (!counters || !part_o || !part_lse)) return LSA_BAD_SHAPE;
  Kv8AttnArgs a;
  a.q = static_cast<const bf16_raw*>(q);
  a.ldq = ldq;
  a.k8 = static_cast<const unsigned char*>(k8);
  a.v8 = static_cast<const unsigned char*>(v8);
  a.ks = ks;
  a.vs = vs;
  a.slot = slot;
  a.pos = pos;
  a.kv_len = kv_len;
  a.rows = rows;
  a.n_heads = n_heads;
  a.n_kv = n_kv;
  a.t_max = t_max;
  a.sl2 = scale * 1.4426950408889634f;
  a.nsplit = nsplit;
  a.min_chunk = min_chunk;
  a.po = part_o;
  a.pl = part_lse;
  a.out = static_cast<bf16_raw*>(out);
  a.ldo = ldo;
  a.cnt = counters;
  a.s = stream;
  const int g = n_heads / n_kv;
  if (head_dim == 128) return kv8_dispatch<128>(g, a);
  if (head_dim == 64) return kv8_dispatch<64>(g, a);
  return LSA_UNSUPPORTED;
}

// Quantise the K and V vectors that the QKV epilogue wrote into the bf16 staging layer at
// (slot[m], h, pos[m], :) into k8 / v8 / ks / vs at the same cell. A row with pos outside
// [0, t_max) (or a slot outside [0, n_slots)) writes nothing. Rows of one launch name distinct cells.
extern "C" int lsa_kv8_append(const void* k_stage, const void* v_stage, void* k8, void* v8, float* ks, float* vs,
                              const int* slot, const int* pos, int rows, int n_slots, int n_kv, int head_dim,
                              int t_max, hipStream_t stream) {
  if (rows < 1 || n_slots < 1 || n_kv < 1 || t_max < 1) return LSA_BAD_SHAPE;
  if (!k_stage || !v_stage || !k8 || !v8 || !ks || !vs || !slot || !pos) return LSA_BAD_SHAPE;
  const long long items = (long long)rows * n_kv * 2;
  if (head_dim != 128 && head_dim != 64) return LSA_UNSUPPORTED;
  const int per = 256 / (head_dim / 8);
  const long long grid = (items + per - 1) / per;
  if (grid >= (1ll << 31)) return LSA_BAD_SHAPE;
  const bf16_raw* kst = static_cast<const bf16_raw*>(k_stage);
  const bf16_raw* vst = static_cast<const bf16_raw*>(v_stage);
  unsigned char* k = static_cast<unsigned char*>(k8);
  unsigned char* v = static_cast<unsigned char*>(v8);
  if (head_dim == 128)
    kv8_append_kernel<128><<<(unsigned)grid, 256, 0, stream>>>(kst, vst, k, v, ks, vs, slot, pos, rows, n_kv, t_max, n_slots);
  else
    kv8_append_kernel<64><<<(unsigned)grid, 256, 0, stream>>>(kst, vst, k, v, ks, vs, slot, pos, rows, n_kv, t_max, n_slots);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// jobs: host array of n_jobs x [slot, len], read before the call returns. Positions [0, len) of every
// kv-head of each named slot are written into the staging layer as bf16(code * s); nothing else.
// Refused before any launch: a slot outside [0, n_slots), len outside [0, t_max]. len == 0 is a no-op.
extern "C" int lsa_kv8_dequant(const void* k8, const void* v8, const float* ks, const float* vs, void* k_stage,
                               void* v_stage, const int* jobs, int n_jobs, int n_slots, int n_kv, int head_dim,
                               int t_max, hipStream_t stream) {
  if (n_jobs < 0 || n_slots < 1 || n_kv < 1 || t_max < 1) return LSA_BAD_SHAPE;
  if (!k_stage || !v_stage || !k8 || !v8 || !ks || !vs || (n_jobs > 0 && !jobs)) return LSA_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return LSA_UNSUPPORTED;
  for (int j = 0; j < n_jobs; ++j)
    if (jobs[2 * j] < 0 || jobs[2 * j] >= n_slots || jobs[2 * j + 1] < 0 || jobs[2 * j + 1] > t_max) return LSA_BAD_SHAPE;
  const int per = 256 / (head_dim / 8);
  const unsigned char* k = static_cast<const unsigned char*>(k8);
  const unsigned char* v = static_cast<const unsigned char*>(v8);
  bf16_raw* kst = static_cast<bf16_raw*>(k_stage);
  bf16_raw* vst = static_cast<bf16_raw*>(v_stage);
  int j = 0;
  while (j < n_jobs) {
    Kv8DqArgs a = {};
    int n = 0, maxlen = 0;
    for (; j < n_jobs && n < KV8_DQ_MAX_JOBS; ++j) {
      if (jobs[2 * j + 1] == 0) continue;
      a.slot[n] = jobs[2 * j];
      a.len[n] = jobs[2 * j + 1];
      maxlen = a.len[n] > maxlen ? a.len[n] : maxlen;
      ++n;
    }
    if (n == 0) continue;
    dim3 grid((maxlen + per - 1) / per, n_kv, n);
    if (head_dim == 128)
      kv8_dequant_kernel<128><<<grid, 256, 0, stream>>>(a, k, v, ks, vs, kst, vst, n_kv, t_max);
    else
      kv8_dequant_kernel<64><<<grid, 256, 0, stream>>>(a, k, v, ks, vs, kst, vst, n_kv, t_max);
    LSA_CHECK_LAUNCH();
  }
  return LSA_OK;
}
