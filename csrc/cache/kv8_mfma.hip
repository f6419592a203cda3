// FP8 KV cache on gfx950 (CDNA4 / MI355X): the GQA decode attention on MFMA that reads the codes.
//
//   lsa_attn_decode_mfma_kv8   lsa_attn_decode_mfma (kernels/attn_prefill.hip gqa_decode_kernel) over
//                              k8 / v8 / ks / vs of csrc/cache/kv8.hip: GQA batches of many
//                              (row, kv-head) items
//
// Contract (ops/kv8.py attn_decode_reference): row m attends keys [0, min(kv_len[m] or pos[m] + 1,
// t_max)) of slot[m]; scores are scale * ks[t] * (q . code_t), the output is
// sum p_t * vs[t] * code_t / sum p_t; softmax in the exp2 domain in fp32, P rounded to bf16 for the
// PV MFMA; nothing is written outside out[m, :n_heads * hd].
//
// Work split: gqa_decode_kernel's. One workgroup per (row, kv-head); the group's G query heads are
// the 16 MFMA columns (columns >= G are zero); wave w takes the 32-key sub-blocks w, w + NW, ...;
// every wave owns a double buffer (registers for K and the scales, LDS for V), waits with a counted
// vmcnt and meets no barrier inside the loop; the NW (m, l, O) states merge through LDS at the end.
//
// Data path (v_mfma_f32_16x16x32_bf16; lane = 16 g + l16; A holds row l16, contraction index
// 8 g + j; B holds column l16, the same contraction index; C holds rows 4 g + r, column l16):
//
//  K   S^T[key][head] = K Q^T. Lane (g, l16) of key tile kt loads the HD / 4 CONTIGUOUS codes
//      [g HD/4, (g + 1) HD/4) of key 16 kt + l16: two 16-byte non-temporal loads at hd 128, one at
//      hd 64, so a wave reads a key tile as one contiguous run of 16 HD bytes. Fragment j of the lane
//      is codes g HD/4 + 8 j .. + 7, turned into 8 bf16 by four v_cvt_scalef32_pk_bf16_fp8 with scale
//      1 (e4m3 is exact in bf16). The contraction does not care which head dims a lane holds as long
//      as A and B agree, so the Q^T fragment j of lane (g, l16) is Q[head l16][g HD/4 + 8 j .. + 7].
//  ks  The accumulator of lane (g, l16) holds keys 16 kt + 4 g + r, r = 0..3: their scales are 16
//      contiguous bytes, one load. Each score is multiplied by ks[t] * scale_log2 beside the length
//      mask: the contract's own expression, 8 multiplies per lane and sub-block. The alternative, the
//      key's scale as the conversion's scale operand, needs the scale of the lane's A row (key
//      16 kt + l16), a second 4-byte load pattern, and moves the scale into every element; it was not
//      built.
//  V   O^T[dim][head] = V^T P^T. A 32-key sub-block of codes is 32 HD bytes (4 KiB at hd 128), staged
//      by non-temporal LDS-DMA in 1 KiB pieces: lane i of piece s writes LDS bytes [16 i, 16 i + 16)
//      of the piece, i.e. 16-byte chunk position cs = i % (HD / 16) of row r = s (1024 / HD) +
//      i / (HD / 16), and fetches global chunk cs ^ swz(r) of that key. So chunk c of row r lies at
//      r HD + 16 (c ^ swz(r)).
//      The A operand of dim tile d comes from ONE ds_read_b64_tr_b8: in each 16-lane group the lane
//      2 k + c (k = 0..7, c = 0..1) supplies the address of 8 bytes M[k][8 c .. 8 c + 7], and lane i
//      receives the column M[0..7][i]. With i = dim 16 d + i, c the half of chunk d and row k mapped
//      to key  kmap(g, k) = 4 g + k (k < 4),  16 + 4 g + k - 4 (k >= 4),  byte j of lane (g, l16) is
//      the code of (key kmap(g, j), dim 16 d + l16). That is exactly the key order of the packed P^T
//      fragment {s[0][0..3], s[1][0..3]} the lane already holds, so P needs no shuffle. Four
//      conversions make the operand.
//      swz: a b64 LDS read is served in two halves of 32 lanes (g = 0, 1 and g = 2, 3), each of which
//      touches rows {8 h .. 8 h + 7} and {16 + 8 h ..}, 16 rows x 16 bytes, and must cover the 64
//      banks once. hd 128: a row is 8 chunks, rows of equal parity share banks, so
//      swz(r) = ((r >> 1) & 3) | ((r >> 4) & 1) << 2; hd 64: a row is 4 chunks, rows equal mod 4 share
//      banks, swz(r) = ((r >> 2) & 1) | ((r >> 4) & 1) << 1. The DMA writes a piece as 1024
//      contiguous bytes, conflict-free by construction.
//  vs  The same 16-byte pattern gives the lane vs[t] of exactly the keys whose p it holds; it packs
//      bf16(p_t * vs[t]) (a power of two: equal to bf16(p_t) * vs[t] away from under / overflow)
//      while l sums the unscaled p.
//
// Masked keys. Code loads of a key >= kl are clamped to key kl - 1; the 16-byte scale loads of a
// four-key group are clamped to the group of key kl - 1, so no byte beyond the row's last group of
// four is read (and none beyond t_max, a multiple of four). Inside that group the scales past kl - 1
// may be anything: a masked score is SELECTED to -inf and a masked p to 0, never multiplied.
// t_max % 4 != 0 or scale tensors off a 16-byte boundary are refused by the entry point
// (LSA_BAD_SHAPE); ops/kv8.py routes such a cache to lsa_attn_decode_kv8.
#include "../kernels/common.h"

namespace {

typedef int kvq_v2i_t __attribute__((ext_vector_type(2)));

template <int HD>
LSA_DEVICE int kvq_swz(int r) {
  if constexpr (HD == 128) return ((r >> 1) & 3) | (((r >> 4) & 1) << 2);
  else return ((r >> 2) & 1) | (((r >> 4) & 1) << 1);
}
LSA_DEVICE void kvq_glds16_nt(const void* src, unsigned char* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_base, 16, 0, 2);
}
LSA_DEVICE f32x4_t kvq_ld4f_nt(const float* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
}
// 8 e4m3 codes (two dwords, byte order) -> 8 bf16
LSA_DEVICE u32x4_t kvq_codes_to_bf16(unsigned lo, unsigned hi) {
  u32x4_t r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  return r;
}

template <int HD, int NW>
__global__ __launch_bounds__(NW * 64) void gqa_decode_kv8_kernel(
    const bf16_raw* __restrict__ q, int ldq, const unsigned char* __restrict__ k8,
    const unsigned char* __restrict__ v8, const float* __restrict__ ks, const float* __restrict__ vs,
    const int* __restrict__ dslot, const int* __restrict__ dpos, const int* __restrict__ dkvlen, int n_heads,
    int n_kv, int t_max, float scale_log2, bf16_raw* __restrict__ out, int ldo) {
  constexpr int SB = 32;                  // keys per sub-block (one 32-deep PV fragment)
  constexpr int KF = HD / 32, DT = HD / 16;
  constexpr int NC = HD / 16;             // 16-byte chunks per row of codes
  constexpr int KL = HD / 64;             // 16-byte K loads per lane and key tile
  constexpr int BLK = SB * HD;            // bytes of one V sub-block
  constexpr int PPW = BLK / 1024;         // 1 KiB DMA pieces per V sub-block
  constexpr int RPP = 1024 / HD;          // rows per piece
  constexpr int NLD = PPW + 2 * KL + 4;   // vector-memory operations of one stage()
  constexpr int WREG = 2 * BLK;           // one wave's staging: [buffer] V only
  constexpr int MERGE = NW * (16 * HD + 32) * 4;
  constexpr int SMEM = NW * WREG > MERGE ? NW * WREG : MERGE;
  static_assert(PPW >= 1 && KL >= 1 && NLD < 64, "geometry");
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

  const int row = blockIdx.x / n_kv, kvh = blockIdx.x % n_kv;
  const int G = n_heads / n_kv;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = dslot[row];
  int kl = dkvlen ? dkvlen[row] : dpos[row] + 1;
  kl = kl < t_max ? kl : t_max;  // never read past the static cache
  const bool col_ok = l16 < G;   // MFMA column l16 = query head kvh * G + l16

  // Q^T fragments (B operand): lane holds Q[head l16][g HD/4 + 8 j .. + 7], the K lanes' dims
  u32x4_t qf[KF];
  {
    const bf16_raw* qrow = q + (size_t)row * ldq + (size_t)(kvh * G + (col_ok ? l16 : 0)) * HD;
#pragma unroll
    for (int j = 0; j < KF; ++j) qf[j] = col_ok ? ld16(qrow + g * (HD / 4) + j * 8) : u32x4_t{0u, 0u, 0u, 0u};
  }
  const size_t sbase = ((size_t)slot * n_kv + kvh) * (size_t)t_max;  // the (slot, kv-head)'s first key
  const unsigned char* kb = k8 + sbase * HD + g * (HD / 4);
  const unsigned char* vb = v8 + sbase * HD;
  const float* ksb = ks + sbase;
  const float* vsb = vs + sbase;
  unsigned char* my = smem + w * WREG;
  const int last = kl - 1;          // the clamp target of code loads
  const int last4 = last & ~3;      // ... and of the four-key scale loads

  struct Regs {
    u32x4_t k[2][KL];   // the lane's HD / 4 codes of its key of either tile
    f32x4_t ks[2], vs[2];  // scales of keys 16 kt + 4 g + 0..3
  };

  // Sub-block sb: V by LDS-DMA into this wave's buffer `buf`, K and the scales into registers.
  auto stage = [&](int sb, int buf, Regs& rg) {
    const int t0 = sb * SB;
    unsigned char* vd = my + buf * BLK;
#pragma unroll
    for (int s = 0; s < PPW; ++s) {
      const int r = s * RPP + lane / NC, cs = lane % NC;
      const int ch = cs ^ kvq_swz<HD>(r);
      const unsigned key = (unsigned)min(t0 + r, last);  // clamped rows are masked in the softmax
      kvq_glds16_nt(vb + (key * HD + ch * 16), vd + s * 1024);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const unsigned key = (unsigned)min(t0 + kt * 16 + l16, last);
#pragma unroll
      for (int i = 0; i < KL; ++i) rg.k[kt][i] = ld16_nt(kb + (key * HD + i * 16));
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int k4 = min(t0 + kt * 16 + 4 * g, last4);
      rg.ks[kt] = kvq_ld4f_nt(ksb + k4);
      rg.vs[kt] = kvq_ld4f_nt(vsb + k4);
    }
  };

  float o[DT][4];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  // tr_b8 source address of this lane: row kmap(g, l16 >> 1), half l16 & 1 of chunk d
  int v_off[DT];
  {
    const int k = l16 >> 1;
    const int vrow = 4 * g + k + (k < 4 ? 0 : 12);
#pragma unroll
    for (int d = 0; d < DT; ++d) v_off[d] = vrow * HD + ((d ^ kvq_swz<HD>(vrow)) << 4) + 8 * (l16 & 1);
  }

  // one sub-block: K and scales from registers rg, V from buffer buf
  auto compute = [&](int sb, int buf, const Regs& rg) {
    const unsigned char* vsm = my + buf * BLK;
    f32x4_t s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      s[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < KF; ++j) {
        const u32x4_t c = rg.k[kt][j / 2];
        s[kt] = mfma16(kvq_codes_to_bf16(c[(j % 2) * 2], c[(j % 2) * 2 + 1]), qf[j], s[kt]);
      }
    }
    float mx = -INFINITY;
    bool live[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        live[kt][r] = sb * SB + kt * 16 + g * 4 + r < kl;
        const float v = live[kt][r] ? s[kt][r] * (rg.ks[kt][r] * scale_log2) : -INFINITY;
        s[kt][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    float psum = 0.f;
    float pf[8];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = __builtin_amdgcn_exp2f(s[kt][r] - m_use);
        psum += pv;
        pf[kt * 4 + r] = live[kt][r] ? pv * rg.vs[kt][r] : 0.f;  // a masked p stays an exact 0
      }
    l_run = l_run * alpha + psum;
    if (__builtin_amdgcn_ballot_w64(m_new != m_run)) {
      // (element by element: no packed FP32 multiply is formed from this)
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[d][r] *= alpha;
    }
    m_run = m_new;
    const u32x4_t b = pack8(pf);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const kvq_v2i_t c =
          __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) kvq_v2i_t*)(vsm + v_off[d]));
      const f32x4_t acc = mfma16(kvq_codes_to_bf16((unsigned)c[0], (unsigned)c[1]), b,
                                 f32x4_t{o[d][0], o[d][1], o[d][2], o[d][3]});
#pragma unroll
      for (int r = 0; r < 4; ++r) o[d][r] = acc[r];
    }
  };

  // gqa_decode_kernel's schedule: two register / LDS buffers alternate with compile-time indices;
  // before reading sub-block sb the wave restages the other buffer with sb + NW and waits until only
  // that later stage's NLD operations are in flight. (The compiler adds waits of its own: it knows
  // that the DMA writes LDS and drains vmcnt in front of the V reads of the odd sub-blocks, and in
  // front of the K conversions of the even ones. Computing a wave's last sub-block in a branch of its
  // own, so that no "restaged or not" join precedes compute(), left those waits in place and cost
  // 40 VGPRs - 193 against 152 at hd 128 - so the plain schedule stays.)
  const int nsb = (kl + SB - 1) / SB;
  Regs r0, r1;
  auto step = [&](int sb, int cur, const Regs& rcur, Regs& rnext) {
    if (sb + NW < nsb) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the other buffer's V reads retired
      __builtin_amdgcn_sched_barrier(0);
      stage(sb + NW, cur ^ 1, rnext);
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NLD) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    compute(sb, cur, rcur);
  };
  int sb = w;
  if (sb < nsb) stage(sb, 0, r0);
  for (; sb < nsb; sb += 2 * NW) {
    step(sb, 0, r0, r1);
    if (sb + NW >= nsb) break;
    step(sb + NW, 1, r1, r0);
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);

  // merge the NW partial states through LDS: per wave O^T[dim][head] (fp32), m[head], l[head]
  __syncthreads();  // every wave is done with its staging buffers
  float* Ow = reinterpret_cast<float*>(smem);           // [NW][16 heads][HD]
  float* mw = Ow + NW * 16 * HD;                          // [NW][16]
  float* lw = mw + NW * 16;                               // [NW][16]
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) Ow[(w * 16 + l16) * HD + d * 16 + 4 * g + r] = o[d][r];
  if (g == 0) {
    mw[w * 16 + l16] = m_run;
    lw[w * 16 + l16] = l_run;
  }
  __syncthreads();
  // 8 output dims per thread-unit: units (head < G, dim octet)
  for (int u = tid; u < G * (HD / 8); u += NW * 64) {
    const int hh = u / (HD / 8), d0 = (u % (HD / 8)) * 8;
    float M = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; ++i) M = fmaxf(M, mw[i * 16 + hh]);
    const float Mu = M == -INFINITY ? 0.f : M;
    float L = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const float f = __builtin_amdgcn_exp2f(mw[i * 16 + hh] - Mu);
      L += lw[i * 16 + hh] * f;
      const float* src = Ow + (i * 16 + hh) * HD + d0;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += src[j] * f;
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    st16(out + (size_t)row * ldo + (size_t)(kvh * G + hh) * HD + d0, pack8(acc));
  }
}

template <int HD, int NW>
void launch_nw(unsigned grid, const bf16_raw* q, int ldq, const unsigned char* k8, const unsigned char* v8,
               const float* ks, const float* vs, const int* slot, const int* pos, const int* kvlen, int n_heads,
               int n_kv, int t_max, float sl2, bf16_raw* o, int ldo, hipStream_t stream) {
  gqa_decode_kv8_kernel<HD, NW><<<grid, NW * 64, 0, stream>>>(q, ldq, k8, v8, ks, vs, slot, pos, kvlen, n_heads, n_kv,
                                                               t_max, sl2, o, ldo);
}

template <int HD>
int launch_gqa_decode_kv8(int nw, unsigned grid, const bf16_raw* q, int ldq, const unsigned char* k8,
                          const unsigned char* v8, const float* ks, const float* vs, const int* slot, const int* pos,
                          const int* kvlen, int n_heads, int n_kv, int t_max, float sl2, bf16_raw* o, int ldo,
                          hipStream_t stream) {
  if (nw == 1)
    launch_nw<HD, 1>(grid, q, ldq, k8, v8, ks, vs, slot, pos, kvlen, n_heads, n_kv, t_max, sl2, o, ldo, stream);
  else if (nw == 2)
    launch_nw<HD, 2>(grid, q, ldq, k8, v8, ks, vs, slot, pos, kvlen, n_heads, n_kv, t_max, sl2, o, ldo, stream);
  else
    launch_nw<HD, 4>(grid, q, ldq, k8, v8, ks, vs, slot, pos, kvlen, n_heads, n_kv, t_max, sl2, o, ldo, stream);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

}  // namespace

// lsa_attn_decode_mfma (kernels/attn_prefill.hip) over an fp8 cache: one workgroup per
// (row, kv-head), the group's 2..16 query heads as the MFMA columns, keys
// [0, min(kv_len or pos + 1, t_max)) of the row's slot, split over ``nw`` = 1 / 2 / 4 waves (0 = 1).
// slot / pos / kv_len are read on the device. Return codes are lsa_attn_decode_mfma's; in addition
// t_max % 4 != 0 and cache tensors off a 16-byte boundary are LSA_BAD_SHAPE (the four-key scale
// loads). A refusal launches nothing.
extern "C" int lsa_attn_decode_mfma_kv8(const void* q, int ldq, const void* k8, const void* v8, const float* ks,
                                        const float* vs, const int* slot, const int* pos, const int* kv_len, int rows,
                                        int n_heads, int n_kv, int head_dim, int t_max, float scale, void* out,
                                        int ldo, int nw, hipStream_t stream) {
  if (rows < 1 || n_kv < 1 || n_heads < 1 || n_heads % n_kv || !slot || !pos) return LSA_BAD_SHAPE;
  const int g = n_heads / n_kv;
  if (g < 2 || g > 16) return LSA_UNSUPPORTED;
  if (ldo % 8 || reinterpret_cast<uintptr_t>(out) % 16 || ldq % 8 || reinterpret_cast<uintptr_t>(q) % 16)
    return LSA_BAD_SHAPE;
  if (head_dim != 128 && head_dim != 64) return LSA_UNSUPPORTED;
  if (!q || !k8 || !v8 || !ks || !vs || !out) return LSA_BAD_SHAPE;
  if (t_max < 4 || t_max % 4 || (long long)t_max * head_dim >= (1ll << 31)) return LSA_BAD_SHAPE;
  if (reinterpret_cast<uintptr_t>(k8) % 16 || reinterpret_cast<uintptr_t>(v8) % 16 ||
      reinterpret_cast<uintptr_t>(ks) % 16 || reinterpret_cast<uintptr_t>(vs) % 16)
    return LSA_BAD_SHAPE;
  if (nw == 0) nw = 1;
  if (nw != 1 && nw != 2 && nw != 4) return LSA_UNSUPPORTED;
  const long long grid = (long long)rows * n_kv;
  if (grid >= (1ll << 31)) return LSA_BAD_SHAPE;
  const float sl2 = scale * 1.4426950408889634f;
  const auto* qq = static_cast<const bf16_raw*>(q);
  const auto* k = static_cast<const unsigned char*>(k8);
  const auto* v = static_cast<const unsigned char*>(v8);
  auto* o = static_cast<bf16_raw*>(out);
  return head_dim == 128 ? launch_gqa_decode_kv8<128>(nw, (unsigned)grid, qq, ldq, k, v, ks, vs, slot, pos, kv_len,
                                                      n_heads, n_kv, t_max, sl2, o, ldo, stream)
                         : launch_gqa_decode_kv8<64>(nw, (unsigned)grid, qq, ldq, k, v, ks, vs, slot, pos, kv_len,
                                                     n_heads, n_kv, t_max, sl2, o, ldo, stream);
}
