// W4A8 decode projection on the block-scaled MFMA, 1..128 rows:
//   y[M, N] = sum over 32-k blocks of 2^(ea + eb) * (a8[M, block] @ w4[N, block]^T)
// with MXFP4 weights (e2m1 codes + one e8m0 exponent per 32: ops/mx4.py), bf16 activations
// quantised here to MXFP8 (e4m3 codes + one e8m0 exponent per row and 32-block, the fp8 KV cache's
// scale convention), fp32 accumulation and the fused RMSNorm / epilogues of the other GEMVs.
//
// v_mfma_scale_f32_16x16x128_f8f6f4 takes the fp4 B fragment as it lies in memory and applies both
// block scales itself, so there is no unpack arithmetic at all:
//  * Wq[nt][K/128][lane][16 B]: lane l = column l & 15, 32-block l >> 4 of the 128-k step, element j
//    at nibble j: the instruction's fp4 operand order (its e4m3 A operand differs: lane group g
//    holds k = 16g .. 16g + 15 in registers 0-3 and 64 + 16g .. in registers 4-7). One 16-B
//    non-temporal load per lane is one MFMA's B operand (blgp:4 reads four VGPRs). Every wave owns
//    TNW 16-column tiles and streams only their loads, three K-steps ahead in a register ring.
//  * S[nt][K/512][lane] dwords: byte i of lane 16b + column = the exponent of 32-block b in
//    K-step 4g + i, selected by op_sel (the instruction takes block b's scale, of A and of B, from
//    lane group b). One load per tile and four K-steps, one group ahead.
//  * A is quantised ONCE per workgroup and K-step, by all threads on their way to LDS: a quad of
//    lanes holds one 32-block as 4 x 8 bf16 (16-B loads, two K-steps ahead in registers), takes the
//    block's largest magnitude over the quad on DPP, scales by the exact power of two, converts
//    with v_cvt_pk_fp8_f32 and writes 8 codes in A-fragment order (two 16-B halves per lane so that
//    each ds_read_b128 pass is contiguous) plus the exponent dword. Double-buffered, one barrier
//    per K-step. The NW waves share it; the fused RMSNorm's sum of squares is taken from the
//    bf16 values on the same pass, so rstd is that of the unquantised row.
//  * K is split over SK workgroups in whole 512-k groups (the last may be short: K / 128 need not
//    be a multiple of 4) with the wait-free hand-off of w4_common.h: partial tiles (and partial
//    sums of squares) through a slab, an arrival counter per column group (w4_coop_tail.h,
//    shared with gemv_coop_int4.hip).
//  * A workgroup's last waves may own tiles past N / 16 (any tile count is served): they run on a
//    clamped tile and their results are dropped.
#include "mx8_quant.h"
#include "w4_coop_tail.h"

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

template <int MB, int TNW, int NW, int EPI, bool NORM>
__global__ __launch_bounds__(NW * 64) void gemv_mx4_kernel(
    const bf16_raw* __restrict__ x, int ldx, const int* __restrict__ a_rows, const unsigned char* __restrict__ wq,
    const unsigned* __restrict__ wscale, int M, int N, int K, int SK, float eps, EpiArgs ep, float* __restrict__ slab,
    unsigned* __restrict__ counters) {
  using Geo = W4CoopGeo<MB, TNW, NW>;
  constexpr int MR = Geo::MR, TG = Geo::TG;
  constexpr int ACODE = MB * 2 * 1024;    // e4m3 codes of one K-step: [MB][2 halves][64 lanes][16 B]
  constexpr int ABUF = ACODE + MB * 256;  // + the exponent dwords [MB][64 lanes]
  constexpr int SMEM = 2 * ABUF > Geo::RED ? 2 * ABUF : Geo::RED;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
  __shared__ float s_ssp[4][MR];  // sums of squares by 32-block of the K-step
  __shared__ float s_ss[MR];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KS = K >> 7, NG = (KS + 3) >> 2, NT = N >> 4;  // K-steps, scale groups, tiles
  const int CG = (NT + TG - 1) / TG;                        // column groups
  const int cg = blockIdx.x % CG, s = blockIdx.x / CG;
  const int tlo = cg * TG, nt0 = tlo + w * TNW;  // the workgroup's / this wave's first tile
  const int ks_lo = (s * NG / SK) * 4;           // host: SK <= NG, so every split has a K-step
  const int ks_end = ((s + 1) * NG / SK) * 4;
  const int last = (ks_end < KS ? ks_end : KS) - ks_lo - 1;

  // ---- A staging: wave-iteration i quantises (row block, 32-block) pair i * NW + w; in it lane
  // -> row lane >> 2, 8-element piece lane & 3 (a quad = one block)
  constexpr int LPT = MB * 4 / NW;
  static_assert(LPT * NW == MB * 4 && LPT >= 1, "the (row block, 32-block) pairs split evenly over the waves");
  const int ar = lane >> 2, asub = lane & 3;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, 0x7fffffff, 0x00020000);
  int a_voff[LPT], a_dst[LPT];
  bool a_valid[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int p = i * NW + w, rb = p >> 2, blk = p & 3, r = rb * 16 + ar;
    a_valid[i] = r < M;
    a_voff[i] = ((a_valid[i] ? (a_rows ? a_rows[r] : r) : 0) * ldx + blk * 32 + asub * 8) * 2;
    // k = 32 blk + 8 asub .. + 7 of the step: the e4m3 operand wants it in register half k / 64 of lane
    // group (k % 64) / 16, at byte k % 16
    a_dst[i] = ((rb * 2 + (blk >> 1)) * 64 + ((blk & 1) * 2 + (asub >> 1)) * 16 + ar) * 16 + (asub & 1) * 8;
  }
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc((void*)wscale, (short)0, 0x7fffffff, 0x00020000);
  int tile[TNW];
#pragma unroll
  for (int t = 0; t < TNW; ++t) tile[t] = nt0 + t < NT ? nt0 + t : NT - 1;
  const int lane16 = lane * 16, lane4 = lane * 4;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};
  float ss[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) ss[i] = 0.f;

  struct AV { u32x4_t v[LPT]; };
  auto load_a = [&](int j) -> AV {
    AV a;
#pragma unroll
    for (int i = 0; i < LPT; ++i) a.v[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, a_voff[i], (ks_lo + j) * 256, 0);
    return a;
  };
  // one piece -> 8 e4m3 codes (+ the block's exponent dword) in LDS. count: 0 for a clamped duplicate
  auto store_a = [&](int buf, const AV& a, float count) {
    unsigned char* ab = smem + buf * ABUF;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const u32x4_t av = a_valid[i] ? a.v[i] : zero;  // rows >= M were loaded from row 0: zero them
      float f[8];
      unpack8(av, f);
      if (NORM) {
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) q += f[j] * f[j];
        ss[i] += count * q;
      }
      u32x2_t c;
      const int e = mx8_quant_quad(f, c);
      *reinterpret_cast<u32x2_t*>(ab + a_dst[i]) = c;
      if (asub == 0) {
        const int p = i * NW + w;
        *reinterpret_cast<unsigned*>(ab + ACODE + ((p >> 2) * 64 + (p & 3) * 16 + ar) * 4) = (unsigned)e;
      }
    }
  };
  auto load_b = [&](int j, u32x4_t (&b)[TNW]) {
#pragma unroll
    for (int t = 0; t < TNW; ++t)  // nt: once-read weight stream
      b[t] = __builtin_amdgcn_raw_buffer_load_b128(wr, lane16, (tile[t] * KS + ks_lo + j) * 1024, 2);
  };
  auto load_sc = [&](int g, unsigned (&sc)[TNW]) {
#pragma unroll
    for (int t = 0; t < TNW; ++t) sc[t] = __builtin_amdgcn_raw_buffer_load_b32(sr, lane4, (tile[t] * NG + g) * 256, 2);
  };

  f32x4_t acc[MB][TNW];
#pragma unroll
  for (int rb = 0; rb < MB; ++rb)
#pragma unroll
    for (int t = 0; t < TNW; ++t) acc[rb][t] = fzero;

  // K-step with scale byte S of the group's dword: MB * TNW MFMAs of K = 128
  auto compute = [&](auto sel, int buf, const u32x4_t (&b)[TNW], const unsigned (&sc)[TNW]) {
    constexpr int S = decltype(sel)::value;
    const unsigned char* ab = smem + buf * ABUF;
    i32x8_t b8[TNW];
#pragma unroll
    for (int t = 0; t < TNW; ++t) {
      const u32x4_t bt = b[t];
      b8[t] = i32x8_t{(int)bt[0], (int)bt[1], (int)bt[2], (int)bt[3], 0, 0, 0, 0};
    }
#pragma unroll
    for (int rb = 0; rb < MB; ++rb) {
      const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(ab + ((rb * 2) * 64 + lane) * 16);
      const u32x4_t hi = *reinterpret_cast<const u32x4_t*>(ab + ((rb * 2 + 1) * 64 + lane) * 16);
      const int sa = *reinterpret_cast<const int*>(ab + ACODE + (rb * 64 + lane) * 4);
      const i32x8_t a8 = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
#pragma unroll
      for (int t = 0; t < TNW; ++t)
        acc[rb][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8[t], acc[rb][t], 0 /* A: e4m3 */,
                                                                      4 /* B: e2m1 */, 0, sa, S, (int)sc[t]);
    }
  };

  {
    // Step j (local K-step, slot S = j & 3): request A of step j + 2 and B of step j + 3, compute
    // step j from LDS buffer j & 1 and ring slot S, then quantise A of step j + 1 into the other
    // buffer - which every wave left at the barrier that ended step j - 1. Loads past the split's
    // end are clamped duplicates (they hit the caches), so every wait is a static count.
    u32x4_t bw[4][TNW];
    unsigned sc[TNW], scn[TNW];
    AV aw[4];
    const int g0 = ks_lo >> 2;
    auto clampj = [&](int j) { return j < last ? j : last; };
    aw[0] = load_a(0);
    aw[1] = load_a(clampj(1));
    load_b(0, bw[0]);
    load_b(clampj(1), bw[1]);
    load_b(clampj(2), bw[2]);
    load_sc(g0, sc);
    store_a(0, aw[0], 1.f);
    __syncthreads();
    for (int j = 0;;) {
      const bool more = static_all(std::make_integer_sequence<int, 4>{}, [&](auto sel) {
        constexpr int S = decltype(sel)::value;
        aw[(S + 2) & 3] = load_a(clampj(j + 2));
        load_b(clampj(j + 3), bw[(S + 3) & 3]);
        if (S == 0) load_sc(g0 + (clampj(j + 4) >> 2), scn);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetches ahead of this step's MFMAs
        compute(sel, S & 1, bw[S], sc);
        __builtin_amdgcn_sched_barrier(0);
        store_a((S + 1) & 1, aw[(S + 1) & 3], j < last ? 1.f : 0.f);
        if (S == 3) {
#pragma unroll
          for (int t = 0; t < TNW; ++t) sc[t] = scn[t];
        }
        __syncthreads();
        return ++j <= last;
      });
      if (!more) break;
    }
  }
  // the loop's last barrier: every wave is done with the A buffers, smem becomes the reduction tile
  if (NORM) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      float t = ss[i];
      t += dpp_mov<0xB1>(t);
      t += dpp_mov<0x4E>(t);
      ss[i] = t;
    }
    // a row's four 32-blocks sit in different wave-iterations: summed below in fixed order
    if (asub == 0) {
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int p = i * NW + w;
        s_ssp[p & 3][(p >> 2) * 16 + ar] = ss[i];
      }
    }
  }

  // the reduction tile, the split-K hand-off and the epilogue: w4_coop_tail.h. A row's sum of
  // squares is the sum of its four 32-block partials, once every wave has written s_ssp
  float* red = reinterpret_cast<float*>(smem);  // [TG][MR][RS]
  auto ss_rows = [&](auto put) {
    __syncthreads();
    if (NORM && tid < MR) put(tid, (s_ssp[0][tid] + s_ssp[1][tid]) + (s_ssp[2][tid] + s_ssp[3][tid]));
  };
  if (!w4_coop_reduce<MB, TNW, NW, NORM, 1>(red, s_ss, &s_last, acc, slab, counters, cg, CG, s, SK, ss_rows)) return;
  w4_coop_epilogue16<MB, TNW, NW, EPI, NORM, true>(red, s_ss, ep, M, K, eps, tlo, NT);
}

template <int MB, int TNW, int NW, int EPI>
int launch_cfg(bool norm, const bf16_raw* x, int ldx, const int* a_rows, const unsigned char* wq, const unsigned* ws,
               int M, int N, int K, int SK, float eps, const EpiArgs& ep, float* slab, unsigned* cnt, hipStream_t s) {
  constexpr int TG = NW * TNW;
  dim3 grid((N / 16 + TG - 1) / TG * SK), block(NW * 64);
  if (norm)
    gemv_mx4_kernel<MB, TNW, NW, EPI, true><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt);
  else
    gemv_mx4_kernel<MB, TNW, NW, EPI, false><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// (mb, tnw, nw): nw waves of tnw tiles each share the quantised A of a workgroup; the
// (row block, 32-block) pairs of a K-step, 4 * mb, split evenly over the waves
#define LSA_MX4_CONFIGS(X) \
  X(1, 1, 4) X(1, 2, 4) X(2, 1, 4) X(2, 2, 4) X(2, 1, 8) X(4, 1, 4) X(4, 2, 4) X(4, 1, 8) X(8, 1, 4) X(8, 1, 8)

template <int EPI>
int launch_epi(int mb, int tnw, int nw, bool norm, const bf16_raw* x, int ldx, const int* a_rows,
               const unsigned char* wq, const unsigned* ws, int M, int N, int K, int SK, float eps, const EpiArgs& ep,
               float* slab, unsigned* cnt, hipStream_t s) {
#define LSA_CFG(B, T, W)                   \
  if (mb == B && tnw == T && nw == W)      \
    return launch_cfg<B, T, W, EPI>(norm, x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt, s);
  LSA_MX4_CONFIGS(LSA_CFG)
#undef LSA_CFG
  return LSA_UNSUPPORTED;
}

// Packed fp4 + exponents -> the packed bf16 fragments of packing.pack_b, Wp[nt][K/32][lane][8], on
// v_cvt_scalef32_pk_bf16_fp4: code * 2^eb is a bf16 normal by the format's clamp, so the values
// are exact. One thread per 16-B fp4 load: its 32 values are the whole bf16 fragment column of
// k-tile 4 * step + block, eight values for each of the four lane groups.
__global__ void dequant_mx4_packed_kernel(const unsigned char* __restrict__ wq, const unsigned* __restrict__ wscale,
                                          bf16_raw* __restrict__ wp, int NT, int KS, int NG) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)NT * KS * 64) return;
  const int lane = (int)(i & 63);
  const size_t st = i >> 6;  // nt * KS + step
  const int nt = (int)(st / KS), step = (int)(st % KS);
  const unsigned scd = wscale[((size_t)nt * NG + (step >> 2)) * 64 + lane];
  const float scale = __uint_as_float(((scd >> (8 * (step & 3))) & 255u) << 23);
  unsigned q[4];
  *reinterpret_cast<u32x4_t*>(q) = ld16(wq + i * 16);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const unsigned qd = q[g];
    unsigned o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const bf16x2_t r = b == 0   ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(qd, scale, 0)
                         : b == 1 ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(qd, scale, 1)
                         : b == 2 ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(qd, scale, 2)
                                  : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(qd, scale, 3);
      o[b] = __builtin_bit_cast(unsigned, r);
    }
    const size_t frag = ((size_t)nt * (4 * KS) + 4 * step + (lane >> 4)) * 64 + g * 16 + (lane & 15);
    st16(wp + frag * 8, u32x4_t{o[0], o[1], o[2], o[3]});
  }
}

}  // namespace

// K is split into sk runs of whole 512-k scale groups, as evenly as possible (1 <= sk <= ceil(K / 512)).
// Workspace (sk > 1), with CG = ceil(N/16 / (nw*tnw)) column groups and MB = 1 / 2 / 4 / 8 row blocks
// for M <= 16 / 32 / 64 / 128: slab >= sk * CG * (nw*tnw*16 + 1) * 16*MB floats; counters: CG
// zero-initialised uint32 (reset by the kernel). Rows of x, out, resid and the caches 16-B aligned.
extern "C" int lsa_gemv_mx4(const void* x, int ldx, const int* a_rows, const void* wq, const void* scales, int M, int N,
                            int K, int norm, float eps, int epi, const EpiArgs* ep, int tnw, int nw, int sk, float* slab,
                            unsigned* counters, hipStream_t stream) {
  if (M < 1 || M > 128 || tnw < 1 || nw < 1 || N < 16 || N % 16 || K < 128 || K % 128 || ldx < K || !scales ||
      sk < 1 || sk > (K / 128 + 3) / 4 || (long long)N * K / 2 >= (1ll << 31))
    return LSA_BAD_SHAPE;
  if (epi == EPI_SWIGLU && (((tnw * nw) % 2) || ((N / 16) % 2))) return LSA_BAD_SHAPE;  // gate / up tile pairs
  if (sk > 1 && (!slab || !counters)) return LSA_BAD_SHAPE;
  const size_t al = (size_t)x | (size_t)(ldx * 2) | (size_t)ep->out | (size_t)ep->resid | (size_t)ep->bias |
                    (size_t)ep->k_cache | (size_t)ep->v_cache | (size_t)ep->cos_t | (size_t)ep->sin_t |
                    (size_t)(ep->ldo * 2) | (size_t)(ep->ldr * 2);
  if (al & 15) return LSA_BAD_SHAPE;  // 16-B loads and stores throughout
  const int mb = M <= 16 ? 1 : (M <= 32 ? 2 : (M <= 64 ? 4 : 8));
  const bf16_raw* xx = static_cast<const bf16_raw*>(x);
  const unsigned char* w = static_cast<const unsigned char*>(wq);
  const unsigned* sc = static_cast<const unsigned*>(scales);
  const bool nrm = norm != 0;
  return dispatch_epi(epi, [&](auto e) {
    return launch_epi<decltype(e)::value>(mb, tnw, nw, nrm, xx, ldx, a_rows, w, sc, M, N, K, sk, eps, *ep, slab,
                                          counters, stream);
  });
}

extern "C" int lsa_dequant_mx4_packed(const void* wq, const void* scales, void* wp, int N, int K, hipStream_t stream) {
  if (N < 16 || N % 16 || K < 128 || K % 128) return LSA_BAD_SHAPE;
  const int NT = N / 16, KS = K / 128;
  const size_t n = (size_t)NT * KS * 64;
  dequant_mx4_packed_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      static_cast<const unsigned char*>(wq), static_cast<const unsigned*>(scales), static_cast<bf16_raw*>(wp), NT, KS,
      (KS + 3) / 4);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
