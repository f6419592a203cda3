// W4A16 decode projection: y[M, N] = sum_g s[n, g] * (A[M, g] @ Q[N, g]^T) for M <= 64, with
// symmetric group-128 int4 weights (|q| <= 7, fp32 scale per output column and 128-k group: the
// ModelSharder's int4 format), bf16 activations, fp32 accumulation and the same fused RMSNorm /
// epilogues as kernels/gemv.hip and kernels/gemv_fp8.hip.
//
// Decode is bound by the weight stream; at 4.25 bits per weight it is a quarter of bf16's:
//  * packed layout Wq4[nt][K/128][lane][16 B]: one 16-B non-temporal buffer load per lane brings
//    the 32 nibbles of the FOUR consecutive 32-k MFMA B fragments of one scale group (dword h =
//    fragment h). A lane's fragments belong to one output column (lane & 15), so one fp32
//    scale S[nt][K/128][lane & 15] covers the whole load.
//  * nibble -> bf16 without a table or a conversion instruction: the packer stores offset
//    nibbles u = q + 8, element 2p at nibble p and element 2p + 1 at nibble p + 4, the dword
//    rotated left by 3. Then ((rotr(w, 4p) & 0x00780078) | 0x41804180) is the bf16 pair
//    (16 + u[2p], 16 + u[2p + 1]) = q + 24, exact (bf16 16.0 has a mantissa step of 1/8 and the
//    nibble sits 3 bits up): one shift and one v_and_or_b32 per pair.
//  * the offset is taken out exactly, per group: one more MFMA per A fragment against an
//    all-ones B fragment gives the row sums r[m] = sum_k a[m, k] in the accumulator layout, and
//    tmp - 24 r is the integer-weight dot product. Then acc += s * (tmp - 24 r): the scale is a
//    per-lane scalar because the C layout puts column lane & 15 in every register of a lane.
//    Weights are never rounded: scaling in bf16 in front of the MFMA would round every one.
//  * fused RMSNorm: the sum of squares is the diagonal of A A^T, which one MFMA per A fragment
//    (the fragment as both operands: A and B fragments share a layout) accumulates beside the
//    projection. The VALU keeps to the nibble conversion.
// Same register double-buffering / K split over waves / LDS reduction as gemv_fp8.hip; a wave's K
// range is a whole number of groups (any group count: a chunk's tail groups are skipped).
#include "../kernels/epilogue.h"

namespace {

constexpr unsigned kNibMask = 0x00780078u;  // a nibble at mantissa bits 3..6 of both halves
constexpr unsigned kBf16x16 = 0x41804180u;  // bf16 (16.0, 16.0)
constexpr float kOffset = 24.0f;            // 16 (the bf16 base) + 8 (the nibble offset)

// one packed dword (8 nibbles = one lane's share of a 32-k B fragment) -> 8 bf16 (q + 24).
// ``mask`` / ``base`` arrive as registers (an SGPR and a VGPR the caller made opaque), so that
// (w & mask) | base is ONE v_and_or_b32: with two literals the compiler has to emit v_and + v_or
LSA_DEVICE u32x4_t int4x8_to_bf16(unsigned w, unsigned mask, unsigned base) {
  u32x4_t r;
  r[0] = (w & mask) | base;
  r[1] = (__builtin_amdgcn_alignbit(w, w, 4) & mask) | base;
  r[2] = (__builtin_amdgcn_alignbit(w, w, 8) & mask) | base;
  r[3] = (__builtin_amdgcn_alignbit(w, w, 12) & mask) | base;
  return r;
}

// UG = 16-B weight loads (= scale groups of 4 k-fragments) per pipeline chunk and tile
template <int TN, int MB, int NW, int UG, int EPI, bool NORM>
__global__ __launch_bounds__(NW * 64) void gemv_int4_kernel(
    const bf16_raw* __restrict__ x, int ldx, const int* __restrict__ a_rows,
    const unsigned char* __restrict__ wq, const float* __restrict__ wscale, int M, int N, int K, float eps,
    EpiArgs ep) {
  constexpr int NTHR = NW * 64;
  constexpr int MR = 16 * MB;
  constexpr int U = 4 * UG;  // k-fragments per chunk
  __shared__ float red[NW * TN * MR * 16];
  __shared__ float s_ss[NW][MR];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = K >> 7;  // scale groups
  const int nt0 = blockIdx.x * TN;
  const int kq = lane >> 4;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wq + (size_t)nt0 * G * 1024), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wscale + (size_t)nt0 * G * 16), (short)0, 0x7fffffff, 0x00020000);
  int xoff[MB];
#pragma unroll
  for (int rb = 0; rb < MB; ++rb) {
    const int m = rb * 16 + (lane & 15);
    const int mm = m < M ? m : 0;
    xoff[rb] = ((a_rows ? a_rows[mm] : mm) * ldx + kq * 8) * 2;
  }

  f32x4_t acc[MB][TN], ssd[MB];
#pragma unroll
  for (int rb = 0; rb < MB; ++rb) {
    ssd[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[rb][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int g_begin = (wu * G) / NW, g_end = ((wu + 1) * G) / NW;
  const int lane16 = lane * 16, lane4 = (lane & 15) * 4;
  unsigned mask = kNibMask, base = kBf16x16;
  asm volatile("" : "+s"(mask), "+v"(base));  // no instruction: hides the constants (int4x8_to_bf16)
  const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};  // bf16 1.0 x 8
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};

  auto load = [&](int g, u32x4_t (&b)[UG][TN], float (&sc)[UG][TN], u32x4_t (&a)[U][MB]) {
#pragma unroll
    for (int u = 0; u < UG; ++u) {
      if (g + u >= g_end) break;  // uniform: the wave's last chunk may be short
#pragma unroll
      for (int t = 0; t < TN; ++t) {  // nt: once-read weight stream
        b[u][t] = __builtin_amdgcn_raw_buffer_load_b128(wr, lane16, (t * G + g + u) * 1024, 2);
        sc[u][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sr, lane4, (t * G + g + u) * 64, 0));
      }
#pragma unroll
      for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int rb = 0; rb < MB; ++rb)
          a[4 * u + h][rb] = __builtin_amdgcn_raw_buffer_load_b128(xr, xoff[rb], ((g + u) * 4 + h) * 64, 0);
    }
  };
  auto compute = [&](int g, u32x4_t (&b)[UG][TN], float (&sc)[UG][TN], u32x4_t (&a)[U][MB]) {
#pragma unroll
    for (int u = 0; u < UG; ++u) {
      if (g + u >= g_end) break;
      u32x4_t bf[4][TN];
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int h = 0; h < 4; ++h) bf[h][t] = int4x8_to_bf16(b[u][t][h], mask, base);
#pragma unroll
      for (int rb = 0; rb < MB; ++rb) {
        f32x4_t rs = fzero, tmp[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t) tmp[t] = fzero;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          // rows >= M hold a copy of row 0: a row of C depends on its own row of A only, and
          // the epilogue stores no row >= M
          const u32x4_t av = a[4 * u + h][rb];
          rs = mfma16(av, ones, rs);
          if (NORM) ssd[rb] = mfma16(av, av, ssd[rb]);
#pragma unroll
          for (int t = 0; t < TN; ++t) tmp[t] = mfma16(av, bf[h][t], tmp[t]);
        }
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[rb][t][r] = __builtin_fmaf(sc[u][t], __builtin_fmaf(-kOffset, rs[r], tmp[t][r]), acc[rb][t][r]);
      }
    }
  };

  if (g_begin < g_end) {
    u32x4_t bX[UG][TN], aX[U][MB], bY[UG][TN], aY[U][MB];
    float sX[UG][TN], sY[UG][TN];
    int g = g_begin;
    load(g, bX, sX, aX);
    for (;;) {
      if (g + UG >= g_end) {
        compute(g, bX, sX, aX);
        break;
      }
      load(g + UG, bY, sY, aY);
      compute(g, bX, sX, aX);
      g += UG;
      if (g + UG >= g_end) {
        compute(g, bY, sY, aY);
        break;
      }
      load(g + UG, bX, sX, aX);
      compute(g, bY, sY, aY);
      g += UG;
    }
  }

#pragma unroll
  for (int rb = 0; rb < MB; ++rb)
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[((w * TN + t) * MR + rb * 16 + kq * 4 + r) * 16 + (lane & 15)] = acc[rb][t][r];
  if (NORM) {
    // the diagonal of A A^T: row m = column m sits in the lanes with (lane & 15) >> 2 == lane >> 4
    if (((lane & 15) >> 2) == kq) {
#pragma unroll
      for (int rb = 0; rb < MB; ++rb) {
        const int r = lane & 3;
        const float v = r == 0 ? ssd[rb][0] : (r == 1 ? ssd[rb][1] : (r == 2 ? ssd[rb][2] : ssd[rb][3]));
        s_ss[w][rb * 16 + (lane & 15)] = v;
      }
    }
  }
  __syncthreads();

  auto rsum = [&](int t, int mm, int n) -> float {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) v += red[((i * TN + t) * MR + mm) * 16 + n];
    return v;
  };
  auto rstd = [&](int mm) -> float {
    if (!NORM) return 1.f;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += s_ss[i][mm];
    return rsqrtf(t / (float)K + eps);
  };

  if (EPI == EPI_SWIGLU) {
    for (int e = tid; e < (TN / 2) * MR * 16; e += NTHR) {
      const int tp = e / (MR * 16), mm = (e >> 4) % MR, n = e & 15;
      if (mm >= M) continue;
      const float r = rstd(mm);
      const float g = rsum(2 * tp, mm, n) * r, u = rsum(2 * tp + 1, mm, n) * r;
      ep.out[(size_t)mm * ep.ldo + (nt0 / 2 + tp) * 16 + n] = f2bf(silu(g) * u);
    }
  } else {
    for (int e = tid; e < TN * MR * 16; e += NTHR) {
      const int t = e / (MR * 16), mm = (e >> 4) % MR, n = e & 15;
      if (mm >= M) continue;
      const float r = rstd(mm);
      const float v = rsum(t, mm, n) * r;
      const int col = (nt0 + t) * 16 + n;
      if (EPI == EPI_STORE) {
        ep.out[(size_t)mm * ep.ldo + col] = f2bf(epi_act(ep, v + epi_bias(ep, col)));
      } else if (EPI == EPI_RESID) {
        ep.out[(size_t)mm * ep.ldo + col] = f2bf(bf2f(ep.resid[(size_t)mm * ep.ldr + col]) + v + epi_bias(ep, col));
      } else if (EPI == EPI_QKV) {
        epi_qkv_store(ep, mm, col, v + epi_bias(ep, col), rsum(t, mm, n ^ 8) * r + epi_bias(ep, col ^ 8), ep.pos[mm],
                      ep.slot[mm]);
      }
    }
  }
}

template <int TN, int MB, int NW, int UG, int EPI>
int launch_cfg(bool norm, const bf16_raw* x, int ldx, const int* a_rows, const unsigned char* wq, const float* ws,
               int M, int N, int K, float eps, const EpiArgs& ep, hipStream_t s) {
  dim3 grid(N / 16 / TN), block(NW * 64);
  if (norm)
    gemv_int4_kernel<TN, MB, NW, UG, EPI, true><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, eps, ep);
  else
    gemv_int4_kernel<TN, MB, NW, UG, EPI, false><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, eps, ep);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// (TN, MB, NW, UG): UG 16-B int4 loads (scale groups) per tile per chunk (= 4*UG k-fragments)
#define LSA_INT4_CONFIGS(X)                                                                          \
  X(1, 1, 4, 1) X(1, 1, 8, 1) X(1, 1, 4, 2) X(1, 1, 8, 2) X(2, 1, 4, 1) X(2, 1, 8, 1) X(2, 1, 4, 2)   \
  X(4, 1, 4, 1) X(1, 2, 4, 1) X(1, 2, 8, 1) X(2, 2, 4, 1) X(2, 2, 8, 1) X(1, 4, 4, 1) X(1, 4, 8, 1)   \
  X(2, 4, 4, 1) X(2, 4, 8, 1)

template <int EPI>
int launch_epi(int tn, int nw, int ug, bool norm, const bf16_raw* x, int ldx, const int* a_rows,
               const unsigned char* wq, const float* ws, int M, int N, int K, float eps, const EpiArgs& ep,
               hipStream_t s) {
  const int mb = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
#define LSA_CFG(T, B, W, UU)                                                                       \
  if (tn == T && mb == B && nw == W && ug == UU) {                                                \
    if constexpr (EPI == EPI_SWIGLU && (T % 2)) return LSA_BAD_SHAPE;                             \
    else return launch_cfg<T, B, W, UU, EPI>(norm, x, ldx, a_rows, wq, ws, M, N, K, eps, ep, s);   \
  }
  LSA_INT4_CONFIGS(LSA_CFG)
#undef LSA_CFG
  return LSA_UNSUPPORTED;
}

// Dequantise packed int4 (Wq4[nt][K/128][lane][16] + S[nt][K/128][16]) into packed bf16
// (Wp[nt][kt][lane][8]), each value bf16_rne(q * s): used to run prefill / >64-row batches through
// the bf16 GEMM / coop kernels from one layer-sized scratch buffer when the weights are kept in int4.
__global__ void dequant_int4_packed_kernel(const unsigned char* __restrict__ wq, const float* __restrict__ wscale,
                                           bf16_raw* __restrict__ wp, int NT, int G) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16-B int4 load = 4 fragments
  if (i >= (size_t)NT * G * 64) return;
  const int lane = (int)(i & 63);
  const size_t blk = i >> 6;  // nt * G + g
  const int nt = (int)(blk / G), g = (int)(blk % G);
  const u32x4_t q = *reinterpret_cast<const u32x4_t*>(wq + i * 16);
  const float sc = wscale[blk * 16 + (lane & 15)];
  for (int h = 0; h < 4; ++h) {
    const unsigned v = __builtin_amdgcn_alignbit(q[h], q[h], 3);  // undo the packer's rotation
    float f[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      f[2 * p] = (float)((int)((v >> (4 * p)) & 15u) - 8) * sc;
      f[2 * p + 1] = (float)((int)((v >> (4 * p + 16)) & 15u) - 8) * sc;
    }
    const size_t frag = ((size_t)nt * (4 * G) + 4 * g + h) * 64 + lane;
    *reinterpret_cast<u32x4_t*>(wp + frag * 8) = pack8(f);
  }
}

}  // namespace

extern "C" int lsa_gemv_int4(const void* x, int ldx, const int* a_rows, const void* wq4, const float* scales, int M,
                             int N, int K, int norm, float eps, int epi, const EpiArgs* ep, int tn, int nw, int ug,
                             hipStream_t stream) {
  if (M < 1 || M > 64 || tn < 1 || ug < 1 || N < 16 || N % (16 * tn) || K < 128 || K % 128 || ldx < K || !scales)
    return LSA_BAD_SHAPE;
  if (epi == EPI_SWIGLU && (tn % 2)) return LSA_BAD_SHAPE;
  const bf16_raw* xx = static_cast<const bf16_raw*>(x);
  const unsigned char* w = static_cast<const unsigned char*>(wq4);
  const bool nrm = norm != 0;
  switch (epi) {
    case EPI_STORE: return launch_epi<EPI_STORE>(tn, nw, ug, nrm, xx, ldx, a_rows, w, scales, M, N, K, eps, *ep, stream);
    case EPI_RESID: return launch_epi<EPI_RESID>(tn, nw, ug, nrm, xx, ldx, a_rows, w, scales, M, N, K, eps, *ep, stream);
    case EPI_SWIGLU: return launch_epi<EPI_SWIGLU>(tn, nw, ug, nrm, xx, ldx, a_rows, w, scales, M, N, K, eps, *ep, stream);
    case EPI_QKV: return launch_epi<EPI_QKV>(tn, nw, ug, nrm, xx, ldx, a_rows, w, scales, M, N, K, eps, *ep, stream);
    default: return LSA_UNSUPPORTED;  // no arg-max epilogue: the lm_head stays bf16
  }
}

extern "C" int lsa_dequant_int4_packed(const void* wq4, const float* scales, void* wp, int N, int K,
                                       hipStream_t stream) {
  if (N < 16 || N % 16 || K < 128 || K % 128) return LSA_BAD_SHAPE;
  const int NT = N / 16, G = K / 128;
  const size_t n = (size_t)NT * G * 64;
  dequant_int4_packed_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      static_cast<const unsigned char*>(wq4), scales, static_cast<bf16_raw*>(wp), NT, G);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
