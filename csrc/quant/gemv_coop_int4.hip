// Cooperative W4A16 decode projection for 17..128 rows: y[M, N] = sum_g s[n, g] * (A[M, g] @ Q[N, g]^T),
// on the operands of gemv_int4.hip (Wq4[nt][K/128][lane][16 B] nibbles, S[nt][K/128][16] fp32 group
// scales, bf16 activations) and with its arithmetic: nibble -> bf16 (q + 24) by one v_alignbit_b32 and
// one v_and_or_b32 per pair, per group acc += s * (tmp - 24 * rowsum) in fp32, weights never rounded.
// Wherever the group partial sums are exact in fp32 the two kernels give the same bits. (With a bias
// on a residual epilogue this kernel adds resid + (y + bias), as kernels/gemv_coop.hip does through
// epi_row16, where gemv_int4.hip adds (resid + y) + bias: the same bits where those sums are exact too.)
//
// gemv_int4.hip splits K over the waves of a workgroup, so every workgroup reads all of A and
// every wave spends one more MFMA per A fragment on the row sums. Here
//  * the NW waves of a workgroup own NW*TNW different 16-column tiles and SHARE each A chunk
//    (16*MB rows x one 128-k scale group = 256 B per row): staged once through LDS in 16-B
//    pieces XOR-swizzled with row & 15 (a 16-row ds_read_b128 pass and a 16-piece row store both
//    cover all 64 banks), double-buffered, one barrier per chunk, register-prefetched D-1
//    chunks ahead;
//  * the row sums of a chunk are formed ONCE per workgroup, by the staging threads on their way
//    to LDS (8 adds per 16-B piece, a DPP sum over the 16 pieces of a row), and handed to the
//    tile waves through LDS in the accumulator layout (4 floats per row block and lane group);
//    the fused RMSNorm's sum of squares is kept by the same threads. No MFMA is spent on either;
//  * every wave streams only its own nibble loads (one 16-B load per tile and group) and their
//    4-byte scales, non-temporal, D-1 chunks ahead in registers;
//  * K is split over SK workgroups in whole groups, with the wait-free hand-off of w4_common.h:
//    fp32 partial tiles (and partial sums of squares) through a slab, an arrival counter per
//    column group (w4_coop_tail.h, shared with gemv_mx4.hip).
#include "w4_coop_tail.h"

namespace {

// byte offset of 16-B piece c16 (0..15) of row ``row`` in an A chunk of 256-B rows
LSA_DEVICE int a_off(int row, int c16) { return row * 256 + ((c16 ^ (row & 15)) << 4); }

template <int MB, int TNW, int NW, int D, int EPI, bool NORM>
__global__ __launch_bounds__(NW * 64) void gemv_coop_int4_kernel(
    const bf16_raw* __restrict__ x, int ldx, const int* __restrict__ a_rows, const unsigned char* __restrict__ wq,
    const float* __restrict__ wscale, int M, int N, int K, int SK, float eps, EpiArgs ep, float* __restrict__ slab,
    unsigned* __restrict__ counters) {
  using Geo = W4CoopGeo<MB, TNW, NW>;
  constexpr int NTHR = Geo::NTHR, MR = Geo::MR, TG = Geo::TG, RS = Geo::RS;
  constexpr int ABUF = MR * 256;  // bytes per A chunk
  constexpr int SMEM = 2 * ABUF > Geo::RED ? 2 * ABUF : Geo::RED;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
  __shared__ __attribute__((aligned(16))) float s_rs[2][MR];  // row sums of the chunk in each A buffer
  __shared__ float s_ss[MR];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = K >> 7, CG = (N >> 4) / TG;  // scale groups, column groups
  const int cg = blockIdx.x % CG, s = blockIdx.x / CG;
  const int tlo = cg * TG, nt0 = tlo + w * TNW;  // the workgroup's / this wave's first tile
  const int g_lo = s * G / SK, nchunk = (s + 1) * G / SK - g_lo, last = nchunk - 1;  // host: SK <= G

  // ---- A staging: thread -> (row arow + i * RSTEP, piece ac16), fixed for all chunks
  constexpr int LPT = MR * 16 / NTHR, RSTEP = NTHR / 16;
  static_assert(LPT * NTHR == MR * 16, "the A chunk splits evenly over the workgroup");
  const int arow = tid >> 4, ac16 = tid & 15;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, 0x7fffffff, 0x00020000);
  int a_voff[LPT];
  bool a_valid[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int r = arow + i * RSTEP;
    a_valid[i] = r < M;
    a_voff[i] = ((a_valid[i] ? (a_rows ? a_rows[r] : r) : 0) * ldx + ac16 * 8) * 2;
  }
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wq + (size_t)nt0 * G * 1024), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wscale + (size_t)nt0 * G * 16), (short)0, 0x7fffffff, 0x00020000);
  const int lane16 = lane * 16, lane4 = (lane & 15) * 4;
  unsigned mask = kNibMask, base = kBf16x16;
  asm volatile("" : "+s"(mask), "+v"(base));  // no instruction: hides the constants (int4x8_to_bf16)
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};
  float ss[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) ss[i] = 0.f;

  struct AV { u32x4_t v[LPT]; };
  auto load_a = [&](int c) -> AV {
    AV a;
#pragma unroll
    for (int i = 0; i < LPT; ++i) a.v[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, a_voff[i], (g_lo + c) * 256, 0);
    return a;
  };
  // A piece -> LDS, its share of the row sum (and of the sum of squares) on the way: the 16
  // pieces of a row sit in 16 consecutive lanes. count: 0 for a clamped duplicate chunk
  auto store_a = [&](int buf, const AV& a, float count) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int r = arow + i * RSTEP;
      const u32x4_t av = a_valid[i] ? a.v[i] : zero;  // rows >= M were loaded from row 0: zero them
      float f[8];
      unpack8(av, f);
      float t = ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
      t = group_sum<16>(t);
      if (NORM) {
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) q += f[j] * f[j];
        ss[i] += count * q;
      }
      *reinterpret_cast<u32x4_t*>(smem + buf * ABUF + a_off(r, ac16)) = av;
      if (ac16 == 0) s_rs[buf][r] = t;
    }
  };
  auto load_b = [&](int c, u32x4_t (&b)[TNW], float (&sc)[TNW]) {
#pragma unroll
    for (int t = 0; t < TNW; ++t) {  // nt: once-read weight stream
      b[t] = __builtin_amdgcn_raw_buffer_load_b128(wr, lane16, (t * G + g_lo + c) * 1024, 2);
      sc[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sr, lane4, (t * G + g_lo + c) * 64, 2));
    }
  };

  f32x4_t acc[MB][TNW];
#pragma unroll
  for (int rb = 0; rb < MB; ++rb)
#pragma unroll
    for (int t = 0; t < TNW; ++t) acc[rb][t] = fzero;

  // one group: RBB row blocks at a time keep RBB * TNW independent MFMA chains in flight and the
  // group's tmp at RBB * TNW * 4 registers
  constexpr int RBB = MB * TNW <= 8 ? MB : 8 / TNW;
  static_assert(MB % RBB == 0, "row-block batches tile the chunk");
  auto compute = [&](int buf, const u32x4_t (&b)[TNW], const float (&sc)[TNW]) {
    const unsigned char* ab = smem + buf * ABUF;
    u32x4_t bf[4][TNW];
#pragma unroll
    for (int t = 0; t < TNW; ++t)
#pragma unroll
      for (int h = 0; h < 4; ++h) bf[h][t] = int4x8_to_bf16(b[t][h], mask, base);
#pragma unroll
    for (int rb0 = 0; rb0 < MB; rb0 += RBB) {
      f32x4_t rs[RBB], tmp[RBB][TNW];
#pragma unroll
      for (int j = 0; j < RBB; ++j) {
        rs[j] = *reinterpret_cast<const f32x4_t*>(&s_rs[buf][(rb0 + j) * 16 + kq * 4]);
#pragma unroll
        for (int t = 0; t < TNW; ++t) tmp[j][t] = fzero;
      }
#pragma unroll
      for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int j = 0; j < RBB; ++j) {
          const u32x4_t av = *reinterpret_cast<const u32x4_t*>(ab + a_off((rb0 + j) * 16 + (lane & 15), h * 4 + kq));
#pragma unroll
          for (int t = 0; t < TNW; ++t) tmp[j][t] = mfma16(av, bf[h][t], tmp[j][t]);
        }
#pragma unroll
      for (int j = 0; j < RBB; ++j)
#pragma unroll
        for (int t = 0; t < TNW; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[rb0 + j][t][r] =
                __builtin_fmaf(sc[t], __builtin_fmaf(-kOffset, rs[j][r], tmp[j][t][r]), acc[rb0 + j][t][r]);
    }
  };

  {
    // D-deep register rings for both operands (prefetch distance D-1 chunks). Loads are
    // unconditional (tail chunk indices clamped, duplicates hit the caches), so every wait is a
    // static count. Step c: prefetch chunk c+D-1, compute chunk c from (LDS c & 1, ring slot
    // c % D), then publish A(c+1) and its row sums into the other LDS buffer - which every wave
    // left at the barrier that ended step c-1.
    u32x4_t bw[D][TNW];
    float sw[D][TNW];
    AV aw[D];
    auto clampc = [&](int c) { return c < last ? c : last; };
    static_all(std::make_integer_sequence<int, D - 1>{}, [&](auto sc) {
      constexpr int S = decltype(sc)::value;
      aw[S] = load_a(clampc(S));
      load_b(clampc(S), bw[S], sw[S]);
      return true;
    });
    store_a(0, aw[0], 1.f);
    __syncthreads();
    for (int c = 0;;) {
      const bool more = static_all(std::make_integer_sequence<int, D>{}, [&](auto sc) {
        constexpr int S = decltype(sc)::value, SN = (S + D - 1) % D, S1 = (S + 1) % D;
        aw[SN] = load_a(clampc(c + D - 1));
        load_b(clampc(c + D - 1), bw[SN], sw[SN]);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetches ahead of this chunk's MFMAs
        compute(c & 1, bw[S], sw[S]);
        __builtin_amdgcn_sched_barrier(0);
        store_a((c + 1) & 1, aw[S1], c < last ? 1.f : 0.f);
        __syncthreads();
        return ++c <= last;
      });
      if (!more) break;
    }
  }
  // the loop's last barrier: every wave is done with the A buffers, smem becomes the reduction tile
  if (NORM) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) ss[i] = group_sum<16>(ss[i]);
  }

  // the reduction tile, the split-K hand-off and the aligned epilogue: w4_coop_tail.h. The sums of
  // squares are in the registers of each row's first staging thread
  float* red = reinterpret_cast<float*>(smem);  // [TG][MR][RS]
  auto ss_rows = [&](auto put) {
    if (NORM && ac16 == 0) {
#pragma unroll
      for (int i = 0; i < LPT; ++i) put(arow + i * RSTEP, ss[i]);
    }
  };
  if (!w4_coop_reduce<MB, TNW, NW, NORM, 4>(red, s_ss, &s_last, acc, slab, counters, cg, CG, s, SK, ss_rows)) return;

  // 16-B stores (and 16-B residual / bias / cos / sin loads) need 16-B aligned rows; a caller
  // whose rows are not gets element stores
  const size_t al = (size_t)ep.out | (size_t)ep.resid | (size_t)ep.bias | (size_t)ep.k_cache | (size_t)ep.v_cache |
                    (size_t)ep.cos_t | (size_t)ep.sin_t | (size_t)(ep.ldo * 2) | (size_t)(ep.ldr * 2);
  if ((al & 15) == 0) {
    w4_coop_epilogue16<MB, TNW, NW, EPI, NORM, false>(red, s_ss, ep, M, K, eps, tlo, 0);
  } else {
    // gemv_int4.hip's element epilogue, for a C caller: ops/hip.py make_epi refuses unaligned rows, so
    // nothing in the Python package reaches this branch and no test runs it
    auto rstd = [&](int mm) -> float { return w4_coop_rstd<NORM>(s_ss, mm, K, eps); };
    auto at = [&](int t, int mm, int n) -> float { return red[(t * MR + mm) * RS + n]; };
    if (EPI == EPI_SWIGLU) {
      for (int e = tid; e < (TG / 2) * MR * 16; e += NTHR) {
        const int tp = e / (MR * 16), mm = (e >> 4) % MR, n = e & 15;
        if (mm >= M) continue;
        const float r = rstd(mm);
        ep.out[(size_t)mm * ep.ldo + (tlo / 2 + tp) * 16 + n] = f2bf(silu(at(2 * tp, mm, n) * r) * (at(2 * tp + 1, mm, n) * r));
      }
    } else {
      for (int e = tid; e < TG * MR * 16; e += NTHR) {
        const int t = e / (MR * 16), mm = (e >> 4) % MR, n = e & 15;
        if (mm >= M) continue;
        const float r = rstd(mm);
        const float v = at(t, mm, n) * r;
        const int col = (tlo + t) * 16 + n;
        if (EPI == EPI_STORE) {
          ep.out[(size_t)mm * ep.ldo + col] = f2bf(epi_act(ep, v + epi_bias(ep, col)));
        } else if (EPI == EPI_RESID) {
          ep.out[(size_t)mm * ep.ldo + col] = f2bf(bf2f(ep.resid[(size_t)mm * ep.ldr + col]) + v + epi_bias(ep, col));
        } else if (EPI == EPI_QKV) {
          epi_qkv_store(ep, mm, col, v + epi_bias(ep, col), at(t, mm, n ^ 8) * r + epi_bias(ep, col ^ 8), ep.pos[mm],
                        ep.slot[mm]);
        }
      }
    }
  }
}

template <int MB, int TNW, int NW, int D, int EPI>
int launch_cfg(bool norm, const bf16_raw* x, int ldx, const int* a_rows, const unsigned char* wq, const float* ws,
               int M, int N, int K, int SK, float eps, const EpiArgs& ep, float* slab, unsigned* cnt, hipStream_t s) {
  dim3 grid(N / 16 / (NW * TNW) * SK), block(NW * 64);
  if (norm)
    gemv_coop_int4_kernel<MB, TNW, NW, D, EPI, true><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt);
  else
    gemv_coop_int4_kernel<MB, TNW, NW, D, EPI, false><<<grid, block, 0, s>>>(x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// (mb, tnw, nw, d): nw waves of tnw tiles each share the A chunks of a workgroup (nw * tnw = 4 or 8
// tiles); d = register-ring depth. No (8, 2, ., .): 64 accumulators + the group's tmp + the rings
// leave no room at two tiles per wave.
#define LSA_INT4_COOP_CONFIGS(X)                                                                   \
  X(2, 1, 8, 4) X(2, 1, 4, 4) X(2, 2, 4, 4) X(4, 1, 8, 4) X(4, 1, 4, 4) X(4, 2, 4, 3) X(8, 1, 8, 3) \
  X(8, 1, 4, 3)

template <int EPI>
int launch_epi(int mb, int tnw, int nw, int d, bool norm, const bf16_raw* x, int ldx, const int* a_rows,
               const unsigned char* wq, const float* ws, int M, int N, int K, int SK, float eps, const EpiArgs& ep,
               float* slab, unsigned* cnt, hipStream_t s) {
#define LSA_CFG(B, T, W, DD)                                                                              \
  if (mb == B && tnw == T && nw == W && d == DD)                                                          \
    return launch_cfg<B, T, W, DD, EPI>(norm, x, ldx, a_rows, wq, ws, M, N, K, SK, eps, ep, slab, cnt, s);
  LSA_INT4_COOP_CONFIGS(LSA_CFG)
#undef LSA_CFG
  return LSA_UNSUPPORTED;
}

}  // namespace

// K is split into sk runs of whole 128-k groups, as evenly as possible (1 <= sk <= K / 128).
// Workspace (sk > 1): slab >= sk*N*16*MB*4 + sk*(N/16/(nw*tnw))*16*MB*4 bytes, MB = 2 / 4 / 8 row
// blocks for M <= 32 / 64 / 128; counters: N/16/(nw*tnw) zero-initialised uint32 (reset by the kernel).
extern "C" int lsa_gemv_coop_int4(const void* x, int ldx, const int* a_rows, const void* wq4, const float* scales,
                                  int M, int N, int K, int norm, float eps, int epi, const EpiArgs* ep, int tnw, int nw,
                                  int d, int sk, float* slab, unsigned* counters, hipStream_t stream) {
  if (M < 17 || M > 128 || tnw < 1 || nw < 1 || N < 16 || N % (16 * tnw * nw) || K < 128 || K % 128 || ldx < K ||
      !scales || sk < 1 || sk > K / 128)
    return LSA_BAD_SHAPE;
  if (epi == EPI_SWIGLU && ((tnw * nw) % 2)) return LSA_BAD_SHAPE;  // gate / up tile pairs stay in one workgroup
  if (sk > 1 && (!slab || !counters)) return LSA_BAD_SHAPE;
  const int mb = M <= 32 ? 2 : (M <= 64 ? 4 : 8);
  const bf16_raw* xx = static_cast<const bf16_raw*>(x);
  const unsigned char* w = static_cast<const unsigned char*>(wq4);
  const bool nrm = norm != 0;
  return dispatch_epi(epi, [&](auto e) {
    return launch_epi<decltype(e)::value>(mb, tnw, nw, d, nrm, xx, ldx, a_rows, w, scales, M, N, K, sk, eps, *ep, slab,
                                          counters, stream);
  });
}
