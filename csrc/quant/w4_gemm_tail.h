// The tail of the two 4-bit-weight GEMMs (gemm_int4.hip, gemm_mx4.hip) behind their main loops:
// 256 threads, a 128-row x BN tile (BN = 64 FN), wave w owning ALL 128 rows x BN/4 columns as
// acc[row block][16-column tile j] in the MFMA's accumulator layout. Split-K hand-off, epilogue,
// and the host checks of both.
#pragma once
#include "w4_common.h"

template <int FN>
struct W4TileGeo {
  static constexpr int BM = 128, NTHR = 256;
  static constexpr int TN = FN * 16, BN = 4 * TN, TILES = 4 * FN;
  static constexpr int ELD = TN + 4;  // fp32 row stride of a wave's epilogue image
  static constexpr int EPI_BYTES = 4 * BM * ELD * 4;
  static constexpr int TILE_F4 = 4 * 8 * FN * 64;  // f32x4 fragments of one partial tile
};

// Split-K hand-off (w4_common.h) of split s of ``tile``. Slab: [SK][tile][wave][row block][j][lane]
// f32x4, fragment-native: a lane reads back exactly the fragments it would have held, so the sum
// needs no layout change. Returns true in the last arriver only, with acc = the sum of the SK
// partials in split order and the tile's counter reset. A whole split (8 FN 16-B loads per lane)
// is in flight per round.
template <int FN>
LSA_DEVICE bool w4_gemm_splitk(f32x4_t (&acc)[8][FN], float* __restrict__ slab, unsigned* __restrict__ counters,
                               int* s_flag, int tile, int ntiles, int s, int SK) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc((void*)slab, (short)0, 0x7fffffff, 0x00020000);
  const int split_stride = ntiles * W4TileGeo<FN>::TILE_F4 * 16;  // bytes (host: SK * split_stride < 2^31)
  const int frag0 = ((tile * 4 + w) * 8 * FN * 64 + lane) * 16;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), pr, frag0 + (i * FN + j) * 1024,
                                             s * split_stride, 16 /* sc1 */);
  if (!splitk_arrive(&counters[tile], SK, s_flag)) return false;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < SK; ++q) {
    f32x4_t v[8][FN];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        v[i][j] = __builtin_bit_cast(
            f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(pr, frag0 + (i * FN + j) * 1024, q * split_stride, 16));
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += v[i][j][r];  // element by element: no packed FP32 adds
  }
  splitk_reset(&counters[tile]);
  return true;
}

// Epilogue of the tile at rows m0.., columns col0..: the fp32 tile through per-wave LDS images at
// ``smem`` (W4TileGeo::EPI_BYTES; the caller's rings are dead and every wave is past its last
// read of them); one thread per (row, 16 columns) unit, the TILES units of a row in consecutive
// threads, runs the row16 epilogues of epilogue.h. The fused-RMSNorm fields as in gemm_sk.hip:
// with ss_in, the row scale first, summed in gemm_sk's order into s_rstd[128]; with ss_out, the
// per-64-column sums of squares of the rounded outputs.
template <int FN, int EPI>
LSA_DEVICE void w4_gemm_epilogue(unsigned char* smem, float* s_rstd, const f32x4_t (&acc)[8][FN], const EpiArgs& ep,
                                 int M, int m0, int col0) {
  using Geo = W4TileGeo<FN>;
  constexpr int BM = Geo::BM, NTHR = Geo::NTHR, TILES = Geo::TILES, ELD = Geo::ELD;
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr bool NORM_IN = EPI == EPI_QKV || EPI == EPI_SWIGLU;
  if (NORM_IN && ep.ss_in) {
    for (int r = tid; r < BM; r += NTHR) {
      const float* sp = ep.ss_in + (size_t)min(m0 + r, M - 1) * ep.ss_n;
      float tsum = 0.f;
      for (int i0 = 0; i0 < ep.ss_n; i0 += 4) {
        const f32x4_t q4 = *reinterpret_cast<const f32x4_t*>(sp + i0);
        tsum += (q4[0] + q4[1]) + (q4[2] + q4[3]);
      }
      s_rstd[r] = rsqrtf(tsum / (float)(64 * ep.ss_n) + ep.ss_eps);
    }
  }
  float* img = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        img[w * (BM * ELD) + (i * 16 + 4 * kq + r) * ELD + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  auto unit = [&](int row, int jt, float* v) {  // 16-column tile jt of the workgroup's BN columns
    const float* src = img + (jt / FN) * (BM * ELD) + row * ELD + (jt % FN) * 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4_t*>(v + 4 * q) = *reinterpret_cast<const f32x4_t*>(src + 4 * q);
  };
  if constexpr (EPI == EPI_SWIGLU) {
    // 16-column tiles interleave gate / up (packing.fuse_gate_up): pair jp of the workgroup
    // writes output columns col0 / 2 + 16 jp
    constexpr int PAIRS = TILES / 2;
#pragma unroll
    for (int s2 = 0; s2 < (BM * PAIRS) / NTHR; ++s2) {
      const int u = tid + NTHR * s2, row = u / PAIRS, jp = u % PAIRS;
      const int m = m0 + row;
      if (m < M) {
        float g[16], up[16];
        unit(row, 2 * jp, g);
        unit(row, 2 * jp + 1, up);
        const float rsc = ep.ss_in ? s_rstd[row] : 1.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) g[q] = silu(g[q] * rsc) * (up[q] * rsc);
        bf16_raw* o = ep.out + (size_t)m * ep.ldo + col0 / 2 + jp * 16;
        st16(o, pack8(g));
        st16(o + 8, pack8(g + 8));
      }
    }
  } else {
#pragma unroll
    for (int s2 = 0; s2 < (BM * TILES) / NTHR; ++s2) {
      const int u = tid + NTHR * s2, row = u / TILES, jt = u % TILES;
      const int m = m0 + row, c0 = col0 + jt * 16;
      float v[16];
      unit(row, jt, v);
      if (EPI == EPI_RESID && ep.ss_out) {
        // residual add + the row's sum of squares of the ROUNDED outputs over the 64 columns of
        // 4 consecutive threads (gemm_sk.hip)
        float ssq = 0.f;
        if (m < M) {
          epi_bias16(ep, c0, v);
          const bf16_raw* rr = ep.resid + (size_t)m * ep.ldr + c0;
          float x0[8], x1[8];
          unpack8(ld16(rr), x0);
          unpack8(ld16(rr + 8), x1);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            x0[q] += v[q];
            x1[q] += v[q + 8];
          }
          const u32x4_t p0 = pack8(x0), p1 = pack8(x1);
          bf16_raw* o = ep.out + (size_t)m * ep.ldo + c0;
          st16(o, p0);
          st16(o + 8, p1);
          unpack8(p0, x0);
          unpack8(p1, x1);
          ssq = ss16(x0, x1);
        }
        // (s0 + s1) + (s2 + s3) over the 4 units of the 64-column block (lsa_row_ss order)
#pragma unroll
        for (int o = 1; o < 4; o <<= 1) ssq = __fadd_rn(ssq, __shfl_xor(ssq, o, 64));
        if (m < M && (jt & 3) == 0) ep.ss_out[(size_t)m * ep.ss_n + (c0 >> 6)] = ssq;
      } else if (m < M) {
        if (EPI == EPI_QKV && ep.ss_in) {
          const float rsc = s_rstd[row];
#pragma unroll
          for (int q = 0; q < 16; ++q) v[q] *= rsc;
        }
        epi_row16<EPI>(ep, m, c0, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------ host checks
// sk in 1 / 2 / 4 / 8 and <= max_sk; the grid fits; for sk > 1 the workspace of w4_gemm_splitk:
// slab_floats >= sk * ceil(M / 128) * 128 * N fp32 (under 2 GiB: the kernel's offsets are ints),
// 16-B aligned, and one zero-initialised counter per output tile.
static inline int check_gemm_split(int sk, int max_sk, int M, int N, int bn, const float* slab, long long slab_floats,
                                   const unsigned* counters, int n_counters) {
  constexpr int BM = W4TileGeo<1>::BM;
  if ((sk != 1 && sk != 2 && sk != 4 && sk != 8) || sk > max_sk) return LSA_BAD_SHAPE;
  const long long mt = (M + BM - 1) / BM, tiles = mt * (N / bn);
  if (tiles * sk > 0x7fffffffLL) return LSA_BAD_SHAPE;
  if (sk > 1) {
    const long long need = (long long)sk * mt * BM * N;
    if (!slab || !counters || slab_floats < need || need * 4 > 0x7fffffffLL || n_counters < tiles || !aligned16(slab))
      return LSA_BAD_SHAPE;
  }
  return LSA_OK;
}

// what w4_gemm_epilogue needs of the epilogue arguments (epi is one of dispatch_epi's four)
static inline int check_epi_args(int epi, const EpiArgs* ep, int N, int K) {
  // the row16 epilogues store and load 16-B runs
  if (!ep->out || !aligned16(ep->out) || !aligned16(ep->bias) || ep->ldo % 8) return LSA_BAD_SHAPE;
  if (epi == EPI_STORE && ep->ldo < N) return LSA_BAD_SHAPE;
  if (epi == EPI_RESID && (!ep->resid || !aligned16(ep->resid) || ep->ldo < N || ep->ldr < N || ep->ldr % 8))
    return LSA_BAD_SHAPE;
  if (epi == EPI_SWIGLU && (ep->ldo < N / 2 || ep->act || ep->bias)) return LSA_BAD_SHAPE;
  if (epi == EPI_QKV) {
    const int hd = ep->head_dim;
    if (!ep->k_cache || !ep->v_cache || !ep->slot || !ep->pos || hd < 16 || (hd & (hd - 1)) ||
        N != (ep->n_heads + 2 * ep->n_kv) * hd || !aligned16(ep->k_cache) || !aligned16(ep->v_cache) ||
        !aligned16(ep->cos_t) || !aligned16(ep->sin_t) || (ep->cos_t == nullptr) != (ep->sin_t == nullptr))
      return LSA_BAD_SHAPE;
  }
  if (epi != EPI_STORE && ep->act) return LSA_BAD_SHAPE;
  if (ep->ss_out && (epi != EPI_RESID || N % 64 || ep->ss_n != N / 64)) return LSA_BAD_SHAPE;
  if (ep->ss_in && ((epi != EPI_QKV && epi != EPI_SWIGLU) || ep->ss_n < 4 || ep->ss_n % 4 || K != 64 * ep->ss_n ||
                    !aligned16(ep->ss_in)))
    return LSA_BAD_SHAPE;
  return LSA_OK;
}
