// The tail of the two cooperative 4-bit-weight GEMVs (gemv_coop_int4.hip, gemv_mx4.hip) behind
// their K loops: NW waves of TNW 16-column tiles each, MB row blocks, wave w holding
// acc[row block][tile] of tiles (cg * NW + w) * TNW + t in the MFMA's accumulator layout. The
// accumulators meet in the fp32 reduction tile red[TG][MR][RS] in LDS, directly or through the
// split-K hand-off of w4_common.h, and the aligned epilogue runs out of it.
#pragma once
#include "w4_common.h"

template <int MB, int TNW, int NW>
struct W4CoopGeo {
  static constexpr int NTHR = NW * 64;
  static constexpr int MR = 16 * MB;
  static constexpr int TG = NW * TNW;           // 16-column tiles per workgroup
  static constexpr int RS = 20;                 // reduction tile row stride (floats): 16 + 4 pad
  static constexpr int RED = TG * MR * RS * 4;  // bytes of the reduction tile
};

// acc -> red, and the rows' sums of squares -> s_ss[MR] (NORM), for split s of column group cg.
// ``ss_rows(put)`` is the kernel's source of its sums of squares over its K range: it calls
// put(row, value) once per row from whichever threads hold them (and may barrier first).
// SK == 1: straight into LDS. SK > 1: through the slab, [SK][CG * TG tiles][MB][64 lanes][4] fp32
// (fragment-native), then [SK][CG][MR] sums of squares, with one arrival counter per column group;
// the last arriver's region is one contiguous run of TG * MB * 256 floats per split, which the
// whole workgroup reads E4 16-B loads per thread and split, QB splits in flight, and sums in
// fixed split order. Returns true, behind a barrier, where red and s_ss are complete: always for
// SK == 1, in the last arriver only for SK > 1.
// QB is the caller's because one value does not serve both kernels: gemv_coop_int4 has 4, and
// gemv_mx4 with 4 measured 4 .. 28 % slower at 64 and 128 rows (o, down and qkv projections of
// Llama-2-7B, sk 2 and 8: a round's 4 E4 loads per thread, or its re-reads of split 0 past SK, cost
// more than they hide) though 5 .. 8 % faster up to 32 rows, so it keeps 1. The sums do not depend
// on QB: the adds run in split order either way.
template <int MB, int TNW, int NW, bool NORM, int QB, typename SS>
LSA_DEVICE bool w4_coop_reduce(float* red, float* s_ss, int* s_last, const f32x4_t (&acc)[MB][TNW],
                               float* __restrict__ slab, unsigned* __restrict__ counters, int cg, int CG, int s, int SK,
                               SS&& ss_rows) {
  using Geo = W4CoopGeo<MB, TNW, NW>;
  constexpr int NTHR = Geo::NTHR, MR = Geo::MR, TG = Geo::TG, RS = Geo::RS;
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (SK == 1) {
#pragma unroll
    for (int rb = 0; rb < MB; ++rb)
#pragma unroll
      for (int t = 0; t < TNW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[((w * TNW + t) * MR + rb * 16 + kq * 4 + r) * RS + (lane & 15)] = acc[rb][t][r];
    ss_rows([&](int row, float v) { s_ss[row] = v; });
  } else {
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc((void*)slab, (short)0, 0x7fffffff, 0x00020000);
    const int split_stride = CG * TG * MR * 16;  // floats
    const int nt0 = cg * TG + w * TNW;           // this wave's first tile
#pragma unroll
    for (int rb = 0; rb < MB; ++rb)
#pragma unroll
      for (int t = 0; t < TNW; ++t)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[rb][t]), pr,
                                               ((((nt0 + t) * MB + rb) * 64 + lane) * 4) * 4, s * split_stride * 4,
                                               16 /* sc1 */);
    const int ss_base = SK * split_stride;  // floats
    ss_rows([&](int row, float v) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), pr, ((s * CG + cg) * MR + row) * 4, ss_base * 4, 16);
    });
    if (!splitk_arrive(&counters[cg], SK, s_last)) return false;
    constexpr int E4 = TG * MB * 64 / NTHR;
    const int gbase = cg * TG * MB * 256;  // floats
    f32x4_t sum[E4];
#pragma unroll
    for (int j = 0; j < E4; ++j) sum[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < SK; q0 += QB) {
      f32x4_t v[QB][E4];
#pragma unroll
      for (int qq = 0; qq < QB; ++qq) {
        const int q = q0 + qq < SK ? q0 + qq : 0;
#pragma unroll
        for (int j = 0; j < E4; ++j)
          v[qq][j] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                     pr, (gbase + (j * NTHR + tid) * 4) * 4, q * split_stride * 4, 16));
      }
#pragma unroll
      for (int qq = 0; qq < QB; ++qq)
        if (q0 + qq < SK)
#pragma unroll
          for (int j = 0; j < E4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[j][r] += v[qq][j][r];  // element by element: no packed FP32 adds
    }
#pragma unroll
    for (int j = 0; j < E4; ++j) {
      const int u = j * NTHR + tid;
      const int tl = u / (MB * 64), rb = (u >> 6) % MB, ln = u & 63;
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(tl * MR + rb * 16 + (ln >> 4) * 4 + r) * RS + (ln & 15)] = sum[j][r];
    }
    if (NORM) {
      for (int r = tid; r < MR; r += NTHR) {
        float t2 = 0.f;
        for (int q = 0; q < SK; ++q)
          t2 += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pr, ((q * CG + cg) * MR + r) * 4, ss_base * 4, 16));
        s_ss[r] = t2;
      }
    }
    splitk_reset(&counters[cg]);
  }
  __syncthreads();
  return true;
}

template <bool NORM>
LSA_DEVICE float w4_coop_rstd(const float* s_ss, int mm, int K, float eps) {
  return NORM ? rsqrtf(s_ss[mm] / (float)K + eps) : 1.f;
}

// The epilogue out of red for 16-B aligned rows (16-B stores and 16-B residual / bias / cos / sin
// loads): one thread per finished 16-column tile row. tlo: the workgroup's first tile; RAGGED: the
// workgroup's last tiles may lie past the NT tiles of the output and are dropped.
template <int MB, int TNW, int NW, int EPI, bool NORM, bool RAGGED>
LSA_DEVICE void w4_coop_epilogue16(const float* red, const float* s_ss, const EpiArgs& ep, int M, int K, float eps,
                                   int tlo, int NT) {
  using Geo = W4CoopGeo<MB, TNW, NW>;
  constexpr int NTHR = Geo::NTHR, MR = Geo::MR, TG = Geo::TG, RS = Geo::RS;
  const int tid = threadIdx.x;
  // rows RS = 20 floats apart: the 16 rows one ds_read_b128 lane group reads start 20 banks apart
  auto load16 = [&](int t, int mm, float r, float* v) {
    const float* rp = red + (t * MR + mm) * RS;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4_t x4 = *reinterpret_cast<const f32x4_t*>(rp + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = x4[j] * r;
    }
  };
  if (EPI == EPI_SWIGLU) {
    // gate tile 2tp / up tile 2tp+1 -> 16 outputs per thread, two 16-B stores (host: TG even, and
    // with RAGGED NT even)
    for (int e = tid; e < (TG / 2) * MR; e += NTHR) {
      const int tp = e / MR, mm = e % MR;
      if (mm >= M || (RAGGED && tlo + 2 * tp >= NT)) continue;
      const float r = w4_coop_rstd<NORM>(s_ss, mm, K, eps);
      float gg[16], uu[16];
      load16(2 * tp, mm, r, gg);
      load16(2 * tp + 1, mm, r, uu);
#pragma unroll
      for (int j = 0; j < 16; ++j) gg[j] = silu(gg[j]) * uu[j];
      bf16_raw* o = ep.out + (size_t)mm * ep.ldo + (tlo / 2 + tp) * 16;
      st16(o, pack8(gg));
      st16(o + 8, pack8(gg + 8));
    }
  } else {
    // epilogue.h epi_row16
    for (int e = tid; e < TG * MR; e += NTHR) {
      const int t = e / MR, mm = e % MR;
      if (mm >= M || (RAGGED && tlo + t >= NT)) continue;
      float v[16];
      load16(t, mm, w4_coop_rstd<NORM>(s_ss, mm, K, eps), v);
      epi_row16<EPI>(ep, mm, (tlo + t) * 16, v);
    }
  }
}
