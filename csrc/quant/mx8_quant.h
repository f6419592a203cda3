// The MXFP8 activation quantiser of the W4A8 kernels (ops/mx4.py quantize_act_mx8), shared by
// gemv_mx4.hip (in-kernel staging) and gemm_mx4.hip (the pre-pass): a quad of lanes holds one
// 32-block as 4 x 8 fp32 values.
#pragma once
#include "../kernels/common.h"

// 4 fp32 -> one dword of e4m3 codes (round to nearest even)
LSA_DEVICE unsigned pack4_fp8(const float* y) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  return (unsigned)w;
}

// This lane's 8 values of the block -> its 8 codes; returns the block's e8m0 byte (the same in
// all four lanes of the quad): E - 7 with E the fp32 exponent field of the block's largest
// magnitude clamped to >= 8, 127 for an all-zero block. The scale is an exact power of two.
LSA_DEVICE int mx8_quant_quad(const float* f, u32x2_t& c) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  amax = fmaxf(amax, dpp_mov<0xB1>(amax));  // quad_perm [1,0,3,2]
  amax = fmaxf(amax, dpp_mov<0x4E>(amax));  // quad_perm [2,3,0,1]
  int e = (int)(__float_as_uint(amax) >> 23);
  e = (e < 8 ? 8 : e) - 7;
  if (amax == 0.f) e = 127;
  const float inv = __uint_as_float((unsigned)(254 - e) << 23);
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = f[j] * inv;
  c[0] = pack4_fp8(y);
  c[1] = pack4_fp8(y + 4);
  return e;
}
