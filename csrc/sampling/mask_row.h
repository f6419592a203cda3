// What the byte-walking mask kernels (grammar_mask.hip, pda_mask.hip) share: the geometry of a row
// cut into chunks of 512 positions, the 256-bit shift register in which a lane keeps the allow bits
// of the 16-byte logit vectors it will store, the workgroup's count of allowed tokens and the
// stores.
//
// Positions p = column + pad (pad = the row base's offset into its 16-byte line, in elements) are cut
// into chunks of MR_CHUNK; wave w takes the chunks w, w + 16, ... In the walk, lane l takes position
// chunk * 512 + i * 64 + l for i = 0..7 and the wave ballots once per i; lane l keeps byte l & 7 of
// the ballot of i = l >> 3: the eight allow bits of positions chunk * 512 + 8 l ..+7. 32 chunks per
// wave fit the register, so V + pad <= 262144. The stores pop the register in reverse chunk order:
// whole aligned vectors, written only if a column changed, scalar at the two ragged ends.
#pragma once

#include "row_scan.h"

constexpr int MR_THREADS = 1024;
constexpr int MR_WAVES = MR_THREADS / LSA_WAVE;
constexpr int MR_CHUNK = 512;             // positions per wave and trip: 64 vectors of 8
constexpr int MR_REG_WORDS = 8;           // the allow bits of 32 chunks per lane
constexpr int MR_MAX_CHUNKS = MR_REG_WORDS * 4;
constexpr int MR_MAX_V = MR_MAX_CHUNKS * MR_WAVES * MR_CHUNK - 8;
constexpr int MR_EOS_MAX = 8;

// The ballots of a chunk's eight tokens per lane (alive[i]: the lane's token i is allowed) into the
// register; returns how many of the wave's 512 tokens are allowed.
LSA_DEVICE int mr_push(unsigned (&reg)[MR_REG_WORDS], const bool (&alive)[8], int lane) {
  unsigned mine = 0u;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned long long m = __ballot(alive[i]);
    cnt += __popcll(m);
    if ((lane >> 3) == i) mine = (unsigned)(m >> ((lane & 7) * 8)) & 0xffu;
  }
#pragma unroll
  for (int k = MR_REG_WORDS - 1; k > 0; --k) reg[k] = (reg[k] << 8) | (reg[k - 1] >> 24);
  reg[0] = (reg[0] << 8) | mine;
  return cnt;
}

// The workgroup's sum of the waves' counts (sh_cnt: MR_WAVES ints of LDS). Every thread calls it.
LSA_DEVICE int mr_total(int cnt, int* sh_cnt, int wave, int lane) {
  if (lane == 0) sh_cnt[wave] = cnt;
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < MR_WAVES; ++w) n += sh_cnt[w];
  return n;
}

// The stores of the wave's chunks, newest first: a column whose bit is clear and whose logit is not
// already -inf becomes -inf.
LSA_DEVICE void mr_store(bf16_raw* __restrict__ row, int V, int pad, int nchunk, unsigned (&reg)[MR_REG_WORDS],
                         int wave, int lane) {
  const int last = nchunk - 1 - ((nchunk - 1 - wave) % MR_WAVES + MR_WAVES) % MR_WAVES;  // the wave's last chunk
  for (int c = last; c >= wave; c -= MR_WAVES) {
    const unsigned bits = reg[0] & 0xffu;
#pragma unroll
    for (int k = 0; k < MR_REG_WORDS - 1; ++k) reg[k] = (reg[k] >> 8) | (reg[k + 1] << 24);
    reg[MR_REG_WORDS - 1] >>= 8;
    const int v0 = c * MR_CHUNK + lane * 8 - pad;
    if (v0 >= V || v0 + 8 <= 0 || bits == 0xffu) continue;
    if (v0 >= 0 && v0 + 8 <= V) {
      u32x4_t lv = ld16(row + v0);
      bool ch = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned l0 = lv[j] & 0xffffu, l1 = lv[j] >> 16;
        if (!(bits >> (2 * j) & 1u) && l0 != BF16_NEG_INF) { l0 = BF16_NEG_INF; ch = true; }
        if (!(bits >> (2 * j + 1) & 1u) && l1 != BF16_NEG_INF) { l1 = BF16_NEG_INF; ch = true; }
        lv[j] = l0 | (l1 << 16);
      }
      if (ch) st16(row + v0, lv);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = v0 + j;
        if (v >= 0 && v < V && !(bits >> j & 1u) && row[v] != (bf16_raw)BF16_NEG_INF) row[v] = (bf16_raw)BF16_NEG_INF;
      }
    }
  }
}
