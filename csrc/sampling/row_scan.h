// Row-scan helpers shared by the sampling kernels (sampling.hip, logprobs.hip): the
// order-preserving 16-bit key of a bf16 logit, the sweep over a row's columns and the wave-0
// search of a 256-bin histogram that both radix selects are built on.
#pragma once

#include "../kernels/common.h"

constexpr unsigned BF16_NEG_INF = 0xFF80u;  // bf16 -inf

// Order-preserving key of a bf16 pattern (larger value -> larger key); -0 counts as +0, so
// values that compare equal share one key.
LSA_DEVICE unsigned key16(unsigned raw) {
  if (raw == 0x8000u) raw = 0u;
  return (raw & 0x8000u) ? (~raw & 0xffffu) : (raw | 0x8000u);
}
LSA_DEVICE unsigned raw_of_key16(unsigned k) { return (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu); }

// f(index, raw bf16) for every column < V of the row, by a workgroup of THREADS threads: 16-byte
// loads over the 8-aligned body when the row starts 16-byte aligned, scalar loads otherwise and
// for the tail.
template <int THREADS, typename F>
LSA_DEVICE void for_row(const bf16_raw* __restrict__ row, int V, F&& f) {
  const int tid = threadIdx.x;
  const int nvec = ((reinterpret_cast<size_t>(row) & 15) == 0) ? (V >> 3) : 0;
  for (int c = tid; c < nvec; c += THREADS) {
    const u32x4_t v = ld16(row + (size_t)c * 8);
    const unsigned w[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(c * 8 + 2 * j, w[j] & 0xffffu);
      f(c * 8 + 2 * j + 1, w[j] >> 16);
    }
  }
  for (int i = nvec * 8 + tid; i < V; i += THREADS) f(i, (unsigned)row[i]);
}

// Wave 0 (threads 0..63): the largest bin b of h[0..256) with  base + sum_{j >= b} h[j] >= target
// and the sum strictly above it, written to out[0] = b, out[1] = base + sum_{j > b} h[j] and,
// with AT, out[2] = h[b]. H is the histogram's element type, A the accumulator's (unsigned for
// counts, unsigned long long for fixed-point masses). target >= 1; if even bin 0 does not reach it
// (cannot happen for a target <= base + the total) bin 0 is returned.
template <bool AT = false, typename H, typename A>
LSA_DEVICE void find_bin(const H* h, A base, A target, A* out) {
  const int lane = threadIdx.x;
  A v[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (A)h[4 * lane + j];
    s += v[j];
  }
  A suf = s;  // sum over lanes >= lane
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const A t = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += t;
  }
  A acc = base + (suf - s), above = 0, at = 0;
  int b = -1;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    const A a0 = acc;
    acc += v[j];
    if (b < 0 && acc >= target) {
      b = 4 * lane + j;
      above = a0;
      at = v[j];
    }
  }
  const unsigned long long found = __ballot(b >= 0);
  if (found == 0ull) {
    if (lane == 0) {
      out[0] = (A)0;
      out[1] = acc - v[0];
      if (AT) out[2] = v[0];
    }
    return;
  }
  const int top = 63 - __clzll((long long)found);
  if (lane == top) {
    out[0] = (A)b;
    out[1] = above;
    if (AT) out[2] = at;
  }
}
