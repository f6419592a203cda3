// Seeded temperature / top-k / top-p sampling of bf16 logits on gfx950 (CDNA4 / MI355X).
//
//   lsa_sample        one workgroup per row: threshold search over the vocabulary + a
//                     counter-based Gumbel-max draw; writes the chosen token as a common.h
//                     argmax_key into keys_out[r], so lsa_argmax_finalize does the token /
//                     position / history bookkeeping exactly as for the greedy argmax.
//   lsa_sample_noise  debug entry: the raw Philox words and Gumbel values of a range of
//                     vocabulary indices (or the Gumbel values of given words).
//
// Contract per row r (bf16 logits l[0..V) in a row of ld >= V columns; columns >= V are never
// read as candidates - the packed lm_head pads the vocabulary with copies of row 0):
//   T == 0      greedy: arg-max of l, lowest index on ties; no noise, filters ignored
//   z = l / T
//   top-k       (0 < k < V) keep z_i >= the k-th largest value (all ties at the threshold kept)
//   top-p       (p < 1) over the softmax of the top-k survivors: z* = the largest value with
//               mass{z_i >= z*} >= p; keep z_i >= z*
//   draw        token = argmax over kept i of z_i + g_i (lowest index on exact ties),
//               g_i = -log(-log(u_i)), u_i = ((x_i >> 9) + 0.5) * 2^-23,
//               x_i = word (i & 3) of Philox4x32-10(counter (i >> 2, c[r], 0, 0), key = seed[r])
// The noise is a pure function of (seed, counter, vocabulary index): a row's token does not
// depend on the row index, the batch size or how the row is split over threads.
//
// T > 0 makes z monotone in the bf16 bit pattern, so both thresholds are found on an
// order-preserving 16-bit key with two 8-bit histogram levels (high byte, then the low byte
// inside the boundary bin). Counts are integers and masses are exp((l - max) / T) as 32-bit
// fixed point summed by 64-bit integer LDS atomics: sums do not depend on arrival order, so the
// same inputs give bitwise the same token on every launch. The row is re-read from L2 per pass.
#include "row_scan.h"

namespace {

constexpr int SAMPLE_THREADS = 512;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / LSA_WAVE;

// ---------------------------------------------------------------------------- Philox4x32-10
struct Philox4 { unsigned x[4]; };

LSA_DEVICE Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.x[0] = c0; o.x[1] = c1; o.x[2] = c2; o.x[3] = c3;
  return o;
}

// u = ((x >> 9) + 0.5) * 2^-23 = (2 (x >> 9) + 1) * 2^-24: exact in fp32, in [2^-24, 1 - 2^-24].
// Accurate logf on both levels: -log(u) is ~6e-8 for u next to 1, where a fast log is far off.
LSA_DEVICE float gumbel_from_bits(unsigned x) {
  const float u = (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f;
  return -logf(-logf(u));
}

LSA_DEVICE unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// Workgroup max of 64-bit keys through s_red[SAMPLE_WAVES]; every thread gets the result.
LSA_DEVICE unsigned long long block_max_u64(unsigned long long v, unsigned long long* s_red) {
  v = wave_max_u64(v);
  __syncthreads();  // s_red may still be read from a previous reduction
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = s_red[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) m = s_red[w] > m ? s_red[w] : m;
  return m;
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    const bf16_raw* __restrict__ logits, long long ld, int V, const float* __restrict__ temp,
    const int* __restrict__ top_k, const float* __restrict__ top_p, const unsigned long long* __restrict__ seed,
    const int* __restrict__ ctr, int ctr_add, unsigned long long* __restrict__ keys_out, int* __restrict__ dbg) {
  __shared__ unsigned long long s_mass[256];
  __shared__ unsigned long long s_red[SAMPLE_WAVES];
  __shared__ unsigned long long s_find[2];
  __shared__ unsigned s_cnt[256];
  __shared__ unsigned s_kept;

  const int r = blockIdx.x, tid = threadIdx.x;
  const bf16_raw* row = logits + (size_t)r * (size_t)ld;
  const float T = temp[r];

  // pass 1: maximum (with its lowest index) and, for top-k, the count histogram of the keys'
  // high bytes (its LDS atomics are the pass's cost: skipped when top-k is off)
  const int k_top = top_k[r];
  const bool use_k = T > 0.f && k_top > 0 && k_top < V;
  s_cnt[tid & 255] = 0u;
  if (tid == 0) s_kept = 0u;
  __syncthreads();
  unsigned long long best = 0ull;
  for_row<SAMPLE_THREADS>(row, V, [&](int i, unsigned raw) {
    const unsigned k = key16(raw);
    const unsigned long long kk = ((unsigned long long)k << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
    best = kk > best ? kk : best;
    if (use_k) atomicAdd(&s_cnt[k >> 8], 1u);
  });
  best = block_max_u64(best, s_red);
  const unsigned kmax = (unsigned)(best >> 32);
  const unsigned imax = 0xffffffffu - (unsigned)(best & 0xffffffffull);
  const float lmax = bf2f((bf16_raw)raw_of_key16(kmax));
  const unsigned long long greedy_key = argmax_key(lmax, imax);

  if (!(T > 0.f)) {  // greedy row
    if (tid == 0) {
      keys_out[r] = greedy_key;
      if (dbg) {
        dbg[2 * r] = (int)kmax;
        dbg[2 * r + 1] = 1;
      }
    }
    return;
  }

  // top-k: threshold key tk = the k-th largest key (0: everything survives)
  unsigned tk = 0u;
  if (use_k) {
    if (tid < 64) find_bin(s_cnt, 0ull, (unsigned long long)k_top, s_find);
    __syncthreads();
    const unsigned hb = (unsigned)s_find[0];
    const unsigned long long above = s_find[1];
    __syncthreads();
    s_cnt[tid & 255] = 0u;
    __syncthreads();
    for_row<SAMPLE_THREADS>(row, V, [&](int, unsigned raw) {
      const unsigned k = key16(raw);
      if ((k >> 8) == hb) atomicAdd(&s_cnt[k & 255u], 1u);
    });
    __syncthreads();
    if (tid < 64) find_bin(s_cnt, above, (unsigned long long)k_top, s_find);
    __syncthreads();
    tk = (hb << 8) | (unsigned)s_find[0];
    __syncthreads();
  }

  // top-p over the survivors: masses as 32-bit fixed point in 64-bit integer sums
  unsigned thr = tk;
  const float p = top_p[r];
  if (p < 1.f) {
    if (tid < 256) s_mass[tid] = 0ull;
    __syncthreads();
    for_row<SAMPLE_THREADS>(row, V, [&](int, unsigned raw) {
      const unsigned k = key16(raw);
      if (k >= tk) {
        const float w = expf((bf2f((bf16_raw)raw) - lmax) / T);
        atomicAdd(&s_mass[k >> 8], (unsigned long long)(w * 4294967296.0f));
      }
    });
    __syncthreads();
    // total mass (wave 0) -> target = ceil(p * total), at least 1
    if (tid < 64) {
      unsigned long long s = s_mass[4 * tid] + s_mass[4 * tid + 1] + s_mass[4 * tid + 2] + s_mass[4 * tid + 3];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const double td = ceil((double)p * (double)s);
      unsigned long long target = td < 1.0 ? 1ull : (unsigned long long)td;
      if (target > s) target = s;
      find_bin(s_mass, 0ull, target, s_find);
      if (tid == 0) s_red[0] = target;  // s_red is free between block reductions
    }
    __syncthreads();
    const unsigned hb = (unsigned)s_find[0];
    const unsigned long long above = s_find[1];
    const unsigned long long target = s_red[0];
    __syncthreads();
    if (tid < 256) s_mass[tid] = 0ull;
    __syncthreads();
    for_row<SAMPLE_THREADS>(row, V, [&](int, unsigned raw) {
      const unsigned k = key16(raw);
      if (k >= tk && (k >> 8) == hb) {
        const float w = expf((bf2f((bf16_raw)raw) - lmax) / T);
        atomicAdd(&s_mass[k & 255u], (unsigned long long)(w * 4294967296.0f));
      }
    });
    __syncthreads();
    if (tid < 64) find_bin(s_mass, above, target, s_find);
    __syncthreads();
    const unsigned tp = (hb << 8) | (unsigned)s_find[0];
    thr = tp > tk ? tp : tk;
    __syncthreads();
  }

  // draw: Gumbel noise for the kept tokens only, reduced with 64-bit max keys
  const unsigned long long sd = seed[r];
  const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32);
  const unsigned c1 = (unsigned)(ctr[r] + ctr_add);
  unsigned long long win = 0ull;
  unsigned kept = 0u, blk_cached = 0xffffffffu;
  Philox4 px = {};
  for_row<SAMPLE_THREADS>(row, V, [&](int i, unsigned raw) {
    if (key16(raw) >= thr) {
      ++kept;
      const unsigned blk = (unsigned)i >> 2;
      if (blk != blk_cached) {
        px = philox4x32_10(blk, c1, 0u, 0u, k0, k1);
        blk_cached = blk;
      }
      const unsigned w = i & 3;
      const unsigned x = w == 0 ? px.x[0] : (w == 1 ? px.x[1] : (w == 2 ? px.x[2] : px.x[3]));
      const float score = bf2f((bf16_raw)raw) / T + gumbel_from_bits(x);
      const unsigned long long kk = argmax_key(score, (unsigned)i);
      win = kk > win ? kk : win;
    }
  });
  if (dbg && kept) atomicAdd(&s_kept, kept);
  win = block_max_u64(win, s_red);  // (its barriers also order the s_kept adds)
  if (tid == 0) {
    keys_out[r] = win ? win : greedy_key;
    if (dbg) {
      dbg[2 * r] = (int)thr;
      dbg[2 * r + 1] = (int)s_kept;
    }
  }
}

__global__ __launch_bounds__(256) void sample_noise_kernel(unsigned long long sd, unsigned c1, unsigned idx0, int n,
                                                           const unsigned* __restrict__ bits_in,
                                                           unsigned* __restrict__ bits_out, float* __restrict__ g_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  unsigned x;
  if (bits_in) {
    x = bits_in[t];
  } else {
    const unsigned i = idx0 + (unsigned)t;
    const Philox4 px = philox4x32_10(i >> 2, c1, 0u, 0u, (unsigned)sd, (unsigned)(sd >> 32));
    const unsigned w = i & 3;
    x = w == 0 ? px.x[0] : (w == 1 ? px.x[1] : (w == 2 ? px.x[2] : px.x[3]));
  }
  if (bits_out) bits_out[t] = x;
  if (g_out) g_out[t] = gumbel_from_bits(x);
}

}  // namespace

// logits bf16 [rows][ld]; T / top_p fp32 [rows]; top_k / ctr int32 [rows]; seed u64 [rows];
// keys_out u64 [rows]; dbg (optional) int32 [rows][2] = (16-bit threshold key, kept count): the
// lowest kept key (0 when neither filter is on; the maximum's key, count 1, on a greedy row).
// The row's Philox counter is ctr[r] + ctr_add: the position the sampled token will occupy.
extern "C" int lsa_sample(const void* logits, long long ld, int V, int rows, const float* T, const int* top_k,
                          const float* top_p, const unsigned long long* seed, const int* ctr, int ctr_add,
                          unsigned long long* keys_out, int* dbg, hipStream_t stream) {
  if (rows < 1 || rows > 65535 || V < 1 || ld < (long long)V) return LSA_BAD_SHAPE;
  if (!logits || !T || !top_k || !top_p || !seed || !ctr || !keys_out) return LSA_BAD_SHAPE;
  sample_kernel<<<rows, SAMPLE_THREADS, 0, stream>>>(static_cast<const bf16_raw*>(logits), ld, V, T, top_k, top_p, seed,
                                                     ctr, ctr_add, keys_out, dbg);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

extern "C" int lsa_sample_noise(unsigned long long seed, unsigned ctr, unsigned idx0, int n, const unsigned* bits_in,
                                unsigned* bits_out, float* g_out, hipStream_t stream) {
  if (n < 1 || (!bits_out && !g_out)) return LSA_BAD_SHAPE;
  sample_noise_kernel<<<(n + 255) / 256, 256, 0, stream>>>(seed, ctr, idx0, n, bits_in, bits_out, g_out);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
