// Per-token log-probabilities and top-N alternatives of bf16 logits on gfx950 (CDNA4 / MI355X).
//
//   lsa_logprobs  one workgroup per row: log-sum-exp of the row, the log-probability and rank of
//                 a target token and the n largest logits with their log-probabilities. In a
//                 decode step it runs behind lsa_sample / lsa_argmax_finalize (sampling.hip,
//                 whose contract is unchanged) on the row lsa_sample has just read, with the
//                 freshly written token as the target.
//
// Contract per row r (bf16 logits l[0..V) in a row of ld >= V columns; columns >= V are never
// read; n_top[r] < 0: the row is skipped and none of its outputs is written):
//   lse       = max + ln(sum_{v < V} exp(l_v - max)); a -inf logit contributes nothing
//               (+inf and NaN logits are outside the contract)
//   tok_lp    = l_t - lse for t = target[r]; t < 0 or t >= V: tok_lp / tok_rank are not written
//   tok_rank  = 1 + #{v < V : l_v > l_t}, on the bf16 values (-0 == +0): an exact integer
//   top_id    [0, n), n = min(n_top[r], TOP_MAX, V): the n largest logits in descending order,
//             equal logits by ascending index; top_lp their log-probabilities;
//             entries [n, TOP_MAX) are -1 / -inf
//
// Determinism: every quantity is an integer count, a maximum, or a sum of 32-bit fixed-point
// masses floor(exp(l - max) * 2^32) in 64-bit integers (per thread, then shuffles and one LDS
// atomic per wave): integer addition is associative, so a row's outputs are bitwise the same on
// every launch, in any row of any batch.
//
// Accuracy (derived; the tests assert 1e-4 absolute for V <= 2^17): S = sum exp(l - max) >= 1.
// Flooring each term to 2^-32 lowers S by at most V * 2^-32 (3.0e-5 at V = 128256), which moves
// ln S by at most that much. expf / logf at a few ulp and the fp32 rounding of S add ~3e-7.
// log-probabilities are formed as (l - max) - ln S: the difference of two bf16 values is exact in
// fp32 for |l| within a factor 2^16 of each other and otherwise rounds at 2^-24 relative, and the
// final subtraction at |lp| <= 200 rounds at 200 * 2^-24 = 1.2e-5. lse = max + ln S rounds at
// |lse| * 2^-24. Sum < 5e-5.
//
// Top-n selection is a radix select on the composite (16-bit order-preserving key of the logit,
// inverted column index): two 8-bit count-histogram levels over the key (high byte, then the low
// byte inside the boundary bin) give the n-th largest value; if more entries tie at that value
// than are still needed, up to four more 8-bit levels over the inverted index (only as many as
// V - 1 has bytes) pick the lowest indices. All composites are distinct, so exactly n entries lie
// at or above the threshold; they are collected into LDS and ordered by rank counting. The row
// is re-read from L2 per pass: 2 passes for n = 0, 3 for n > 0, + 1 per index level on ties.
#include "row_scan.h"

namespace {

constexpr int LP_THREADS = 512;
constexpr int LP_TOP_MAX = 20;

__global__ __launch_bounds__(LP_THREADS) void logprobs_kernel(
    const bf16_raw* __restrict__ logits, long long ld, int V, const int* __restrict__ n_top,
    const int* __restrict__ target, float* __restrict__ lse, float* __restrict__ tok_lp, int* __restrict__ tok_rank,
    int* __restrict__ top_id, float* __restrict__ top_lp, float* __restrict__ lp_hist, int hist_stride, int hist_len,
    const int* __restrict__ step_ctr) {
  __shared__ unsigned long long s_list[LP_TOP_MAX];
  __shared__ unsigned long long s_sum;
  __shared__ unsigned s_cnt[256];
  __shared__ unsigned s_find[3];
  __shared__ unsigned s_kmax, s_rank, s_n;

  const int r = blockIdx.x, tid = threadIdx.x;
  const int nt = n_top[r];
  if (nt < 0) return;
  const int n = nt < LP_TOP_MAX ? (nt < V ? nt : V) : (LP_TOP_MAX < V ? LP_TOP_MAX : V);
  const bf16_raw* row = logits + (size_t)r * (size_t)ld;
  const int t = target[r];
  const bool has_t = t >= 0 && t < V;
  const unsigned kt = has_t ? key16((unsigned)row[t]) : 0xffffu;

  // pass 1: maximum key, the target's rank and (n > 0) the count histogram of the high bytes
  if (tid < 256) s_cnt[tid] = 0u;
  if (tid == 0) {
    s_kmax = 0u;
    s_rank = 0u;
    s_n = 0u;
    s_sum = 0ull;
  }
  __syncthreads();
  unsigned kbest = 0u, above_t = 0u;
  for_row<LP_THREADS>(row, V, [&](int, unsigned raw) {
    const unsigned k = key16(raw);
    kbest = k > kbest ? k : kbest;
    above_t += k > kt ? 1u : 0u;
    if (n > 0) atomicAdd(&s_cnt[k >> 8], 1u);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned kb = __shfl_xor(kbest, o, 64), ab = __shfl_xor(above_t, o, 64);
    kbest = kb > kbest ? kb : kbest;
    above_t += ab;
  }
  if ((tid & 63) == 0) {
    atomicMax(&s_kmax, kbest);
    atomicAdd(&s_rank, above_t);
  }
  __syncthreads();
  const unsigned kmax = s_kmax;
  const float lmax = bf2f((bf16_raw)raw_of_key16(kmax));

  unsigned hb = 0u, above = 0u;
  if (n > 0) {
    if (tid < 64) find_bin<true>(s_cnt, 0u, (unsigned)n, s_find);
    __syncthreads();
    hb = s_find[0];
    above = s_find[1];
    __syncthreads();
    if (tid < 256) s_cnt[tid] = 0u;
    __syncthreads();
  }

  // pass 2: the fixed-point mass and (n > 0) the low-byte histogram inside the boundary bin
  unsigned long long mass = 0ull;
  for_row<LP_THREADS>(row, V, [&](int, unsigned raw) {
    const float w = expf(bf2f((bf16_raw)raw) - lmax);
    mass += (unsigned long long)(w * 4294967296.0f);
    if (n > 0) {
      const unsigned k = key16(raw);
      if ((k >> 8) == hb) atomicAdd(&s_cnt[k & 255u], 1u);
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o, 64);
  if ((tid & 63) == 0) atomicAdd(&s_sum, mass);
  __syncthreads();
  const float lnS = logf((float)((double)s_sum * 2.3283064365386963e-10));  // * 2^-32

  if (tid == 0) {
    lse[r] = lmax + lnS;
    if (has_t) {
      const float lp = (bf2f((bf16_raw)raw_of_key16(kt)) - lmax) - lnS;
      tok_lp[r] = lp;
      tok_rank[r] = (int)s_rank + 1;
      if (lp_hist) {  // beside the token history: lsa_argmax_finalize has already advanced the counter
        const int step = *step_ctr - 1;
        if (step >= 0 && step < hist_len) lp_hist[(size_t)step * hist_stride + r] = lp;
      }
    }
  }
  if (tid >= LP_THREADS - LP_TOP_MAX) {  // the -1 / -inf tail
    const int j = tid - (LP_THREADS - LP_TOP_MAX);
    if (j >= n) {
      top_id[(size_t)r * LP_TOP_MAX + j] = -1;
      top_lp[(size_t)r * LP_TOP_MAX + j] = -__builtin_inff();
    }
  }
  if (n == 0) return;

  // threshold key tk = the n-th largest key; `above` entries are strictly larger
  if (tid < 64) find_bin<true>(s_cnt, above, (unsigned)n, s_find);
  __syncthreads();
  const unsigned tk = (hb << 8) | s_find[0];
  above = s_find[1];
  const unsigned tied = s_find[2];
  __syncthreads();

  // more entries tie at tk than are needed: radix select over the inverted index q = V - 1 - i
  // (a larger q is a lower index), most significant byte of V - 1 first
  unsigned qthr = 0u;
  if (above + tied > (unsigned)n) {
    const unsigned vm = (unsigned)(V - 1);
    int level = vm >> 24 ? 3 : (vm >> 16 ? 2 : (vm >> 8 ? 1 : 0));
    for (; level >= 0; --level) {
      const int sh = 8 * level;
      if (tid < 256) s_cnt[tid] = 0u;
      __syncthreads();
      for_row<LP_THREADS>(row, V, [&](int i, unsigned raw) {
        if (key16(raw) == tk) {
          const unsigned q = vm - (unsigned)i;
          // bytes above this level match the prefix found so far (sh + 8 == 32: no such bytes)
          if (level == 3 || (q >> (sh + 8)) == (qthr >> (sh + 8))) atomicAdd(&s_cnt[(q >> sh) & 255u], 1u);
        }
      });
      __syncthreads();
      if (tid < 64) find_bin<true>(s_cnt, above, (unsigned)n, s_find);
      __syncthreads();
      qthr |= s_find[0] << sh;
      above = s_find[1];
      __syncthreads();
    }
  }

  // collect the n winners (composite >= (tk, qthr)) and order them by rank counting
  for_row<LP_THREADS>(row, V, [&](int i, unsigned raw) {
    const unsigned k = key16(raw), q = (unsigned)(V - 1) - (unsigned)i;
    if (k > tk || (k == tk && q >= qthr)) {
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)LP_TOP_MAX) s_list[slot] = ((unsigned long long)k << 32) | (unsigned long long)q;
    }
  });
  __syncthreads();
  const int got = (int)(s_n < (unsigned)n ? s_n : (unsigned)n);
  if (tid < got) {
    const unsigned long long c = s_list[tid];
    int rank = 0;
    for (int j = 0; j < got; ++j) rank += s_list[j] > c ? 1 : 0;
    const unsigned k = (unsigned)(c >> 32), q = (unsigned)(c & 0xffffffffull);
    top_id[(size_t)r * LP_TOP_MAX + rank] = (int)((unsigned)(V - 1) - q);
    top_lp[(size_t)r * LP_TOP_MAX + rank] = (bf2f((bf16_raw)raw_of_key16(k)) - lmax) - lnS;
  }
}

}  // namespace

// logits bf16 [rows][ld]; n_top / target int32 [rows]; lse / tok_lp fp32 [rows]; tok_rank int32
// [rows]; top_id int32 [rows][20]; top_lp fp32 [rows][20]. lp_hist (optional) fp32
// [hist_len][hist_stride >= rows] with step_ctr, the device-side step counter of
// lsa_argmax_finalize read after its increment: tok_lp is also stored at lp_hist[*step_ctr - 1][r].
extern "C" int lsa_logprobs(const void* logits, long long ld, int V, int rows, const int* n_top, const int* target,
                            float* lse, float* tok_lp, int* tok_rank, int* top_id, float* top_lp, float* lp_hist,
                            int hist_stride, int hist_len, const int* step_ctr, hipStream_t stream) {
  if (rows < 1 || rows > 65535 || V < 1 || ld < (long long)V) return LSA_BAD_SHAPE;
  if (!logits || !n_top || !target || !lse || !tok_lp || !tok_rank || !top_id || !top_lp) return LSA_BAD_SHAPE;
  if (lp_hist && (!step_ctr || hist_stride < rows || hist_len < 1)) return LSA_BAD_SHAPE;
  logprobs_kernel<<<rows, LP_THREADS, 0, stream>>>(static_cast<const bf16_raw*>(logits), ld, V, n_top, target, lse,
                                                   tok_lp, tok_rank, top_id, top_lp, lp_hist, hist_stride, hist_len,
                                                   step_ctr);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
