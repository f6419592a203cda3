// Speculative decoding around the decode step on gfx950 (CDNA4 / MI355X): draft k tokens per
// sequence from the sequence's own history (or from a script), and after the model has run the
// k + 1 rows accept the longest prefix of the drafts the model agrees with. Both kernels read and
// write device state only, so draft -> embed -> layers -> head -> accept is captured once and
// replayed with no host work per step.
//
//   lsa_spec_draft   one workgroup per sequence: rows' tokens / positions of the next step
//   lsa_spec_accept  one thread per sequence: accepted count, history append, finished flag
//
// State. `hist` int32 [n_seq, ld] (ld >= max_seq): the known tokens of sequence s, prompt +
// accepted; `hlen` [n_seq] their number; `limit` [n_seq] the absolute cap on hlen; `done` [n_seq];
// `eos` [8] end-of-sequence ids padded with -1; `tokens`, `pos` [rows], rows = n_seq * (k + 1),
// row r0 + j with r0 = s * (k + 1) belongs to sequence s; `script` [n_seq, ld] (optional) a
// proposed token per absolute position; `cand` [rows] the model's token per row.
// Invariant: the KV cache of the sequence's slot holds positions [0, hlen - 1); the last known
// token has not been fed yet.
//
// Both kernels take L = min(max(hlen[s], 1), ld), which is hlen[s] itself for every state the
// contract allows (the clamp only keeps the kernels' own accesses inside the row of hist). The
// caller guarantees limit[s] + k <= max_seq: hlen never passes limit, so no row carries a position
// outside [0, max_seq) (the attention kernels read pos + 1 keys).
//
// Draft. Row 0: tokens = hist[L-1], pos = L-1. Row j (1..k): draft d[j-1], pos = L-1+j.
//  * lookup (script == null), 1 <= nmin <= nmax <= 8: for every end position e in [0, L-2], m(e) =
//    the largest m <= nmax with e - t >= 0 and hist[e-t] == hist[L-1-t] for all t < m. Among e with
//    m(e) >= nmin the maximum of the 64-bit key (m(e) << 32) | e wins (the longest match, the most
//    recent among equals; an integer max-reduction, so deterministic). With c = e + 1:
//    d[j] = hist[c+j] if c + j < L, else d[c+j-L] - the continuation runs on through the drafts
//    themselves, i.e. d[j] = hist[c + j mod (L - c)]. No match (or L < 2): d[j] = hist[L-1].
//    matched[s] = the winning m (0: none).
//  * script: d[j] = script[s, L+j] if L + j < ld, else 0; matched[s] = 1.
//  A done sequence is drafted like any other. match_ctr[s] (optional) counts the steps of a
//  sequence that is not done in which matched[s] != 0.
//
// Accept. If done[s]: n_acc[s] = 0, nothing else of the sequence is written. Otherwise a = the
// number of leading j in [0, k) with tokens[r0+j+1] == cand[r0+j]; m = min(a + 1, limit[s] - L)
// (and never beyond the row of hist: m <= ld - L); the first j < m whose cand[r0+j] is an EOS id
// makes m = j + 1 and done = 1; L + m == limit[s] makes done = 1 (so does m <= 0, with m = 0);
// hist[s, L .. L+m) = cand[r0 .. r0+m), hlen[s] = L + m, n_acc[s] = m and, with a history buffer,
// acc_history[step, s] = m for step = *step_ctr < hist_len. *step_ctr advances by one per launch.
// Cells of hist at >= L + m keep their contents.
//
// Refused with LSA_BAD_SHAPE before any launch: k outside [1, 15], n_seq * (k + 1) above 128 (the
// decode path's row limit), nmin / nmax outside 1 <= nmin <= nmax <= 8, ld < max_seq, a null
// pointer among the required arrays.
#include "../kernels/common.h"

namespace {

constexpr int SPD_THREADS = 1024;  // positions of the history compared per pass (max_seq 4096: 4 passes)
constexpr int SPD_WAVES = SPD_THREADS / LSA_WAVE;
constexpr int SPD_MAX_K = 15;
constexpr int SPD_MAX_ROWS = 128;  // StageEngine.DECODE_MAX_ROWS
constexpr int SPD_MAX_NGRAM = 8;
constexpr int SPD_EOS = 8;

LSA_DEVICE int clamp_len(int L, long long ld) {
  L = L < 1 ? 1 : L;
  return (long long)L > ld ? (int)ld : L;
}

__global__ __launch_bounds__(SPD_THREADS) void spec_draft_kernel(
    const int* __restrict__ hist, long long ld, const int* __restrict__ hlen, int k, int nmin, int nmax,
    const int* __restrict__ script, int* __restrict__ tokens, int* __restrict__ pos,
    int* __restrict__ matched, const int* __restrict__ done, int* __restrict__ match_ctr) {
  __shared__ long long s_best[SPD_WAVES];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int* h = hist + (size_t)s * (size_t)ld;
  const int L = clamp_len(hlen[s], ld);
  const int r0 = s * (k + 1);
  const int last = h[L - 1];
  long long best = -1;
  if (script == nullptr) {
    int suf[SPD_MAX_NGRAM];
#pragma unroll
    for (int t = 0; t < SPD_MAX_NGRAM; ++t) suf[t] = (t < nmax && L - 1 - t >= 0) ? h[L - 1 - t] : -1;
    for (int e = tid; e <= L - 2; e += SPD_THREADS) {
      if (h[e] != suf[0]) continue;
      int m = 1;
      bool go = true;
#pragma unroll
      for (int t = 1; t < SPD_MAX_NGRAM; ++t) {
        go = go && t < nmax && e - t >= 0 && h[e - t] == suf[t];
        m += go ? 1 : 0;
      }
      if (m >= nmin) {
        const long long key = ((long long)m << 32) | (long long)e;
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long other = __shfl_xor(best, o, LSA_WAVE);
      best = other > best ? other : best;
    }
    if ((tid & (LSA_WAVE - 1)) == 0) s_best[tid / LSA_WAVE] = best;
    __syncthreads();
    best = s_best[0];
#pragma unroll
    for (int w = 1; w < SPD_WAVES; ++w) best = s_best[w] > best ? s_best[w] : best;
  }
  const int m_best = script != nullptr ? 1 : (best < 0 ? 0 : (int)(best >> 32));
  if (tid == 0) {
    tokens[r0] = last;
    pos[r0] = L - 1;
    if (matched) matched[s] = m_best;
    if (match_ctr && m_best != 0 && !(done && done[s] != 0)) match_ctr[s] += 1;
  } else if (tid <= k) {
    const int j = tid - 1;
    int d;
    if (script != nullptr) {
      d = (long long)L + j < ld ? script[(size_t)s * (size_t)ld + (size_t)(L + j)] : 0;
    } else if (best < 0) {
      d = last;
    } else {
      const int c = (int)(best & 0xffffffffll) + 1;  // c <= L - 1: the period L - c is >= 1
      d = h[c + j % (L - c)];
    }
    tokens[r0 + tid] = d;
    pos[r0 + tid] = L - 1 + tid;
  }
}

__global__ __launch_bounds__(LSA_WAVE) void spec_accept_kernel(
    int* __restrict__ hist, long long ld, int* __restrict__ hlen, const int* __restrict__ limit,
    int* __restrict__ done, const int* __restrict__ eos, const int* __restrict__ tokens,
    const int* __restrict__ cand, int n_seq, int k, int* __restrict__ n_acc,
    int* __restrict__ acc_history, int hist_stride, int hist_len, int* __restrict__ step_ctr) {
  const int s = threadIdx.x;
  int step = 0;
  if (step_ctr) step = *step_ctr;
  __syncthreads();
  if (s < n_seq) {
    if (done[s] != 0) {
      n_acc[s] = 0;
    } else {
      const int L = clamp_len(hlen[s], ld);
      const int r0 = s * (k + 1);
      int a = 0;
      while (a < k && tokens[r0 + a + 1] == cand[r0 + a]) ++a;
      int m = a + 1;
      const int room = limit[s] - L;
      m = m < room ? m : room;
      m = (long long)m < ld - L ? m : (int)(ld - L);
      int fin = 0;
      if (m <= 0) {
        m = 0;
        fin = 1;
      }
      int e[SPD_EOS];
#pragma unroll
      for (int q = 0; q < SPD_EOS; ++q) e[q] = eos[q];
      for (int j = 0; j < m; ++j) {
        const int c = cand[r0 + j];
        bool hit = false;
#pragma unroll
        for (int q = 0; q < SPD_EOS; ++q) hit = hit || (e[q] >= 0 && c == e[q]);
        if (hit) {
          m = j + 1;
          fin = 1;
        }
      }
      if (L + m == limit[s]) fin = 1;
      int* h = hist + (size_t)s * (size_t)ld;
      for (int j = 0; j < m; ++j) h[L + j] = cand[r0 + j];
      hlen[s] = L + m;
      n_acc[s] = m;
      if (fin) done[s] = 1;
      if (acc_history && step < hist_len) acc_history[(size_t)step * hist_stride + s] = m;
    }
  }
  if (s == 0 && step_ctr) *step_ctr = step + 1;
}

bool bad_common(long long ld, int n_seq, int k, int max_seq) {
  if (k < 1 || k > SPD_MAX_K || n_seq < 1 || n_seq * (k + 1) > SPD_MAX_ROWS) return true;
  return max_seq < 1 || ld < max_seq || ld > 0x7fffffffll;
}

}  // namespace

extern "C" int lsa_spec_draft(const int* hist, long long ld, const int* hlen, int n_seq, int k, int nmin, int nmax,
                              const int* script, int max_seq, int* tokens, int* pos, int* matched, const int* done,
                              int* match_ctr, hipStream_t stream) {
  if (bad_common(ld, n_seq, k, max_seq)) return LSA_BAD_SHAPE;
  if (!script && (nmin < 1 || nmax < nmin || nmax > SPD_MAX_NGRAM)) return LSA_BAD_SHAPE;
  if (!hist || !hlen || !tokens || !pos) return LSA_BAD_SHAPE;
  spec_draft_kernel<<<n_seq, SPD_THREADS, 0, stream>>>(hist, ld, hlen, k, nmin, nmax, script, tokens, pos,
                                                      matched, done, match_ctr);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

extern "C" int lsa_spec_accept(int* hist, long long ld, int* hlen, const int* limit, int* done, const int* eos,
                               const int* tokens, const int* cand, int n_seq, int k, int max_seq, int* n_acc,
                               int* acc_history, int hist_stride, int hist_len, int* step_ctr, hipStream_t stream) {
  if (bad_common(ld, n_seq, k, max_seq)) return LSA_BAD_SHAPE;
  if (!hist || !hlen || !limit || !done || !eos || !tokens || !cand || !n_acc) return LSA_BAD_SHAPE;
  if (acc_history && (hist_stride < n_seq || hist_len < 1)) return LSA_BAD_SHAPE;
  spec_accept_kernel<<<1, LSA_WAVE, 0, stream>>>(hist, ld, hlen, limit, done, eos, tokens, cand, n_seq, k,
                                                 n_acc, acc_history, hist_stride, hist_len, step_ctr);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
