// Speculative decoding with a draft model on gfx950 (CDNA4 / MI355X): the glue between a small
// draft engine and the target's verification step, so that
//
//   dm_begin -> [draft embed -> layers -> head -> argmax_finalize -> dm_chain] x k
//            -> target embed -> layers -> head -> lsa_spec_accept
//
// is captured once and replayed with no host work. Both kernels read and write device state only.
//
//   lsa_spec_dm_begin  one thread per sequence: the draft engine's two catch-up rows, the target's
//                      row 0 and the positions of all its k + 1 rows
//   lsa_spec_dm_chain  one thread per sequence: iteration j's arg-max token d[j] into the target's
//                      row j + 1 and, while j + 1 < k, into the draft engine's next 1-row input
//
// State: spec_decode.hip's (`hist` int32 [n_seq, ld], `hlen`, `done` [n_seq], `tokens` / `pos`
// [n_seq * (k + 1)], row r0 + j with r0 = s * (k + 1) belongs to sequence s), plus the draft
// engine's inputs: `d_tokens` / `d_pos` / `d_slot` int32 [2 * n_seq] (rows 2s and 2s + 1 belong to
// sequence s; iteration 0), `d_tokens1` / `d_pos1` int32 [n_seq] (iterations 1 .. k-1; their slot
// vector is `slots` itself) and `amax` int32 [n_seq], the draft's arg-max token per sequence.
// L = min(max(hlen[s], 1), ld) as in spec_decode.hip. dmax = the draft engine's max_seq.
//
// Invariant: before a step the draft engine's slot holds valid K/V for positions [0, L - 2) at
// least. The previous step fed the draft positions L' - 2 .. L' + k - 2; after a accepted drafts
// (L = L' + a + 1 at most) only position L - 2 can be missing, and only when a == k.
//
// Begin. Draft row 2s: token hist[pa] at pa = max(L - 2, 0); row 2s + 1: token hist[L - 1] at L - 1
// (L == 1: both rows are (hist[0], 0), two stores of the same cell contents); both with slot
// slots[s]. Draft positions are clamped into [0, dmax): a no-op under the caller's guarantee
// limit[s] + k <= max_seq <= dmax. Target: tokens[r0] = hist[L-1], pos[r0 + j] = L - 1 + j for
// j = 0 .. k, matched[s] = 1, match_ctr[s] += 1 for a sequence that is not done - what
// lsa_spec_draft writes in script mode, drafts excepted. A done sequence is treated like any other.
//
// Chain(j), 0 <= j < k: d = amax[s]; tokens[r0 + j + 1] = d; if j + 1 < k: d_tokens1[s] = d,
// d_pos1[s] = min(L + j, dmax - 1). Nothing else is written.
//
// Refused with LSA_BAD_SHAPE before any launch: k outside [1, 15], n_seq * (k + 1) above 128,
// ld < max_seq, dmax < max_seq, j outside [0, k), a null pointer among the required arrays.
#include "../kernels/common.h"

namespace {

constexpr int SDM_MAX_K = 15;
constexpr int SDM_MAX_ROWS = 128;  // StageEngine.DECODE_MAX_ROWS: n_seq <= 64, one wave

LSA_DEVICE int sdm_len(int L, long long ld) {
  L = L < 1 ? 1 : L;
  return (long long)L > ld ? (int)ld : L;
}

LSA_DEVICE int sdm_pos(int p, int dmax) {
  p = p < 0 ? 0 : p;
  return p < dmax ? p : dmax - 1;
}

__global__ __launch_bounds__(LSA_WAVE) void spec_dm_begin_kernel(
    const int* __restrict__ hist, long long ld, const int* __restrict__ hlen, const int* __restrict__ slots,
    int n_seq, int k, int dmax, int* __restrict__ d_tokens, int* __restrict__ d_pos, int* __restrict__ d_slot,
    int* __restrict__ tokens, int* __restrict__ pos, int* __restrict__ matched, const int* __restrict__ done,
    int* __restrict__ match_ctr) {
  const int s = threadIdx.x;
  if (s >= n_seq) return;
  const int* h = hist + (size_t)s * (size_t)ld;
  const int L = sdm_len(hlen[s], ld);
  const int pa = L >= 2 ? L - 2 : 0;
  const int last = h[L - 1];
  const int slot = slots[s];
  d_tokens[2 * s] = h[pa];
  d_pos[2 * s] = sdm_pos(pa, dmax);
  d_slot[2 * s] = slot;
  d_tokens[2 * s + 1] = last;
  d_pos[2 * s + 1] = sdm_pos(L - 1, dmax);
  d_slot[2 * s + 1] = slot;
  const int r0 = s * (k + 1);
  tokens[r0] = last;
  for (int j = 0; j <= k; ++j) pos[r0 + j] = L - 1 + j;
  if (matched) matched[s] = 1;
  if (match_ctr && !(done && done[s] != 0)) match_ctr[s] += 1;
}

__global__ __launch_bounds__(LSA_WAVE) void spec_dm_chain_kernel(
    const int* __restrict__ amax, const int* __restrict__ hlen, long long ld, int n_seq, int k, int j, int dmax,
    int* __restrict__ tokens, int* __restrict__ d_tokens1, int* __restrict__ d_pos1) {
  const int s = threadIdx.x;
  if (s >= n_seq) return;
  const int d = amax[s];
  tokens[s * (k + 1) + j + 1] = d;
  if (j + 1 < k) {
    d_tokens1[s] = d;
    d_pos1[s] = sdm_pos(sdm_len(hlen[s], ld) + j, dmax);
  }
}

bool sdm_bad(long long ld, int n_seq, int k, int max_seq, int dmax) {
  if (k < 1 || k > SDM_MAX_K || n_seq < 1 || n_seq * (k + 1) > SDM_MAX_ROWS) return true;
  return max_seq < 1 || ld < max_seq || ld > 0x7fffffffll || dmax < max_seq;
}

}  // namespace

extern "C" int lsa_spec_dm_begin(const int* hist, long long ld, const int* hlen, const int* slots, int n_seq, int k,
                                 int max_seq, int draft_max_seq, int* d_tokens, int* d_pos, int* d_slot, int* tokens,
                                 int* pos, int* matched, const int* done, int* match_ctr, hipStream_t stream) {
  if (sdm_bad(ld, n_seq, k, max_seq, draft_max_seq)) return LSA_BAD_SHAPE;
  if (!hist || !hlen || !slots || !d_tokens || !d_pos || !d_slot || !tokens || !pos) return LSA_BAD_SHAPE;
  spec_dm_begin_kernel<<<1, LSA_WAVE, 0, stream>>>(hist, ld, hlen, slots, n_seq, k, draft_max_seq, d_tokens, d_pos,
                                                   d_slot, tokens, pos, matched, done, match_ctr);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

extern "C" int lsa_spec_dm_chain(const int* amax, const int* hlen, long long ld, int n_seq, int k, int j, int max_seq,
                                 int draft_max_seq, int* tokens, int* d_tokens1, int* d_pos1, hipStream_t stream) {
  if (sdm_bad(ld, n_seq, k, max_seq, draft_max_seq) || j < 0 || j >= k) return LSA_BAD_SHAPE;
  if (!amax || !hlen || !tokens) return LSA_BAD_SHAPE;
  if (j + 1 < k && (!d_tokens1 || !d_pos1)) return LSA_BAD_SHAPE;
  spec_dm_chain_kernel<<<1, LSA_WAVE, 0, stream>>>(amax, hlen, ld, n_seq, k, j, draft_max_seq, tokens, d_tokens1,
                                                   d_pos1);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}
