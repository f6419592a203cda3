// Repetition / presence / frequency penalties on bf16 logits, in place, on gfx950 (CDNA4 / MI355X).
//
//   lsa_penalize        one workgroup per row: counts the step's input token into the row's slot
//                       of the per-sequence token statistics and edits the row's logits, in front
//                       of lsa_sample (sampling.hip), whose contract is unchanged.
//   lsa_penalize_calls  debug: how often this process has enqueued the kernel (a captured graph
//                       counts once, at capture).
//
// Statistics: one uint16 per (sequence slot, vocabulary entry), state[slot][v]:
//   bit 15      v occurs in the prompt
//   bits 0..14  number of times v has been generated, saturating at 32767
// The host zeroes a slot's row and sets its prompt bits when a penalised request is admitted.
//
// Contract per row r with slot s = slot[r], input token t = tokens_in[r] (the token the previous
// step generated and this step embeds; tokens_in == null or t < 0: none) and parameters
// rho = rep[r] (repetition, finite and > 0, 1 = off), alpha = pres[r] (presence, finite, 0 = off),
// beta = freq[r] (frequency, finite, 0 = off):
//   rho == 1 && alpha == 0 && beta == 0: the row is skipped - logits and state stay bit-identical,
//   nothing is counted. Otherwise, for every column v < V:
//   1. c = min((state & 0x7fff) + (v == t), 0x7fff); the new count is stored, the prompt bit kept
//   2. x = fp32(l_v)
//   3. rho != 1 and (prompt bit set or c > 0):  x = x < 0 ? x * rho : x / rho   (the set semantics
//      of HF's RepetitionPenaltyLogitsProcessor over prompt + generated tokens; a correctly
//      rounded fp32 division, not a reciprocal multiply)
//   4. c > 0:  pen = fp32(c) * beta;  pen = pen + alpha;  x = x - pen   (three separately rounded
//      fp32 operations, no FMA contraction; generated tokens only, as OpenAI / vLLM define it)
//   5. l_v = bf16_rne(x), written only where step 3 or 4 applied
// Columns >= V (the lm_head padding) are never read or written. A slot outside [0, n_slots)
// skips its row. Rows of one launch must name distinct slots.
//
// The row is swept once: 16-byte loads of 8 logits and 8 states when both row starts are 16-byte
// aligned, scalar loads otherwise and for the V % 8 tail. The thread that owns column t applies
// the increment in registers, so there are no atomics and no ordering inside the workgroup. A
// logits vector is written back only if one of its columns changed, a state vector only if it
// holds t: the traffic is 2 x 2 x V bytes of reads per active row and a few stores.
#include "../kernels/common.h"

namespace {

constexpr int PEN_THREADS = 512;

long long g_penalize_calls = 0;

// One column: raw bf16 logit and its state, both updated in place. Returns bit 0 = the logit
// changed, bit 1 = the state changed.
LSA_DEVICE unsigned pen_one(unsigned& raw, unsigned& st, bool hit, float rho, float alpha, float beta) {
  // plain operators under contract(off), not the __f*_rn intrinsics: those are header functions
  // compiled with contraction on, and once inlined c * beta + alpha and x * rho - pen fuse into
  // FMAs, which round once where the contract rounds twice
#pragma clang fp contract(off)
  unsigned c = st & 0x7fffu, ch = 0u;
  if (hit && c < 0x7fffu) {
    ++c;
    st = (st & 0x8000u) | c;
    ch = 2u;
  }
  if (st == 0u) return ch;
  float x = bf2f((bf16_raw)raw);
  bool edit = false;
  if (rho != 1.f) {
    x = x < 0.f ? x * rho : x / rho;
    edit = true;
  }
  if (c > 0u) {
    float pen = (float)c * beta;
    pen = pen + alpha;
    x = x - pen;
    edit = true;
  }
  if (edit) {
    raw = (unsigned)f2bf(x);
    ch |= 1u;
  }
  return ch;
}

__global__ __launch_bounds__(PEN_THREADS) void penalize_kernel(
    bf16_raw* __restrict__ logits, long long ld, int V, const int* __restrict__ slot, int n_slots,
    const int* __restrict__ tokens_in, unsigned short* __restrict__ state, long long ld_state,
    const float* __restrict__ rep, const float* __restrict__ pres, const float* __restrict__ freq) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const float rho = rep[r], alpha = pres[r], beta = freq[r];
  if (rho == 1.f && alpha == 0.f && beta == 0.f) return;
  const int s = slot[r];
  if (s < 0 || s >= n_slots) return;
  const int t = tokens_in ? tokens_in[r] : -1;
  bf16_raw* row = logits + (size_t)r * (size_t)ld;
  unsigned short* srow = state + (size_t)s * (size_t)ld_state;

  const bool aligned = ((reinterpret_cast<size_t>(row) | reinterpret_cast<size_t>(srow)) & 15) == 0;
  const int nvec = aligned ? (V >> 3) : 0;
  for (int c = tid; c < nvec; c += PEN_THREADS) {
    u32x4_t lv = ld16(row + (size_t)c * 8);
    u32x4_t sv = ld16(srow + (size_t)c * 8);
    const int hit = t - c * 8;  // 0..7: this vector holds column t
    if ((sv[0] | sv[1] | sv[2] | sv[3]) == 0u && (unsigned)hit >= 8u) continue;
    unsigned ch = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned l0 = lv[j] & 0xffffu, l1 = lv[j] >> 16, s0 = sv[j] & 0xffffu, s1 = sv[j] >> 16;
      ch |= pen_one(l0, s0, hit == 2 * j, rho, alpha, beta);
      ch |= pen_one(l1, s1, hit == 2 * j + 1, rho, alpha, beta);
      lv[j] = l0 | (l1 << 16);
      sv[j] = s0 | (s1 << 16);
    }
    if (ch & 1u) st16(row + (size_t)c * 8, lv);
    if (ch & 2u) st16(srow + (size_t)c * 8, sv);
  }
  for (int i = nvec * 8 + tid; i < V; i += PEN_THREADS) {
    unsigned l = row[i], st = srow[i];
    const unsigned ch = pen_one(l, st, i == t, rho, alpha, beta);
    if (ch & 1u) row[i] = (bf16_raw)l;
    if (ch & 2u) srow[i] = (unsigned short)st;
  }
}

}  // namespace

// logits bf16 [rows][ld], edited in place; slot int32 [rows] (distinct, each in [0, n_slots));
// tokens_in int32 [rows] or null; state uint16 [n_slots][ld_state >= V]; rep / pres / freq fp32
// [rows].
extern "C" int lsa_penalize(void* logits, long long ld, int V, int rows, const int* slot, const int* tokens_in,
                            void* state, long long ld_state, int n_slots, const float* rep, const float* pres,
                            const float* freq, hipStream_t stream) {
  if (rows < 1 || rows > 65535 || V < 1 || ld < (long long)V || ld_state < (long long)V || n_slots < 1)
    return LSA_BAD_SHAPE;
  if (!logits || !slot || !state || !rep || !pres || !freq) return LSA_BAD_SHAPE;
  penalize_kernel<<<rows, PEN_THREADS, 0, stream>>>(static_cast<bf16_raw*>(logits), ld, V, slot, n_slots, tokens_in,
                                                    static_cast<unsigned short*>(state), ld_state, rep, pres, freq);
  LSA_CHECK_LAUNCH();
  ++g_penalize_calls;
  return LSA_OK;
}

extern "C" long long lsa_penalize_calls() { return g_penalize_calls; }
