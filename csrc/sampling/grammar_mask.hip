// Regex-constrained decoding on bf16 logits, in place, on gfx950 (CDNA4 / MI355X): a byte-level DFA
// per sequence, walked over the byte string of every vocabulary entry each step.
//
//   lsa_grammar_mask             one workgroup per row: advances the row's DFA state by the bytes of
//                                the step's input token and masks every token whose bytes die in the
//                                automaton, between lsa_penalize and lsa_logit_process.
//   lsa_grammar_mask_calls       debug: how often this process has enqueued the kernel (a captured
//                                graph counts once, at capture).
//   lsa_grammar_mask_alt         the same kernel with LDS_STATES = 128 instead of 256: measurement and tests.
//   lsa_grammar_mask_lds_states / _alt_lds_states / _threads / _max_v   the constants below, for the
//                                binding and tests.
//
// Tables (GrammarState, runtime/sampling.py), all on the device:
//   arena    int16 [dfa_rows][256]: one row per DFA state, entry = the next state relative to the
//            automaton's first row, -1 = dead
//   accept   uint8 [dfa_rows]: bit 0 = accepting state, bit 1 = last row of its automaton
//   offsets  int32 [V + 1], data uint8 [data_len, a multiple of 4]: the byte string of every token;
//            length 0 = a special or unknown token, never allowed
//   gstate   int32 [n_slots]: arena row of the slot's current state, -1 = no grammar
//   gbase    int32 [n_slots]: arena row of the slot's automaton's state 0
//   gfault   int32 [n_slots]: bit 0 = a forbidden token was fed, bit 1 = a state allowed no token,
//            bit 2 = a state or base outside the arena
//   eos      int32 [8]: the EOS ids, -1 padded
//
// Contract per row r with slot s = slot[r] and input token t = tokens_in[r] (tokens_in == null or
// t < 0: none):
//   0. gstate[s] < 0: the row is skipped - logits and state stay bit-identical, no table is read.
//      (gstate[s] >= dfa_rows, gbase[s] < 0 or gbase[s] > gstate[s]: gfault[s] |= 4, row skipped.)
//   1. advance: t < 0 or t an EOS id: nothing. Otherwise walk bytes(t) from q = gstate[s]; t >= V, a
//      token of length 0 or a walk that dies: the state stays and gfault[s] |= 1; otherwise
//      gstate[s] = gbase[s] + walked state. One thread writes.
//   2. allowed(v), v < V, from the state after step 1: an EOS id: accept[q] & 1 (its bytes are
//      ignored); any other token: len(v) > 0 and the walk of bytes(v) from q stays alive through its
//      last byte.
//   3. n = the number of allowed v. n == 0: gfault[s] |= 2 and the row is left untouched. Otherwise
//      every v < V that is not allowed and whose logit is not already 0xFF80 becomes 0xFF80.
// Columns >= V are never read or written. A slot outside [0, n_slots) skips its row. Rows of one
// launch must name distinct slots. No floating-point arithmetic: an exact function of the inputs.
//
// Shape: 1024 threads. Positions p = column + pad (pad = the row base's offset into its 16-byte line,
// in elements) are cut into chunks of 512; wave w takes the chunks w, w + 16, ... In the walk, lane l
// takes position chunk * 512 + i * 64 + l for i = 0..7: offsets and token bytes of 64 consecutive
// tokens per wave instruction, one ballot per i. A walk is a chain of dependent loads (offsets ->
// token bytes -> one table entry per byte), so the lane's eight tokens are walked in lockstep, four
// bytes per trip, and every batch of eight loads is issued unconditionally, on clamped addresses,
// before its first use: one token at a time measured 35 us (tight pattern) to 91 us (every token
// walks to its end) for one row of 32000, loads left inside branches the same, this form 28 to 50 us
// (profiles/grammar_mask.md). The trips end when none of the lane's tokens is alive and unfinished.
// Lane l keeps the eight allow bits of the 16-byte logit vector it will store (positions
// chunk * 512 + 8 l ..+7: byte l & 7 of the ballot of i = l >> 3) in a 256-bit shift register - 32
// chunks per wave, V + pad <= 262144 - so the count is known before any store and no bit is
// recomputed or spilled. The stores pop the register in reverse chunk order: whole aligned vectors,
// written only if a column changed, scalar at the two ragged ends. A DFA of up to LDS_STATES states
// (its size is read off the 'last row' bits of accept) is staged into LDS and walked there; a larger
// one is walked from global memory (L2), 1.7 x slower. lsa_grammar_mask_alt is the same kernel with
// the other threshold that was measured.
#include "mask_row.h"

namespace {

constexpr int GM_THREADS = MR_THREADS;
constexpr int GM_WAVES = MR_WAVES;
constexpr int GM_LDS_STATES = 256;        // 128 KiB of the CU's 160 KiB: one workgroup per CU
constexpr int GM_ALT_LDS_STATES = 128;    // 64 KiB: no faster (registers, not LDS, keep a second workgroup off the CU)
constexpr int GM_CHUNK = MR_CHUNK;        // positions per wave and trip (mask_row.h)
constexpr int GM_REG_WORDS = MR_REG_WORDS;
constexpr int GM_MAX_V = MR_MAX_V;
constexpr int GM_EOS_MAX = MR_EOS_MAX;

long long g_grammar_mask_calls = 0;

// The state after the bytes [off, end) from state q of the table tab (rows of 256 relative entries);
// -1 once dead. nlim: entries >= nlim count as dead (they would leave the table).
LSA_DEVICE int gm_walk(const short* tab, int nlim, const unsigned* __restrict__ data32, int off, int end, int q) {
  int p = off;
  unsigned w = data32[p >> 2] >> ((p & 3) * 8);
  while (true) {
    const int n = tab[q * 256 + (int)(w & 0xffu)];
    if (n < 0 || n >= nlim) return -1;
    q = n;
    if (++p == end) return q;
    w = (p & 3) ? w >> 8 : data32[p >> 2];
  }
}

template <bool LDS>
LSA_DEVICE void gm_row(bf16_raw* __restrict__ row, int V, const short* tab, int nlim, int q, bool accepting,
                       const int* __restrict__ offsets, const unsigned* __restrict__ data32, int data_len,
                       const int* __restrict__ eos, int* __restrict__ gfault_s, int* sh_cnt) {
  const int tid = threadIdx.x, lane = tid & (LSA_WAVE - 1), wave = tid / LSA_WAVE;
  const int pad = (int)((reinterpret_cast<size_t>(row) & 15) >> 1);
  const int P = V + pad;                       // positions [pad, P) hold the columns [0, V)
  const int nchunk = (P + GM_CHUNK - 1) / GM_CHUNK;
  int e[GM_EOS_MAX];
#pragma unroll
  for (int j = 0; j < GM_EOS_MAX; ++j) e[j] = eos[j];

  // 2. the walk: allow bits into the shift register, the wave's count of allowed tokens
  unsigned reg[GM_REG_WORDS];
#pragma unroll
  for (int k = 0; k < GM_REG_WORDS; ++k) reg[k] = 0u;
  int cnt = 0;
  for (int c = wave; c < nchunk; c += GM_WAVES) {
    // The lane's eight tokens of the chunk, walked in lockstep: eight independent chains of offset,
    // byte and table loads in flight instead of one (st: the walk's state, -1 once dead or not
    // allowed). Every load is unconditional, on a clamped address, and each batch of eight is issued before
    // its first use: a load inside a branch waits there, and the chains run one after the other.
    int off[8], len[8], st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = c * GM_CHUNK + i * LSA_WAVE + lane - pad;
      const int vc = min(max(v, 0), V - 1);
      off[i] = offsets[vc];
      len[i] = offsets[vc + 1];
      st[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = st[i], o = off[i], en = len[i];
      bool is_eos = false;
#pragma unroll
      for (int j = 0; j < GM_EOS_MAX; ++j) is_eos |= e[j] == v;
      const bool in = v >= 0 && v < V;
      const bool walk = in && !is_eos && o >= 0 && en > o && en <= data_len;
      off[i] = walk ? o : 0;
      len[i] = walk ? en - o : 0;
      st[i] = walk ? q : (in && is_eos && accepting ? 0 : -1);
    }
    const int last_dw = (data_len >> 2) - 1;
    for (int pos = 0;; pos += 4) {
      unsigned lo[8], hi[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {              // the four bytes from off + pos on: two aligned dwords
        const int a = min(off[i] + pos, data_len - 1) >> 2;
        lo[i] = data32[a];
        hi[i] = data32[min(a + 1, last_dw)];
      }
      unsigned w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        w[i] = (unsigned)((((unsigned long long)hi[i] << 32) | lo[i]) >> (((off[i] + pos) & 3) * 8));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int n[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) n[i] = tab[max(st[i], 0) * 256 + (int)((w[i] >> (8 * k)) & 0xffu)];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (pos + k < len[i] && st[i] >= 0) st[i] = n[i] < nlim ? n[i] : -1;
      }
      bool more = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) more |= pos + 4 < len[i] && st[i] >= 0;
      if (!more) break;
    }
    bool alive[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) alive[i] = st[i] >= 0;
    cnt += mr_push(reg, alive, lane);
  }
  const int n = mr_total(cnt, sh_cnt, wave, lane);
  if (n == 0) {                                // 3. a stuck state: the row stays as it is
    if (tid == 0) *gfault_s |= 2;
    return;
  }

  mr_store(row, V, pad, nchunk, reg, wave, lane);   // 3. the stores, newest chunk first
}

template <int LS>
__global__ __launch_bounds__(GM_THREADS) void grammar_mask_kernel(
    bf16_raw* __restrict__ logits, long long ld, int V, const int* __restrict__ slot, int n_slots,
    const int* __restrict__ tokens_in, const short* __restrict__ arena, const unsigned char* __restrict__ accept,
    int dfa_rows, const int* __restrict__ offsets, const unsigned* __restrict__ data32, int data_len,
    int* __restrict__ gstate, const int* __restrict__ gbase, int* __restrict__ gfault, const int* __restrict__ eos) {
  __shared__ __attribute__((aligned(16))) short sh_tab[LS * 256];
  __shared__ int sh_cnt[GM_WAVES];
  __shared__ int sh_q, sh_states;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int s = slot[r];
  if (s < 0 || s >= n_slots) return;
  const int q0 = gstate[s];
  if (q0 < 0) return;
  const int base = gbase[s];
  if (q0 >= dfa_rows || base < 0 || base > q0) {
    if (tid == 0) gfault[s] |= 4;
    return;
  }
  const int nlim = dfa_rows - base;
  const short* gtab = arena + (size_t)base * 256;
  if (tid == 0) sh_states = LS + 1;
  __syncthreads();
  // the automaton's size: the first 'last row' bit from its base on
  if (tid < LS && tid < nlim && (accept[base + tid] & 2)) atomicMin(&sh_states, tid + 1);
  // 1. advance: every thread has read the old state above; thread 0 alone decides and writes
  if (tid == 0) {
    int q = q0 - base;
    const int t = tokens_in ? tokens_in[r] : -1;
    bool is_eos = false;
#pragma unroll
    for (int j = 0; j < GM_EOS_MAX; ++j) is_eos |= eos[j] == t;
    if (t >= 0 && !is_eos) {
      int n = -1;
      if (t < V) {
        const int off = offsets[t], end = offsets[t + 1];
        if (off >= 0 && end > off && end <= data_len) n = gm_walk(gtab, nlim, data32, off, end, q);
      }
      if (n >= 0) {
        q = n;
        gstate[s] = base + n;
      } else {
        gfault[s] |= 1;
      }
    }
    sh_q = q;
  }
  __syncthreads();
  const int q = sh_q, S = sh_states;
  const bool accepting = (accept[base + q] & 1) != 0;
  bf16_raw* row = logits + (size_t)r * (size_t)ld;
  if (S <= LS && q < S) {
    const int nvec = S * 32;                   // 16-byte vectors of S rows of 512 B
    for (int i = tid; i < nvec; i += GM_THREADS) st16(sh_tab + (size_t)i * 8, ld16(gtab + (size_t)i * 8));
    __syncthreads();
    gm_row<true>(row, V, sh_tab, S, q, accepting, offsets, data32, data_len, eos, gfault + s, sh_cnt);
  } else {
    gm_row<false>(row, V, gtab, nlim, q, accepting, offsets, data32, data_len, eos, gfault + s, sh_cnt);
  }
}

template <int LS>
int grammar_mask_launch(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                        const int* tokens_in, const void* arena, const void* accept, int dfa_rows,
                        const int* offsets, const void* data, long long data_len, int* gstate,
                        const int* gbase, int* gfault, const int* eos, hipStream_t stream) {
  if (rows < 1 || rows > 32768 || V < 1 || ld < (long long)V || n_slots < 1 || dfa_rows < 1 || data_len < 4 ||
      data_len > 0x7fffffffLL || (data_len & 3))
    return LSA_BAD_SHAPE;
  if (!logits || !slot || !arena || !accept || !offsets || !data || !gstate || !gbase || !gfault || !eos)
    return LSA_BAD_SHAPE;
  if ((reinterpret_cast<size_t>(arena) & 15) || (reinterpret_cast<size_t>(data) & 3) ||
      (reinterpret_cast<size_t>(logits) & 1))
    return LSA_BAD_SHAPE;
  if (V > GM_MAX_V) return LSA_UNSUPPORTED;
  grammar_mask_kernel<LS><<<rows, GM_THREADS, 0, stream>>>(
      static_cast<bf16_raw*>(logits), ld, V, slot, n_slots, tokens_in, static_cast<const short*>(arena),
      static_cast<const unsigned char*>(accept), dfa_rows, offsets, static_cast<const unsigned*>(data), (int)data_len,
      gstate, gbase, gfault, eos);
  LSA_CHECK_LAUNCH();
  ++g_grammar_mask_calls;
  return LSA_OK;
}

}  // namespace

// logits bf16 [rows][ld], edited in place; slot int32 [rows] (distinct); tokens_in int32 [rows] or
// null; the tables as above (arena and data 16- and 4-byte aligned).
extern "C" int lsa_grammar_mask(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                                const int* tokens_in, const void* arena, const void* accept, int dfa_rows,
                                const int* offsets, const void* data, long long data_len, int* gstate,
                                const int* gbase, int* gfault, const int* eos, hipStream_t stream) {
  return grammar_mask_launch<GM_LDS_STATES>(logits, ld, V, rows, slot, n_slots, tokens_in, arena, accept, dfa_rows,
                                            offsets, data, data_len, gstate, gbase, gfault, eos, stream);
}

// The same kernel with the other LDS threshold: for measurement and for testing both sides of it.
// Same bits as lsa_grammar_mask.
extern "C" int lsa_grammar_mask_alt(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                                    const int* tokens_in, const void* arena, const void* accept, int dfa_rows,
                                    const int* offsets, const void* data, long long data_len, int* gstate,
                                    const int* gbase, int* gfault, const int* eos, hipStream_t stream) {
  return grammar_mask_launch<GM_ALT_LDS_STATES>(logits, ld, V, rows, slot, n_slots, tokens_in, arena, accept, dfa_rows,
                                                offsets, data, data_len, gstate, gbase, gfault, eos, stream);
}

extern "C" long long lsa_grammar_mask_calls() { return g_grammar_mask_calls; }
extern "C" int lsa_grammar_mask_lds_states() { return GM_LDS_STATES; }
extern "C" int lsa_grammar_mask_alt_lds_states() { return GM_ALT_LDS_STATES; }
extern "C" int lsa_grammar_mask_threads() { return GM_THREADS; }
extern "C" int lsa_grammar_mask_max_v() { return GM_MAX_V; }
