// JSON-constrained decoding on bf16 logits, in place, on gfx950 (CDNA4 / MI355X): a byte-level
// pushdown automaton with 1-bit stack symbols per sequence, walked over the byte string of every
// vocabulary entry each step.
//
//   lsa_pda_mask                 one workgroup per row: advances the row's configuration by the bytes
//                                of the step's input token and masks every token whose bytes die in
//                                the automaton; launched right after lsa_grammar_mask (a slot holds a
//                                regex or JSON, never both, and each kernel skips the other's slots).
//   lsa_pda_mask_calls           debug: how often this process has enqueued the kernel (a captured
//                                graph counts once, at capture).
//   lsa_pda_mask_lds_states / _threads / _max_v   the constants below, for the binding and tests.
//
// Tables (GrammarState, runtime/logit_stages.py), all on the device:
//   ptab     int16 [3][S][256], 1 <= S <= 1023: plane 0 = empty stack, 1 = top symbol 0, 2 = top
//            symbol 1; an entry is -1 (dead) or state | op << 10 with op 0 none, 1 push 0, 2 push 1,
//            3 pop
//   paccept  uint8 [S]: bit 0 = accepting state
//   offsets  int32 [V + 1], data uint8 [data_len, a multiple of 4]: the byte string of every token;
//            length 0 = a special or unknown token, never allowed
//   jstate   int32 [n_slots]: the slot's state, -1 = no JSON
//   jdepth   int32 [n_slots]: its stack depth d, 0..64
//   jstack   int64 [n_slots]: bit i = the symbol at level i, bits >= d zero
//   gfault   int32 [n_slots] (shared with the regex): bit 0 = a forbidden token was fed, bit 1 = a
//            configuration allowed no token, bit 2 = a state or depth out of range
//   eos      int32 [8]: the EOS ids, -1 padded
//
// A step on byte b from (q, d, stack): the plane by the top symbol; a dead entry, a push at d == 64
// and a pop at d == 0 kill the walk; a push sets bit d and increments d, a pop decrements d and clears
// bit d. A configuration accepts iff paccept[q] & 1 and d == 0.
//
// Contract per row r with slot s = slot[r] and input token t = tokens_in[r] (tokens_in == null or
// t < 0: none):
//   0. jstate[s] < 0: the row is skipped - logits and state stay bit-identical, no table is read.
//      (jstate[s] >= S or jdepth[s] outside [0, 64]: gfault[s] |= 4, row skipped.)
//   1. advance: t < 0 or t an EOS id: nothing. Otherwise walk bytes(t) from the configuration;
//      t >= V, a token of length 0 or a walk that dies: the configuration stays and gfault[s] |= 1;
//      otherwise jstate, jdepth and jstack of s are stored. One thread writes.
//   2. allowed(v), v < V, from the configuration after step 1: an EOS id: the configuration accepts
//      (its bytes are ignored); any other token: len(v) > 0 and the walk of bytes(v) stays alive
//      through its last byte. The walk's pushes and pops stay in registers.
//   3. n = the number of allowed v. n == 0: gfault[s] |= 2 and the row is left untouched. Otherwise
//      every v < V that is not allowed and whose logit is not already 0xFF80 becomes 0xFF80.
// Columns >= V are never read or written. A slot outside [0, n_slots) skips its row. Rows of one
// launch must name distinct slots. No floating-point arithmetic: an exact function of the inputs.
//
// Shape: that of grammar_mask.hip (mask_row.h): 1024 threads, chunks of 512 positions per wave, the
// lane's eight tokens of a chunk walked in lockstep four bytes per trip with every batch of loads
// issued unconditionally on clamped addresses, the allow bits in a 256-bit shift register, the
// stores last. Beside the state each walk keeps its depth and its stack, a 64-bit register, and
// every step picks its plane from them. An automaton of up to PM_LDS_STATES states (its three
// planes: 1536 B per state) is staged into LDS and walked there; a larger one is walked from global
// memory (L2).
#include "mask_row.h"

namespace {

constexpr int PM_LDS_STATES = 85;         // 3 * 85 * 512 B = 127.5 KiB of the CU's 160 KiB, as the regex kernel's 128 KiB
constexpr int PM_MAX_STATES = 1023;
constexpr int PM_MAX_DEPTH = 64;
constexpr int PM_ENTRY_END = 4 << 10;     // entries from here on carry no known op: dead

long long g_pda_mask_calls = 0;

struct PmConfig {
  int q, d;                               // q < 0: dead
  unsigned long long stack;
};

// One byte from c (alive) through the entry e of its plane.
LSA_DEVICE PmConfig pm_apply(PmConfig c, int e, int S) {
  const int op = e >> 10, nq = e & 0x3ff;
  const bool push = op == 1 || op == 2, pop = op == 3;
  const bool dead = e < 0 || e >= PM_ENTRY_END || nq >= S || (push && c.d == PM_MAX_DEPTH) || (pop && c.d == 0);
  const unsigned long long pbit = (unsigned long long)(op == 2) << (c.d & 63);
  const unsigned long long cbit = 1ull << ((c.d - 1) & 63);
  PmConfig o;
  o.q = dead ? -1 : nq;
  o.d = c.d + (push ? 1 : 0) - (pop ? 1 : 0);
  o.stack = push ? (c.stack | pbit) : (pop ? (c.stack & ~cbit) : c.stack);
  return o;
}

// The row of ptab the configuration (alive or not) reads next: plane * S + state.
LSA_DEVICE int pm_row_of(int q, int d, unsigned long long stack, int S) {
  const int top = (int)((stack >> ((d - 1) & 63)) & 1ull);
  return (d > 0 ? (1 + top) * S : 0) + max(q, 0);
}

// The configuration after the bytes [off, end) from c; q = -1 once dead.
LSA_DEVICE PmConfig pm_walk(const short* tab, int S, const unsigned* __restrict__ data32, int off, int end, PmConfig c) {
  int p = off;
  unsigned w = data32[p >> 2] >> ((p & 3) * 8);
  while (true) {
    c = pm_apply(c, tab[pm_row_of(c.q, c.d, c.stack, S) * 256 + (int)(w & 0xffu)], S);
    if (c.q < 0 || ++p == end) return c;
    w = (p & 3) ? w >> 8 : data32[p >> 2];
  }
}

template <bool LDS>
LSA_DEVICE void pm_row(bf16_raw* __restrict__ row, int V, const short* tab, int S, PmConfig c0, bool accepting,
                       const int* __restrict__ offsets, const unsigned* __restrict__ data32, int data_len,
                       const int* __restrict__ eos, int* __restrict__ gfault_s, int* sh_cnt) {
  const int tid = threadIdx.x, lane = tid & (LSA_WAVE - 1), wave = tid / LSA_WAVE;
  const int pad = (int)((reinterpret_cast<size_t>(row) & 15) >> 1);
  const int P = V + pad;                       // positions [pad, P) hold the columns [0, V)
  const int nchunk = (P + MR_CHUNK - 1) / MR_CHUNK;
  int e[MR_EOS_MAX];
#pragma unroll
  for (int j = 0; j < MR_EOS_MAX; ++j) e[j] = eos[j];

  // 2. the walk: allow bits into the shift register, the wave's count of allowed tokens
  unsigned reg[MR_REG_WORDS];
#pragma unroll
  for (int k = 0; k < MR_REG_WORDS; ++k) reg[k] = 0u;
  int cnt = 0;
  for (int c = wave; c < nchunk; c += MR_WAVES) {
    // The lane's eight tokens of the chunk in lockstep, as in grammar_mask.hip; st < 0: dead or not
    // allowed. dp and sk: the walk's depth and stack.
    int off[8], len[8], st[8], dp[8];
    unsigned long long sk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = c * MR_CHUNK + i * LSA_WAVE + lane - pad;
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
      for (int j = 0; j < MR_EOS_MAX; ++j) is_eos |= e[j] == v;
      const bool in = v >= 0 && v < V;
      const bool walk = in && !is_eos && o >= 0 && en > o && en <= data_len;
      off[i] = walk ? o : 0;
      len[i] = walk ? en - o : 0;
      st[i] = walk ? c0.q : (in && is_eos && accepting ? 0 : -1);
      dp[i] = c0.d;
      sk[i] = c0.stack;
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
        for (int i = 0; i < 8; ++i)
          n[i] = tab[pm_row_of(st[i], dp[i], sk[i], S) * 256 + (int)((w[i] >> (8 * k)) & 0xffu)];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (pos + k < len[i] && st[i] >= 0) {
            PmConfig cur;
            cur.q = st[i];
            cur.d = dp[i];
            cur.stack = sk[i];
            const PmConfig nx = pm_apply(cur, n[i], S);
            st[i] = nx.q;
            dp[i] = nx.d;
            sk[i] = nx.stack;
          }
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
  if (n == 0) {                                // 3. a stuck configuration: the row stays as it is
    if (tid == 0) *gfault_s |= 2;
    return;
  }
  mr_store(row, V, pad, nchunk, reg, wave, lane);   // 3. the stores, newest chunk first
}

__global__ __launch_bounds__(MR_THREADS) void pda_mask_kernel(
    bf16_raw* __restrict__ logits, long long ld, int V, const int* __restrict__ slot, int n_slots,
    const int* __restrict__ tokens_in, const short* __restrict__ ptab, const unsigned char* __restrict__ paccept,
    int S, const int* __restrict__ offsets, const unsigned* __restrict__ data32, int data_len,
    int* __restrict__ jstate, int* __restrict__ jdepth, long long* __restrict__ jstack, int* __restrict__ gfault,
    const int* __restrict__ eos) {
  __shared__ __attribute__((aligned(16))) short sh_tab[PM_LDS_STATES * 3 * 256];
  __shared__ int sh_cnt[MR_WAVES];
  __shared__ int sh_q, sh_d;
  __shared__ unsigned long long sh_stack;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int s = slot[r];
  if (s < 0 || s >= n_slots) return;
  const int q0 = jstate[s];
  if (q0 < 0) return;
  const int d0 = jdepth[s];
  if (q0 >= S || d0 < 0 || d0 > PM_MAX_DEPTH) {
    if (tid == 0) gfault[s] |= 4;
    return;
  }
  // 1. advance: every thread has read the old state above; thread 0 alone reads the stack, decides and writes
  if (tid == 0) {
    PmConfig c;
    c.q = q0;
    c.d = d0;
    c.stack = (unsigned long long)jstack[s];
    if (d0 < 64) c.stack &= (1ull << d0) - 1ull;   // bits >= d are zero by contract: keep the walk inside it
    const int t = tokens_in ? tokens_in[r] : -1;
    bool is_eos = false;
#pragma unroll
    for (int j = 0; j < MR_EOS_MAX; ++j) is_eos |= eos[j] == t;
    if (t >= 0 && !is_eos) {
      PmConfig n;
      n.q = -1;
      n.d = 0;
      n.stack = 0ull;
      if (t < V) {
        const int off = offsets[t], end = offsets[t + 1];
        if (off >= 0 && end > off && end <= data_len) n = pm_walk(ptab, S, data32, off, end, c);
      }
      if (n.q >= 0) {
        c = n;
        jstate[s] = n.q;
        jdepth[s] = n.d;
        jstack[s] = (long long)n.stack;
      } else {
        gfault[s] |= 1;
      }
    }
    sh_q = c.q;
    sh_d = c.d;
    sh_stack = c.stack;
  }
  __syncthreads();
  PmConfig c;
  c.q = sh_q;
  c.d = sh_d;
  c.stack = sh_stack;
  const bool accepting = (paccept[c.q] & 1) != 0 && c.d == 0;
  bf16_raw* row = logits + (size_t)r * (size_t)ld;
  if (S <= PM_LDS_STATES) {
    const int nvec = S * 3 * 32;               // 16-byte vectors of 3 S rows of 512 B
    for (int i = tid; i < nvec; i += MR_THREADS) st16(sh_tab + (size_t)i * 8, ld16(ptab + (size_t)i * 8));
    __syncthreads();
    pm_row<true>(row, V, sh_tab, S, c, accepting, offsets, data32, data_len, eos, gfault + s, sh_cnt);
  } else {
    pm_row<false>(row, V, ptab, S, c, accepting, offsets, data32, data_len, eos, gfault + s, sh_cnt);
  }
}

}  // namespace

// logits bf16 [rows][ld], edited in place; slot int32 [rows] (distinct); tokens_in int32 [rows] or
// null; the tables as above (ptab and data 16- and 4-byte aligned, jstack 8-byte aligned).
extern "C" int lsa_pda_mask(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                            const int* tokens_in, const void* ptab, const void* paccept, int n_states,
                            const int* offsets, const void* data, long long data_len, int* jstate, int* jdepth,
                            long long* jstack, int* gfault, const int* eos, hipStream_t stream) {
  if (rows < 1 || rows > 32768 || V < 1 || ld < (long long)V || n_slots < 1 || n_states < 1 ||
      n_states > PM_MAX_STATES || data_len < 4 || data_len > 0x7fffffffLL || (data_len & 3))
    return LSA_BAD_SHAPE;
  if (!logits || !slot || !ptab || !paccept || !offsets || !data || !jstate || !jdepth || !jstack || !gfault || !eos)
    return LSA_BAD_SHAPE;
  if ((reinterpret_cast<size_t>(ptab) & 15) || (reinterpret_cast<size_t>(data) & 3) ||
      (reinterpret_cast<size_t>(logits) & 1) || (reinterpret_cast<size_t>(jstack) & 7))
    return LSA_BAD_SHAPE;
  if (V > MR_MAX_V) return LSA_UNSUPPORTED;
  pda_mask_kernel<<<rows, MR_THREADS, 0, stream>>>(
      static_cast<bf16_raw*>(logits), ld, V, slot, n_slots, tokens_in, static_cast<const short*>(ptab),
      static_cast<const unsigned char*>(paccept), n_states, offsets, static_cast<const unsigned*>(data), (int)data_len,
      jstate, jdepth, jstack, gfault, eos);
  LSA_CHECK_LAUNCH();
  ++g_pda_mask_calls;
  return LSA_OK;
}

extern "C" long long lsa_pda_mask_calls() { return g_pda_mask_calls; }
extern "C" int lsa_pda_mask_lds_states() { return PM_LDS_STATES; }
extern "C" int lsa_pda_mask_threads() { return MR_THREADS; }
extern "C" int lsa_pda_mask_max_v() { return MR_MAX_V; }
