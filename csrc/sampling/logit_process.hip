// Constrained decoding on bf16 logits, in place, on gfx950 (CDNA4 / MI355X): logit bias, banned
// tokens, min_tokens, min-p and a per-sequence token automaton.
//
//   lsa_logit_process        one workgroup per row: advances the row's automaton state by the step's
//                            input token and edits the row's logits, between lsa_penalize and
//                            lsa_sample (sampling.hip), whose contracts are unchanged.
//   lsa_logit_process_calls  debug: how often this process has enqueued the kernel (a captured
//                            graph counts once, at capture).
//
// Tables (ConstraintState, runtime/sampling.py), all on the device:
//   arena      int16 [state_rows][ld_arena >= V]: one row per automaton state, entry < 0 = the token
//              is forbidden in this state, any other value = the next state, relative to the
//              automaton's first row
//   astate     int32 [n_slots]: arena row of the slot's current state, -1 = no automaton
//   abase      int32 [n_slots]: arena row of the slot's automaton's state 0
//   bias_n     int32 [n_slots], bias_tok int32 [n_slots][320], bias_val fp32 [n_slots][320]: the
//              slot's bias entries (distinct tokens; -inf = banned)
//   min_until  int32 [n_slots]: the first position at which an EOS id may be produced
//   minp_delta fp32 [n_slots]: T * ln(min_p), -inf = off
//   fault      int32 [n_slots]: set to 1 when a forbidden token was fed
//   eos        int32 [8]: the EOS ids, -1 padded
//
// Contract per row r with slot s = slot[r], input token t = tokens_in[r] (tokens_in == null or
// t < 0: none) and c = ctr[r] + ctr_add, the position the sampled token will occupy:
//   0. astate[s] < 0, bias_n[s] == 0, c >= min_until[s] and minp_delta[s] == -inf: the row is skipped
//      - logits and state stay bit-identical and no table row is read.
//   1. a = astate[s]. With a >= 0 and a token t: n = arena[a][t]; n >= 0: a = abase[s] + n and
//      astate[s] = a; otherwise (also for t >= V) a stays and fault[s] = 1. A state outside
//      [0, state_rows) sets fault[s] = 1 and the row runs without an automaton.
//   2. for every column v < V, x = fp32(l_v):
//        (v, b) a bias entry of s:       x = fp32(bf16_rne(x + b))   (one fp32 add)
//        c < min_until[s] and v an EOS:  x = -inf
//        a >= 0 and arena[a][v] < 0:     x = -inf
//   3. minp_delta[s] > -inf: m = max_v x, thr = m + minp_delta[s] (one fp32 add), every x < thr
//      becomes -inf. The maximum always survives.
//   4. l_v is rewritten only where it changed: the rounded sum, or the bf16 pattern 0xFF80.
// Columns >= V (the lm_head padding) are never read or written. A slot outside [0, n_slots) skips
// its row. Rows of one launch must name distinct slots. There is no floating-point sum of more
// than two terms anywhere: every result is an exact function of the inputs.
//
// Shape: thread 0 advances the state and publishes it through LDS; the bias entries and the EOS
// ids are applied by one thread each (scalar 2-byte stores; an entry that is also a masked EOS
// writes the same -inf as the EOS thread, so there is no race on values) in front of a workgroup
// barrier. A row without automaton and min-p ends there. Otherwise the row is swept in 16-byte
// vectors of 8 logits and 8 arena entries, four vectors per thread in flight, scalar when a row
// start is not 16-byte aligned and for the V % 8 tail; a vector is stored only if one of its
// columns changed. min-p needs the row maximum before the threshold: a 16-byte-aligned row of up to
// 8 x 512 vectors (V <= 32768) stays in registers between the two (eight vectors per thread, indexed
// at compile time only) and is stored once; a longer or unaligned row is swept, stored and re-read
// from L2, as lsa_sample's passes do. Both give the same bits (profiles/logit_process.md has the times).
#include "row_scan.h"

namespace {

constexpr int LGP_THREADS = 512;
constexpr int LGP_UNROLL = 4;
constexpr int LGP_BIAS_MAX = 320;
constexpr int LGP_EOS_MAX = 8;

constexpr int LGP_REG_VECS = 8;            // min-p in registers: rows of up to 8 x 512 vectors (V <= 32768)

long long g_logit_process_calls = 0;

LSA_DEVICE float lp_neg_inf() { return __uint_as_float(0xFF800000u); }

// Automaton mask of one vector: logits lv, arena entries av. Returns the maximum of the eight
// values after masking; *ch is set when a column changed.
LSA_DEVICE float lp_mask8(u32x4_t& lv, const u32x4_t av, bool* ch) {
  float m = lp_neg_inf();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned l0 = lv[j] & 0xffffu, l1 = lv[j] >> 16;
    if ((av[j] & 0x8000u) && l0 != BF16_NEG_INF) { l0 = BF16_NEG_INF; *ch = true; }
    if ((av[j] & 0x80000000u) && l1 != BF16_NEG_INF) { l1 = BF16_NEG_INF; *ch = true; }
    lv[j] = l0 | (l1 << 16);
    m = fmaxf(m, fmaxf(bf2f((bf16_raw)l0), bf2f((bf16_raw)l1)));
  }
  return m;
}

// min-p mask of one vector: every value below thr becomes -inf.
LSA_DEVICE bool lp_thr8(u32x4_t& lv, float thr) {
  bool ch = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned l0 = lv[j] & 0xffffu, l1 = lv[j] >> 16;
    if (bf2f((bf16_raw)l0) < thr && l0 != BF16_NEG_INF) { l0 = BF16_NEG_INF; ch = true; }
    if (bf2f((bf16_raw)l1) < thr && l1 != BF16_NEG_INF) { l1 = BF16_NEG_INF; ch = true; }
    lv[j] = l0 | (l1 << 16);
  }
  return ch;
}

// Maximum over the workgroup (every thread calls it).
LSA_DEVICE float lp_block_max(float m, float* sh_max) {
  const int tid = threadIdx.x;
  m = wave_max(m);
  if ((tid & (LSA_WAVE - 1)) == 0) sh_max[tid / LSA_WAVE] = m;
  __syncthreads();
  m = sh_max[0];
#pragma unroll
  for (int w = 1; w < LGP_THREADS / LSA_WAVE; ++w) m = fmaxf(m, sh_max[w]);
  return m;
}

__global__ __launch_bounds__(LGP_THREADS) void logit_process_kernel(
    bf16_raw* __restrict__ logits, long long ld, int V, const int* __restrict__ slot, int n_slots,
    const int* __restrict__ tokens_in, const int* __restrict__ ctr, int ctr_add,
    const unsigned short* __restrict__ arena, long long ld_arena, int state_rows, int* __restrict__ astate,
    const int* __restrict__ abase, const int* __restrict__ bias_n, const int* __restrict__ bias_tok,
    const float* __restrict__ bias_val, const int* __restrict__ min_until, const float* __restrict__ minp_delta,
    int* __restrict__ fault, const int* __restrict__ eos, int reread) {
  __shared__ int sh_a;
  __shared__ float sh_max[LGP_THREADS / LSA_WAVE];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int s = slot[r];
  if (s < 0 || s >= n_slots) return;
  const int c = ctr[r] + ctr_add;
  const int a0 = astate[s];
  const int bn = min(max(bias_n[s], 0), LGP_BIAS_MAX);
  const bool eos_on = c < min_until[s];
  const float delta = minp_delta[s];
  const bool minp = delta > lp_neg_inf();
  if (a0 < 0 && bn == 0 && !eos_on && !minp) return;
  bf16_raw* row = logits + (size_t)r * (size_t)ld;

  // 1. advance: every thread has read the old state above; thread 0 alone decides and writes
  if (tid == 0) {
    int a = a0;
    if (a >= state_rows) {
      fault[s] = 1;
      a = -1;
    } else if (a >= 0) {
      const int t = tokens_in ? tokens_in[r] : -1;
      if (t >= 0) {
        const int n = t < V ? (int)(short)arena[(size_t)a * (size_t)ld_arena + t] : -1;
        const int a1 = n >= 0 ? abase[s] + n : -1;
        if (a1 >= 0 && a1 < state_rows) {
          a = a1;
          astate[s] = a;
        } else {
          fault[s] = 1;
        }
      }
    }
    sh_a = a;
  }
  // 2a. bias entries and EOS ids, one thread each
  if (tid < bn) {
    const int v = bias_tok[(size_t)s * LGP_BIAS_MAX + tid];
    if (v >= 0 && v < V) {
      bool is_eos = false;
      if (eos_on) {
#pragma unroll
        for (int j = 0; j < LGP_EOS_MAX; ++j) is_eos |= eos[j] == v;
      }
      const float x = bf2f(row[v]) + bias_val[(size_t)s * LGP_BIAS_MAX + tid];
      row[v] = is_eos ? (bf16_raw)BF16_NEG_INF : f2bf(x);
    }
  } else if (eos_on && tid >= LGP_BIAS_MAX && tid < LGP_BIAS_MAX + LGP_EOS_MAX) {
    const int v = eos[tid - LGP_BIAS_MAX];
    if (v >= 0 && v < V) row[v] = (bf16_raw)BF16_NEG_INF;
  }
  __syncthreads();
  const int a = sh_a;
  if (a < 0 && !minp) return;

  // 2b. the automaton's mask and the row maximum
  const unsigned short* arow = a >= 0 ? arena + (size_t)a * (size_t)ld_arena : nullptr;
  const size_t align = reinterpret_cast<size_t>(row) | (arow ? reinterpret_cast<size_t>(arow) : 0);
  const int nvec = (align & 15) == 0 ? (V >> 3) : 0;
  float m = lp_neg_inf();
  if (minp && !reread && nvec > 0 && nvec <= LGP_REG_VECS * LGP_THREADS) {
    // min-p with the row kept in registers (compile-time indexing only): one trip over the row
    u32x4_t lv[LGP_REG_VECS], av[LGP_REG_VECS];
    unsigned chm = 0u;
#pragma unroll
    for (int u = 0; u < LGP_REG_VECS; ++u) {
      const int cv = tid + u * LGP_THREADS;
      if (cv < nvec) {
        lv[u] = ld16(row + (size_t)cv * 8);
        av[u] = arow ? ld16(arow + (size_t)cv * 8) : u32x4_t{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int u = 0; u < LGP_REG_VECS; ++u) {
      if (tid + u * LGP_THREADS < nvec) {
        bool ch = false;
        m = fmaxf(m, lp_mask8(lv[u], av[u], &ch));
        chm |= ch ? 1u << u : 0u;
      }
    }
    unsigned tl = 0u;
    const int ti = nvec * 8 + tid;  // the V % 8 tail: at most one column per thread
    if (ti < V) {
      tl = row[ti];
      if (arow && (arow[ti] & 0x8000u)) tl = BF16_NEG_INF;
      m = fmaxf(m, bf2f((bf16_raw)tl));
    }
    const float thr = lp_block_max(m, sh_max) + delta;
#pragma unroll
    for (int u = 0; u < LGP_REG_VECS; ++u) {
      const int cv = tid + u * LGP_THREADS;
      if (cv < nvec) {
        const bool ch = lp_thr8(lv[u], thr);
        if (ch || (chm >> u & 1u)) st16(row + (size_t)cv * 8, lv[u]);
      }
    }
    if (ti < V) {
      if (bf2f((bf16_raw)tl) < thr) tl = BF16_NEG_INF;
      if (tl != row[ti]) row[ti] = (bf16_raw)tl;
    }
    return;
  }
  for (int c0 = tid; c0 < nvec; c0 += LGP_UNROLL * LGP_THREADS) {
    u32x4_t lv[LGP_UNROLL], av[LGP_UNROLL];
#pragma unroll
    for (int u = 0; u < LGP_UNROLL; ++u) {
      const int cv = c0 + u * LGP_THREADS;
      if (cv < nvec) {
        lv[u] = ld16(row + (size_t)cv * 8);
        av[u] = arow ? ld16(arow + (size_t)cv * 8) : u32x4_t{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int u = 0; u < LGP_UNROLL; ++u) {
      const int cv = c0 + u * LGP_THREADS;
      if (cv < nvec) {
        bool ch = false;
        m = fmaxf(m, lp_mask8(lv[u], av[u], &ch));
        if (ch) st16(row + (size_t)cv * 8, lv[u]);
      }
    }
  }
  for (int i = nvec * 8 + tid; i < V; i += LGP_THREADS) {
    unsigned l = row[i];
    if (arow && (arow[i] & 0x8000u) && l != BF16_NEG_INF) {
      l = BF16_NEG_INF;
      row[i] = (bf16_raw)l;
    }
    m = fmaxf(m, bf2f((bf16_raw)l));
  }
  if (!minp) return;

  // 3. min-p: the row maximum, then every value below it by more than |delta|
  const float thr = lp_block_max(m, sh_max) + delta;
  for (int c0 = tid; c0 < nvec; c0 += LGP_UNROLL * LGP_THREADS) {
    u32x4_t lv[LGP_UNROLL];
#pragma unroll
    for (int u = 0; u < LGP_UNROLL; ++u) {
      const int cv = c0 + u * LGP_THREADS;
      if (cv < nvec) lv[u] = ld16(row + (size_t)cv * 8);
    }
#pragma unroll
    for (int u = 0; u < LGP_UNROLL; ++u) {
      const int cv = c0 + u * LGP_THREADS;
      if (cv < nvec && lp_thr8(lv[u], thr)) st16(row + (size_t)cv * 8, lv[u]);
    }
  }
  for (int i = nvec * 8 + tid; i < V; i += LGP_THREADS) {
    const unsigned l = row[i];
    if (bf2f((bf16_raw)l) < thr && l != BF16_NEG_INF) row[i] = (bf16_raw)BF16_NEG_INF;
  }
}

}  // namespace

namespace {

int logit_process_launch(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                         const int* tokens_in, const int* ctr, int ctr_add, const void* arena, long long ld_arena,
                         int state_rows, int* astate, const int* abase, const int* bias_n, const int* bias_tok,
                         const float* bias_val, const int* min_until, const float* minp_delta, int* fault,
                         const int* eos, int reread, hipStream_t stream) {
  if (rows < 1 || rows > 65535 || V < 1 || ld < (long long)V || ld_arena < (long long)V || n_slots < 1 ||
      state_rows < 1)
    return LSA_BAD_SHAPE;
  if (!logits || !slot || !ctr || !arena || !astate || !abase || !bias_n || !bias_tok || !bias_val || !min_until ||
      !minp_delta || !fault || !eos)
    return LSA_BAD_SHAPE;
  logit_process_kernel<<<rows, LGP_THREADS, 0, stream>>>(
      static_cast<bf16_raw*>(logits), ld, V, slot, n_slots, tokens_in, ctr, ctr_add,
      static_cast<const unsigned short*>(arena), ld_arena, state_rows, astate, abase, bias_n, bias_tok, bias_val,
      min_until, minp_delta, fault, eos, reread);
  LSA_CHECK_LAUNCH();
  ++g_logit_process_calls;
  return LSA_OK;
}

}  // namespace

// logits bf16 [rows][ld], edited in place; slot int32 [rows] (distinct); tokens_in int32 [rows] or
// null; ctr int32 [rows]; the tables as above.
extern "C" int lsa_logit_process(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                                 const int* tokens_in, const int* ctr, int ctr_add, const void* arena,
                                 long long ld_arena, int state_rows, int* astate, const int* abase, const int* bias_n,
                                 const int* bias_tok, const float* bias_val, const int* min_until,
                                 const float* minp_delta, int* fault, const int* eos, hipStream_t stream) {
  return logit_process_launch(logits, ld, V, rows, slot, n_slots, tokens_in, ctr, ctr_add, arena, ld_arena, state_rows,
                              astate, abase, bias_n, bias_tok, bias_val, min_until, minp_delta, fault, eos, 0, stream);
}

// The same launch with the min-p pass re-reading the row from L2 at every size, the path rows of
// more than 8 x 512 vectors always take: for measurement and for testing that path on short rows.
// Same bits as lsa_logit_process.
extern "C" int lsa_logit_process_reread(void* logits, long long ld, int V, int rows, const int* slot, int n_slots,
                                        const int* tokens_in, const int* ctr, int ctr_add, const void* arena,
                                        long long ld_arena, int state_rows, int* astate, const int* abase,
                                        const int* bias_n, const int* bias_tok, const float* bias_val,
                                        const int* min_until, const float* minp_delta, int* fault, const int* eos,
                                        hipStream_t stream) {
  return logit_process_launch(logits, ld, V, rows, slot, n_slots, tokens_in, ctr, ctr_add, arena, ld_arena, state_rows,
                              astate, abase, bias_n, bias_tok, bias_val, min_until, minp_delta, fault, eos, 1, stream);
}

extern "C" long long lsa_logit_process_calls() { return g_logit_process_calls; }
