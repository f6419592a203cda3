// Split-K projection GEMM whose fix-up is shared by all contributors of a tile (entry
// lsa_gemm_skp). Tiles, main loop (Kern::run_segment), fragment-native fp32 slabs and the row16
// epilogues are gemm_sk.hip's, included below with its entry points renamed; only the end of the
// work differs:
//
//  * every tile is split into exactly C equal K ranges (2 <= C <= 8), one workgroup each
//    (contributor c = 0..C-1 in K order), tiles * C workgroups in one round;
//  * the tile's 16-row x 64-column fragment rows (wave w, row block i: four 1 KiB slab blocks,
//    whole 16-column row segments and whole ss_out cells) are dealt into C bands,
//    band(w, i) = (w + i) % C - the same blocks in every contributor;
//  * a contributor stores its bands write-through in the rotated order (c + s) % C, s = 0..C-1,
//    all stores in flight at once; as band s's stores retire (counted vmcnt, then the workgroup
//    barrier) lane 0 of wave s takes an agent-scope ticket on counter [tile][band] and does not
//    wait for it: the C tickets of a workgroup are in flight together;
//  * whoever drew C-1 on a band reduces that band alone: it reads the other contributors' blocks
//    of the band with sc1 loads, sums in K order p0 + p1 + ... (its own partial from registers at
//    its own position, the sum initialised from p0 itself), runs the epilogue on the band's rows
//    and resets the counter. With simultaneous arrival band b's last arriver is contributor
//    (b + 1) % C, so C compute units each read (C-1)/C of one slab and run 1/C of the epilogue;
//    with skewed arrival one workgroup reduces more bands (gemm_sk's behaviour in the limit).
//
// Nobody waits or polls: a workgroup's progress never depends on another workgroup being
// resident. The memory recipe is gemm_sk's (write-through slab stores, drained before the
// ticket; every read of another workgroup's slab is an sc1 load). The partials and the summation
// order are gemm_sk's at the same (bm, bn, split), so results are bitwise equal to it.
//
// Epilogues: EPI_STORE and EPI_RESID (with or without the fused-norm ss_out partials); bn 128 / 256.

// the included file's extern "C" entry becomes a function template that is never instantiated
// (no second copy of its kernels); its diagnostic stamp symbols get names of their own
#define lsa_gemm_sk lsa_gemm_skp_unused_decl_(); template <int SKP_UNUSED_> int lsa_gemm_skp_unused_
#define lsa_gemm_sk_set_stamps lsa_gemm_skp_set_stamps
#define g_stamps g_stamps_skp
#include "../kernels/gemm_sk.hip"
#undef lsa_gemm_sk

namespace {

constexpr int SKP_MAX_C = 8;  // contributors per tile (= waves: wave s takes ticket s) and counters per tile

// counted wait leaving `rows` fragment rows (4 slab stores each) of this wave's stores in flight
LSA_DEVICE void vm_wait_rows(int rows) {
  switch (rows) {
    case 0: vm_wait<0>(); break;
    case 1: vm_wait<4>(); break;
    case 2: vm_wait<8>(); break;
    case 3: vm_wait<12>(); break;
    case 4: vm_wait<16>(); break;
    case 5: vm_wait<20>(); break;
    case 6: vm_wait<24>(); break;
    default: vm_wait<28>(); break;  // FM <= 8: at most 7 rows remain behind the first band
  }
}

// The ticket: an agent-scope fetch-add (sc0: return the old value; the instruction the compiler
// emits for a relaxed agent-scope __hip_atomic_fetch_add on a global counter) whose result is
// NOT waited for at the issue - with the builtin the issuing wave stalls a memory round trip
// before it reaches the next band's barrier, and the C tickets of a workgroup serialise.
// `old` is written when the atomic returns; ticket_wait() is the only place that may read it.
LSA_DEVICE void ticket_issue(unsigned& old, unsigned* counter) {
  asm volatile("global_atomic_add %0, %1, %2, off sc0" : "+v"(old) : "v"(counter), "v"(1u) : "memory");
}
LSA_DEVICE void ticket_wait(unsigned& old) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(old)::"memory"); }

template <int BM, int BN, int EPI, int NB>
struct Band {
  using K_ = Kern<BM, BN, EPI, NB>;
  using G_ = Geo<BM, BN, NB>;
  static constexpr int FM = K_::FM, FN = K_::FN, TM = K_::TM, TN = K_::TN;
  static_assert(FN == 4 && TN == 64 && FM <= 8, "a fragment row is one wave's 16 rows x 64 columns");
  static_assert(EPI == EPI_STORE || EPI == EPI_RESID, "band epilogues");

  // byte offset of slab block (w, i, j) for this lane
  LSA_DEVICE static int blk_off(const K_& k, int i, int j) { return ((k.w * FM * FN + i * FN + j) * 64 + k.lane) * 16; }

  LSA_DEVICE static __amdgpu_buffer_rsrc_t slab_rsrc(float* slab, int unit) {
    return __builtin_amdgcn_make_buffer_rsrc(slab + (size_t)unit * 2 * (size_t)(BM * BN), (short)0, BM * BN * 4,
                                             0x00020000);
  }

  // fragment row i of the tile: t = p0 + p1 + ... + p(C-1), this contributor's partial taken
  // from acc at position c, the others read sc1 from their slabs (CH contributors, 4 * CH
  // loads, in flight at a time: what the tile's register budget allows)
  static constexpr int CH = (BM == 256 && BN == 256) ? 2 : 4;
  template <typename UnitOf>
  LSA_DEVICE static void reduce_row(const K_& k, float* slab, int C, int c, UnitOf unit_of, int i,
                                    const f32x4_t (&own)[FN], f32x4_t (&t)[FN]) {
#pragma unroll
    for (int ch = 0; ch < SKP_MAX_C / CH; ++ch) {
      if (ch * CH >= C) break;
      f32x4_t ld[CH][FN];
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int ci = ch * CH + q;
        if (ci < C && ci != c) {
          const __amdgpu_buffer_rsrc_t sr = slab_rsrc(slab, unit_of(ci));
#pragma unroll
          for (int j = 0; j < FN; ++j)
            ld[q][j] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(sr, blk_off(k, i, j), 0, 16 /* sc1 */));
        } else {
#pragma unroll
          for (int j = 0; j < FN; ++j) ld[q][j] = own[j];
        }
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int ci = ch * CH + q;
        if (ci < C) {
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            if (ch == 0 && q == 0) t[j] = ld[q][j]; else t[j] += ld[q][j];
          }
        }
      }
    }
  }

  // the fused epilogue of one fragment row (16 rows x 64 columns of wave w): gemm_sk's transpose
  // pass on 16 rows - one lane per (row, 16-column segment), the same arithmetic per element
  LSA_DEVICE static void epilogue_row(const K_& k, const EpiArgs& ep, const f32x4_t (&t)[FN], int mt, int nt, int i) {
    const SkParams& P = *k.p;
    constexpr int ELD = G_::ELD;
    float* img = reinterpret_cast<float*>(k.smem) + k.w * (G_::EROWS * ELD);
    const int lane = k.lane;
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) img[(4 * (lane >> 4) + r) * ELD + j * 16 + (lane & 15)] = t[j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int row = lane / FN, j = lane % FN;
    const int m = mt * BM + k.wr * TM + i * 16 + row;
    const int col_base = nt * BN + k.wc * TN;
    const int c0 = col_base + j * 16;
    const float* src = img + row * ELD + j * 16;
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4_t*>(v + 4 * q) = *reinterpret_cast<const f32x4_t*>(src + 4 * q);
    if (EPI == EPI_RESID && ep.ss_out) {
      // residual add + the row's sum of squares of the ROUNDED outputs over this wave's 64
      // columns (4 consecutive lanes per row), one float per (row, 64-column block)
      float ssq = 0.f;
      if (m < P.M) {
        epi_bias16(ep, c0, v);
        const bf16_raw* rr = ep.resid + (size_t)m * ep.ldr + c0;
        float x0[8], x1[8];
        unpack8(ld16(rr), x0);
        unpack8(ld16(rr + 8), x1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          x0[q] += v[q];
          x1[q] += v[q + 8];
        }
        const u32x4_t p0 = pack8(x0), p1 = pack8(x1);
        bf16_raw* o = ep.out + (size_t)m * ep.ldo + c0;
        st16(o, p0);
        st16(o + 8, p1);
        unpack8(p0, x0);
        unpack8(p1, x1);
        ssq = ss16(x0, x1);
      }
#pragma unroll
      for (int o = 1; o < FN; o <<= 1) ssq = __fadd_rn(ssq, __shfl_xor(ssq, o, 64));
      if (m < P.M && (lane % FN) == 0) ep.ss_out[(size_t)m * ep.ss_n + (col_base >> 6)] = ssq;
    } else if (m < P.M) {
      epi_row16<EPI>(ep, m, c0, v);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};

// prm: dp_rounds = 0, sk_tiles = all tiles, split = C, G = tiles * C (= the grid).
// tile_major: 0 - unit u is tile u % tiles, range u / tiles (gemm_sk's split mode: neighbouring
// workgroups of an XCD stream the same K range of neighbouring tiles); 1 - unit u is tile u / C,
// range u % C (gemm_sk's stream-K placement: a tile's contributors are neighbours on one XCD)
template <int BM, int BN, int EPI, int NB>
__global__ __launch_bounds__(NTHR) void gemm_skp_kernel(const bf16_raw* __restrict__ A, const bf16_raw* __restrict__ W,
                                                         SkParams prm, EpiArgs ep, float* __restrict__ slab,
                                                         unsigned* __restrict__ counters, int tile_major) {
  using K_ = Kern<BM, BN, EPI, NB>;
  using B_ = Band<BM, BN, EPI, NB>;
  constexpr int FM = K_::FM, FN = K_::FN;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Geo<BM, BN, NB>::SMEM];
  K_ k;
  k.smem = smem;
  k.A = A;
  k.W = W;
  k.p = &prm;
  k.tid = threadIdx.x;
  k.lane = threadIdx.x & 63;
  k.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  k.wr = k.w / K_::WN;
  k.wc = k.w % K_::WN;
  k.group = k.w >> 2;
  const int C = prm.split, tiles = prm.sk_tiles, U = prm.G;
  // XCD-aware remap (bijective): blocks that share an XCD get consecutive units
  const int hw = blockIdx.x;
  int su;
  {
    const int q = U / 8, r = U % 8, x = hw % 8;
    su = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + hw / 8;
  }
  const int ts = tile_major ? su / C : su % tiles;
  const int c = tile_major ? su % C : su / tiles;
  auto unit_of = [&](int ci) { return tile_major ? ts * C + ci : ts + ci * tiles; };
  const int ka = c * prm.NKT / C, kb = (c + 1) * prm.NKT / C;
  int mt, nt;
  tile_coords(prm, ts, mt, nt);
  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  k.run_segment(acc, mt, nt, ka, kb);
  LSA_STAMP(2);

  // band of this wave's fragment row i
  int band[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) band[i] = (k.w + i) % C;

  // every band's stores, write-through, in the rotated order
  const __amdgpu_buffer_rsrc_t own = B_::slab_rsrc(slab, su);
  for (int s = 0; s < C; ++s) {
    const int b = c + s < C ? c + s : c + s - C;
#pragma unroll
    for (int i = 0; i < FM; ++i)
      if (band[i] == b) {
#pragma unroll
        for (int j = 0; j < FN; ++j)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), own, B_::blk_off(k, i, j), 0, 16);
      }
  }
  // one ticket per band as its stores retire; wave s draws ticket s and leaves it in flight (a
  // later counted wait of that wave may also wait for its ticket: never fewer stores retired)
  unsigned* cnt = counters + (size_t)ts * SKP_MAX_C;
  unsigned old = 0u;
  int rem = FM;
  for (int s = 0; s < C; ++s) {
    const int b = c + s < C ? c + s : c + s - C;
#pragma unroll
    for (int i = 0; i < FM; ++i) rem -= band[i] == b ? 1 : 0;
    vm_wait_rows(rem);
    barrier();  // raw s_barrier: the counted wait above is this hand-off's drain, nothing else is pending
    if (k.w == s && k.lane == 0) ticket_issue(old, &cnt[b]);
  }
  ticket_wait(old);
  unsigned char* last = smem + Geo<BM, BN, NB>::SMEM - 16;  // last[s]: this workgroup reduces band (c + s) % C
  if (k.w < C && k.lane == 0) last[k.w] = old == (unsigned)(C - 1);
  __syncthreads();
  LSA_STAMP(3);

  for (int s = 0; s < C; ++s) {
    if (!__builtin_amdgcn_readfirstlane((int)last[s])) continue;
    const int b = c + s < C ? c + s : c + s - C;
#pragma unroll
    for (int i = 0; i < FM; ++i)
      if (band[i] == b) {
        f32x4_t t[FN];
        B_::reduce_row(k, slab, C, c, unit_of, i, acc[i], t);
        B_::epilogue_row(k, ep, t, mt, nt, i);
      }
    // all C tickets of the band are drawn: the counter is free for the next launch
    if (k.tid == 0) __hip_atomic_store(&cnt[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  LSA_STAMP(5);
}

template <int BM, int BN, int EPI, int NB>
int launch_p(const bf16_raw* A, const bf16_raw* W, const SkParams& prm, const EpiArgs& ep, float* slab, unsigned* cnt,
             int tile_major, hipStream_t s) {
  gemm_skp_kernel<BM, BN, EPI, NB><<<prm.G, NTHR, 0, s>>>(A, W, prm, ep, slab, cnt, tile_major);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

template <int BM, int EPI>
int dispatch_p(const bf16_raw* A, const bf16_raw* W, const SkParams& prm, const EpiArgs& ep, float* slab, unsigned* cnt,
               int bn, int nb, int tile_major, hipStream_t s) {
  if (bn == 256) {
    if constexpr (BM == 128) {
      if (nb == 3) return launch_p<BM, 256, EPI, 3>(A, W, prm, ep, slab, cnt, tile_major, s);
    }
    return launch_p<BM, 256, EPI, 2>(A, W, prm, ep, slab, cnt, tile_major, s);
  }
  return nb == 3 ? launch_p<BM, 128, EPI, 3>(A, W, prm, ep, slab, cnt, tile_major, s)
                 : launch_p<BM, 128, EPI, 2>(A, W, prm, ep, slab, cnt, tile_major, s);
}

}  // namespace

// C[M, N] = A[M, K] @ W^T with every bm x bn tile (bm 256 / 128, bn 256 / 128, N % bn == 0) split
// into exactly `contributors` (2..8) equal K ranges, tiles * contributors <= 1024 workgroups in one
// round. epi: EPI_STORE or EPI_RESID (ep->ss_out allowed). nb as lsa_gemm_sk. tile_major: 0 / 1,
// the unit -> (tile, range) placement (above). slab: >= 2 * tiles * contributors * bm * bn floats;
// counters: >= 8 * tiles, zero before the first launch (every launch leaves them zero).
// Returns LSA_BAD_SHAPE on any shape the kernel's indexing cannot take, fewer K-tiles than
// contributors included.
extern "C" int lsa_gemm_skp(const void* a, int lda, const void* wp, int M, int N, int K, int epi, const EpiArgs* ep,
                            int bm, int bn, int nb, int contributors, int tile_major, int group_m, float* slab,
                            unsigned* counters, long long slab_floats, int n_counters, hipStream_t stream) {
  if (M < 1 || K < BK || K % BK || lda < K || lda % 8 || !ep) return LSA_BAD_SHAPE;
  if (bn != 256 && bn != 128) return LSA_UNSUPPORTED;
  if (bm != 256 && bm != 128) return LSA_UNSUPPORTED;
  if (epi != EPI_STORE && epi != EPI_RESID) return LSA_UNSUPPORTED;
  if (nb == 0) nb = (bn == 128 || (bm == 128 && bn == 256)) ? 3 : 2;
  if (nb != 2 && !(nb == 3 && (bn == 128 || (bm == 128 && bn == 256)))) return LSA_UNSUPPORTED;
  if (N < bn || N % bn || group_m < 1 || (tile_major != 0 && tile_major != 1)) return LSA_BAD_SHAPE;
  if (contributors < 2 || contributors > SKP_MAX_C || contributors > K / BK) return LSA_BAD_SHAPE;
  if (!ep->out || (epi == EPI_RESID && !ep->resid)) return LSA_BAD_SHAPE;
  if (ep->ss_in || (ep->ss_out && (epi != EPI_RESID || N % 64 || ep->ss_n != N / 64))) return LSA_BAD_SHAPE;
  SkParams prm;
  prm.M = M;
  prm.N = N;
  prm.K = K;
  prm.lda = lda;
  prm.MT = (M + bm - 1) / bm;
  prm.NT = N / bn;
  prm.NKT = K / BK;
  prm.group_m = group_m;
  const long long tiles = (long long)prm.MT * prm.NT;
  if (tiles * contributors > 1024) return LSA_BAD_SHAPE;
  prm.G = (int)tiles * contributors;
  prm.dp_rounds = 0;
  prm.sk_tiles = (int)tiles;
  prm.split = contributors;
  if (!slab || !counters || slab_floats < 2LL * prm.G * bm * bn || n_counters < prm.sk_tiles * SKP_MAX_C)
    return LSA_BAD_SHAPE;
  const bf16_raw* A = static_cast<const bf16_raw*>(a);
  const bf16_raw* W = static_cast<const bf16_raw*>(wp);
#define LSA_GP(E) (bm == 256 ? dispatch_p<256, E>(A, W, prm, *ep, slab, counters, bn, nb, tile_major, stream) \
                     : dispatch_p<128, E>(A, W, prm, *ep, slab, counters, bn, nb, tile_major, stream))
  return epi == EPI_STORE ? LSA_GP(EPI_STORE) : LSA_GP(EPI_RESID);
#undef LSA_GP
}
