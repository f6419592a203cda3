// W4A16 GEMM for prefill chunks and decode batches above 128 rows:
//   y[M, N] = sum_g s[n, g] * (A[M, g] @ Q[N, g]^T),  any M >= 1,
// on the operands of gemv_int4.hip / gemv_coop_int4.hip (Wq4[nt][K/128][lane][16 B] nibbles,
// S[nt][K/128][16] fp32 group scales, bf16 activations with 16-byte aligned rows) and with their
// arithmetic: nibble -> bf16 (q + 24) by one v_alignbit_b32 and one v_and_or_b32 per pair, products
// accumulated in fp32 on v_mfma_f32_16x16x32_bf16, per 128-k group acc += s * (tmp - 24 * rowsum) in
// fp32, weights never rounded, one rounding to bf16 after the epilogue's adds. Wherever the group
// partial sums are exact in fp32 it gives the bits of the two GEMVs.
//
// The structure is kernels/gemm_wr.hip's, which suits this format better than it suits bf16:
//  * 4 waves (one per SIMD), a 128-row x BN tile (BN = 128), each wave owns ALL 128 rows x
//    BN/4 columns, so every packed weight word is fetched by exactly one wave: one 16-byte load per
//    lane is a whole scale group of a 16-column tile (four 32-k B fragments), its scale a 4-byte load
//    beside it, both non-temporal, straight into a register ring NS-1 = 3 groups ahead. A ring slot
//    is 5 registers per tile and 128 k, a quarter of gemm_wr's. The nibbles become bf16 pairs in
//    registers right before the MFMAs that use them; weights never touch LDS.
//  * only A goes through LDS: LDS-DMA (global_load_lds) of whole 128-byte rows into gemm_wr's
//    XOR-swizzled image (16-B piece c of row r at piece c ^ (r & 7): the fragment ds_read_b128s are
//    conflict-free), two such images per 128-k group, a ring of NS = 4 groups. One barrier per group
//    behind a counted vmcnt: at barrier(c) the groups c and c + 1 are in LDS for every wave, the loads
//    of group c + 2 stay in flight, and the DMA of group c + 3 (one instruction per MFMA phase, eight
//    phases per group) refills the slot every wave left before the barrier. Rows >= M of the last row
//    tile are clamped to row M - 1 on load and masked on store.
//  * row sums: the per-group row sums of A are needed in the accumulator layout. Each wave forms them
//    for TWO of the eight row blocks, one group ahead, by four MFMAs per row block against an
//    all-ones B fragment (8 MFMAs beside the 32 * FN of the group: +12.5 % at BN 128, +6.25 % at BN
//    256, where one such MFMA per (row block, k-fragment) in every wave costs +50 % / +25 %), and hands
//    them to the other waves through 1 KiB of LDS, double-buffered across the group's barrier. The
//    fold is two fp32 FMAs per accumulator and group, done for four row blocks at a time so that it
//    overlaps the other four row blocks' MFMAs.
//  * registers: the running accumulators are 32 * FN registers per lane, the group's tmp 16 * FN
//    (four row blocks at a time), the converted fragments 16 * FN, the ring 20 * FN. hipcc's report
//    (-Rpass-analysis=kernel-resource-usage), the same for all four epilogues: BN 128 (FN 2): 240
//    VGPRs + 68 AGPRs (the group's tmp lives in AGPRs), no scratch, no spill. BN 256 (FN 4): 256 +
//    256 registers, 54 VGPRs spilled to 148 bytes of scratch per lane - a kernel that spills is not
//    done, so ONLY BN 128 IS BUILT; the body stays a template on FN.
//  * K is split over SK workgroups in whole groups (SK in 1 / 2 / 4 / 8, SK <= K / 128) where
//    ceil(M / 128) * N / BN tiles do not fill the CUs, with the wait-free hand-off of w4_common.h,
//    one arrival counter per output tile (w4_gemm_tail.h, shared with gemm_mx4.hip).
//  * epilogues: EPI_STORE (bias, GELU), EPI_RESID (bias; ss_out), EPI_SWIGLU (ss_in), EPI_QKV (RoPE
//    or bias, KV append; ss_in), with the fused-RMSNorm fields: w4_gemm_tail.h.
#include "w4_gemm_tail.h"

namespace {

constexpr int GI_BM = W4TileGeo<1>::BM, GI_NS = 4;
constexpr int GI_HALF = GI_BM * 128;  // one 64-k image of 128-byte rows: 16 KiB
constexpr int GI_ABUF = 2 * GI_HALF;  // one 128-k group of A: 32 KiB

template <int FN>
struct GiGeo : W4TileGeo<FN> {
  using W4TileGeo<FN>::EPI_BYTES;
  static constexpr int ADMA = GI_ABUF / 1024 / 4;  // A DMA instructions per wave and group (8)
  static constexpr int PER = ADMA + 2 * FN;        // VMEM instructions per wave and group
  static constexpr int RING = GI_NS * GI_ABUF;
  static constexpr int RS_OFF = RING > EPI_BYTES ? RING : EPI_BYTES;  // row sums [2][128] fp32
  static constexpr int RSTD_OFF = RS_OFF + 2 * GI_BM * 4;             // row rstd [128] fp32
  static constexpr int FLAG_OFF = RSTD_OFF + GI_BM * 4;
  static constexpr int SMEM = FLAG_OFF + 16;
  static_assert(SMEM <= 160 * 1024, "LDS budget");
  static_assert(ADMA == 8, "one A DMA per MFMA phase");
  static_assert(PER <= 63, "vmcnt range");
};

// Group c of this workgroup's K range, ring slot c % NS:
//   vmcnt(PER) + barrier: groups c and c + 1 are in LDS for every wave, every wave has left slot
//            (c - 1) % NS and published the row sums of group c
//   the weight loads of group c + NS - 1 into register slot (c - 1) % NS
//   8 phases (4 row blocks x one 32-k fragment each): 4 * FN MFMAs, the 4 fragment reads of the
//            next phase (the last phase: of group c + 1), one A DMA of group c + NS - 1
//   the row sums of group c + 1 for this wave's two row blocks -> LDS
//   the fold of group c
template <int FN, int EPI>
LSA_DEVICE void gemm_int4_body(unsigned char* smem, const bf16_raw* __restrict__ A, int lda,
                               const unsigned char* __restrict__ wq, const float* __restrict__ wscale, int M, int N,
                               int K, int SK, const EpiArgs& ep, float* __restrict__ slab,
                               unsigned* __restrict__ counters) {
  using Geo = GiGeo<FN>;
  constexpr int TN = Geo::TN, BN = Geo::BN, NS = GI_NS;
  const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // column owner
  const int G = K >> 7, MT = (M + GI_BM - 1) / GI_BM, NT = N / BN, NTILES = MT * NT;
  const int tile = blockIdx.x % NTILES, s = blockIdx.x / NTILES;  // row tiles fastest: they share a weight panel
  const int mt = tile % MT, nt = tile / MT;
  const int m0 = mt * GI_BM, n16 = (nt * BN + w * TN) >> 4;  // this wave's first 16-column tile
  const int g_lo = s * G / SK, nchunk = (s + 1) * G / SK - g_lo, last = nchunk - 1;  // host: SK <= G

  float* s_rs = reinterpret_cast<float*>(smem + Geo::RS_OFF);
  float* s_rstd = reinterpret_cast<float*>(smem + Geo::RSTD_OFF);
  int* s_flag = reinterpret_cast<int*>(smem + Geo::FLAG_OFF);

  // A DMA: wave w fills 8-row blocks w * 4 + (d & 3) of half d >> 2 of every ring slot; lane ->
  // row lane / 8 of the block, LDS piece lane % 8, which holds global piece (lane % 8) ^ (row % 8)
  unsigned aoff[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int row = (w * 4 + d) * 8 + (lane >> 3);
    const int ch = (lane & 7) ^ ((lane >> 3) & 7);
    aoff[d] = (unsigned)((min(m0 + row, M - 1) * lda + ch * 8) * 2);
  }
  const unsigned char* abase = reinterpret_cast<const unsigned char*>(A) + (size_t)g_lo * 256;
  auto dma = [&](int ring, int d, int c) {
    __builtin_amdgcn_global_load_lds(
        abase + (size_t)c * 256 + (d >> 2) * 128 + aoff[d & 3],
        (__attribute__((address_space(3))) void*)(smem + ring * GI_ABUF + (d >> 2) * GI_HALF + (w * 4 + (d & 3)) * 1024),
        16, 0, 0);
  };
  // fragment h (32 k) of row block i: row lane % 16, global piece (h & 1) * 4 + lane / 16 of half h / 2
  const unsigned roff0 = (lane & 15) * 128 + ((kq ^ (lane & 7)) * 16);
  const unsigned roff1 = (lane & 15) * 128 + (((4 + kq) ^ (lane & 7)) * 16);
  auto rd = [&](int ring, int h, int i) -> u32x4_t {
    return ld16(smem + ring * GI_ABUF + (h >> 1) * GI_HALF + i * 2048 + ((h & 1) ? roff1 : roff0));
  };

  // weights: wave-uniform bases of this wave's column panel (SGPRs; + 1 KiB / 64 B per group) and
  // per-lane offsets per 16-column tile j: the saddr form, no per-load address VALU. Inline asm, as
  // in gemm_wr.hip: the compiler cannot count a register load whose value is used NS-1 groups later
  // and would drain the whole prefetch (vmcnt(0)) at the loop head; the counted wait at the top of
  // every group covers these loads.
  const unsigned char* wsb = wq + ((size_t)n16 * G + g_lo) * 1024;
  const unsigned char* ssb = reinterpret_cast<const unsigned char*>(wscale + ((size_t)n16 * G + g_lo) * 16);
  unsigned wvo[FN], svo[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    wvo[j] = (unsigned)(lane * 16 + j * G * 1024);
    svo[j] = (unsigned)((lane & 15) * 4 + j * G * 64);
  }
  auto load_b = [&](int c, u32x4_t (&b)[FN], float (&sc)[FN]) {
    const unsigned char* wb = wsb + (size_t)c * 1024;
    const unsigned char* sb = ssb + (size_t)c * 64;
#pragma unroll
    for (int j = 0; j < FN; ++j) {  // nt: once-read weight stream
      asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(b[j]) : "v"(wvo[j]), "s"(wb) : "memory");
      asm volatile("global_load_dword %0, %1, %2 nt" : "=v"(sc[j]) : "v"(svo[j]), "s"(sb) : "memory");
    }
  };
  unsigned mask = kNibMask, base = kBf16x16;
  asm volatile("" : "+s"(mask), "+v"(base));  // no instruction: hides the constants (int4x8_to_bf16)
  const u32x4_t ones = {kBf16One, kBf16One, kBf16One, kBf16One};
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};

  f32x4_t acc[8][FN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = fzero;
  u32x4_t bw[NS][FN];  // indexed by compile-time slots only (the loop is unrolled by NS)
  float sw[NS][FN];
  u32x4_t af[2][4];    // the A fragments of this phase and of the next

  // row sums of the group in ring slot ``ring`` for row blocks 2w, 2w + 1 -> s_rs[buf]: against the
  // all-ones fragment every column of the MFMA result is the row sum, in the accumulator layout
  auto row_sums = [&](int ring, int buf) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      f32x4_t t = fzero;
#pragma unroll
      for (int h = 0; h < 4; ++h) t = mfma16(rd(ring, h, 2 * w + rb), ones, t);
      if ((lane & 15) == 0) *reinterpret_cast<f32x4_t*>(s_rs + buf * GI_BM + (2 * w + rb) * 16 + kq * 4) = t;
    }
  };

  // prologue: groups 0 .. NS-2 in flight (per group: W then A)
  static_for(std::make_integer_sequence<int, NS - 1>{}, [&](auto sc) {
    constexpr int S = decltype(sc)::value;
    load_b(min(S, last), bw[S], sw[S]);
#pragma unroll
    for (int d = 0; d < Geo::ADMA; ++d) dma(S, d, min(S, last));
  });
  vm_wait<Geo::PER>();
  fenced_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) af[0][i] = rd(0, 0, i);
  row_sums(0, 0);

  auto step = [&](int c, auto slot_c) {
    constexpr int slot = decltype(slot_c)::value, nslot = (slot + NS - 1) % NS, s1 = (slot + 1) % NS;
    vm_wait<Geo::PER>();
    fenced_barrier();
    const int cp = min(c + NS - 1, last);  // past the end: re-fetch the last group (dead)
    load_b(cp, bw[nslot], sw[nslot]);
    u32x4_t bf[4][FN];
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int h = 0; h < 4; ++h) bf[h][j] = int4x8_to_bf16(bw[slot][j][h], mask, base);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      f32x4_t tmp[4][FN];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) tmp[i][j] = fzero;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int p = b * 4 + h;  // phase
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < FN; ++j) tmp[i][j] = mfma16(af[p & 1][i], bf[h][j], tmp[i][j]);
          if (p < 7)
            af[(p + 1) & 1][i] = rd(slot, (p + 1) & 3, ((p + 1) >> 2) * 4 + i);
          else
            af[0][i] = rd(s1, 0, i);
        }
        dma(nslot, p, cp);
      }
      if (b == 1 && c < last) row_sums(s1, (c + 1) & 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4_t rs = *reinterpret_cast<const f32x4_t*>(s_rs + (c & 1) * GI_BM + (b * 4 + i) * 16 + kq * 4);
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[b * 4 + i][j][r] =
                __builtin_fmaf(sw[slot][j], __builtin_fmaf(-kOffset, rs[r], tmp[i][j][r]), acc[b * 4 + i][j][r]);
      }
    }
  };
  for (int c = 0; c < nchunk; c += NS) {
    static_for(std::make_integer_sequence<int, NS>{}, [&](auto sc) {
      if (c + decltype(sc)::value < nchunk) step(c + decltype(sc)::value, sc);
    });
  }
  vm_wait<0>();  // the dead prefetches land before the LDS is reused ...
  // ... and before their destination registers are (gemm_wr.hip): keep the ring live up to here
#pragma unroll
  for (int sl = 0; sl < NS; ++sl)
#pragma unroll
    for (int j = 0; j < FN; ++j) asm volatile("" ::"v"(bw[sl][j]), "v"(sw[sl][j]));
  fenced_barrier();

  // the split-K hand-off and the epilogue: w4_gemm_tail.h
  if (SK > 1 && !w4_gemm_splitk<FN>(acc, slab, counters, s_flag, tile, NTILES, s, SK)) return;
  w4_gemm_epilogue<FN, EPI>(smem, s_rstd, acc, ep, M, m0, nt * BN);
}

template <int FN, int EPI>
__global__ __launch_bounds__(GiGeo<FN>::NTHR) void gemm_int4_kernel(
    const bf16_raw* __restrict__ A, int lda, const unsigned char* __restrict__ wq, const float* __restrict__ wscale,
    int M, int N, int K, int SK, EpiArgs ep, float* __restrict__ slab, unsigned* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[GiGeo<FN>::SMEM];
  gemm_int4_body<FN, EPI>(smem, A, lda, wq, wscale, M, N, K, SK, ep, slab, counters);
}

}  // namespace

// (bn, depth) built: (128, 4) - llm_sharding_amd/ops/int4.py INT4_GEMM_CONFIGS. K is split
// into sk runs of whole 128-k groups, as evenly as possible (sk in 1 / 2 / 4 / 8, sk <= K / 128).
// Workspace (sk > 1): slab_floats >= sk * ceil(M / 128) * 128 * N fp32 (under 2 GiB), n_counters >=
// ceil(M / 128) * N / bn zero-initialised uint32 (reset by the kernel). Anything the kernel's indexing
// cannot take returns LSA_BAD_SHAPE / LSA_UNSUPPORTED before any launch.
extern "C" int lsa_gemm_int4(const void* a, int lda, const void* wq4, const float* scales, int M, int N, int K, int epi,
                             const EpiArgs* ep, int bn, int depth, int sk, float* slab, long long slab_floats,
                             unsigned* counters, int n_counters, hipStream_t stream) {
  if (!a || !wq4 || !scales || !ep || M < 1 || N < 1 || K < 128 || K % 128 || lda < K || lda % 8 || !aligned16(a))
    return LSA_BAD_SHAPE;
  if (bn != 128 || depth != GI_NS) return LSA_UNSUPPORTED;
  return dispatch_epi(epi, [&](auto e) -> int {  // an unknown epilogue is refused before the checks below
    constexpr int FN = 2, EPI = decltype(e)::value;
    if (N % bn || (long long)M * lda > 0x3fffffffLL) return LSA_BAD_SHAPE;
    if (check_gemm_split(sk, K / 128, M, N, bn, slab, slab_floats, counters, n_counters) != LSA_OK ||
        check_epi_args(epi, ep, N, K) != LSA_OK)
      return LSA_BAD_SHAPE;
    const int tiles = ((M + GiGeo<FN>::BM - 1) / GiGeo<FN>::BM) * (N / GiGeo<FN>::BN);
    gemm_int4_kernel<FN, EPI><<<tiles * sk, GiGeo<FN>::NTHR, 0, stream>>>(
        static_cast<const bf16_raw*>(a), lda, static_cast<const unsigned char*>(wq4), scales, M, N, K, sk, *ep, slab,
        counters);
    LSA_CHECK_LAUNCH();
    return LSA_OK;
  });
}
