// W4A8 GEMM on the block-scaled MFMA for prefill chunks and decode batches above 128 rows:
//   y[M, N] = sum over 32-k blocks of 2^(ea + eb) * (a8[M, block] @ w4[N, block]^T),  any M >= 1,
// on gemv_mx4.hip's weights (Wq[nt][K/128][lane][16 B] fp4 fragments, S[nt][K/512][lane] exponent
// dwords) and with its arithmetic: v_mfma_scale_f32_16x16x128_f8f6f4 applies both block scales,
// fp32 accumulation, one rounding to bf16 after the epilogue's adds.
//
// Two kernels:
//  * lsa_quant_act_mx8, the pre-pass: bf16 rows -> the MXFP8 image of A, once per projection input
//    (in the GEMM every column workgroup would repeat it). The quantiser is gemv_mx4.hip's
//    (mx8_quant.h). Codes A8[ceil(M/16)][K/128][2 halves][64 lanes][16 B] in gemv_mx4.hip's LDS
//    order: k of the step in half k / 64, lane 16 * ((k % 64) / 16) + row, byte k % 16 - a row
//    block's K-step is 2 KiB contiguous and is the MFMA's A operand as two ds_read_b128. Exponents
//    EA[ceil(M/16)][ceil(K/512)][64 lanes] dwords: byte i of lane 16 b + row = the e8m0 byte of
//    32-block b in K-step 4 g + i, picked by op_sel as the weight scales are (127 past K). Rows
//    >= M of the last row block: zero codes, exponent 127. One wave per (row block, 512-k group,
//    32-block): a lane quantises its quad's block in the group's four K-steps and the quad's
//    first lane stores the exponent dword.
//  * lsa_gemm_mx4: 256 threads (one wave per SIMD), a 128-row x BN tile (BN = 64 FN), each wave owns
//    ALL 128 rows x BN/4 columns (gemm_wr.hip's and gemm_int4.hip's split), so every fp4 fragment is
//    fetched by exactly one wave: one non-temporal 16-B load per lane, 16-column tile and K-step,
//    straight into the MFMA's B registers through a ring three K-steps ahead; the weight scale
//    dwords and the A exponent dwords (8 row blocks, one dword each: no LDS read for them at all)
//    come one 512-k group ahead. Weights never touch LDS and there is no unpack arithmetic.
//    A comes by LDS-DMA from the pre-pass image: a K-step of the row tile is 16 KiB, already in
//    fragment order, so the copy is linear (four 1-KiB instructions per wave), needs no swizzle
//    and the ds_read_b128s are conflict-free. A ring of 4 K-steps (64 KiB), one barrier per K-step
//    behind a counted vmcnt; the DMA of step c + 3 is issued in pieces between the MFMA groups of
//    step c into the slot every wave left before the barrier. Per K-step and wave: 8 row blocks x
//    FN MFMAs of K = 128 and 16 ds_read_b128, with no branch in the step so that the reads run
//    ahead of the MFMAs. Row blocks past ceil(M/16) re-read the last one and are masked at the store.
//  * K is split over SK workgroups in whole 512-k scale groups (the last may be short) where the
//    output tiles do not fill the CUs, with the wait-free hand-off of w4_common.h, one arrival
//    counter per output tile (w4_gemm_tail.h, shared with gemm_int4.hip).
//  * epilogues and the fused-RMSNorm fields: w4_gemm_tail.h.
//  * registers, hipcc's report (-Rpass-analysis=kernel-resource-usage): BN 128 (FN 2): 146-147
//    VGPRs + 64 AGPRs, 74256 B of LDS, no scratch, for all four epilogues. BN 256 (FN 4): 254 VGPRs +
//    128 AGPRs, 139792 B of LDS, no scratch for STORE / RESID but 36 bytes of scratch per lane for
//    SWIGLU / QKV - a kernel that spills is not done, so ONLY BN 128 IS BUILT; the body stays a
//    template on FN.
#include "mx8_quant.h"
#include "w4_gemm_tail.h"

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));

constexpr int GM_BM = W4TileGeo<1>::BM, GM_NS = 4;
constexpr int GM_ASTEP = GM_BM * 128;  // e4m3 codes of one K-step of a row tile: 16 KiB
constexpr int GM_ADMA = GM_ASTEP / 1024 / 4;  // A DMA instructions per wave and K-step (4)

// ------------------------------------------------------------------------------ the pre-pass
__global__ __launch_bounds__(256) void quant_act_mx8_kernel(const bf16_raw* __restrict__ x, int ldx,
                                                            const int* __restrict__ a_rows,
                                                            unsigned char* __restrict__ a8,
                                                            unsigned* __restrict__ ea, int M, int KS, int NG) {
  const int lane = threadIdx.x & 63, blk = threadIdx.x >> 6;  // wave = 32-block of the K-step
  const int g = blockIdx.x % NG, rb = blockIdx.x / NG;
  const int ar = lane >> 2, asub = lane & 3, r = rb * 16 + ar;
  const bool valid = r < M;
  const bf16_raw* xp = x + (size_t)(valid ? (a_rows ? a_rows[r] : r) : 0) * ldx + blk * 32 + asub * 8;
  // k = 32 blk + 8 asub .. + 7 of the step: register half k / 64 of lane group (k % 64) / 16, byte k % 16
  const int dst = ((blk >> 1) * 64 + ((blk & 1) * 2 + (asub >> 1)) * 16 + ar) * 16 + (asub & 1) * 8;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  u32x4_t v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (valid && 4 * g + i < KS) ? ld16(xp + (size_t)(4 * g + i) * 128) : zero;
  unsigned ew = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    unpack8(v[i], f);
    u32x2_t c;
    const int e = mx8_quant_quad(f, c);  // an absent K-step: all zero, exponent 127
    ew |= (unsigned)e << (8 * i);
    if (4 * g + i < KS) *reinterpret_cast<u32x2_t*>(a8 + ((size_t)rb * KS + 4 * g + i) * 2048 + dst) = c;
  }
  if (asub == 0) ea[((size_t)rb * NG + g) * 64 + blk * 16 + ar] = ew;
}

// ------------------------------------------------------------------------------ the GEMM
template <int FN>
struct GmGeo : W4TileGeo<FN> {
  using W4TileGeo<FN>::EPI_BYTES;
  static constexpr int PER = FN + GM_ADMA;  // VMEM instructions per wave and K-step
  static constexpr int GRP = FN + 8;        // + per 512-k group: FN weight scale dwords, 8 A exponent dwords
  static constexpr int RING = GM_NS * GM_ASTEP;
  static constexpr int RSTD_OFF = RING > EPI_BYTES ? RING : EPI_BYTES;  // row rstd [128] fp32
  static constexpr int FLAG_OFF = RSTD_OFF + GM_BM * 4;
  static constexpr int SMEM = FLAG_OFF + 16;
  static_assert(SMEM <= 160 * 1024, "LDS budget");
  static_assert(GM_ADMA == 4, "one A DMA per pair of row blocks' MFMAs");
  static_assert(2 * PER + GRP <= 63, "vmcnt range");
};

// K-step c of this workgroup's range (slot c % 4 of the A ring and of the weight ring; the range
// starts on a scale group, so the slot is also the step's byte in the scale dwords). In program
// order a wave issues, in step c: the weight loads of step c + 3, in slot 0 the scale / exponent
// dwords of the NEXT group, the A DMA of step c + 3. At the top of step c everything issued up to
// step c - 3 must have landed: the waits leave the loads of steps c - 2 and c - 1 in flight, which
// include a group's dwords when one of them had slot 0.
template <int FN, int EPI>
LSA_DEVICE void gemm_mx4_body(unsigned char* smem, const unsigned char* __restrict__ a8,
                              const unsigned* __restrict__ ea, const unsigned char* __restrict__ wq,
                              const unsigned* __restrict__ wscale, int M, int N, int K, int SK, const EpiArgs& ep,
                              float* __restrict__ slab, unsigned* __restrict__ counters) {
  using Geo = GmGeo<FN>;
  constexpr int TN = Geo::TN, BN = Geo::BN, NS = GM_NS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // column owner
  const int KS = K >> 7, NG = (KS + 3) >> 2, RB = (M + 15) >> 4;
  const int MT = (M + GM_BM - 1) / GM_BM, NT = N / BN, NTILES = MT * NT;
  const int tile = blockIdx.x % NTILES, s = blockIdx.x / NTILES;  // row tiles fastest: they share a weight panel
  const int mt = tile % MT, nt = tile / MT;
  const int m0 = mt * GM_BM, n16 = (nt * BN + w * TN) >> 4;  // this wave's first 16-column tile
  const int g0 = s * NG / SK;                                // host: SK <= NG, so every split has a group
  const int ks_lo = g0 * 4, ks_hi = min(((s + 1) * NG / SK) * 4, KS);
  const int nstep = ks_hi - ks_lo, last = nstep - 1, glast = last >> 2;

  float* s_rstd = reinterpret_cast<float*>(smem + Geo::RSTD_OFF);
  int* s_flag = reinterpret_cast<int*>(smem + Geo::FLAG_OFF);

  // A DMA: wave w fills row blocks 2w, 2w + 1 of every ring slot, piece d = (row block, half);
  // a piece is 1 KiB in the image and in LDS, 16 B per lane. A row block past the image: the last.
  const int lane16 = lane * 16, lane4 = lane * 4;
  const unsigned char* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    asrc[i] = a8 + ((size_t)min(mt * 8 + 2 * w + i, RB - 1) * KS + ks_lo) * 2048 + lane16;
  auto dma = [&](int ring, int d, int c) {
    __builtin_amdgcn_global_load_lds(
        asrc[d >> 1] + (size_t)c * 2048 + (d & 1) * 1024,
        (__attribute__((address_space(3))) void*)(smem + ring * GM_ASTEP + ((2 * w + (d >> 1)) * 2 + (d & 1)) * 1024),
        16, 0, 0);
  };
  // Weights, scales and A exponents: wave-uniform bases + one per-lane offset (the saddr form).
  // Inline asm, as in gemm_wr.hip / gemm_int4.hip: the compiler cannot count a register load
  // whose value is used steps later and would drain the whole prefetch at the loop head; the
  // counted wait at the top of every step covers these loads.
  const unsigned char* wsb = wq + ((size_t)n16 * KS + ks_lo) * 1024;
  const unsigned char* ssb = reinterpret_cast<const unsigned char*>(wscale + ((size_t)n16 * NG + g0) * 64);
  const unsigned char* esb = reinterpret_cast<const unsigned char*>(ea + (size_t)g0 * 64);
  auto load_b = [&](int c, u32x4_t (&b)[FN]) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {  // nt: once-read weight stream
      const unsigned char* p = wsb + ((size_t)j * KS + c) * 1024;
      asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(b[j]) : "v"(lane16), "s"(p) : "memory");
    }
  };
  auto load_grp = [&](int g, unsigned (&sc)[FN], unsigned (&ex)[8]) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const unsigned char* p = ssb + ((size_t)j * NG + g) * 256;
      asm volatile("global_load_dword %0, %1, %2 nt" : "=v"(sc[j]) : "v"(lane4), "s"(p) : "memory");
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned char* p = esb + ((size_t)min(mt * 8 + i, RB - 1) * NG + g) * 256;
      asm volatile("global_load_dword %0, %1, %2" : "=v"(ex[i]) : "v"(lane4), "s"(p) : "memory");
    }
  };
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};

  f32x4_t acc[8][FN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = fzero;
  u32x4_t bw[NS][FN];  // indexed by compile-time slots only (the loop is unrolled by NS)
  unsigned sc[FN], scn[FN], ex[8], exn[8];

  // prologue: the first group's dwords, then steps 0 .. 2 (per step: W then A)
  load_grp(0, sc, ex);
  static_for(std::make_integer_sequence<int, NS - 1>{}, [&](auto sl) {
    constexpr int S = decltype(sl)::value;
    load_b(min(S, last), bw[S]);
#pragma unroll
    for (int d = 0; d < GM_ADMA; ++d) dma(S, d, min(S, last));
  });

  auto step = [&](int c, auto slot_c) {
    constexpr int S = decltype(slot_c)::value, nslot = (S + NS - 1) % NS;
    vm_wait<2 * Geo::PER + ((S == 1 || S == 2) ? Geo::GRP : 0)>();
    fenced_barrier();
    const int cp = min(c + NS - 1, last);  // past the end: re-fetch the last step (dead)
    load_b(cp, bw[nslot]);
    if (S == 0) load_grp(min((c >> 2) + 1, glast), scn, exn);
    i32x8_t b8[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const u32x4_t bt = bw[S][j];
      b8[j] = i32x8_t{(int)bt[0], (int)bt[1], (int)bt[2], (int)bt[3], 0, 0, 0, 0};
    }
    const unsigned char* ab = smem + S * GM_ASTEP + lane16;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u32x4_t lo = ld16(ab + (i * 2) * 1024), hi = ld16(ab + (i * 2 + 1) * 1024);
      const i32x8_t av = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, b8[j], acc[i][j], 0 /* A: e4m3 */,
                                                                     4 /* B: e2m1 */, S, (int)ex[i], S, (int)sc[j]);
      if (i & 1) dma(nslot, i >> 1, cp);
    }
    if (S == 3) {  // landed: issued four steps ago, and every wait since covered them
#pragma unroll
      for (int j = 0; j < FN; ++j) sc[j] = scn[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) ex[i] = exn[i];
    }
  };
  for (int c = 0; c < nstep; c += NS) {
    static_for(std::make_integer_sequence<int, NS>{}, [&](auto sl) {
      if (c + decltype(sl)::value < nstep) step(c + decltype(sl)::value, sl);
    });
  }
  vm_wait<0>();  // the dead prefetches land before the LDS is reused ...
  // ... and before their destination registers are (gemm_wr.hip): keep the rings live up to here
#pragma unroll
  for (int sl = 0; sl < NS; ++sl)
#pragma unroll
    for (int j = 0; j < FN; ++j) asm volatile("" ::"v"(bw[sl][j]));
#pragma unroll
  for (int j = 0; j < FN; ++j) asm volatile("" ::"v"(sc[j]), "v"(scn[j]));
#pragma unroll
  for (int i = 0; i < 8; ++i) asm volatile("" ::"v"(ex[i]), "v"(exn[i]));
  fenced_barrier();

  // the split-K hand-off and the epilogue: w4_gemm_tail.h
  if (SK > 1 && !w4_gemm_splitk<FN>(acc, slab, counters, s_flag, tile, NTILES, s, SK)) return;
  w4_gemm_epilogue<FN, EPI>(smem, s_rstd, acc, ep, M, m0, nt * BN);
}

template <int FN, int EPI>
__global__ __launch_bounds__(GmGeo<FN>::NTHR) void gemm_mx4_kernel(
    const unsigned char* __restrict__ a8, const unsigned* __restrict__ ea, const unsigned char* __restrict__ wq,
    const unsigned* __restrict__ wscale, int M, int N, int K, int SK, EpiArgs ep, float* __restrict__ slab,
    unsigned* __restrict__ counters) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[GmGeo<FN>::SMEM];
  gemm_mx4_body<FN, EPI>(smem, a8, ea, wq, wscale, M, N, K, SK, ep, slab, counters);
}

}  // namespace

// bf16 rows x[M, >= K] (16-B aligned, optionally gathered through a_rows) -> the MXFP8 image of A:
// a8: ceil(M/16) * 16 * K code bytes, ea: ceil(M/16) * ceil(K/512) * 64 exponent dwords (layouts
// above). Every byte of both is written by every call.
extern "C" int lsa_quant_act_mx8(const void* x, int ldx, const int* a_rows, void* a8, void* ea, int M, int K,
                                 hipStream_t stream) {
  if (!x || !a8 || !ea || M < 1 || K < 128 || K % 128 || ldx < K || ldx % 8 || !aligned16(x) || !aligned16(a8) ||
      (reinterpret_cast<size_t>(ea) & 3))
    return LSA_BAD_SHAPE;
  const long long RB = (M + 15) / 16, KS = K / 128, NG = (KS + 3) / 4;
  if (RB * NG > 0x7fffffffLL) return LSA_BAD_SHAPE;
  quant_act_mx8_kernel<<<(unsigned)(RB * NG), 256, 0, stream>>>(static_cast<const bf16_raw*>(x), ldx, a_rows,
                                                                static_cast<unsigned char*>(a8),
                                                                static_cast<unsigned*>(ea), M, (int)KS, (int)NG);
  LSA_CHECK_LAUNCH();
  return LSA_OK;
}

// bn built: 128 - llm_sharding_amd/ops/mx4.py MX4_GEMM_CONFIGS. K is split into sk runs of
// whole 512-k scale groups, as evenly as possible (sk in 1 / 2 / 4 / 8, sk <= ceil(K / 512)).
// Workspace (sk > 1): slab_floats >= sk * ceil(M / 128) * 128 * N fp32 (under 2 GiB), n_counters >=
// ceil(M / 128) * N / bn zero-initialised uint32 (reset by the kernel). Anything the kernel's indexing
// cannot take returns LSA_BAD_SHAPE / LSA_UNSUPPORTED before any launch.
extern "C" int lsa_gemm_mx4(const void* a8, const void* ea, const void* wq, const void* scales, int M, int N, int K,
                            int epi, const EpiArgs* ep, int bn, int sk, float* slab, long long slab_floats,
                            unsigned* counters, int n_counters, hipStream_t stream) {
  if (!a8 || !ea || !wq || !scales || !ep || M < 1 || N < 1 || K < 128 || K % 128 || !aligned16(a8) ||
      !aligned16(wq) || (reinterpret_cast<size_t>(ea) & 3) || (reinterpret_cast<size_t>(scales) & 3))
    return LSA_BAD_SHAPE;
  if (bn != 128) return LSA_UNSUPPORTED;
  return dispatch_epi(epi, [&](auto e) -> int {  // an unknown epilogue is refused before the checks below
    constexpr int FN = 2, EPI = decltype(e)::value;
    if (N % bn || (long long)N * K / 2 >= (1ll << 31)) return LSA_BAD_SHAPE;
    if (check_gemm_split(sk, (K / 128 + 3) / 4, M, N, bn, slab, slab_floats, counters, n_counters) != LSA_OK ||
        check_epi_args(epi, ep, N, K) != LSA_OK)
      return LSA_BAD_SHAPE;
    const int tiles = ((M + GmGeo<FN>::BM - 1) / GmGeo<FN>::BM) * (N / GmGeo<FN>::BN);
    gemm_mx4_kernel<FN, EPI><<<tiles * sk, GmGeo<FN>::NTHR, 0, stream>>>(
        static_cast<const unsigned char*>(a8), static_cast<const unsigned*>(ea), static_cast<const unsigned char*>(wq),
        static_cast<const unsigned*>(scales), M, N, K, sk, *ep, slab, counters);
    LSA_CHECK_LAUNCH();
    return LSA_OK;
  });
}
