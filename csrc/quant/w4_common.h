// What the 4-bit-weight kernels of this folder share below their tails: the int4 nibble unpack, the
// software-pipeline helpers, the epilogue dispatch and the arrival ticket of the wait-free split-K
// hand-off (w4_gemm_tail.h and w4_coop_tail.h build the two hand-offs on it). Header code compiles
// under the including file's flags.
#pragma once
#include "../kernels/epilogue.h"

#include <utility>

// ------------------------------------------------------------------------------ int4 unpack
constexpr unsigned kNibMask = 0x00780078u;  // a nibble at mantissa bits 3..6 of both halves
constexpr unsigned kBf16x16 = 0x41804180u;  // bf16 (16.0, 16.0)
constexpr unsigned kBf16One = 0x3f803f80u;  // bf16 (1.0, 1.0)
constexpr float kOffset = 24.0f;            // 16 (the bf16 base) + 8 (the nibble offset)

// one packed dword (8 nibbles = one lane's share of a 32-k B fragment) -> 8 bf16 (q + 24).
// ``mask`` / ``base`` arrive as registers (an SGPR and a VGPR the caller made opaque), so that
// (w & mask) | base is ONE v_and_or_b32: with two literals the compiler has to emit v_and + v_or
LSA_DEVICE u32x4_t int4x8_to_bf16(unsigned w, unsigned mask, unsigned base) {
  u32x4_t r;
  r[0] = (w & mask) | base;
  r[1] = (__builtin_amdgcn_alignbit(w, w, 4) & mask) | base;
  r[2] = (__builtin_amdgcn_alignbit(w, w, 8) & mask) | base;
  r[3] = (__builtin_amdgcn_alignbit(w, w, 12) & mask) | base;
  return r;
}

// ------------------------------------------------------------------------------ pipeline helpers
template <int N>
LSA_DEVICE void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// f(integral_constant<S>) for every S: ring slots stay compile-time indices
template <int... S, typename F>
LSA_DEVICE void static_for(std::integer_sequence<int, S...>, F&& f) {
  (f(std::integral_constant<int, S>{}), ...);
}

// f(integral_constant<S>) for S = 0, 1, ... while f returns true
template <int... S, typename F>
LSA_DEVICE bool static_all(std::integer_sequence<int, S...>, F&& f) {
  return (f(std::integral_constant<int, S>{}) && ...);
}

// a workgroup barrier the scheduler moves nothing across
LSA_DEVICE void fenced_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// ------------------------------------------------------------------------------ host side
static inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// f(integral_constant<EPI>) for the four projection epilogues. No arg-max epilogue: the lm_head
// stays bf16.
template <typename F>
int dispatch_epi(int epi, F&& f) {
  switch (epi) {
    case EPI_STORE: return f(std::integral_constant<int, EPI_STORE>{});
    case EPI_RESID: return f(std::integral_constant<int, EPI_RESID>{});
    case EPI_SWIGLU: return f(std::integral_constant<int, EPI_SWIGLU>{});
    case EPI_QKV: return f(std::integral_constant<int, EPI_QKV>{});
    default: return LSA_UNSUPPORTED;
  }
}

// ------------------------------------------------------------------------------ split-K arrival
// The wait-free hand-off (kernels/gemv_coop.hip's): K is split over SK workgroups per output unit
// (a GEMM tile, a GEMV column group). Each stores its fp32 partials to a slab with write-through
// (sc1) 16-B stores - the bytes are in memory, visible to every CU / XCD, once the store has
// completed, so no release fence is needed - then calls splitk_arrive: every wave drains its
// stores, the workgroup barriers, and one lane takes a relaxed agent-scope ticket from the unit's
// counter. The workgroup that draws SK - 1 is the last arriver: all SK partials are in memory, it
// reads them back with sc1 loads, sums them in fixed split order (deterministic, whoever arrives
// last), calls splitk_reset so that the counters are zero again for the next launch (replay-safe
// in a captured graph: nothing else touches the counter once the last ticket is drawn) and runs
// the epilogue. Every other workgroup returns; none waits for another.
LSA_DEVICE bool splitk_arrive(unsigned* counter, int SK, int* s_flag) {
  vm_wait<0>();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_flag = old == (unsigned)(SK - 1);
  }
  __syncthreads();
  return *s_flag;
}

LSA_DEVICE void splitk_reset(unsigned* counter) {
  if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
