// KV-cache fork on gfx950 (CDNA4 / MI355X): copy the first `len` positions of one sequence slot
// into up to 8 other slots, over every layer's K and V tensor, in one launch.
//
//   lsa_kv_fork        validates on the host, then one launch per chunk of the job list (one launch
//                      for every call whose tensors and jobs fit the kernel-argument struct)
//   lsa_kv_fork_calls  debug: how many launches this process has enqueued
//
// Contract. `tensors`: n_tensors base pointers, each a contiguous bf16 [n_slots, nkv, t_max, hd]
// (hd % 8 == 0, 16-byte aligned). `jobs`: n_jobs records of KVF_JOB_INTS int32
// [src, len, f, dst_0 .. dst_7] with 1 <= f <= 8. For every tensor, head h < nkv and destination d
// the len * hd elements of [src, h, 0:len, :] are copied bit for bit to [d, h, 0:len, :]; nothing
// else is written. len == 0 is a no-op. Refused with LSA_BAD_SHAPE before any launch: a slot out of
// range, len outside [0, t_max], a destination equal to its source, a slot that is a destination
// twice, a slot that is both a source and a destination.
//
// Shape of the work. A (tensor, head) span of a job is len * hd * 2 contiguous bytes in the source
// and in every destination. Spans are cut into chunks of KVF_THREADS * KVF_UNROLL 16-byte vectors
// (16 KiB); a work item is one chunk of one span of one job. Workgroups grid-stride over the work
// items of all jobs (the grid is sized to the chip, not to the byte count), so the only divisions
// are 32-bit, uniform per workgroup and once per 16 KiB. A thread issues its KVF_UNROLL loads
// before the first store; each source vector is read once and stored to all f destinations.
// Pointers and jobs travel by value in the kernel arguments: no per-call host-to-device copy.
// Byte offsets are 64-bit (a 7B layer tensor with 512 slots at t_max 2048 is 8.6 GB).
//
// `flags` bit 0 / bit 1 select non-temporal loads / stores (profiles/kv_fork.md has the
// measurement behind the default the Python binding passes).
#include "../kernels/common.h"

#include <vector>

namespace {

constexpr int KVF_THREADS = 256;
constexpr int KVF_UNROLL = 4;
constexpr int KVF_CHUNK = KVF_THREADS * KVF_UNROLL;  // 16-byte vectors per work item
constexpr int KVF_MAX_DST = 8;
constexpr int KVF_JOB_INTS = 3 + KVF_MAX_DST;
constexpr int KVF_MAX_TENSORS = 256;  // 2048 B of kernel arguments
constexpr int KVF_MAX_JOBS = 24;      // 24 x 52 B; the struct (3328 B) stays below the 4 KiB argument limit
constexpr int KVF_MAX_GRID = 256 * 8;  // 256 CUs x 8 workgroups of 256 threads

struct KvfJob {
  unsigned first;           // index of the job's first work item in the launch
  unsigned vps;             // 16-byte vectors per (tensor, head) span: len * hd / 8
  unsigned cps;             // chunks per span
  int src;
  int nd;
  int dst[KVF_MAX_DST];
};

struct KvfArgs {
  unsigned short* tensors[KVF_MAX_TENSORS];
  KvfJob jobs[KVF_MAX_JOBS];
  unsigned total;           // work items of the launch
  int n_jobs;
  int nkv;
  long long slot_elems;     // nkv * t_max * hd
  long long head_elems;     // t_max * hd
};
static_assert(sizeof(KvfArgs) <= 4096, "kernel arguments are limited to 4 KiB");

long long g_kv_fork_calls = 0;

template <bool NT_LD, bool NT_ST>
__global__ __launch_bounds__(KVF_THREADS) void kv_fork_kernel(const KvfArgs a) {
  const unsigned tid = threadIdx.x;
  for (unsigned w = blockIdx.x; w < a.total; w += gridDim.x) {
    int j = 0;
    while (j + 1 < a.n_jobs && w >= a.jobs[j + 1].first) ++j;
    const unsigned vps = a.jobs[j].vps, cps = a.jobs[j].cps;
    const unsigned local = w - a.jobs[j].first;
    const unsigned span = local / cps, chunk = local - span * cps;
    const unsigned t = span / (unsigned)a.nkv, h = span - t * (unsigned)a.nkv;
    unsigned short* base = a.tensors[t] + (size_t)h * (size_t)a.head_elems;
    const unsigned short* src = base + (size_t)a.jobs[j].src * (size_t)a.slot_elems;
    const unsigned v0 = chunk * KVF_CHUNK + tid;
    u32x4_t r[KVF_UNROLL];
#pragma unroll
    for (int k = 0; k < KVF_UNROLL; ++k) {
      const unsigned v = v0 + k * KVF_THREADS;
      if (v < vps) r[k] = NT_LD ? ld16_nt(src + (size_t)v * 8) : ld16(src + (size_t)v * 8);
    }
    const int nd = a.jobs[j].nd;
    for (int d = 0; d < nd; ++d) {
      unsigned short* dst = base + (size_t)a.jobs[j].dst[d] * (size_t)a.slot_elems;
#pragma unroll
      for (int k = 0; k < KVF_UNROLL; ++k) {
        const unsigned v = v0 + k * KVF_THREADS;
        if (v < vps) {
          if (NT_ST)
            __builtin_nontemporal_store(r[k], reinterpret_cast<u32x4_t*>(dst + (size_t)v * 8));
          else
            st16(dst + (size_t)v * 8, r[k]);
        }
      }
    }
  }
}

void launch(const KvfArgs& a, int flags, hipStream_t stream) {
  const unsigned grid = a.total < (unsigned)KVF_MAX_GRID ? a.total : (unsigned)KVF_MAX_GRID;
  switch (flags & 3) {
    case 0: kv_fork_kernel<false, false><<<grid, KVF_THREADS, 0, stream>>>(a); break;
    case 1: kv_fork_kernel<true, false><<<grid, KVF_THREADS, 0, stream>>>(a); break;
    case 2: kv_fork_kernel<false, true><<<grid, KVF_THREADS, 0, stream>>>(a); break;
    default: kv_fork_kernel<true, true><<<grid, KVF_THREADS, 0, stream>>>(a); break;
  }
}

}  // namespace

// tensors: host array of n_tensors device pointers; jobs: host array of n_jobs x KVF_JOB_INTS int32.
// Both are read before the call returns.
extern "C" int lsa_kv_fork(const void* const* tensors, int n_tensors, const int* jobs, int n_jobs, int n_slots,
                           int nkv, int t_max, int hd, int flags, hipStream_t stream) {
  if (n_tensors < 1 || n_jobs < 0 || n_slots < 1 || nkv < 1 || t_max < 1 || hd < 8 || (hd & 7)) return LSA_BAD_SHAPE;
  if (!tensors || (n_jobs > 0 && !jobs)) return LSA_BAD_SHAPE;
  for (int t = 0; t < n_tensors; ++t)
    if (!tensors[t] || (reinterpret_cast<uintptr_t>(tensors[t]) & 15)) return LSA_BAD_SHAPE;
  // 1 = source, 2 = destination
  std::vector<unsigned char> role((size_t)n_slots, 0);
  for (int j = 0; j < n_jobs; ++j) {
    const int* q = jobs + (size_t)j * KVF_JOB_INTS;
    const int src = q[0], len = q[1], nd = q[2];
    if (src < 0 || src >= n_slots || len < 0 || len > t_max || nd < 1 || nd > KVF_MAX_DST) return LSA_BAD_SHAPE;
    if (role[src] & 2) return LSA_BAD_SHAPE;
    role[src] |= 1;
    for (int d = 0; d < nd; ++d) {
      const int s = q[3 + d];
      if (s < 0 || s >= n_slots || s == src || role[s]) return LSA_BAD_SHAPE;
      role[s] = 2;
    }
  }
  const long long head_elems = (long long)t_max * hd;
  // the work items of one launch are counted in 32 bits
  if ((long long)KVF_MAX_TENSORS * nkv * ((head_elems / 8 + KVF_CHUNK - 1) / KVF_CHUNK) * KVF_MAX_JOBS >= (1ll << 31))
    return LSA_UNSUPPORTED;
  for (int t0 = 0; t0 < n_tensors; t0 += KVF_MAX_TENSORS) {
    const int nt = n_tensors - t0 < KVF_MAX_TENSORS ? n_tensors - t0 : KVF_MAX_TENSORS;
    int j = 0;
    while (j < n_jobs) {
      KvfArgs a = {};
      for (int t = 0; t < nt; ++t) a.tensors[t] = static_cast<unsigned short*>(const_cast<void*>(tensors[t0 + t]));
      a.n_jobs = 0;
      a.total = 0;
      a.nkv = nkv;
      a.head_elems = head_elems;
      a.slot_elems = head_elems * nkv;
      for (; j < n_jobs && a.n_jobs < KVF_MAX_JOBS; ++j) {
        const int* q = jobs + (size_t)j * KVF_JOB_INTS;
        if (q[1] == 0) continue;
        KvfJob& o = a.jobs[a.n_jobs++];
        o.first = a.total;
        o.vps = (unsigned)((long long)q[1] * hd / 8);
        o.cps = (o.vps + KVF_CHUNK - 1) / KVF_CHUNK;
        o.src = q[0];
        o.nd = q[2];
        for (int d = 0; d < KVF_MAX_DST; ++d) o.dst[d] = d < q[2] ? q[3 + d] : 0;
        a.total += (unsigned)nt * (unsigned)nkv * o.cps;
      }
      if (a.n_jobs == 0) continue;
      launch(a, flags, stream);
      LSA_CHECK_LAUNCH();
      ++g_kv_fork_calls;
    }
  }
  return LSA_OK;
}

extern "C" long long lsa_kv_fork_calls() { return g_kv_fork_calls; }
