#!/usr/bin/env python3
"""Where a gemm_skp launch spends its time: the per-workgroup s_memrealtime stamps (100 MHz) of
scripts/gemm_stamps.py, from the diagnostic build of csrc/gemm_skp/gemm_skp.hip
(-DLSA_GEMM_STAMPS -> _native/liblsa_gemm_skp_stamps.so, built by `--build` on the CPU host).

Stamps per workgroup: 0 segment start, 1 prologue DMA landed, 2 main loop done, 3 every band
stored and every ticket drawn, 5 the bands this workgroup reduced are written (kernel end).
usage: gemm_skp_stamps.py M N K bm bn contributors tile_major [reps] | --build"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "llm_sharding_amd", "_native", "liblsa_gemm_skp_stamps.so")


def build():
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-DLSA_GEMM_STAMPS",
           "-fno-slp-vectorize", os.path.join(ROOT, "csrc", "gemm_skp", "gemm_skp.hip"), "-o", SO]
    subprocess.check_call(cmd)
    print("built", SO)


def main():
    if sys.argv[1] == "--build":
        build()
        return
    import torch
    sys.path.insert(0, ROOT)
    from llm_sharding_amd.ops import gemm_skp, hip, packing
    M, N, K, bm, bn, C, tm = (int(v) for v in sys.argv[1:8])
    reps = int(sys.argv[8]) if len(sys.argv) > 8 else 5
    L = ctypes.CDLL(SO)
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.lsa_gemm_skp.argtypes = [vp, i, vp, i, i, i, i, ctypes.POINTER(hip.EpiArgs), i, i, i, i, i, i, vp, vp,
                               ctypes.c_longlong, i, vp]
    grid = gemm_skp.tiles(M, N, bm, bn) * C
    nbuf = max(2, (600 << 20) // (N * K * 2) + 1)
    wps = [packing.pack_b(torch.randn(N, K, device="cuda").mul_(0.02).to(torch.bfloat16)) for _ in range(nbuf)]
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    ep = hip.make_epi(out=out, ldo=N)
    ws = hip.SkWorkspace("cuda", grid=max(256, grid), bn=256)
    st = torch.zeros(max(256, grid) * 32, dtype=torch.int64, device="cuda")
    L.lsa_gemm_skp_set_stamps(ctypes.c_void_p(st.data_ptr()))
    for r in range(reps):
        st.zero_()
        rc = L.lsa_gemm_skp(ctypes.c_void_p(x.data_ptr()), x.stride(0), ctypes.c_void_p(wps[r % nbuf].data_ptr()), M, N, K,
                            hip.EPI_STORE, ctypes.byref(ep), bm, bn, 0, C, tm, 8, ctypes.c_void_p(ws.slab.data_ptr()),
                            ctypes.c_void_p(ws.counters.data_ptr()), ws.slab.numel(), ws.counters.numel(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
    s = st.view(-1, 32).cpu().double()
    s = s[s[:, 0] > 0]
    us = (s - s[:, 0].min()) / 100.0  # 100 MHz -> us
    print(f"config M={M} N={N} K={K} bm={bm} bn={bn} contributors={C} tile_major={tm}: {s.shape[0]} workgroups, "
          f"kernel span {float(us[:, 5].max()):.2f} us")
    for name, col in (("seg_start", 0), ("prologue", 1), ("loop_end", 2), ("tickets", 3), ("end", 5)):
        c = us[:, col]
        print(f"  {name:9s} median {float(c.median()):7.2f}  max {float(c.max()):7.2f}")


if __name__ == "__main__":
    main()
