"""The mxfp4 GEMM's torch statements and chooser (ops/mx4.py), no GPU."""
import pytest
import torch

from llm_sharding_amd.ops import hip, mx4

LLAMA7B = ((6144, 4096), (4096, 4096), (22016, 4096), (4096, 11008))


@pytest.mark.parametrize("M,K", [(1, 128), (17, 640), (33, 1152)])
def test_pack_a_mx8_is_quantize_act_mx8_element_by_element(M, K):
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 3).to(torch.bfloat16)
    x[0, :32] = 0
    codes, e = mx4.quantize_act_mx8(x)
    a8, ea = mx4.pack_a_mx8(x)
    rb, ks, ng = -(-M // 16), K // 128, mx4.scale_groups(K)
    assert (a8.numel(), ea.numel()) == mx4.a_image_bytes(M, K) == (rb * 16 * K, rb * ng * 256)
    a8, ea = a8.view(rb, ks, 2, 4, 16, 16), ea.view(rb, ng, 4, 16, 4)  # [half][lane group][row][byte]; [block][row][step]
    for m in range(rb * 16):
        for k in range(0, K, 7):
            st, kk = divmod(k, 128)
            assert int(a8[m // 16, st, kk // 64, (kk % 64) // 16, m % 16, kk % 16]) == (int(codes[m, k]) if m < M else 0)
            assert int(ea[m // 16, st // 4, kk // 32, m % 16, st % 4]) == (int(e[m, k // 32]) if m < M else 127)
    assert bool((ea[:, -1, :, :, ks - 4 * (ng - 1):] == 127).all())  # K-steps past K in the last group


def test_gemm_config_rule_and_switch(monkeypatch):
    for M in (1, 129, 256, 512, 2048):
        for N, K in LLAMA7B + ((256, 128), (512, 384)):
            cands = mx4.mx4_gemm_candidates(M, N, K, hip.EPI_RESID)
            assert cands and mx4.mx4_gemm_config(M, N, K, hip.EPI_RESID) in cands
            for bn, sk in cands:
                assert (bn, 4) in mx4.MX4_GEMM_CONFIGS and N % bn == 0 and 1 <= sk <= mx4.scale_groups(K)
                assert mx4.mx4_gemm_slab_floats(M, N, sk) == (0 if sk == 1 else sk * -(-M // 128) * 128 * N)
    assert mx4.mx4_gemm_candidates(129, 192, 384) == [] and mx4.mx4_gemm_candidates(129, 256, 320) == []
    assert mx4.mx4_gemm_candidates(129, 256, 384, hip.EPI_ARGMAX) == []
    assert mx4.mx4_gemm_config(512, 4096, 11008, slab_floats=0) == (128, 1)       # no room for partial tiles
    monkeypatch.delenv("LSA_MX4_GEMM", raising=False)                             # opt-in: off by default
    x = torch.zeros(129, 256, dtype=torch.bfloat16)
    assert not mx4.mx4_gemm_enabled() and not mx4.mx4_gemm_serves(LLAMA7B, 512)
    assert mx4.proj_gemm_mx4(x, x, x, 129, 256, 256, hip.EPI_STORE, None, a_scratch=x) is False
    monkeypatch.setenv("LSA_MX4_GEMM", "1")
    assert mx4.mx4_gemm_serves(LLAMA7B, 512) and not mx4.mx4_gemm_serves(((192, 384),), 129)
