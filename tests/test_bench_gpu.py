"""bench.py on one MI355X: the JSON line's placement block ("dist") names the device the rank
really ran on - its PCI address / UUID from the HIP runtime - so the same keys on an 8-GPU run
prove 8 distinct GPUs. A short run of a 2-layer cut of the 7B (stage profile)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_names_the_device(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "16",
                        "--prompt-len", "8", "--stage-layers", "2", "--latency-steps", "0", "--mid-batch", "0",
                        "--ttft-lens", "", "--extras", "", "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    # --dump-outputs: the last timed step's ids and final hidden state of the 16 sequences
    import numpy as np
    tok, hid = np.load(tmp_path / "tokens_last_step.npy"), np.load(tmp_path / "hidden_last_step.npy")
    assert tok.shape == (1, 16) and tok.dtype == np.float64 and ((tok >= 0) & (tok < 32000)).all()
    assert hid.shape == (1, 16, 4096) and hid.dtype == np.float32 and np.isfinite(hid).all() and np.abs(hid).max() > 0
    assert np.load(tmp_path / "tokens_mb0.npy").shape == (16, 3)
    assert line["ms_per_step"] > 0 and line["steps"] == 2 and line["b1_p50_tpot_ms"] is None and "extra" not in line
    d = line["dist"]
    assert d["world_size"] == 1 and len(d["ranks"]) == 1 and d["edges"] == {}
    rk = d["ranks"][0]
    import torch
    p = torch.cuda.get_device_properties(0)
    print(f"[bench-gpu] rank 0 on {rk}, torch reports uuid={p.uuid} pci={p.pci_domain_id}:{p.pci_bus_id}:{p.pci_device_id}")
    assert rk["device_index"] == 0
    assert rk["pci_bus_id"] and rk["pci_bus_id"] != "0000:00:00" or str(rk["uuid"]).strip("0-"), rk
    assert d["distinct_devices"] is True
