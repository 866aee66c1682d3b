"""bench.py's plain one-GPU run at a small size: setup, warmup, the timed
steps, the JSON line -- and nothing of what --full adds (no CPU baseline, no
serial-schedule roofline, no MSM / NTT lines, no anchor, no details file).
--dump-outputs writes the last timed step's proof as .npy arrays that equal
the line's own proof, and equal from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("serial_schedule", "pcie_inclusive", "msm_g1", "ntt", "strong_scaling_anchor", "bit_exact_vs_oracle")


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--log-n", "10", "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.timeout(240)
def test_plain_run_line_and_dumped_proof(zkp, tmp_path):
    rec = _run(tmp_path / "a", 3)
    import bench
    assert rec["metric"] == bench.METRIC and rec["unit"] == "constraints/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "u32" and rec["n_gpus"] == 1 and rec["steps"] == 3
    assert rec["ms_per_step"] > 0
    # ms_per_step is rounded to 1 us in the line: 1 % covers a 0.05-ms step
    assert rec["value"] == pytest.approx((1 << 10) / (rec["ms_per_step"] / 1e3), rel=1e-2)
    for k in FULL_ONLY:
        assert k not in rec, k
    assert rec["cpu_baseline"] is None and rec["roofline"] is None and rec["details"] is None
    # the dumped arrays are the proof the line reports
    words = np.load(tmp_path / "a" / "proof_words.npy")
    comp = np.load(tmp_path / "a" / "proof_compressed.npy")
    assert words.dtype == np.float64 and words.shape == (2 * (2 * zkp.G1_WORDS + zkp.G2_WORDS),)
    assert comp.dtype == np.float32 and comp.shape == (192,)
    assert bytes(comp.astype(np.uint8)).hex() == rec["proof_compressed"]
    proof = zkp.Proof(words.astype("<u4").view("<u8"))
    assert proof.serialize_compressed().hex() == rec["proof_compressed"]
    # the same arguments give the same inputs, so the same outputs
    rec2 = _run(tmp_path / "b", 3)
    assert np.array_equal(np.load(tmp_path / "b" / "proof_words.npy"), words)
    assert rec2["proof_compressed"] == rec["proof_compressed"]
