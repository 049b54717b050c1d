"""GPU: scripts/train.py with OPTIM.UNLIKELIHOOD_ALPHA - the fused path logs `ul` beside `nll`, records the key in config.yml and
resumes from a checkpoint into the uninterrupted run's log line; the autograd path carries the term too; the self-critical steps
ignore it with a notice."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["--config-override", "OPTIM.UNLIKELIHOOD_ALPHA", "0.5"]


def _train(tmp_path, name, extra, fused=True, stop=2):
    from test_scripts_gpu import YAML
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / name
    args = [os.path.join(ROOT, "scripts", "train.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150",
            "--num-boxes", "5", "--zero-eps", "--serialization-dir", str(out), "--stop-after", str(stop), "--checkpoint-every", "1"] + (
                ["--fused-optimizer"] if fused else []) + extra
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out, r


def read(d):
    return [json.loads(x) for x in open(d / "scalars.jsonl")]


def test_train_script_logs_ul_records_the_key_and_resumes(tmp_path):
    out, _ = _train(tmp_path, "ul", KEYS)
    log = read(out)
    assert [rec["iteration"] for rec in log] == [1, 2]
    for rec in log:
        assert math.isfinite(rec["ul"]) and rec["ul"] > 0 and math.isfinite(rec["nll"]) and rec["nll"] > 0
        assert abs(rec["1reconstr_loss"] - (rec["nll"] + 0.5 * rec["ul"])) <= 1e-4 * max(1.0, rec["nll"])     # loss = nll + alpha * ul
    assert "UNLIKELIHOOD_ALPHA: 0.5" in open(out / "config.yml").read()
    # the checkpoint resumes: the log line of iteration 2 again
    res, _ = _train(tmp_path, "resumed", KEYS + ["--start-from-checkpoint", str(out / "checkpoint_1.pth")])
    strip = lambda rec: {k: v for k, v in rec.items() if k != "elapsed_s"}
    assert [strip(rec) for rec in read(res)] == [strip(rec) for rec in log[1:]]
    # a run without the key logs what it logged, and another loss
    plain, _ = _train(tmp_path, "plain", [], stop=1)
    p = read(plain)[0]
    assert "ul" not in p and "nll" not in p and abs(p["1reconstr_loss"] - log[0]["nll"]) <= 1e-4 * max(1.0, log[0]["nll"])
    assert "UNLIKELIHOOD_ALPHA: 0.0" in open(plain / "config.yml").read()


def test_autograd_path_carries_the_term(tmp_path):
    fused, _ = _train(tmp_path, "fused", KEYS, stop=1)
    auto, _ = _train(tmp_path, "autograd", KEYS, fused=False, stop=1)
    a, f = read(auto)[0], read(fused)[0]
    assert a["ul"] > 0 and abs(a["ul"] - f["ul"]) <= 1e-3 * max(1.0, abs(f["ul"])) and abs(a["3loss"] - f["3loss"]) < 1e-3


def test_self_critical_steps_ignore_the_key_with_a_notice(tmp_path):
    out, r = _train(tmp_path, "scst", KEYS + ["--scst-references", "synthetic", "--scst-samples", "2", "--scst-max-steps", "8"], stop=1)
    assert "OPTIM.UNLIKELIHOOD_ALPHA 0.5 is ignored by the self-critical steps" in r.stdout
    assert "ul" not in read(out)[0]
