"""GPU: bench.py --dump-outputs writes what the last timed train step computed, from inputs that are the same on every run
with the same arguments, and the result line carries the timed step count and ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(out_dir, steps, flags=("--timed-only", "--prewarm", "0")):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        *flags, "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return res, {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_dump_outputs_of_the_timed_train_step(tmp_path):
    res, a = bench(tmp_path / "a", 3)
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert sorted(a) == ["grads_sample", "kld", "loss", "params_sample"]
    assert a["loss"].shape == a["kld"].shape == (64,)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # the same arguments again: the same inputs and a train step without order-dependent sums, so the same outputs bit for bit
    _, b = bench(tmp_path / "b", 3)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # one timed step more is a different last step
    _, c = bench(tmp_path / "c", 4)
    assert not np.allclose(a["loss"], c["loss"], rtol=1e-4, atol=1e-6)


FULL_ONLY = ("roofline", "roofline_step", "attention_roofline", "decode", "decode_tokens_per_s", "decode_cbs", "exact_fp32_mode",
             "c5_train", "cpu_baseline")


def test_plain_run_times_what_the_full_run_times(tmp_path):
    """A plain run leaves every other leg to --full; the decode legs that --full runs before the train steps change nothing the
    timed steps compute, so both runs dump the same arrays bit for bit."""
    plain, a = bench(tmp_path / "plain", 2, flags=())
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["metric"] == "captions/sec (train step)" and plain["unit"] == "captions/s" and plain["dtype"] == "f32"
    assert plain["higher_is_better"] is True and plain["steps"] == 2 and plain["value"] > 0
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    full, b = bench(tmp_path / "full", 2, flags=("--full", "--no-cpu-baseline"))
    assert all(k in full for k in FULL_ONLY if k != "cpu_baseline"), sorted(full)
    assert full["decode"]["value"] > 0 and full["roofline"]["achieved"] > 0
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
