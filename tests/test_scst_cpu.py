"""CPU: the definition of the self-critical step's glue (tests/scstref.py) on hand-made cases, the argument checks of
ssc_scst_prepare that need no GPU, the seed derivation, and the new flags of scripts/train.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import scstref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_leave_one_out_advantages_of_an_image_sum_to_zero():
    g = np.random.default_rng(3)
    for P, N in ((1, 2), (3, 5), (4, 64), (2, 128)):
        s = g.random((P, N, 6))
        s[..., 5] *= 10
        out = R.advantage(s, None, (0, 0, 0, 0.5, 0.25, 1), 1, 1.0 / (P * N), 1e-5)
        r = out["reward64"]
        # each b_i carries a few ulps of the image's sum: N of them add to at most N * 4 ulp(sum |r|)
        assert (np.abs(out["advantage64"].sum(1)) <= 4 * N * np.finfo(np.float64).eps * np.abs(r).sum(1)).all()
        assert np.abs(out["stats"][0] - out["stats"][1]) <= 1e-12 * out["stats"][0]      # mean baseline = mean reward
        assert out["gk"].dtype == np.float32 and (out["gk"] == np.float32(1e-5)).all()


def test_two_equal_rewards_give_advantage_zero():
    s = np.zeros((2, 2, 6))
    s[0, :, :] = [0.7, 0.5, 0.3, 0.1, 0.61, 1.2345678901234]
    s[1, 0, 5], s[1, 1, 5] = 0.3, 0.9
    out = R.advantage(s, None, (0.1, 0.2, 0.3, 0.4, 0.5, 1.0), 1, 0.25, 1e-3)
    assert (out["advantage"][:2] == 0).all() and (out["gl"][:2] == 0).all()
    a0, a1 = out["advantage64"][1]
    assert abs(a0 + a1) < 1e-15 and a0 == pytest.approx(-0.6, abs=1e-15)
    # an image without references scores 0 everywhere: reward 0, advantage 0
    z = R.advantage(np.zeros((1, 5, 6)), None, (0, 0, 0, 0, 0, 1), 1, 0.2, 1e-3)
    assert (z["reward"] == 0).all() and (z["advantage"] == 0).all() and (z["stats"][:3] == 0).all()


def test_baselines_none_and_given():
    s = np.zeros((2, 3, 6))
    s[..., 5] = [[1, 2, 3], [4, 5, 6]]
    base = np.zeros((2, 6))
    base[:, 5] = [2, 10]
    w = (0, 0, 0, 0, 0, 1)
    assert R.advantage(s, None, w, 0, 1.0, 0.0)["advantage"].tolist() == [1, 2, 3, 4, 5, 6]
    out = R.advantage(s, base, w, 2, 0.5, 0.0)
    assert out["advantage"].tolist() == [-1, 0, 1, -6, -5, -4] and out["gl"].tolist() == [-0.5, 0, 0.5, -3, -2.5, -2]
    assert out["stats"][:3].tolist() == [3.5, 6.0, 17 / 6]


def test_pack_edge_cases():
    end = 1
    pred = np.array([[1, 5, 6, 7],      # an end in column 0: the empty caption
                     [5, 6, 7, 8],      # no end: every token kept
                     [5, 6, 7, 1],      # an end in the last column
                     [5, 0, 7, 1],      # id 0 inside a caption is passed on
                     [5, 1, 7, 1]])     # cut at the FIRST end
    caps, lengths = R.pack(pred, end, 6)
    assert lengths.tolist() == [0, 4, 3, 3, 1]
    assert caps.tolist() == [[0] * 6, [5, 6, 7, 8, 0, 0], [5, 6, 7, 0, 0, 0], [5, 0, 7, 0, 0, 0], [5, 0, 0, 0, 0, 0]]
    caps4, _ = R.pack(pred, end, 4)
    assert (caps4 == caps[:, :4]).all()
    out = R.advantage(np.zeros((1, 5, 6)), None, (0,) * 6, 0, 1.0, 1.0, lengths, 4)
    assert out["stats"][3] == 0.2                                             # one row of five has no end
    with pytest.raises(AssertionError):
        R.pack(pred, end, 3)


def test_prepare_rejects_bad_arguments_without_a_gpu():
    from ssc_runtime import lib as L
    lib = L.load()
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_scst_prepare(None, None)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value

    def desc(**kw):
        d = L.ScstDesc()
        d.P, d.N, d.steps, d.L, d.end_index, d.baseline = 1, 2, 4, 4, 1, 1
        for f in ("predictions", "scores", "base_scores", "caps", "lengths", "reward", "advantage", "gl", "gk", "stats"):
            setattr(d, f, p)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    # (a valid descriptor is not tried here: it would launch)
    for bad in (dict(L=3), dict(N=0), dict(N=129), dict(P=0), dict(steps=0), dict(baseline=3), dict(baseline=1, N=1),
                dict(baseline=2, base_scores=None), dict(caps=None), dict(stats=None), dict(end_index=-1)):
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_scst_prepare(C.byref(desc(**bad)), None)


def test_seed_is_a_function_of_seed_iteration_and_rank():
    from ssc_runtime.scst import parse_reward_weights, scst_seed
    seen = {scst_seed(s, i, r) for s in (0, 1, 2) for i in range(1, 50) for r in range(8)}
    assert len(seen) == 3 * 49 * 8 and all(0 <= v < 2 ** 62 for v in seen)
    assert scst_seed(7, 123, 3) == scst_seed(7, 123, 3)
    assert parse_reward_weights("0,0,0,0.5,0,1") == (0.0, 0.0, 0.0, 0.5, 0.0, 1.0)
    with pytest.raises(ValueError):
        parse_reward_weights("1,2,3")


def _train_script(monkeypatch):
    """scripts/train.py as a module; what importing it leaves in the process (its sys.path entry, the environment default it sets
    for its own multi-GPU runs) is undone after the test."""
    import sys
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    spec = importlib.util.spec_from_file_location("ssc_train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the namespace scripts/train.py built from `--config c --gpu-ids 0` before the self-critical flags were added
OLD_DEFAULTS = {
    "config": "c", "config_override": [], "gpu_ids": [0], "cpu_workers": 0, "in_memory": False, "skip_validation": False,
    "val_tensors": "", "val_every": 1000, "val_samples": 1, "val_images": 0, "serialization_dir": "checkpoints/experiment",
    "checkpoint_every": 10000, "start_from_checkpoint": "", "train_tensors": "", "synthetic": 0, "vocab_size": 10000, "num_boxes": 36,
    "eps_source": "device", "zero_eps": False, "stop_after": 0, "attribute_table": "", "fused_optimizer": False,
}


def test_train_script_flags(monkeypatch):
    from ssc_runtime import sampling
    t = _train_script(monkeypatch)
    a = vars(t.parser.parse_args(["--config", "c", "--gpu-ids", "0"]))
    assert {k: a[k] for k in OLD_DEFAULTS} == OLD_DEFAULTS
    new = {k: v for k, v in a.items() if k not in OLD_DEFAULTS}
    assert new == {"scst_references": "", "scst_samples": 5, "scst_baseline": "loo", "scst_sampler": "multinomial",
                   "scst_temperature": 1.0, "scst_top_k": 40, "scst_top_p": 0.9, "scst_reward": "0,0,0,0,0,1", "scst_max_steps": 20}
    a = t.parser.parse_args(["--config", "c", "--gpu-ids", "0", "--scst-references", "r.json", "--scst-samples", "7", "--scst-baseline",
                             "greedy", "--scst-sampler", "top-p", "--scst-top-p", "0.8", "--scst-temperature", "0.7", "--scst-reward",
                             "0,0,0,0.5,0,1", "--scst-max-steps", "16"])
    assert (a.scst_references, a.scst_samples, a.scst_baseline, a.scst_max_steps) == ("r.json", 7, "greedy", 16)
    s = t.scst_sampler(a)
    assert isinstance(s, sampling.TopPSampler) and s.temperature == pytest.approx(0.7)
    a = t.parser.parse_args(["--config", "c", "--gpu-ids", "0", "--scst-sampler", "top-k", "--scst-top-k", "3"])
    assert isinstance(t.scst_sampler(a), sampling.TopKSampler)
    assert isinstance(t.scst_sampler(t.parser.parse_args(["--config", "c", "--gpu-ids", "0"])), sampling.MultinomialSampler)
    with pytest.raises(SystemExit):
        t.parser.parse_args(["--config", "c", "--gpu-ids", "0", "--scst-baseline", "critic"])
