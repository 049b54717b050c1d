"""GPU: scripts/train.py under OPTIM.OPTIMIZER adam - the fused cross-entropy path and the self-critical path resume bit for bit,
an SGD checkpoint is refused by name (and accepted with --reset-optimizer), a torch.optim.Adam checkpoint of the autograd path
continues on the fused path and back; two data-parallel ranks keep bit-identical parameters and moments through three Adam steps."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import oracle
from test_scripts_gpu import YAML
from test_scst_gpu import YAML as SCST_YAML

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "scripts", "train.py")
ADAM = ["OPTIM.OPTIMIZER", "adam", "OPTIM.LR", "0.001"]


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def run(args, expect_ok=True):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if expect_ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def base(cfg, every):
    return [TRAIN, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "32", "--vocab-size", "150", "--num-boxes", "5",
            "--eps-source", "cpu", "--zero-eps", "--checkpoint-every", str(every)]


def load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def assert_same_checkpoint(want, got, iteration):
    assert set(want) == {"model", "optimizer"} == set(got) and got["optimizer"]["iteration"] == iteration
    for k, v in want["model"].items():
        assert torch.equal(bits(got["model"][k]), bits(v)), k
    assert sorted(want["optimizer"]["state"]) == sorted(got["optimizer"]["state"])
    for i, st in want["optimizer"]["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        for k in st:
            assert torch.equal(bits(got["optimizer"]["state"][i][k]), bits(st[k])), (i, k)


def test_fused_adam_six_iterations_equal_three_plus_resume(tmp_path):
    """Iterations 1-4 of the toy schedule train the decoder LSTM on every second one: its step count lags, and the resumed run
    must carry both counts."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    ref, a, b = tmp_path / "ref", tmp_path / "a", tmp_path / "b"
    common = base(cfg, 3) + ["--fused-optimizer"]
    run(common + ["--serialization-dir", str(ref), "--config-override"] + ADAM)
    run(common + ["--serialization-dir", str(a), "--stop-after", "3", "--config-override"] + ADAM)
    run(common + ["--serialization-dir", str(b), "--start-from-checkpoint", str(a / "checkpoint_3.pth"), "--config-override"] + ADAM)
    want, got = load(ref / "checkpoint_6.pth"), load(b / "checkpoint_6.pth")
    assert_same_checkpoint(want, got, 6)
    steps = sorted({float(st["step"]) for st in got["optimizer"]["state"].values()})
    assert steps == [4.0, 6.0], steps                       # decoder LSTM: iterations 2, 4, 5, 6
    grp = got["optimizer"]["param_groups"][0]
    assert tuple(grp["betas"]) == (0.9, 0.999) and grp["eps"] == 1e-8 and grp["amsgrad"] is False
    log = [json.loads(x) for x in open(b / "scalars.jsonl")]
    assert log[0]["iteration"] == 4 and abs(log[0]["4learning_rate"] - 0.001 * (1 - 3 / 6)) < 1e-12


def test_self_critical_adam_resumes_bit_for_bit(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(SCST_YAML)
    common = [TRAIN, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "16", "--vocab-size", "60", "--num-boxes", "5",
              "--checkpoint-every", "1", "--scst-references", "synthetic", "--scst-samples", "4", "--scst-max-steps", "8",
              "--scst-sampler", "top-k", "--scst-top-k", "20"]
    over = ["--config-override", "OPTIM.OPTIMIZER", "adamw", "OPTIM.LR", "5e-5"]
    a, b = tmp_path / "a", tmp_path / "b"
    run(common + ["--serialization-dir", str(a)] + over)
    run(common + ["--serialization-dir", str(b), "--start-from-checkpoint", str(a / "checkpoint_2.pth")] + over)
    want, got = load(a / "checkpoint_3.pth"), load(b / "checkpoint_3.pth")
    assert_same_checkpoint(want, got, 3)
    assert got["optimizer"]["param_groups"][0]["decoupled_weight_decay"] is True
    first = load(a / "checkpoint_1.pth")
    assert any(not torch.equal(first["model"][k], v) for k, v in want["model"].items())      # (the steps moved the parameters)


def test_sgd_checkpoint_under_adam_is_refused_unless_reset(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    common = base(cfg, 1) + ["--fused-optimizer"]
    run(common + ["--serialization-dir", str(a), "--stop-after", "1"])
    ckpt = str(a / "checkpoint_1.pth")
    assert "momentum_buffer" in load(ckpt)["optimizer"]["state"][0]
    r = run(common + ["--serialization-dir", str(b), "--start-from-checkpoint", ckpt, "--stop-after", "2", "--config-override"] + ADAM,
            expect_ok=False)
    assert r.returncode != 0 and "'sgd'" in r.stderr and "'adam'" in r.stderr and "--reset-optimizer" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(b / "checkpoint_2.pth")
    run(common + ["--serialization-dir", str(c), "--start-from-checkpoint", ckpt, "--reset-optimizer", "--stop-after", "1",
                  "--config-override"] + ADAM)
    log = [json.loads(x) for x in open(c / "scalars.jsonl")]
    assert log[0]["iteration"] == 1
    got = load(c / "checkpoint_1.pth")
    assert got["optimizer"]["iteration"] == 1 and "exp_avg" in got["optimizer"]["state"][0]
    assert float(got["optimizer"]["state"][0]["step"]) == 1.0


def test_autograd_adam_checkpoint_resumes_on_the_fused_path(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    a, b = tmp_path / "a", tmp_path / "b"
    run(base(cfg, 3) + ["--serialization-dir", str(a), "--stop-after", "3", "--config-override"] + ADAM)
    first = load(a / "checkpoint_3.pth")
    assert sorted({float(st["step"]) for st in first["optimizer"]["state"].values()}) == [1.0, 3.0]     # torch.optim.Adam's own counts
    run(base(cfg, 1) + ["--fused-optimizer", "--serialization-dir", str(b), "--start-from-checkpoint", str(a / "checkpoint_3.pth"),
                        "--stop-after", "4", "--config-override"] + ADAM)
    got = load(b / "checkpoint_4.pth")
    assert got["optimizer"]["iteration"] == 4
    assert sorted({float(st["step"]) for st in got["optimizer"]["state"].values()}) == [2.0, 4.0]       # carried over, one more each
    for i, st in first["optimizer"]["state"].items():
        assert float(got["optimizer"]["state"][i]["step"]) == float(st["step"]) + 1
        assert not torch.equal(got["optimizer"]["state"][i]["exp_avg"], st["exp_avg"].cpu())
    # ... and the other way round: the fused path's checkpoint continues under torch.optim.Adam
    c = tmp_path / "c"
    run(base(cfg, 1) + ["--serialization-dir", str(c), "--start-from-checkpoint", str(b / "checkpoint_4.pth"), "--stop-after", "5",
                        "--config-override"] + ADAM)
    back = load(c / "checkpoint_5.pth")
    assert back["optimizer"]["iteration"] == 5
    assert sorted({float(st["step"]) for st in back["optimizer"]["state"].values()}) == [3.0, 5.0]


# ---- data parallel ------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    from gpuutil import engine_from
    from ssc_runtime.engine import OptimSpec
    from test_dp_gpu import CFG, _inputs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = oracle.OracleConfig(**CFG)
    eng = engine_from(cfg, oracle.init_params(cfg, seed=4))
    feats, caps, senti, eps = _inputs()
    per = feats.size(0) // world
    sl = slice(rank * per, (rank + 1) * per)
    spec = OptimSpec("adam")
    start = eng.params.flat.clone()
    for frozen in (True, False, False):
        eng.train_step(feats[sl].cuda(), caps[sl].cuda(), senti[sl].cuda(), eps[:, sl].cuda().contiguous(), lr=1e-3, weight_decay=0.001,
                       max_norm=0.7, decoder_frozen=frozen, optim=spec)
    torch.cuda.synchronize()
    mine = torch.stack([eng.params.flat, eng.exp_avg, eng.exp_avg_sq]).cpu()
    both = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    if rank == 0:
        same = all(torch.equal(both[0].view(torch.int32), x.view(torch.int32)) for x in both[1:])
        ret.put({"same": same, "moved": not torch.equal(start.cpu(), mine[0]), "steps": list(eng.adam_steps),
                 "moments": bool(mine[1].abs().sum() > 0) and bool(mine[2].sum() > 0)})
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_identical_parameters_and_moments():
    from test_dp_gpu import _join_then_get
    ctx = mp.get_context("spawn")
    ret = ctx.SimpleQueue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    got = _join_then_get(procs, ret)
    assert got == {"same": True, "moved": True, "steps": [3, 2], "moments": True}, got
