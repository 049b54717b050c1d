"""GPU: prompted decoding through the module and the inference script - UpDownCaptioner.decode_prefix in the eval forward (the
beam search and a word sampler), scripts/inference.py --prefix / --prefix-json, and the flag combinations the script refuses before
it loads anything."""
import json
import os
import subprocess
import sys

import pytest
import torch

from ssc_runtime import sampling
from ssc_runtime.prefix import DecodePrefix
from ssc_runtime.vocab import Vocabulary
from var_updown.models import UpDownCaptioner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "inference.py")
YAML = ("RANDOM_SEED: 2\nDATA:\n  MAX_CAPTION_LENGTH: 6\n  CBS:\n    MAX_GIVEN_CONSTRAINTS: 0\nMODEL:\n"
        "  IMAGE_FEATURE_SIZE: 64\n  EMBEDDING_SIZE: 40\n  HIDDEN_SIZE: 48\n  ATTENTION_PROJECTION_SIZE: 32\n"
        "  BEAM_SIZE: 3\n  MIN_CONSTRAINTS_TO_SATISFY: 0\n  Z_SPACE: 16\n  SENTIMENT_VAE: 1\n  SENTI_PRIOR_MULTIP: 0.5\n"
        "  SIMPLE_VAE: False\n  N_Z_SAMPLES: 2\n")


def captioner(sampler=None, V=120):
    torch.manual_seed(13)
    m = UpDownCaptioner(Vocabulary.synthetic(V), image_feature_size=64, embedding_size=40, hidden_size=48, attention_projection_size=24,
                        max_caption_length=6, beam_size=1 if sampler is not None else 3, z_space=8, prior_std=1.0, simple_vae=False, latent_embedding="glove",
                        sentiment_vae=1, senti_prior_multip=0.5, sampler=sampler, device=torch.device("cuda")).to("cuda")
    m.eval()
    m._engine()
    return m


@pytest.mark.parametrize("decoder", ["beam", "top-k"])
def test_decode_prefix_through_the_eval_forward(decoder):
    """decode_prefix on the eval forward, beam search and a word sampler: every returned caption starts with its prompt - one
    prompt for the whole batch, then one per image with mixed lengths and an image without one -, the output is Lp words wider, and
    clearing the prefix restores the unprefixed output bit for bit."""
    m = captioner(sampling.TopKSampler(k=4) if decoder == "top-k" else None)
    vocab = m._vocabulary
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(3, 5, 64, generator=g).cuda()
    senti = torch.tensor([[1.0], [0.0], [-1.0]]).cuda()

    def forward():
        torch.manual_seed(21)
        return m(feats, sentiment=senti)["predictions"]

    plain = forward()
    assert plain.shape[0] == 3 and plain.shape[1] <= 6
    m.decode_prefix(DecodePrefix.from_words(vocab, "w7 w9"))
    one = forward()
    assert one.shape[0] == 3 and one.shape[1] >= 3 and (one[:, :2].cpu() == torch.tensor([7, 9])).all()
    m.decode_prefix(DecodePrefix.from_words(vocab, ["w5 w6 w8", None, "w11"]))
    mixed = forward()
    assert mixed[0, :3].tolist() == [5, 6, 8] and mixed[2, 0].item() == 11
    m.decode_prefix(None)
    assert torch.equal(forward(), plain)
    with pytest.raises(ValueError, match="DecodePrefix"):
        m.decode_prefix("w7")
    with pytest.raises(ValueError, match="BOUNDARY|outside"):
        m.decode_prefix(DecodePrefix(torch.tensor([[5, 1]])))
    m.decode_prefix(DecodePrefix.from_words(vocab, "w7"))
    m.decode_attention("summary")
    with pytest.raises(NotImplementedError, match="attention"):
        forward()
    m.decode_attention(None)
    m.decode_prefix(DecodePrefix.from_words(vocab, ["w7", "w8"]))
    with pytest.raises(ValueError, match="2 rows"):
        forward()


def run_script(tmp_path, *extra):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    out = tmp_path / "pred.json"
    r = subprocess.run([sys.executable, SCRIPT, "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "4", "--vocab-size", "150",
                        "--num-boxes", "5", "--output-path", str(out)] + list(extra), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    return r, out


def test_inference_script_with_a_prefix(tmp_path):
    r, out = run_script(tmp_path, "--prefix", "w20 w30")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    caps = json.load(open(out))
    assert len(caps) == 4 * 2 and all(c["caption"].startswith("w20 w30") for c in caps)


def test_inference_script_with_a_prefix_per_image(tmp_path):
    """--prefix-json: prompts of one and three words share one call; image 2 has no entry and decodes without a prompt."""
    pj = tmp_path / "prefix.json"
    pj.write_text(json.dumps({"0": "w20", "1": "w21 w22 w23", "3": "w24 w25"}))
    r, out = run_script(tmp_path, "--prefix-json", str(pj), "--config-override", "MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", "5",
                        "MODEL.BEAM_SIZE", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    caps = json.load(open(out))
    assert len(caps) == 4 * 2
    starts = {0: "w20", 1: "w21 w22 w23", 3: "w24 w25"}
    for c in caps:
        if c["image_id"] in starts:
            assert c["caption"].startswith(starts[c["image_id"]]), c
    assert any(c["image_id"] == 2 for c in caps)


def test_inference_script_refuses_before_loading(tmp_path):
    """The three refused combinations exit non-zero from the argument checks, with the prefix flags' own message: none of the
    named files exists, and a run that got as far as the other flags' checks or as loading would fail on that instead.  The
    remaining refusals of the check are made in this process (the script's check_prefix_args on a namespace)."""
    pj = tmp_path / "prefix.json"
    pj.write_text(json.dumps({"0": "w20"}))
    for extra in (["--prefix", "w20", "--attention-output", str(tmp_path / "a.pt")],
                  ["--prefix-json", str(pj), "--exemplar-tensors", str(tmp_path / "none.pt")],
                  ["--prefix", "w20", "--checkpoint-path", str(tmp_path / "c0.pth"), "--ensemble-checkpoints", str(tmp_path / "c1.pth")]):
        r, out = run_script(tmp_path, *extra)
        assert r.returncode != 0 and "--prefix / --prefix-json is not available with " + extra[-2] in r.stderr, (extra, r.stderr[-1500:])
        assert not os.path.exists(out)
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("inference_script", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns = lambda **kw: argparse.Namespace(**dict(dict(prefix="", prefix_json="", ensemble_checkpoints=None, exemplar_tensors="",
                                                     attention_output=""), **kw))
    assert mod.check_prefix_args(ns()) is None and mod.check_prefix_args(ns(prefix="w20 w30")) is None
    assert mod.check_prefix_args(ns(prefix_json=str(pj))) == {0: "w20"}
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"zero": "w20"}))
    for kw, msg in ((dict(prefix="w20", prefix_json=str(pj)), "exclude each other"), (dict(prefix="   "), "at least one word"),
                    (dict(prefix_json=str(tmp_path / "missing.json")), "no such file"), (dict(prefix_json=str(bad)), "image ids")):
        with pytest.raises(SystemExit, match=msg):
            mod.check_prefix_args(ns(**kw))
