"""CPU: prompted decoding without a GPU - DecodePrefix parsing and its refusals, the NumPy restatement of the join, and the
self-consistency of the reference itself (tests/prefixref.py): a beam-1 oracle search's own first words, used as the prefix of a
second search with the noise re-aligned, reproduce the rest of that caption."""
import numpy as np
import pytest
import torch

import oracle
import prefixref as PR
from ssc_runtime.prefix import DecodePrefix
from ssc_runtime.vocab import Vocabulary


def test_decode_prefix_parsing_and_refusals():
    vocab = Vocabulary(["@@UNKNOWN@@", "@@BOUNDARY@@", "a", "happy", "two", "dogs", "sad"])
    one = DecodePrefix.from_words(vocab, "a happy")
    assert one.ids.tolist() == [[2, 3]] and one.ids.dtype == torch.int64 and (one.n, one.Lp) == (1, 2)
    assert DecodePrefix.from_words(vocab, "a happy", n=3).ids.tolist() == [[2, 3]] * 3
    mixed = DecodePrefix.from_words(vocab, ["two dogs a", None, ["sad"], ""])
    assert mixed.ids.tolist() == [[4, 5, 2], [-1, -1, -1], [6, -1, -1], [-1, -1, -1]] and not mixed.empty
    assert DecodePrefix.from_words(vocab, [None, ""]).ids.tolist() == [[-1], [-1]]
    assert DecodePrefix.from_words(vocab, [None, ""]).empty
    assert mixed.expand(2).ids.tolist() == [r for r in mixed.ids.tolist() for _ in range(2)]
    assert mixed.expand(1) is mixed
    with pytest.raises(ValueError, match="not in the vocabulary"):
        DecodePrefix.from_words(vocab, "a cat")
    with pytest.raises(ValueError, match="@@BOUNDARY@@"):
        DecodePrefix.from_words(vocab, "a @@BOUNDARY@@")
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        DecodePrefix.from_words(vocab, "a sad", vocab_size=6)
    with pytest.raises(ValueError, match="2 prompts for 3 images"):
        DecodePrefix.from_words(vocab, ["a", "sad"], n=3)
    with pytest.raises(ValueError):
        mixed.expand(0)
    for bad in (torch.zeros(3), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 2)):
        with pytest.raises(ValueError):
            DecodePrefix(bad)


def test_prefix_lengths_end_at_the_first_id_that_is_no_word():
    p = [[5, 6, 7], [-1, 5, 6], [5, -1, 6], [5, 90, 6], [5, 1, 6], [5, 6, 89], [0, 0, 0]]
    assert PR.prefix_lengths(p, 90, 1).tolist() == [3, 0, 1, 1, 1, 3, 3]


def test_join_restatement():
    end = 1
    prefix = np.array([[5, 6, 7], [-1, -1, -1], [8, -1, -1]])
    lengths = np.array([3, 0, 1])
    pred = np.arange(3 * 2 * 4).reshape(3, 2, 4) + 10
    lps = np.array([[-1.5, -np.inf], [-2.0, -1e20], [-0.25, -3.0]], dtype=np.float32)
    plp = np.array([-4.0, 0.0, -0.5], dtype=np.float32)
    caps, total = PR.join(prefix, lengths, pred, None, lps, plp, end)
    assert caps.shape == (3, 2, 7)
    assert caps[0, 1].tolist() == [5, 6, 7, 14, 15, 16, 17]
    assert caps[1, 0].tolist() == [18, 19, 20, 21, 1, 1, 1]
    assert caps[2, 1].tolist() == [8, 30, 31, 32, 33, 1, 1]
    assert total.dtype == np.float32
    assert total.tolist() == [[-5.5, -np.inf], [-2.0, np.float32(-1e20)], [-0.75, -3.5]]
    # an early-stopped call: the columns from ctl[0] on are END whatever the block holds
    caps2, _ = PR.join(prefix, lengths, pred, 2, lps, plp, end)
    assert caps2[0, 0].tolist() == [5, 6, 7, 10, 11, 1, 1] and caps2[1, 1].tolist() == [22, 23, 1, 1, 1, 1, 1]


def sharp_toy(sharp=8.0, H=32, V=90, sv=1, seed=4, end_bias=0.0):
    """A toy captioner whose output layer is scaled by `sharp`: as initialised its distributions are nearly uniform and the best
    tokens of a row lie ~1e-4 apart, so that hardly any selection could be compared."""
    cfg = oracle.OracleConfig(vocab_size=V, image_feature_size=48, embedding_size=24, hidden_size=H, attention_projection_size=16,
                              z_space=8, max_caption_length=9, sentiment_vae=sv, senti_prior_multip=0.5, beam_size=1)
    params = {k: v.clone() for k, v in oracle.init_params(cfg, seed=seed).items()}
    params["_output_layer.weight"] *= sharp
    params["_output_layer.bias"][cfg.boundary_index] += end_bias
    return cfg, params


@pytest.mark.parametrize("k", [1, 3])
def test_oracle_beam1_prefix_of_its_own_caption_reproduces_the_rest(k):
    """Beam 1, 8 steps, 3 images x 2 samples: the unprefixed oracle search's first k words as the prefix, primed on the noise of
    its first k steps, continued on the rest of the noise - the words of the continuation are the rest of the caption and prefix
    log-prob + continuation log-prob is the caption's within 1e-5.  Every arg-max of the unprefixed search has a margin above 2e-4
    (asserted), so rounding cannot have flipped a word."""
    cfg, params = sharp_toy()
    nimg, ns, R, steps = 3, 2, 5, 8
    B = nimg * ns
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.tensor([1.0, 0.0, -1.0])
    eps0 = torch.randn(B, cfg.z_space, generator=g)
    eps = torch.randn(steps - 1, B, cfg.z_space, generator=g)
    full, full_lp, margin = PR.search(params, cfg, feats, senti, None, ns, eps0, eps, 1, 1, steps, early_stop=False)
    assert margin > PR.MARGIN, margin
    full = full.view(B, steps)
    assert (full[:, :k] != cfg.boundary_index).all(), "a caption ends inside the prefix: pick another seed"
    all_eps = torch.cat([eps0.unsqueeze(0), eps])
    primed = PR.prime(params, cfg, feats, senti, full[:, :k].numpy(), ns, all_eps[:k])
    assert primed["lengths"].tolist() == [k] * B and (primed["tokens"] == full[:, k - 1].numpy()).all()
    rest, rest_lp, _ = PR.search(params, cfg, feats, senti, primed, ns, all_eps[k], all_eps[k + 1:], 1, 1, steps - k, early_stop=False)
    assert torch.equal(rest.view(B, steps - k), full[:, k:])
    total = primed["log_probs"] + rest_lp.view(B).double().numpy()
    assert np.abs(total - full_lp.view(B).double().numpy()).max() < 1e-5
    caps, tot = PR.join(full[:, :k].numpy(), primed["lengths"], rest.view(B, 1, -1).numpy(), None, rest_lp.view(B, 1).numpy(),
                        primed["log_probs"].astype(np.float32), cfg.boundary_index)
    assert (caps[:, 0] == full.numpy()).all() and np.abs(tot[:, 0] - full_lp.view(B).numpy()).max() < 1e-5
