"""CPU: the definition of caption scoring (tests/scoreref.py: the float64 restatement of ssc_score_rows and the teacher-forced
oracle loop) against the oracle's own greedy decode, on hand-made rows, on absent / truncated / out-of-range captions; and the
arithmetic of CaptionScores.summary()."""
import math

import numpy as np
import pytest
import torch

import oracle
import scoreref as SR
from ssc_runtime.inference import CaptionScores


def toy(seed=7, bias=1.5):
    cfg = oracle.OracleConfig(vocab_size=90, image_feature_size=48, embedding_size=24, hidden_size=32, attention_projection_size=16,
                              z_space=8, max_caption_length=9, sentiment_vae=1, senti_prior_multip=0.5, beam_size=1)
    params = oracle.init_params(cfg, seed=seed)
    params["_output_layer.bias"][cfg.boundary_index] += bias
    return cfg, params


def test_scoring_the_greedy_caption_reproduces_its_log_prob():
    """oracle.eval_forward at beam 1 is the arg-max chain: scoring its caption with the same noise gives its log-prob (1e-5) and
    rank 0 at every scored token."""
    cfg, params = toy()
    g = torch.Generator().manual_seed(2)
    B, R, L = 4, 5, cfg.max_caption_length
    feats = torch.randn(B, R, cfg.image_feature_size, generator=g)
    senti = torch.tensor([1.0, -1.0, 0.0, 1.0])
    eps = [torch.randn(B, cfg.z_space, generator=g) for _ in range(L)]
    fsm = torch.ones(B, 1, 1, cfg.vocab_size, dtype=torch.uint8)
    want = oracle.eval_forward(params, cfg, feats, senti.view(B, 1), fsm, torch.zeros(B, dtype=torch.long), eps, beam_size=1,
                               early_stop=False)
    caps = want["beams"][:, 0, 0, :]
    assert caps.shape == (B, L)
    got = SR.score_captions(params, cfg, feats, senti, caps.view(B, 1, L), 1, eps[0], torch.stack(eps[1:]))
    assert np.abs(got["log_probs"] - want["log_probs"].view(B).double().numpy()).max() < 1e-5
    scored = got["token_rank"] >= 0
    assert (got["token_rank"][scored] == 0).all()
    ends = (caps == cfg.boundary_index)
    first = torch.where(ends.any(-1), ends.float().argmax(-1) + 1, torch.full((B,), L)).numpy()
    assert (got["n_tokens"].reshape(B) == first).all() and (scored.sum(1) == first).all()
    assert (first < L).any()   # (some caption ends early: the ended steps were left out)


def test_rank_restatement_on_a_row_with_ties():
    x = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5, 1.0]], dtype=np.float32)
    lse = math.log(sum(math.exp(v) for v in x[0].astype(np.float64)))
    for t, rank in ((1, 0), (2, 1), (4, 2), (0, 3), (6, 4), (5, 5), (3, 6)):
        lp, rk, run = SR.score_rows(x, [t], None, 0, row_lp=[-1.0])
        assert rk[0] == rank
        assert abs(lp[0] - (float(x[0, t]) - lse)) < 1e-12
        assert abs(run[0] - (-1.0 + lp[0])) < 1e-12
    # ended rows: by the previous token, by a negative target - not looked at (NaN), nothing accumulated; an id >= V: -inf
    bad = np.full((3, 7), np.nan, dtype=np.float32)
    lp, rk, run = SR.score_rows(bad, [2, -1, 7], [0, 5, 5], 0, row_lp=[-1.0, -2.0, -3.0])
    assert list(lp) == [0.0, 0.0, -np.inf] and list(rk) == [-1, -1, -1]
    assert list(run) == [-1.0, -2.0, -np.inf]
    # a spread of +-80 around 1e4: the maximum is subtracted first
    big = (1e4 + np.linspace(-80, 80, 9)).astype(np.float32).reshape(1, 9)
    lp, rk, _ = SR.score_rows(big, [0], None, 1)
    assert rk[0] == 8 and abs(lp[0] - (-160.0 - math.log(sum(math.exp(-20.0 * k) for k in range(9))))) < 1e-9


def test_absent_truncated_and_out_of_range_captions():
    cfg, params = toy(seed=9)
    V, end = cfg.vocab_size, cfg.boundary_index
    g = torch.Generator().manual_seed(4)
    nimg, C, N, R, L = 2, 3, 2, 4, 5
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.tensor([1.0, -1.0])
    G = nimg * C * N
    eps0 = torch.randn(G, cfg.z_space, generator=g)
    eps = torch.randn(L - 1, G, cfg.z_space, generator=g)
    caps = torch.tensor([[[5, 6, end, end, end],      # ends at its third token
                          [-1, 7, 8, 9, 10],          # absent
                          [11, 12, 13, 14, 15]],      # no room for END: truncated, scored over L tokens
                         [[end, end, end, end, end],  # the empty caption: its END alone
                          [20, V, 21, end, end],      # an id outside the vocabulary
                          [30, 31, 32, 33, end]]])
    out = SR.score_captions(params, cfg, feats, senti, caps, N, eps0, eps)
    assert out["n_tokens"].tolist() == [[3, 0, 5], [1, 2, 5]]
    lp = out["log_probs"].reshape(nimg, C, N)
    tl = out["token_lp"].reshape(nimg, C, N, L)
    rk = out["token_rank"].reshape(nimg, C, N, L)
    assert (lp[0, 1] == 0).all() and (tl[0, 1] == 0).all() and (rk[0, 1] == -1).all()          # absent
    assert (tl[0, 0, :, 3:] == 0).all() and (rk[0, 0, :, 3:] == -1).all() and (tl[0, 0, :, :3] < 0).all()
    assert (rk[0, 2] >= 0).all() and np.isfinite(lp[0, 2]).all()                                 # truncated: every step scored
    assert (rk[1, 0, :, 0] >= 0).all() and (rk[1, 0, :, 1:] == -1).all()
    assert np.isneginf(lp[1, 1]).all() and np.isneginf(tl[1, 1, :, 1]).all() and (tl[1, 1, :, 2:] == 0).all()
    assert np.isfinite(tl[1, 1, :, 0]).all()
    assert np.allclose(np.where(np.isfinite(tl), tl, 0).sum(-1)[np.isfinite(lp)], lp[np.isfinite(lp)], atol=1e-12)
    # the two samples of a caption see different noise
    assert (lp[0, 0, 0] != lp[0, 0, 1]) and (lp[1, 2, 0] != lp[1, 2, 1])
    # a caption's score does not depend on its neighbours in the call: the same caption alone, with its rows' noise (the oracle
    # computes in fp32 and its products round differently at another batch size: 1e-5 on a sum near -20)
    g0 = (1 * C + 2) * N
    alone = SR.score_captions(params, cfg, feats[1:], senti[1:], caps[1:, 2:], N, eps0[g0:g0 + N], eps[:, g0:g0 + N])
    assert np.abs(alone["log_probs"] - lp[1, 2]).max() < 1e-5


def test_summary_arithmetic_on_a_worked_example():
    lp = torch.tensor([[[-2.0, -4.0], [0.0, 0.0]], [[-6.0, -6.0], [-1.0, -3.0]]])     # (2 images, 2 captions, 2 samples)
    ntok = torch.tensor([[2, 0], [3, 2]], dtype=torch.int32)                           # (image 0, caption 1) is absent
    marg = torch.logsumexp(lp, -1) - math.log(2)
    rank = torch.tensor([[0, 3, -1], [0, 0, -1], [-1, -1, -1], [-1, -1, -1], [0, 7, 4], [1, 0, 0], [0, 5, -1], [2, 0, -1]],
                        dtype=torch.int32).view(2, 2, 2, 3)
    s = CaptionScores(lp, ntok, marg, token_rank=rank).summary()
    assert s["n_tokens"] == 7 and s["n_captions"] == 3
    assert s["nll_per_token"] == pytest.approx((3.0 + 0.0 + 6.0 + 2.0) / 7, abs=1e-12)
    assert s["perplexity"] == pytest.approx(math.exp(11.0 / 7), rel=1e-12)
    m = [math.log((math.exp(a) + math.exp(b)) / 2) for a, b in ((-2, -4), (0, 0), (-6, -6), (-1, -3))]
    assert torch.allclose(marg.view(-1).double(), torch.tensor(m, dtype=torch.float64), atol=1e-6)
    assert s["marginal_nll_per_token"] == pytest.approx(-sum(m) / 7, abs=1e-6)
    assert marg[0, 1] == 0 and marg[1, 0] == pytest.approx(-6.0)
    assert -s["marginal_nll_per_token"] >= -s["nll_per_token"]          # Jensen: log mean p >= mean log p
    assert s["top1"] == pytest.approx(8 / 14) and s["top5"] == pytest.approx(12 / 14)
    assert "top1" not in CaptionScores(lp, ntok, marg).summary()
    both = CaptionScores.concat([CaptionScores(lp[:1], ntok[:1], marg[:1], token_rank=rank[:1, ..., :2]),
                                 CaptionScores(lp[1:], ntok[1:], marg[1:], token_rank=rank[1:])])
    assert both.token_rank.shape == (2, 2, 2, 3) and both.summary() == s
