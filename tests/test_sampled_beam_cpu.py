"""CPU: the sampled-node beam search's argument checks, config keys, and the float64 restatement the GPU tests compare against -
checked against the reference's own BeamSearch with MultinomialSampler / TopKSampler / TopPSampler
(tests/golden/g19_sampled_beam.npz)."""
import ctypes as C

import numpy as np
import pytest

import sampledbeamref as R
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.config import Config


def _beam_desc(B, k, n, V):
    d = L.BeamDesc()
    d.scores, d.ld, d.raw_logits = C.c_void_p(256), V, 1
    d.dims = L.FsmDims(0, 1, V, 0, 1)
    d.B, d.beam, d.per_node, d.end_index = B, k, n, 1
    d.last_pred, d.last_lp, d.pred, d.lp_out, d.backptr = [C.c_void_p(256)] * 5
    d.scratch_val, d.scratch_idx = C.c_void_p(256), C.c_void_p(256)
    d.step_index = 1
    return d


def test_sampled_step_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    multi = sampling.MultinomialSampler().desc(1)
    for B, k, n, V in ((2, 3, 4, 3),       # n > V
                       (2, 4, 2, 3),       # k > V
                       (2, 33, 2, 100),    # past the 32-beam limit
                       (2, 3, 33, 100),    # past the 32-candidate limit
                       (2, 3, 0, 50),
                       (2, 0, 1, 50)):
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_beam_step_sampled(C.byref(_beam_desc(B, k, n, V)), C.byref(multi), 0, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # top-k with n > top_k (beam_search.py:180-183)
        lib.ssc_beam_step_sampled(C.byref(_beam_desc(2, 3, 4, 50)), C.byref(sampling.TopKSampler(k=3).desc(1)), 0, None)
    with pytest.raises(L.SscError, match="SSC_EINVAL"):   # top-k past V
        lib.ssc_beam_step_sampled(C.byref(_beam_desc(2, 3, 2, 50)), C.byref(sampling.TopKSampler(k=51).desc(1)), 1, None)
    for T in (0.0, float("inf"), float("nan")):
        bad = sampling.MultinomialSampler().desc(1)
        bad.temperature = T
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_beam_step_sampled(C.byref(_beam_desc(2, 3, 2, 50)), C.byref(bad), 0, None)
    d = _beam_desc(2, 3, 2, 50)
    d.step_index = 0                                      # step 0 is ssc_beam_first_fsm
    with pytest.raises(L.SscError, match="SSC_EINVAL"):
        lib.ssc_beam_step_sampled(C.byref(d), C.byref(multi), 0, None)
    cfg = L.ModelCfg(10, 4, 4, 4, 4, 4, 0, 0, 0, 0.0, 1.0, 0, 1, 0)
    sd = L.SearchDesc()
    sd.nimg, sd.R, sd.n_samples, sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = 2, 3, 4, 1, 3, 1, 5, 1
    # every pointer the search descriptor needs is set (never read: the sampler / beam limits refuse first), so that only the
    # limit under test can fail the call
    sd.feats, sd.imgbuf, sd.eps0, sd.eps, sd.predictions, sd.log_probs, sd.ctl = [C.c_void_p(256)] * 7
    assert lib.ssc_decode_sampled_beam_workspace_bytes(C.byref(cfg), C.byref(sd)) > 0
    for beam, per_node, s in ((3, 1, L.SamplerDesc(0, 0, 1.0, 0.0, 1)),    # T 0
                              (3, 4, L.SamplerDesc(1, 3, 1.0, 1.0, 1)),    # top-k 3 < per_node 4
                              (11, 1, L.SamplerDesc(0, 0, 1.0, 1.0, 1)),   # beam > V (10)
                              (3, 2, L.SamplerDesc(3, 0, 1.0, 1.0, 1))):   # no such kind
        sd.beam, sd.per_node = beam, per_node
        with pytest.raises(L.SscError, match="SSC_EINVAL"):
            lib.ssc_decode_sampled_beam(C.byref(cfg), C.byref(L.Params()), C.byref(sd), C.byref(s), 0, C.c_void_p(256), 1 << 30,
                                        None)


def test_config_keys():
    m = Config().MODEL
    assert m.SAMPLED_BEAM_SEARCH is False and m.SAMPLER_WITH_REPLACEMENT is False
    assert sampling.sampled_beam_from_config(m) is False
    m = Config(config_override=["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLER_TOP_P", "0.8", "MODEL.SAMPLED_BEAM_SEARCH", "True",
                                "MODEL.SAMPLER_WITH_REPLACEMENT", "True", "MODEL.BEAM_SIZE", "5"]).MODEL
    s = sampling.from_config(m)
    assert isinstance(s, sampling.TopPSampler) and s.with_replacement is True and s.p == 0.8
    assert sampling.sampled_beam_from_config(m) is True
    assert sampling.from_config(Config(config_override=["MODEL.DECODE_SAMPLER", "top-k", "MODEL.SAMPLER_TOP_K", "4"]).MODEL
                                ).with_replacement is False
    for over in (["MODEL.SAMPLED_BEAM_SEARCH", "True"],                                       # beam search: no word sampler
                 ["MODEL.SAMPLED_BEAM_SEARCH", "True", "MODEL.DECODE_SAMPLER", "multinomial",
                  "MODEL.STOCHASTIC_BEAM_SEARCH", "True"]):
        with pytest.raises(ValueError, match="SAMPLED_BEAM_SEARCH"):
            sampling.from_config(Config(config_override=over).MODEL)
        with pytest.raises(ValueError, match="SAMPLED_BEAM_SEARCH"):
            sampling.sampled_beam_from_config(Config(config_override=over).MODEL)


def _check_step(what, rec, t, tok, lp, bp=None, tol_lp=1e-6):
    ok = rec["gap"][t] > 1e-5   # entries whose every decision at this step has a margin above 1e-5
    np.testing.assert_array_equal(tok[ok], rec["tok"][t][ok], err_msg=str(what))
    if bp is not None:
        np.testing.assert_array_equal(bp[ok], rec["bp"][t][ok], err_msg=str(what))
    np.testing.assert_allclose(lp[ok], rec["lp_t"][t][ok], atol=tol_lp, rtol=tol_lp, err_msg=str(what))
    return int(ok.sum())


def test_restatement_reproduces_the_reference():
    fx, cases = R.load_fixture()
    checked = total = 0
    for c in cases:
        rec = fx[c["name"]]
        B, k, n = c["B"], c["k"], c["n"]
        kind, top_k, top_p, T = R.sampler_args(c)
        for t, rows in R.replay(c, rec):   # teacher-forced on the reference's own selections
            total += B
            if t == 0:
                tok, lp = R.first_step(rows, k)
                checked += _check_step((c["name"], t), rec, t, tok, lp)
            else:
                tok, lp, bp, _ = R.next_step(rows, rec["tok"][t - 1], rec["lp_t"][t - 1], B, k, n, c["kind"], top_k, top_p, T,
                                             c["rep"], R.SEED, t)
                checked += _check_step((c["name"], t), rec, t, tok, lp, bp, tol_lp=2e-6)
        steps = rec["tok"].shape[0]
        assert rec["pred"].shape == (B, k, steps)
        np.testing.assert_array_equal(rec["pred"][:, :, -1], rec["tok"][-1])
    assert checked > 0.9 * total
    # the fixture covers what it is meant to: beams that end at different steps, duplicated finished captions with replacement,
    # and the forced keep of top-p without replacement (p below the top token's mass, yet n distinct tokens per beam)
    ends = fx["multinomial_r0_ends"]["pred"]
    first_end = np.where((ends == R.END).any(-1), (ends == R.END).argmax(-1), ends.shape[-1])
    assert len(np.unique(first_end)) > 1
    dup = fx["multinomial_r1_ends"]["pred"]
    assert any(len({tuple(x) for x in dup[b]}) < dup.shape[1] for b in range(dup.shape[0]))
    forced = fx["top-p_forced"]
    assert len(np.unique(forced["tok"][1])) > 1


def test_kept_set_forced_keep():
    x = np.array([5.0, 1.0, 0.5, 0.2, 0.1])
    kept, _ = R.kept_set(x, "top-p", top_p=0.1, T=1.0, n=3, rep=False)
    assert kept.tolist() == [True, True, True, False, False]
    kept, _ = R.kept_set(x, "top-p", top_p=0.1, T=1.0, n=3, rep=True)
    assert kept.tolist() == [True, False, False, False, False]
    kept, m = R.kept_set(x, "top-k", top_k=2)
    assert kept.tolist() == [True, True, False, False, False] and m == 0.5


def test_training_builds_with_the_decode_keys_on():
    """scripts/train.py builds the model through from_config without a sampler: a config that turns the sampled-node beam search
    on for inference (DECODE_SAMPLER top-p, SAMPLED_BEAM_SEARCH, BEAM_SIZE 5) builds the training model as it is; with the
    sampler passed (scripts/inference.py) the eval forward takes the sampled-node beam search."""
    import torch

    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    C_ = Config(config_override=["MODEL.DECODE_SAMPLER", "top-p", "MODEL.SAMPLED_BEAM_SEARCH", "True", "MODEL.BEAM_SIZE", "5",
                                 "MODEL.IMAGE_FEATURE_SIZE", "16", "MODEL.EMBEDDING_SIZE", "8", "MODEL.HIDDEN_SIZE", "16",
                                 "MODEL.ATTENTION_PROJECTION_SIZE", "8", "MODEL.Z_SPACE", "4"])
    m = UpDownCaptioner.from_config(C_, vocabulary=Vocabulary.synthetic(50), cbs_simple=C_.MODEL.CBS_SIMPLE,
                                    device=torch.device("cpu"))
    assert m.sampler is None and not m.sampled_beam
    m = UpDownCaptioner.from_config(C_, vocabulary=Vocabulary.synthetic(50), device=torch.device("cpu"),
                                    sampler=sampling.from_config(C_.MODEL))
    assert isinstance(m.sampler, sampling.TopPSampler) and m.sampled_beam
