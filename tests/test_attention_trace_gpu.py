"""GPU: attention traces - ssc_attn_gather alone against the NumPy restatement (tests/attnref.py), and the traces the one-call
decodes record (every search, the sampled decode, the scoring call) against the restated ancestry fed the device's own words and
back-pointers and against a teacher-forced replay of the returned captions in the CPU oracle; the module's output dict and
scripts/inference.py --attention-output."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import attnref as AR
import oracle
import scoreref as SR
from gpuutil import engine_from
from oracle.seqcvae_oracle import zero_states
from ssc_runtime import lib as L
from ssc_runtime import sampling
from ssc_runtime.decode import CompiledFsm, DecodeEngine
from ssc_runtime.inference import diverse_decode, score_captions
from ssc_runtime.vocab import Vocabulary
from test_score_gpu import YAML, run_child
from var_updown.models import UpDownCaptioner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8
ENTROPY_TOL = 5e-5    # an unordered fp32 sum of R = 128 terms of at most 0.37 each, total at most ln 128: 127 * 2^-24 * 4.85 = 3.7e-5, + the terms' rounding
MAP_TOL = 1e-4        # the project's decode tolerance
TOP_MARGIN = 2e-4     # the oracle's top two weights must differ by more for its arg-max to bind the device


# ---- the gather alone ----------------------------------------------------------------------------------------------------------------
def trace_case(R, steps, n_caps, seed):
    """-> (hist (steps, rows, R) float32 - softmax rows, some with exact ties at the top, row 0 of every slab NaN and never
    referenced -, anc (n_caps, steps) int32 with -1 entries and one entry past the last row)."""
    rng = np.random.default_rng(seed)
    rows = n_caps + 3
    x = rng.standard_normal((steps, rows, R)).astype(np.float32) * 2
    hist = np.exp(x - x.max(-1, keepdims=True))
    hist = (hist / hist.sum(-1, keepdims=True)).astype(np.float32)
    if R > 1:   # exact ties at the maximum, the winner not the first entry
        for t in range(steps):
            for r in range(1, rows, 2):
                i, j = sorted(rng.choice(R, 2, replace=False))
                hist[t, r, i] = hist[t, r, j] = hist[t, r].max()
    hist[:, 0] = np.nan
    anc = rng.integers(1, rows, (n_caps, steps)).astype(np.int32)
    anc[rng.random((n_caps, steps)) < 0.3] = -1
    anc[0, 0] = -1
    anc[-1, -1] = rows + 5   # (not a row of the slab: read as -1, never as an address)
    if n_caps * steps > 2:
        anc[n_caps // 2, steps // 2] = 1
    return hist, anc


def guarded(shape, dtype, fill):
    """-> (flat buffer with GUARD sentinel words on either side, the view of `shape` between them)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD: GUARD + n].view(*shape)


def run_gather(hist_d, rows, R, steps, anc_d, n_caps, sel_d, n, ld, want=("maps", "top", "wgt", "ent")):
    """-> {name: (buffer, view)} of the outputs asked for; every buffer pre-filled with a sentinel."""
    lib = L.load()
    out = {}
    if "maps" in want:
        out["maps"] = guarded((n, steps, ld), torch.float32, 777.0)
    if "top" in want:
        out["top"] = guarded((n, steps), torch.int32, -99)
    if "wgt" in want:
        out["wgt"] = guarded((n, steps), torch.float32, 777.0)
    if "ent" in want:
        out["ent"] = guarded((n, steps), torch.float32, 777.0)
    p = lambda k: C.c_void_p(out[k][1].data_ptr()) if k in out else None
    d = L.AttnGatherDesc(C.c_void_p(hist_d.data_ptr()), rows, R, steps, L.ptr(anc_d), n_caps, L.ptr(sel_d), n, p("maps"), ld, p("top"),
                         p("wgt"), p("ent"))
    lib.ssc_attn_gather(C.byref(d), L.stream_ptr())
    torch.cuda.synchronize()
    return out


def guards_intact(out):
    for name, (buf, view) in out.items():
        fill = -99 if name == "top" else 777.0
        if not (bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())):
            return False
    return True


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("R", [1, 3, 4, 36, 37, 65, 128, 129])
def test_gather_against_the_restatement(R, pad):
    """maps, top_region (exact ties included) and top_weight bit-equal to tests/attnref.py, entropy within 5e-5 of float64; the pad
    columns of ld_maps = R + 3 and the guard words around every output untouched; zero rows never read (their history is NaN);
    every output optional in turn; two calls bit-equal.  ld_maps = R with R % 4 == 0 takes the 16-byte form, everything else - and
    a history that is not 16-byte aligned - the scalar one.  Measured on one MI355X: the largest |entropy - float64| over all cases is 7.1e-7."""
    worst = 0.0
    for steps, n_caps in ((1, 1), (2, 7), (20, 70)):
        hist, anc = trace_case(R, steps, n_caps, seed=R * 100 + steps)
        rows = hist.shape[1]
        rng = np.random.default_rng(steps)
        perm = rng.integers(0, n_caps, n_caps + 3)          # a permutation with repeats
        oob = perm.copy()
        oob[len(oob) // 2] = n_caps                          # one entry outside [0, n_caps)
        oob[0] = -1
        for off in ((0, 1) if R % 4 == 0 and pad == 0 else (0,)):
            flat = torch.full((off + hist.size + 4,), float("nan"), device="cuda")
            hist_d = flat[off: off + hist.size].view(steps, rows, R)
            hist_d.copy_(torch.from_numpy(hist))
            assert (hist_d.data_ptr() % 16 == 0) == (off == 0)
            anc_d = torch.from_numpy(anc).cuda()
            for sel in (None, perm, oob):
                sel_d = torch.from_numpy(sel.astype(np.int64)).cuda() if sel is not None else None
                n = n_caps if sel is None else len(sel)
                ld = R + pad
                maps, top, wgt, ent = AR.gather(hist, anc, sel)
                out = run_gather(hist_d, rows, R, steps, anc_d, n_caps, sel_d, n, ld)
                got = out["maps"][1].cpu().numpy()
                assert np.array_equal(got[..., :R].view(np.uint32), maps.view(np.uint32)), (steps, n_caps, off)
                assert (got[..., R:] == 777.0).all()
                assert np.array_equal(out["top"][1].cpu().numpy(), top)
                assert np.array_equal(out["wgt"][1].cpu().numpy().view(np.uint32), wgt.view(np.uint32))
                e = np.abs(out["ent"][1].cpu().double().numpy() - ent).max()
                worst = max(worst, float(e))
                assert e <= ENTROPY_TOL, e
                assert guards_intact(out)
                zero = (top == -1)
                assert (got[..., :R][zero] == 0).all() and (out["ent"][1].cpu().numpy()[zero] == 0).all()
                if sel is oob:
                    assert zero[0].all() and zero[len(oob) // 2].all()
                again = run_gather(hist_d, rows, R, steps, anc_d, n_caps, sel_d, n, ld)
                for k in out:
                    assert torch.equal(out[k][0].view(torch.int32), again[k][0].view(torch.int32)), k
                # each output on its own: what the others do not change
                for k in ("maps", "top", "wgt", "ent"):
                    one = run_gather(hist_d, rows, R, steps, anc_d, n_caps, sel_d, n, ld, want=(k,))
                    assert torch.equal(one[k][0].view(torch.int32), out[k][0].view(torch.int32)), k
    print(f"R {R} pad {pad}: max |entropy - float64| {worst:.3e}")


# ---- the decodes ---------------------------------------------------------------------------------------------------------------------
VARIANTS = {"untied-sv1": (False, 1, 0), "tied-sv0": (True, 0, 0), "untied-sv0-fp32": (False, 0, 2), "tied-sv1-fp32": (True, 1, 2)}
DECODERS = ("beam1", "beam3", "cbs", "stochastic", "sampled", "diverse", "rules", "sample")
V_, F_, R_, STEPS = 300, 64, 9, 8
END_BIAS = 1.2
# seeds of (model, inputs) per variant, checked on the CPU with the oracle alone (the 4 entries' captions of the best / second-best
# word, 8 steps; the large case: 128 entries at H 32, R 36, inputs seed 29): the share of steps whose two largest attention weights
# differ by more than 2e-4 is 1.0 for each of them (smallest gap 3.2e-2; the large case 1.1e-3)
SEEDS = {"untied-sv1": (4, 17), "tied-sv0": (4, 17), "untied-sv0-fp32": (4, 17), "tied-sv1-fp32": (4, 17)}


@functools.lru_cache(maxsize=None)
def medium_params(variant, H=48):
    """-> (cfg, params) of the medium model, on the CPU."""
    tied, sv, mode = VARIANTS[variant]
    cfg = oracle.OracleConfig(vocab_size=V_, image_feature_size=F_, embedding_size=32, hidden_size=H, attention_projection_size=24,
                              z_space=8, max_caption_length=STEPS, sentiment_vae=sv, senti_prior_multip=0.5, tied=tied, beam_size=3)
    params = oracle.init_params(cfg, seed=SEEDS[variant][0])
    # attention logits of a freshly initialised model are nearly flat; a wider attention layer spreads the weights over the regions
    params = {k: v.clone() for k, v in params.items()}
    params["_updown_cell._butd_attention._attention_layer.weight"] *= 8.0
    if not tied:   # a sharper head whose END competes: captions that end at different steps
        params["_output_layer.weight"] *= 8.0
        params["_output_layer.bias"][cfg.boundary_index] += END_BIAS
    return cfg, params


@functools.lru_cache(maxsize=None)
def medium(variant, H=48):
    cfg, params = medium_params(variant, H)
    mode = VARIANTS[variant][2]
    eng = engine_from(cfg, params)
    dec = DecodeEngine(eng.dims, eng.params.c_struct, "cuda")
    if mode:
        dec._cfg.gemm_mode = mode   # (what an engine-wide ModelDims.gemm_mode sets)
    return cfg, params, eng, dec


def entry_inputs(cfg, nimg, ns, R, seed, steps):
    """Noise per BATCH ENTRY: the S * beam rows of an entry share it at every step, so a caption's noise does not depend on its
    ancestry.  -> feats (nimg, R, F), senti (nimg,) or None, eps0 (B, Z), eps (steps - 1, B, Z)."""
    g = torch.Generator().manual_seed(seed)
    B = nimg * ns
    feats = torch.randn(nimg, R, cfg.image_feature_size, generator=g)
    senti = torch.randint(-1, 2, (nimg,), generator=g).float() if cfg.sentiment_vae else None
    eps0 = torch.randn(B, cfg.z_space, generator=g)
    eps = torch.randn(steps - 1, B, cfg.z_space, generator=g)
    return feats, senti, eps0, eps


def two_constraint_machines(B, V, seed):
    """One machine per batch entry over the states {neither, first, second, both} of two constraint words."""
    g = torch.Generator().manual_seed(seed)
    fsm = torch.zeros(B, 4, 4, V, dtype=torch.uint8)
    for b in range(B):
        w = (torch.randperm(V - 2, generator=g)[:2] + 2).tolist()
        for s in range(4):
            fsm[b, s, s] = 1
            for i in range(2):
                fsm[b, s, s, w[i]] = 0
                fsm[b, s, s | (1 << i), w[i]] = 1
    return fsm


def run_decoder(name, dec, ctx, sent_b, ns, steps, end, eps0, eps, B, attention, skip_dead=True, early_stop=True, machines=None):
    """-> (pred (n_caps, steps'), log_probs (n_caps,), record or None, SB, driver of ssc_debug_decode_view); eps (steps - 1, B, Z) is per
    batch entry and repeated over the entry's rows here."""
    beam = {"beam1": 1, "sample": 1}.get(name, 3)
    if name == "diverse":
        beam = 4
    S = 4 if name == "cbs" else 1
    SB = S * beam
    e = eps.repeat_interleave(SB, dim=1)
    kw = dict(early_stop=early_stop, attention=attention)
    if name in ("beam1", "beam3"):
        out = dec.search(ctx, sent_b, ns, beam, min(beam, 2), steps, end, eps0, e, skip_dead=skip_dead, **kw)
    elif name == "cbs":
        fsm, compiled = machines
        out = dec.search(ctx, sent_b, ns, beam, 2, steps, end, eps0, e, fsm=fsm, compiled=compiled, skip_dead=skip_dead, **kw)
    elif name == "stochastic":
        out = dec.stochastic_beam(ctx, sent_b, ns, beam, 2, steps, end, eps0, e, sampling.GumbelSampler(1.0), 11, skip_dead=skip_dead, **kw)
    elif name == "sampled":
        out = dec.sampled_beam(ctx, sent_b, ns, beam, 2, steps, end, eps0, e, sampling.TopKSampler(k=20), 12, skip_dead=skip_dead, **kw)
    elif name == "diverse":
        out = dec.diverse_beam(ctx, sent_b, ns, beam, 1, steps, end, eps0, e, sampling.DiverseBeam(2, 0.5), skip_dead=skip_dead, **kw)
    elif name == "rules":
        out = dec.rules_beam(ctx, sent_b, ns, beam, 2, steps, end, eps0, e, sampling.DecodeRules(2, 2, 0.7, (0,)), skip_dead=skip_dead, **kw)
        out = (out[0], out[1]) + tuple(out[4:])
    else:
        out = dec.sample(ctx, sent_b, ns, steps, end, eps0, e, sampling.MultinomialSampler(1.0), 13, **kw)
    pred, lps = out[0], out[1]
    rec = out[2] if attention else None
    return pred.reshape(B * SB, -1), lps.reshape(B * SB), rec, SB, 1 if name == "sample" else 0


def device_words(dec, sd_like, driver, steps, rows):
    """The words and back-pointers the call that has just run left in the engine's workspace (include/ssc_debug.h)."""
    lib = L.load()
    ws = C.c_void_p(dec._sws.data_ptr())
    out = []
    for which, n in ((0, steps), (1, steps - 1)):
        p = lib.ssc_debug_decode_view(C.byref(dec._cfg), C.byref(sd_like), ws, driver, which)
        if not p or n == 0:
            out.append(None)
            continue
        off = p - dec._sws.data_ptr()
        out.append(dec._sws[off: off + n * rows * 8].view(torch.int64).view(n, rows).cpu().numpy())
    return out


def search_desc_like(ctx, ns, S, beam, per_node, steps, end):
    """The extents ssc_debug_decode_view sizes the workspace with (the pointers are not looked at)."""
    d = L.SearchDesc()
    d.nimg, d.R, d.n_samples, d.S, d.beam, d.per_node, d.max_steps, d.end_index = ctx.nimg, ctx.R, ns, S, beam, per_node, steps, end
    return d


def replay(cfg, params, feats, senti, caps, SB, ns, eps0, eps):
    """Teacher-forced replay of the captions caps (n_caps, T) - caption q belongs to batch entry q // SB, image q // (SB * ns) - in
    oracle.decode_step with the entry's noise.  -> alpha (T, n_caps, R) float32: the attention behind word t of every caption."""
    n, T = caps.shape
    q = torch.arange(n)
    entry, img = q // SB, q // (SB * ns)
    fr = feats[img]
    se = senti[img].view(n, 1) if senti is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, n, fr)
    states = zero_states(n, cfg.hidden_size, fr)
    fed = torch.full((n,), cfg.boundary_index, dtype=torch.int64)
    out = []
    with torch.no_grad():
        for t in range(T):
            e = eps0[entry] if t == 0 else eps[t - 1][entry]
            _, states, _, _, alpha = oracle.decode_step(params, cfg, fr, fed, states, False, se, pm, pv, e)
            out.append(alpha.numpy())
            fed = caps[:, t].clone()
    return np.stack(out)


def check_trace(name, dec, cfg, params, feats, senti, ns, eps0, eps, machines=None, run=None):
    """Everything a decode's trace must satisfy; `run`: the decoder, called like run_decoder (default: run_decoder itself).
    -> (max |map - oracle|, share of non-zero rows whose arg-max was compared, predictions, record, trace, S * beam, non-zero rows)."""
    run = run or run_decoder
    nimg = feats.size(0)
    B = nimg * ns
    end, steps = cfg.boundary_index, STEPS
    ctx = dec.prepare(feats.cuda())
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B).cuda() if senti is not None else None
    args = (name, dec, ctx, sent_b, ns, steps, end, eps0.cuda(), eps.cuda(), B)
    plain, plain_lp, _, SB, driver = run(*args, attention=False, machines=machines)
    pred, lps, rec, _, _ = run(*args, attention=True, machines=machines)
    n_caps, nsteps = pred.shape
    assert rec.rows == n_caps and rec.steps == steps and rec.R == ctx.R
    # predictions and log-probs: the same bits as without the trace
    assert torch.equal(pred, plain) and torch.equal(lps.view(torch.int32), plain_lp.view(torch.int32))
    # anc: the restated ancestry fed the device's own words and back-pointers
    S = 4 if name == "cbs" else 1
    like = search_desc_like(ctx, ns, S, SB // S, 1, steps, end)
    words, backs = device_words(dec, like, driver, steps, n_caps)
    anc = rec.anc.cpu().numpy()
    want_anc = AR.ancestry(words.reshape(steps, B, SB), None if backs is None else backs.reshape(steps - 1, B, SB), nsteps, end,
                           lps.cpu().numpy().reshape(B, SB))
    assert np.array_equal(anc, want_anc), name
    assert (anc[:, nsteps:] == -1).all() and (anc[:, 0] == np.arange(n_caps) // SB)[lps.cpu().numpy() > -1e19].all()
    tr = dec.attention(rec)
    maps, top = tr.maps.cpu().numpy(), tr.top_region.cpu().numpy()
    live = anc >= 0
    # the zero pattern, exactly
    assert (maps[~live] == 0).all() and (maps[live].sum(-1) > 0.5).all() and ((top == -1) == ~live).all()
    assert (tr.top_weight.cpu().numpy()[~live] == 0).all() and (tr.entropy.cpu().numpy()[~live] == 0).all()
    # the first END keeps its attention, what follows it reads nothing
    p = pred.cpu().numpy()
    ended = np.cumsum(p == end, axis=1) - (p == end) > 0       # words after the first END
    assert not (live[:, :nsteps] & ended).any()
    alive = lps.cpu().numpy() > -1e19
    assert (live[:, :nsteps] | ended)[alive].all()
    # against the teacher-forced replay of every returned caption in the oracle
    want = replay(cfg, params, feats, senti, pred.cpu(), SB, ns, eps0, eps)            # (nsteps, n_caps, R)
    want = np.transpose(want, (1, 0, 2))
    diff = np.abs(maps[:, :nsteps].astype(np.float64) - want)[live[:, :nsteps]]
    worst = float(diff.max())
    assert worst < MAP_TOL, (name, worst)
    # arg-max: the device's own map on every row, the oracle's wherever its top two are further apart than the margin
    assert (top[live] == maps[live].argmax(-1)).all()
    srt = np.sort(want, -1)
    clear = (srt[..., -1] - srt[..., -2] > TOP_MARGIN) & live[:, :nsteps]
    assert (top[:, :nsteps][clear] == want.argmax(-1)[clear]).all()
    share = clear.sum() / max(live.sum(), 1)
    assert share >= 0.9, (name, share)
    # two calls: the same bits
    pred2, lps2, rec2, _, _ = run(*args, attention=True, machines=machines)
    tr2 = dec.attention(rec2)
    assert torch.equal(rec2.anc, rec.anc) and torch.equal(tr2.maps.view(torch.int32), tr.maps.view(torch.int32))
    assert torch.equal(tr2.entropy.view(torch.int32), tr.entropy.view(torch.int32))
    # skip_dead on and off: the same ancestry and the same zero pattern
    if name != "sample":
        pred3, _, rec3, _, _ = run(*args, attention=True, skip_dead=False, machines=machines)
        tr3 = dec.attention(rec3)
        same = alive if name == "cbs" else np.ones(n_caps, dtype=bool)   # (a beam without a finite log-prob may hold other tokens)
        assert np.array_equal(rec3.anc.cpu().numpy(), anc)
        assert np.array_equal(tr3.maps.cpu().numpy() == 0, maps == 0)
        assert torch.equal(pred3.cpu()[torch.from_numpy(same)], pred.cpu()[torch.from_numpy(same)])
    return worst, share, pred, rec, tr, SB, live


@pytest.mark.parametrize("name", DECODERS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_decode_traces(variant, name):
    """Every one-call decode on the medium model (V 300, H 48, R 9, 2 images x 2 samples, 8 steps; untied and tied heads, SENTIMENT_VAE
    0 and 1, the default GEMM mode and exact fp32): see check_trace.  Then DecodeEngine.score(attention=True) on the call's own
    captions - one slot absent, the columns cut so that some captions have no END - with the entries' noise: the search's maps
    within 1e-4.  Measured on one MI355X: max |map - oracle| 4.5e-7 over all cases, score against decode 0 (the same bits), every non-zero row's arg-max
    compared."""
    cfg, params, _, dec = medium(variant)
    nimg, ns = 2, 2
    B = nimg * ns
    feats, senti, eps0, eps = entry_inputs(cfg, nimg, ns, R_, SEEDS[variant][1], STEPS)
    machines = None
    if name == "cbs":
        fsm = two_constraint_machines(B, V_, seed=3).cuda()
        machines = (fsm, CompiledFsm(fsm, fill=8))
    worst, share, pred, rec, tr, SB, live = check_trace(name, dec, cfg, params, feats, senti, ns, eps0, eps, machines)
    print(f"{variant} {name}: steps {pred.size(1)}, max |map - oracle| {worst:.3e}, arg-max compared on {share:.3f} of the rows")
    if not VARIANTS[variant][0] and name == "beam3":
        assert ((pred == cfg.boundary_index).sum(1) > 1).any(), "no caption ends early: the forced-END rule is not exercised"
    # the scoring call on the same captions
    n_caps, nsteps = pred.shape
    # cut the columns at the latest first END: that caption then has no END inside the call (none at all: every column stays)
    is_end = (pred == cfg.boundary_index).cpu()
    first_end = torch.where(is_end.any(1), is_end.float().argmax(1), torch.full((n_caps,), nsteps))
    Lc = int(first_end[lps_alive(rec, pred)].max())
    assert Lc >= 2
    caps = pred[:, :Lc].clone().view(nimg, ns * SB, Lc).cpu()
    absent = (int(first_end.argmax()) + 1) % n_caps                         # an absent slot (not the caption without an END)
    caps.view(n_caps, Lc)[absent, 0] = -1
    ctx = dec.prepare(feats.cuda())
    sent_g = senti.view(nimg, 1).expand(nimg, ns * SB).reshape(n_caps).cuda() if senti is not None else None
    e0 = eps0.repeat_interleave(SB, 0).cuda()
    e = eps.repeat_interleave(SB, 1)[: Lc - 1].cuda()
    lp_s, ntok, _, _, srec = dec.score(ctx, sent_g, caps, 1, cfg.boundary_index, e0, e, attention=True)
    assert srec.rows == n_caps and srec.steps == Lc
    lp_plain = dec.score(ctx, sent_g, caps, 1, cfg.boundary_index, e0, e)[0]
    assert torch.equal(lp_plain.view(torch.int32), lp_s.view(torch.int32))
    sanc = srec.anc.cpu().numpy()
    tgt = SR.prepare_targets(caps, 1, cfg.vocab_size, cfg.boundary_index)[0].T   # (G, L)
    assert np.array_equal(sanc, np.where(tgt >= 0, np.arange(n_caps)[:, None], -1))
    assert (sanc[absent] == -1).all() and int(ntok.view(-1)[absent]) == 0
    no_end = (caps.view(n_caps, Lc) != cfg.boundary_index).all(1).numpy()
    no_end[absent] = False
    assert no_end.any() and (sanc[no_end] >= 0).all()
    smaps = dec.attention(srec).maps.cpu().numpy()
    assert (smaps[sanc < 0] == 0).all()
    both = (sanc >= 0) & live[:, :Lc]
    d = np.abs(smaps.astype(np.float64) - tr.maps.cpu().numpy()[:, :Lc])[both]
    print(f"{variant} {name}: score vs decode max |map| difference {d.max():.3e} over {both.sum()} rows")
    assert both.sum() > 0 and d.max() < MAP_TOL


def lps_alive(rec, pred):
    """Captions whose trace holds a word at all (a beam without a finite log-prob holds none)."""
    return (rec.anc[:, 0] >= 0).cpu()


@pytest.mark.parametrize("ungathered", [1, 0])
def test_large_call_forms(ungathered):
    """512 rows per step at small width (H 32, V 300, R 36): 8 images x 16 samples x beam 4, where ssc_decode_ungathered_ok says
    yes (the states stay in the previous step's row order), and 4 images x 32 samples x beam 4, where it says no (fewer than 8
    images: the states are re-ordered); both with the attended-feature table and skipped rows.  The same checks as above."""
    cfg, params, _, dec = medium("untied-sv1", H=32)
    nimg, ns, beam = (8, 16, 4) if ungathered else (4, 32, 4)
    B = nimg * ns
    lib = L.load()
    assert lib._raw_ssc_decode_ungathered_ok(C.byref(dec._cfg), nimg, B * beam, beam, 1) == ungathered
    feats, senti, eps0, eps = entry_inputs(cfg, nimg, ns, 36, 29, STEPS)

    def run(name, dec_, ctx, sent_b, ns_, steps, end, eps0_, eps_, B_, attention, skip_dead=True, early_stop=True, machines=None):
        e = eps_.repeat_interleave(beam, dim=1)
        out = dec_.search(ctx, sent_b, ns_, beam, 2, steps, end, eps0_, e, skip_dead=skip_dead, early_stop=early_stop, attention=attention)
        return out[0].reshape(B_ * beam, -1), out[1].reshape(B_ * beam), (out[2] if attention else None), beam, 0

    worst, share, pred, rec, tr, SB, live = check_trace("beam4", dec, cfg, params, feats, senti, ns, eps0, eps, run=run)
    print(f"ungathered {ungathered}: steps {pred.size(1)}, max |map - oracle| {worst:.3e}, arg-max compared on {share:.3f}")


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def test_diverse_decode_returns_the_trace_of_its_captions():
    """diverse_decode(attention=...) over every decoder: the captions of the same call without it (same global random state), the
    trace shaped like them, words after a caption's END at region -1; "summary" carries no maps; with return_groups the groups'."""
    cfg, params, _, dec = medium("untied-sv1")
    nimg, ns = 3, 2
    feats, senti, _, _ = entry_inputs(cfg, nimg, ns, R_, 5, STEPS)
    feats, senti = feats.cuda(), senti.cuda()
    end = cfg.boundary_index
    fsm = two_constraint_machines(nimg, V_, seed=4).cuda()
    cases = [dict(beam=3), dict(beam=1, sampler=sampling.TopPSampler(0.9)), dict(beam=3, sampler=sampling.GumbelSampler(1.0)),
             dict(beam=3, sampler=sampling.TopKSampler(k=10), sampled_beam=True), dict(beam=4, diverse_beam=sampling.DiverseBeam(2, 0.5)),
             dict(beam=4, diverse_beam=sampling.DiverseBeam(2, 0.5), return_groups=True),
             dict(beam=3, rules=sampling.DecodeRules(2, 2, 0.7, (0,))),
             dict(beam=3, fsm=fsm, num_constraints=torch.full((nimg * ns,), 2), min_constraints_to_satisfy=2)]
    for kw in cases:
        torch.manual_seed(7)
        plain = diverse_decode(dec, feats, senti, ns, kw["beam"], STEPS, end, **{k: v for k, v in kw.items() if k != "beam"})
        state = torch.random.get_rng_state()
        for mode in ("summary", "full"):
            torch.manual_seed(7)
            out = diverse_decode(dec, feats, senti, ns, kw["beam"], STEPS, end, attention=mode,
                                 **{k: v for k, v in kw.items() if k != "beam"})
            assert torch.equal(torch.random.get_rng_state(), state)
            assert len(out) == len(plain) + 1 and torch.equal(out[0], plain[0]) and out[1] == plain[1]
            tr, pred = out[-1], out[0]
            assert tr.top_region.shape == pred.shape and tr.entropy.shape == pred.shape and tr.top_weight.shape == pred.shape
            assert (tr.maps is None) == (mode == "summary")
            if tr.maps is not None:
                assert tr.maps.shape == pred.shape + (R_,)
                assert torch.equal(tr.maps.argmax(-1)[tr.top_region >= 0], tr.top_region[tr.top_region >= 0].long())
                assert ((tr.maps.sum(-1) - 1).abs() < 1e-5)[tr.top_region >= 0].all()
            after = ((pred == end).cumsum(-1) - (pred == end).long()) > 0
            assert torch.equal(tr.top_region < 0, after), kw
    with pytest.raises(ValueError, match="attention"):
        diverse_decode(dec, feats, senti, ns, 3, STEPS, end, attention="maps")


def test_score_captions_carries_the_trace_and_concat_pads_it():
    cfg, _, _, dec = medium("untied-sv1")
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(3, R_, F_, generator=g).cuda()
    senti = torch.tensor([1.0, 0.0, -1.0]).cuda()
    caps = torch.zeros(3, 2, 6, dtype=torch.int64)
    for k in range(6):
        caps[k // 2, k % 2, : k + 1] = torch.randint(2, V_, (k + 1,), generator=g)
    caps[1, 1] = 0   # absent
    torch.manual_seed(1)
    plain = score_captions(dec, feats, senti, caps, 2, cfg.boundary_index, "padded")
    torch.manual_seed(1)
    full = score_captions(dec, feats, senti, caps, 2, cfg.boundary_index, "padded", attention="full")
    assert plain.attention is None and torch.equal(plain.log_probs, full.log_probs)
    tr = full.attention
    Lc = int(full.n_tokens.max())
    assert tr.maps.shape == (3, 2, 2, Lc, R_) and tr.top_region.shape == (3, 2, 2, Lc)
    scored = torch.arange(Lc, device="cuda").view(1, 1, 1, Lc) < full.n_tokens.view(3, 2, 1, 1)
    assert torch.equal(tr.top_region >= 0, scored.expand(3, 2, 2, Lc))
    torch.manual_seed(1)
    short = score_captions(dec, feats[:1], senti[:1], caps[:1], 2, cfg.boundary_index, "padded", attention="full")
    both = type(full).concat([short, full])
    assert both.attention.maps.shape == (4, 2, 2, Lc, R_) and (both.attention.top_region[0, :, :, short.attention.top_region.size(3):] == -1).all()
    assert (both.attention.maps[0, :, :, short.attention.maps.size(3):] == 0).all()
    assert type(full).concat([plain, full]).attention is None


def test_module_output_dict_with_the_mode_set_and_unset():
    """UpDownCaptioner.decode_attention: unset, the eval forward returns {"predictions"} alone; "summary" adds the three summaries,
    "full" the maps as well - for the plain beam search, a word sampler, the diverse search and the rules - and the predictions
    are those of the unset forward under the same noise."""
    torch.manual_seed(3)
    V, F, R, L_, Z = 120, 64, 5, 8, 16
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(4, R, F, generator=g).cuda()
    senti = torch.randint(-1, 2, (4, 1), generator=g).float().cuda()
    kinds = [dict(), dict(sampler=sampling.TopKSampler(k=5), beam_size=1), dict(diverse_beam=sampling.DiverseBeam(2, 0.5), beam_size=4),
             dict(decode_rules=sampling.DecodeRules(2, 2, 0.7, (0,)))]
    for kw in kinds:
        torch.manual_seed(3)
        args = dict(max_caption_length=L_, beam_size=3, z_space=Z, sentiment_vae=1, senti_prior_multip=0.5, device=torch.device("cuda"))
        args.update(kw)
        m = UpDownCaptioner(Vocabulary.synthetic(V), F, 40, 48, 32, **args).cuda().eval()

        def forward():   # (the same global random state in: the same latent noise and word seed, drawn in the same order)
            torch.manual_seed(11)
            return m(feats, sentiment=senti)

        base = forward()
        assert set(base) == {"predictions"}
        m.decode_attention("summary")
        out = forward()
        assert set(out) == {"predictions", "attention_top_region", "attention_top_weight", "attention_entropy"}
        n = min(out["predictions"].size(1), base["predictions"].size(1))
        assert torch.equal(out["predictions"][:, :n].cpu(), base["predictions"][:, :n].cpu()), kw
        assert out["attention_top_region"].shape == out["predictions"].shape
        m.decode_attention("full")
        out = forward()
        assert out["attention"].shape == out["predictions"].shape + (R,)
        live = out["attention_top_region"] >= 0
        assert torch.equal(out["attention"].argmax(-1)[live], out["attention_top_region"][live].long()) and live[:, 0].all()
        m.decode_attention(None)
        assert set(forward()) == {"predictions"}
        with pytest.raises(ValueError, match="mode"):
            m.decode_attention("all")


def test_inference_script_attention_output(tmp_path):
    """scripts/inference.py --attention-output [--attention-full]: predictions.json is the file of a run without the flag, byte for
    byte; one entry per written caption, cut behind the caption's END; the maps' arg-max is the top region."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(YAML)
    base = [os.path.join(ROOT, "scripts", "inference.py"), "--config", str(cfg), "--gpu-ids", "0", "--synthetic", "5", "--vocab-size", "150",
            "--num-boxes", "5", "--images-per-call", "3"]
    rc, log = run_child(base + ["--output-path", str(tmp_path / "plain.json")])
    assert rc == 0, log
    rc, log = run_child(base + ["--output-path", str(tmp_path / "traced.json"), "--attention-output", str(tmp_path / "attn.pt"),
                                "--attention-full"])
    assert rc == 0, log
    assert open(tmp_path / "plain.json", "rb").read() == open(tmp_path / "traced.json", "rb").read()
    preds = json.load(open(tmp_path / "plain.json"))
    traces = torch.load(tmp_path / "attn.pt", weights_only=True)
    assert len(traces) == len(preds) == 20
    for p, e in zip(preds, traces):
        assert e["image_id"] == p["image_id"]
        n = len(p["caption"].split())
        assert e["tokens"].numel() in (n, n + 1) and e["tokens"].numel() <= 8          # words + END (no END: all 8 steps)
        assert e["top_region"].shape == e["top_weight"].shape == e["entropy"].shape == e["tokens"].shape
        assert e["maps"].shape == (e["tokens"].numel(), 5) and (e["top_region"] >= 0).all()
        assert torch.equal(e["maps"].argmax(-1), e["top_region"].long()) and (e["entropy"] > 0).all()
    rc, log = run_child(base + ["--output-path", str(tmp_path / "x.json"), "--attention-full"])
    assert rc != 0 and "--attention-output" in log
