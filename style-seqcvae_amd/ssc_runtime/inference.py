"""Diverse decoding: N_Z stochastic beam-search decodes per image, batched over images x samples on one GPU.

Reference: var_updown/scripts/inference.py:117-189 runs, per image (batch forced to 1, :95), a Python loop of
N_Z_SAMPLES calls of model(...) - 20 x <=20 steps x G=beam rows: launch-bound.  Here the (image, sample) pairs are
the batch entries of ONE constrained beam search (rows ordered image, sample, fsm state, beam), per-image terms are
computed once per image and shared by its N_Z * beam rows; the result per (image, sample) equals the reference's
per-call result given the same per-row noise.
"""
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import lib as _lib
from .decode import AttentionTrace, DecodeEngine, EnsembleDecodeEngine
from .decoding import select_best_beam_simple_batched, select_best_state_simple_batched




def diverse_decode(dec: Union[DecodeEngine, EnsembleDecodeEngine], feats: torch.Tensor, sentiment: Optional[torch.Tensor], n_samples: int, beam: int,
                   max_steps: int, boundary_index: int, fsm: Optional[torch.Tensor] = None,
                   num_constraints: Optional[torch.Tensor] = None, min_constraints_to_satisfy: int = 0,
                   eps_steps: Optional[List[torch.Tensor]] = None, early_stop: bool = True, per_node: Optional[int] = None,
                   skip_dead: bool = True, compiled=None, obj_means: Optional[torch.Tensor] = None, sampler=None,
                   sample_seed: Optional[int] = None, sampled_beam: bool = False, diverse_beam=None, return_groups: bool = False,
                   rules=None, attention: Optional[str] = None, guide=None, logit_rules=None, prefix=None,
                   prefix_eps: Optional[torch.Tensor] = None, truncation=None, contrast=None, contrast_stats: bool = False, mirostat=None,
                   mirostat_stats: bool = False, arithmetic=None):
    """feats (nimg,R,F), sentiment (nimg,) or None -> predictions (nimg, n_samples, steps) int64 on device.
    dec: a DecodeEngine, or an EnsembleDecodeEngine (ssc_runtime.decode) - the beam search, plain or constrained (fsm), then runs
    over the ensemble's members in one call; the sampled / stochastic / diverse / rules decodes and attention traces belong to a
    single engine and raise NotImplementedError with an ensemble.
    fsm: None (trivial one-state machine, what MAX_GIVEN_CONSTRAINTS: 0 produces), or (nimg, S, S, V) uint8 - ONE machine per
    image, shared by its n_samples latent samples through an index list -, or (nimg*n_samples, S, S, V) (a copy per sample).
    eps_steps: optional explicit noise per step call [(rows_k, Z)]; default: a generator of this call's own, seeded by ONE draw
    from the global CPU generator - the global random state a call consumes does not depend on how many steps it ran.
    skip_dead: rows that hold no finite beam - the states an image's constraints never reach,
    every state before its first constraint word has been decoded - and rows whose beam has ended are neither stepped nor scored from
    logits (cbs_search(skip_dead=True)).  Every caption with a finite log-prob is the exact search's; should a selected caption
    have none (its constraints were not reachable within max_steps), the call is repeated exactly, with the same noise.
    compiled: the machines' CompiledFsm when the caller has it already.
    obj_means (nimg, R, Z): per-region attribute means, SENTIMENT_VAE = 2 only (UpDownCaptioner.translate_obj_atts2obj_means).
    sampler: None - beam search, as above -, or a word sampler of ssc_runtime.sampling (multinomial / top-k / top-p): every word
    of every caption is then drawn on the device (DecodeEngine.sample, one library call); needs beam = 1 and fsm = None.  Or
    sampling.GumbelSampler: the stochastic beam search (DecodeEngine.stochastic_beam) at any beam, per_node as for beam search;
    beam 0 - the sampled caption with the highest log-prob - of every (image, sample) is returned; needs fsm = None.
    sample_seed: the 64-bit seed of the word draws; default: the call's one draw from the global generator (the seed of the
    latent noise as well; with eps_steps given, one draw is made for the words), so a sampled call consumes the global random
    state as a beam call does and sees the same latent noise as a beam-1 call.
    sampled_beam: with a word sampler, run it as the reference's BeamSearch does (DecodeEngine.sampled_beam) at any beam: step 0
    takes the top `beam` words, every later step draws per_node (default beam // 2, or beam) candidates per beam and keeps the
    `beam` best by summed log-prob; beam 0 of every (image, sample) is returned; needs fsm = None.
    diverse_beam: a sampling.DiverseBeam(groups, strength) - the deterministic diverse beam search (DecodeEngine.diverse_beam) at
    `beam`, per_node by default the reference's rule on the group width (beam // groups // 2, or beam // groups); needs
    sampler = None and fsm = None.  The caption with the highest log-prob of every (image, sample) is returned (ties: the lower
    beam); with return_groups=True instead every group's best: (predictions (nimg, n_samples, groups, steps), steps, log_probs
    (nimg, n_samples, groups)).
    rules: a sampling.DecodeRules - the beam search runs under them (DecodeEngine.rules_beam: n-gram blocking, minimum length,
    suppressed tokens, length penalty); needs sampler = None, no diverse_beam and fsm = None.  Beam 0 - the best caption under the
    length penalty - of every (image, sample) is returned.  None, or rules with every control off: the plain beam search.
    attention: None, "summary" or "full" - with it the call additionally returns, as its last value, the AttentionTrace
    (ssc_runtime.decode) of exactly the captions it returns, whatever the decoder: top_region / top_weight / entropy (nimg,
    n_samples, steps) - with return_groups (nimg, n_samples, groups, steps) - and, under "full", maps (..., steps, R).  Words after
    a caption's first END read nothing: region -1, zeros.  The captions, log-probs and the random state consumed do not change.
    guide: a LatentGuide (ssc_runtime.guide) over the nimg * n_samples entries (image, sample), or None - the latents are then
    drawn around the guide's path instead of the prior, for the beam search (with or without fsm) and for word sampling; every
    other decoder and an ensemble raise NotImplementedError naming the feature.
    logit_rules: a sampling.LogitRules - with a word sampler the raw logits of every step are edited in front of the draw
    (DecodeEngine.sample(logit_rules=): word bias, repetition / presence / frequency penalties, n-gram / length / token bans);
    ValueError with any other decoder, NotImplementedError with an ensemble.  None, or rules with every control off: the plain
    sampled decode.  (`rules` stays the beam search's and keeps refusing a sampler.)
    truncation: a sampling.Truncation (typical / min-p / eta / epsilon) - with a word sampler every step's distribution is cut
    between the logit rules and the draw (DecodeEngine.sample(truncation=)); ValueError naming the decoder with any other one,
    NotImplementedError with an ensemble.  None or an inactive one: the call without it.  Composes with logit_rules, guide, prefix
    and attention.
    contrast: a contrast.Contrast - contrastive decoding with a word sampler (DecodeEngine.sample(contrast=)): an amateur stream -
    degraded features, z at the prior mean, a neutral sentiment, no exemplar or a weak checkpoint - is decoded in lock-step and every
    step's logits are contrasted with it in front of the logit rules.  The amateur's image context is prepared here ("noise:g"
    features from a generator seeded by the call's one draw of the global generator); with prefix= both streams are primed on the
    same prefix noise.  ValueError naming the decoder with any other one, NotImplementedError with an ensemble.  None or an inactive
    one: the call without it.  Greedy contrastive decoding is the top-k sampler with k = 1.  contrast_stats=True: the result is
    followed by (kept, divergence) of shape (nimg, n_samples, steps) - over the continuation with a prefix.
    mirostat: a sampling.Mirostat - with a word sampler the surprise of every caption's words is held at its target by feedback
    (DecodeEngine.sample(mirostat=): a cut behind the truncation, an update behind the draw); ValueError naming the decoder with any
    other one, NotImplementedError with an ensemble.  None or an inactive one: the call without it.  Composes with logit_rules,
    truncation, contrast, guide, prefix (the control starts at the continuation) and attention.  mirostat_stats=True: the result is
    followed - behind the contrast's statistics - by (mu, surprise, kept) of shape (nimg, n_samples, steps), in the object's unit.
    arithmetic: a sampling.Arithmetic - with a word sampler every step's draw is made by inverse CDF along a code point per caption
    (DecodeEngine.sample(arithmetic=)), the codes of an image a randomly shifted lattice: the n_samples captions of an image are
    stratified, each still an exact draw.  With share_latent=True all samples of an image are given the noise (eps0, eps and a
    prefix's) of its sample 0 - contiguous copies made here - and differ by their codes alone.  ValueError naming the decoder with
    any decoder but a word sampler, NotImplementedError with an ensemble.  None: the call without it.  Composes with logit_rules,
    truncation, contrast, mirostat, guide, prefix (the codes start at the continuation) and attention.
    prefix: a DecodePrefix (ssc_runtime.prefix) with one row per image - or per (image, sample) entry -, or None.  With it every
    caption starts with its image's prompt: the prompt is teacher-forced on the nimg * n_samples rows (DecodeEngine.prime), whichever
    decoder was chosen continues from there (start=) and the call returns the FULL captions (nimg, n_samples, Lp + steps) - the
    prompt's words, the continuation, then @@BOUNDARY@@ - with return_groups the grouped form, its log-probs the prompt's included.
    The second value stays the number of SEARCH steps executed; max_steps bounds the continuation.  The machine of a constrained
    search starts in its start state after the prompt (constraint words inside the prompt do not count), and the rules and logit
    rules see the continuation only.  An image whose row holds no word decodes as without a prefix.
    prefix_eps (Lp, nimg * n_samples, Z): the noise of the prompt's steps; default: drawn from the call's own generator AFTER the
    noise of the search, so that the search sees the noise of the same call without a prefix.  NotImplementedError together with
    attention=, guide= or an ensemble."""
    if prefix is not None:
        from .prefix import prefix_unsupported
        if isinstance(dec, EnsembleDecodeEngine):
            prefix_unsupported("an ensemble (EnsembleDecodeEngine)")
        if guide is not None:
            prefix_unsupported("latent guides (guide=)")
        if attention is not None:
            prefix_unsupported("attention traces (attention=): the trace would not cover the prefix words")
    if logit_rules is not None and not logit_rules.active:
        logit_rules = None
    if logit_rules is not None:
        if isinstance(dec, EnsembleDecodeEngine):
            raise NotImplementedError("logit rules (logit_rules) are not implemented for an ensemble (EnsembleDecodeEngine)")
        if sampler is None or sampler.beam_search or sampled_beam:
            raise ValueError("the logit rules belong to the word samplers: logit_rules needs a multinomial / top-k / top-p sampler "
                             "without sampled_beam (the beam search takes rules=)")
    if truncation is not None and not truncation.active:
        truncation = None
    if truncation is not None:
        if isinstance(dec, EnsembleDecodeEngine):
            raise NotImplementedError("truncation (truncation=) is not implemented for an ensemble (EnsembleDecodeEngine)")
        other = ("the beam search under decode rules (rules)" if rules is not None and rules.active else
                 "the diverse beam search (diverse_beam)" if diverse_beam is not None else
                 "the sampled-node beam search (sampled_beam)" if sampled_beam else
                 "the stochastic beam search (GumbelSampler)" if sampler is not None and sampler.beam_search else
                 "the beam search" if sampler is None else None)
        if other is not None:
            raise ValueError(f"the truncation belongs to the word samplers: truncation= needs a multinomial / top-k / top-p sampler, "
                             f"not {other}")
    if mirostat is not None and not mirostat.active:
        mirostat = None
    if mirostat_stats and mirostat is None:
        raise ValueError("mirostat_stats needs an active mirostat")
    if mirostat is not None:
        if isinstance(dec, EnsembleDecodeEngine):
            raise NotImplementedError("Mirostat (mirostat=) is not implemented for an ensemble (EnsembleDecodeEngine)")
        other = ("the beam search under decode rules (rules)" if rules is not None and rules.active else
                 "the diverse beam search (diverse_beam)" if diverse_beam is not None else
                 "the sampled-node beam search (sampled_beam)" if sampled_beam else
                 "the stochastic beam search (GumbelSampler)" if sampler is not None and sampler.beam_search else
                 "the beam search" if sampler is None else None)
        if other is not None:
            raise ValueError(f"Mirostat belongs to the word samplers: mirostat= needs a multinomial / top-k / top-p sampler, "
                             f"not {other}")
    if arithmetic is not None:
        if isinstance(dec, EnsembleDecodeEngine):
            raise NotImplementedError("arithmetic sampling (arithmetic=) is not implemented for an ensemble (EnsembleDecodeEngine)")
        other = ("the beam search under decode rules (rules)" if rules is not None and rules.active else
                 "the diverse beam search (diverse_beam)" if diverse_beam is not None else
                 "the sampled-node beam search (sampled_beam)" if sampled_beam else
                 "the stochastic beam search (GumbelSampler)" if sampler is not None and sampler.beam_search else
                 "the beam search" if sampler is None else None)
        if other is not None:
            raise ValueError(f"arithmetic sampling belongs to the word samplers: arithmetic= needs a multinomial / top-k / top-p "
                             f"sampler, not {other}")
    if contrast is not None and not contrast.active:
        contrast = None
    if contrast_stats and contrast is None:
        raise ValueError("contrast_stats needs an active contrast")
    if contrast is not None:
        if isinstance(dec, EnsembleDecodeEngine):
            raise NotImplementedError("contrastive decoding (contrast=) is not implemented for an ensemble (EnsembleDecodeEngine)")
        other = ("the beam search under decode rules (rules)" if rules is not None and rules.active else
                 "the diverse beam search (diverse_beam)" if diverse_beam is not None else
                 "the sampled-node beam search (sampled_beam)" if sampled_beam else
                 "the stochastic beam search (GumbelSampler)" if sampler is not None and sampler.beam_search else
                 "the beam search" if sampler is None else None)
        if other is not None:
            raise ValueError(f"the contrast belongs to the word samplers: contrast= needs a multinomial / top-k / top-p sampler, "
                             f"not {other}")
    if guide is not None:
        from .guide import guide_unsupported
        if isinstance(dec, EnsembleDecodeEngine):
            guide_unsupported("an ensemble (EnsembleDecodeEngine)")
        if rules is not None and rules.active:
            guide_unsupported("the beam search under decode rules (rules)")
        if diverse_beam is not None:
            guide_unsupported("the diverse beam search (diverse_beam)")
        if sampled_beam:
            guide_unsupported("the sampled-node beam search (sampled_beam)")
        if sampler is not None and sampler.beam_search:
            guide_unsupported("the stochastic beam search (GumbelSampler)")
    if attention not in (None, "summary", "full"):
        raise ValueError(f'attention must be None, "summary" or "full", got {attention!r}')
    want_attn = attention is not None
    if rules is not None and not rules.active:
        rules = None
    if rules is not None:
        if sampler is not None or sampled_beam:
            raise ValueError("the decode rules belong to the deterministic beam search: they take no sampler")
        if diverse_beam is not None:
            raise ValueError("the decode rules cannot be combined with diverse_beam")
        if fsm is not None:
            raise ValueError("the beam search under decode rules does not take constraints (fsm)")
        rules.check(dec.dims.V, boundary_index, max_steps)
    if diverse_beam is not None:
        if sampler is not None or sampled_beam:
            raise ValueError("the diverse beam search is deterministic: it takes no sampler")
        if fsm is not None:
            raise ValueError("the diverse beam search does not take constraints (fsm)")
        diverse_beam.check_beam(beam)
        per_node = per_node or diverse_beam.per_node(beam)
    elif return_groups:
        raise ValueError("return_groups needs diverse_beam")
    gumbel = sampler is not None and sampler.beam_search
    if sampled_beam:
        if sampler is None or gumbel:
            raise ValueError("sampled_beam needs a word sampler (multinomial / top-k / top-p)")
        if fsm is not None:
            raise ValueError("the sampled-node beam search does not take constraints (fsm): constrained sampling is not supported")
    words = sampler is not None and not gumbel and not sampled_beam
    if gumbel and fsm is not None:
        raise ValueError("the stochastic beam search does not take constraints (fsm): constrained sampling is not supported")
    if words:
        if beam != 1:
            raise ValueError(f"word sampling draws one word per row: beam must be 1, got {beam}")
        if fsm is not None:
            raise ValueError("word sampling does not take constraints (fsm): constrained sampling is not supported")
    dev = feats.device
    nimg = feats.size(0)
    d = dec.dims
    B = nimg * n_samples
    ctx = dec.prepare(feats, obj_means)
    trivial = fsm is None   # one-state machine: cbs_search(fsm=None) reads no mask at all
    if trivial:
        num_constraints = torch.zeros(B, dtype=torch.long)
    sent_b = sentiment.reshape(nimg, 1).expand(nimg, n_samples).reshape(B) if sentiment is not None else None
    calls = {"k": 0}
    mach = None
    if not trivial and fsm.size(0) != B:
        assert fsm.size(0) == nimg, (fsm.shape, nimg, n_samples)
        mach = torch.arange(nimg, dtype=torch.int32, device=dev).repeat_interleave(n_samples)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (eps_steps is None or (sampler is not None and sample_seed is None)) else None
    skip = bool(skip_dead) and (trivial or fsm.size(1) > 1)   # (trivial machine: only ended beams are left out of the steps)
    if not trivial and fsm.size(1) > 1 and compiled is None:
        from .decode import CompiledFsm
        compiled = CompiledFsm(fsm, fill=max(8, per_node or (beam // 2) or beam))

    per_node = per_node or (beam // 2) or beam
    S = 1 if trivial else fsm.size(1)
    G = B * S * beam

    gkw = {"guide": guide} if guide is not None else {}   # (an unguided call is made exactly as before)
    primed = {}   # with a prefix: "ids" (B, Lp), "start" the StartState - formed by the first search, reused by a repeat
    pseed = None
    if prefix is not None and prefix_eps is None and eps_steps is not None:
        pseed = int(torch.randint(0, 2 ** 62, (1,)).item())   # (the prefix noise of a call whose search noise is the caller's)

    share = arithmetic is not None and arithmetic.share_latent

    def shared(x):
        """noise (..., B, Z) -> every sample of an image given the noise of its sample 0 (share_latent), a contiguous copy"""
        if not share:
            return x
        lead = x.shape[:-2]
        return x.reshape(*lead, nimg, n_samples, d.Z)[..., :1, :].expand(*lead, nimg, n_samples, d.Z).reshape(*lead, B, d.Z).contiguous()

    def prime(gen):
        """-> the start= of this call's decoder: {} without a prefix"""
        if prefix is None:
            return {}
        if not primed:
            from .prefix import DecodePrefix
            ids = (prefix if isinstance(prefix, DecodePrefix) else DecodePrefix(prefix)).ids
            if ids.size(0) == nimg:
                ids = ids.repeat_interleave(n_samples, 0)
            if ids.size(0) != B:
                raise ValueError(f"the prefix has {ids.size(0)} rows for {nimg} images x {n_samples} samples")
            if prefix_eps is not None:
                peps = prefix_eps
            else:
                if gen is None:
                    gen = torch.Generator(device=dev)
                    gen.manual_seed(pseed)
                peps = torch.randn(ids.size(1), B, d.Z, device=dev, generator=gen)
            peps = shared(peps)
            primed["ids"] = ids.to(dev)
            primed["start"] = dec.prime(ctx, sent_b, n_samples, primed["ids"], boundary_index, peps)
            if contrast is not None and contrast.steps_amateur:   # the amateur reads the same prompt under the same noise
                a_sent = sent_b
                if contrast.sentiment is not None:
                    a_sent = torch.as_tensor(contrast.sentiment, dtype=torch.float32, device=dev)
                    a_sent = (a_sent.reshape(1).expand(B) if a_sent.numel() == 1 else
                              a_sent.reshape(nimg, 1).expand(nimg, n_samples).reshape(B) if a_sent.numel() == nimg else a_sent.reshape(B))
                contrast.start = (contrast.engine or dec).prime(contrast.ctx if contrast.ctx is not None else ctx, a_sent, n_samples,
                                                                primed["ids"], boundary_index, peps)
        return {"start": primed["start"]}

    def joined(beams, lps):
        """-> (the full captions of a prefixed call, their log-probs); the search's own without a prefix"""
        if prefix is None:
            return beams, lps
        from .prefix import join_prefix
        return join_prefix(primed["ids"], primed["start"], beams, lps, boundary_index)
    rkw = {"logit_rules": logit_rules} if logit_rules is not None else {}
    if truncation is not None:
        rkw["truncation"] = truncation
    if mirostat is not None:
        rkw["mirostat"] = mirostat
        if mirostat_stats:
            rkw["mirostat_stats"] = True
    if arithmetic is not None:
        rkw["arithmetic"] = arithmetic
    stats = {}
    if contrast is not None:
        cgen = torch.Generator(device=dev)
        cgen.manual_seed(seed if seed is not None else sample_seed)   # (no draw of the call's own: the caller gave the draws' seed)
        contrast.prepare(dec, ctx.feats, ctx.obj, generator=cgen)
        contrast.start = None
        rkw["contrast"] = contrast
        if contrast_stats:
            rkw["contrast_stats"] = True

    def search(skip_now):
        # the noise of ALL steps is drawn up front - from the caller's list, or from a generator of this call's own seeded by ONE draw
        # of the global generator: the search may stop early (or, polled late, a few steps after it could have), and what the
        # global random state looks like after the call must not depend on that
        if eps_steps is not None:
            eps0 = eps_steps[0]
            rest = [e.to(dev, torch.float32) for e in eps_steps[1:max_steps]]
            eps = torch.zeros(max(max_steps - 1, 1), G, d.Z, device=dev)
            if rest:
                eps[: len(rest)] = torch.stack(rest)
            skw = prime(None)
        else:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
            eps0 = torch.randn(B, d.Z, device=dev, generator=gen)
            eps = torch.randn(max(max_steps - 1, 1), G, d.Z, device=dev, generator=gen)
            skw = prime(gen)
        if rules is not None:
            beams, lps, _, _, *rec = dec.rules_beam(ctx, sent_b, n_samples, beam, per_node, max_steps, boundary_index, eps0, eps, rules,
                                                    early_stop=early_stop, skip_dead=skip_now, attention=want_attn, **skw)
            calls["k"] = beams.size(-1)
            return beams.view(B, 1, beam, -1), lps.view(B, 1, beam), rec
        if diverse_beam is not None:
            beams, lps, *rec = dec.diverse_beam(ctx, sent_b, n_samples, beam, per_node, max_steps, boundary_index, eps0, eps,
                                                diverse_beam, early_stop=early_stop, skip_dead=skip_now, attention=want_attn, **skw)
            calls["k"] = beams.size(-1)
            return beams.view(B, 1, beam, -1), lps.view(B, 1, beam), rec
        if sampled_beam:
            beams, lps, *rec = dec.sampled_beam(ctx, sent_b, n_samples, beam, per_node, max_steps, boundary_index, eps0, eps, sampler,
                                                seed if sample_seed is None else sample_seed, early_stop=early_stop,
                                                skip_dead=skip_now, attention=want_attn, **skw)
            calls["k"] = beams.size(-1)
            return beams.view(B, 1, beam, -1), lps.view(B, 1, beam), rec
        if gumbel:
            beams, lps, *rec = dec.stochastic_beam(ctx, sent_b, n_samples, beam, per_node, max_steps, boundary_index, eps0, eps,
                                                   sampler, seed if sample_seed is None else sample_seed, early_stop=early_stop,
                                                   skip_dead=skip_now, attention=want_attn, **skw)
            calls["k"] = beams.size(-1)
            return beams.view(B, 1, beam, -1), lps.view(B, 1, beam), rec
        if sampler is not None:
            eps0, eps = shared(eps0), shared(eps)
            pred, lps, *rec = dec.sample(ctx, sent_b, n_samples, max_steps, boundary_index, eps0, eps, sampler,
                                         seed if sample_seed is None else sample_seed, early_stop=early_stop, attention=want_attn,
                                         **gkw, **rkw, **skw)
            if mirostat_stats:   # (the last of the statistics DecodeEngine.sample appends)
                stats["mirostat"] = rec.pop()
            if contrast_stats:
                stats["kept"], stats["divergence"] = rec.pop()
            calls["k"] = pred.size(-1)
            return pred.view(B, 1, 1, -1), lps.view(B, 1, 1), rec
        beams, lps, *rec = dec.search(ctx, sent_b, n_samples, beam, per_node, max_steps, boundary_index, eps0, eps,
                                      fsm=None if trivial else fsm.contiguous(), compiled=compiled, mach=mach, skip_dead=skip_now,
                                      early_stop=early_stop, attention=want_attn, **gkw, **skw)
        calls["k"] = beams.size(-1)   # one step call per column (cbs.py:127,170)
        return beams, lps, rec

    def trace(rec, sel, lead):
        """-> () without attention, else (the AttentionTrace of captions `sel` of the call behind `rec`, shaped lead + (steps[, R])
        and cut to the executed steps,)"""
        if not want_attn:
            return ()
        tr = dec.attention(rec[0], sel.reshape(lead), maps=attention == "full", summary=True)
        k = calls["k"]
        return (type(tr)(*(None if x is None else x[:, :, :k] if len(lead) == 2 else x[:, :, :, :k] for x in tr)),)

    beams, lps, rec = search(skip)
    beams, total = joined(beams, lps)   # (the selections below go by the search's own log-probs: the prefix's is the same for an entry's beams)
    if diverse_beam is not None:   # group-major, not sorted across groups: the arg-max inside each group, then over the entry
        Gr = diverse_beam.groups
        steps = beams.size(-1)
        glp = lps.view(B, Gr, beam // Gr)
        gi = glp.argmax(-1)   # (ties: the lower beam)
        gbest = beams.view(B, Gr, beam // Gr, steps).gather(2, gi.view(B, Gr, 1, 1).expand(B, Gr, 1, steps)).squeeze(2)
        gbest_lp = total.view(B, Gr, beam // Gr).gather(2, gi.unsqueeze(-1)).squeeze(-1)
        # the call's caption number of every group's best: entry b, group g, beam gi inside it (group-major)
        rows = torch.arange(B, device=dev).view(B, 1) * beam + torch.arange(Gr, device=dev).view(1, Gr) * (beam // Gr) + gi
        if return_groups:
            return (gbest.view(nimg, n_samples, Gr, steps), calls["k"], gbest_lp.view(nimg, n_samples, Gr)) + \
                trace(rec, rows, (nimg, n_samples, Gr))
        bi = gbest_lp.argmax(-1)
        best = gbest.gather(1, bi.view(B, 1, 1).expand(B, 1, steps)).squeeze(1)
        return (best.view(nimg, n_samples, -1), calls["k"]) + trace(rec, rows.gather(1, bi.view(B, 1)), (nimg, n_samples))
    state = torch.zeros(B, dtype=torch.long, device=dev)   # the machine state whose beam 0 is returned
    if trivial or fsm.size(1) == 1:
        best = beams[:, 0, 0, :]
    else:
        best, best_lp = select_best_beam_simple_batched(beams, lps, num_constraints, min_constraints_to_satisfy)
        if skip and bool((best_lp <= -1e19).any()):   # (one read of the device; the captions are about to be read anyway)
            beams, lps, rec = search(False)   # (and with it the trace: the repeat's record; a prefix's start state is reused)
            beams, total = joined(beams, lps)
            best, _ = select_best_beam_simple_batched(beams, lps, num_constraints, min_constraints_to_satisfy)
        if want_attn:
            state = select_best_state_simple_batched(lps, num_constraints, min_constraints_to_satisfy)
    sel = (torch.arange(B, device=dev) * S + state) * beam
    cstats = ((stats["kept"].view(nimg, n_samples, -1), stats["divergence"].view(nimg, n_samples, -1)),) if contrast_stats else ()
    mstats = (tuple(x.view(nimg, n_samples, -1) for x in stats["mirostat"]),) if mirostat_stats else ()
    return (best.view(nimg, n_samples, -1), calls["k"]) + trace(rec, sel, (nimg, n_samples)) + cstats + mstats


def count_tokens(pred: torch.Tensor, boundary_index: int) -> int:
    """Tokens emitted before the first @@BOUNDARY@@ of every caption (inference.py:180-182)."""
    is_end = (pred == boundary_index)
    steps = pred.size(-1)
    first = torch.where(is_end.any(-1), is_end.float().argmax(-1), torch.full(pred.shape[:-1], steps, device=pred.device))
    return int(first.sum().item())


@dataclass
class CaptionScores:
    """What score_captions returns.  log_probs (nimg, C, N): log p(caption | z^n, image), the END included; n_tokens (nimg, C): the
    scored tokens, the END included (0: an absent slot, whose log-probs are 0); marginal (nimg, C) = logsumexp_n log_probs - log N,
    the Monte-Carlo estimate of log p(caption | image) with z^n drawn from the prior; token_lp (nimg, C, N, L) / token_rank
    (nimg, C, N, L) int32 when asked for (0 / -1 after a caption's end; rank 0: the token was the model's arg-max)."""
    log_probs: torch.Tensor
    n_tokens: torch.Tensor
    marginal: torch.Tensor
    token_lp: Optional[torch.Tensor] = None
    token_rank: Optional[torch.Tensor] = None
    attention: Optional[AttentionTrace] = None   # score_captions(attention=...): (nimg, C, N, L[, R]) per part

    @staticmethod
    def concat(parts: "List[CaptionScores]") -> "CaptionScores":
        """The scores of several calls over different images as one (token arrays padded to the longest call: 0 / -1; the attention
        trace padded as the steps after a caption's end are: region -1, zeros)."""
        def cat_trace():
            trs = [p.attention for p in parts]
            if any(t is None for t in trs):
                return None
            L = max(t.top_region.size(3) for t in trs)
            out = []
            for name, fill in (("maps", 0.0), ("top_region", -1), ("top_weight", 0.0), ("entropy", 0.0)):
                ts = [getattr(t, name) for t in trs]
                if any(x is None for x in ts):
                    out.append(None)
                    continue
                pad = lambda x: (0, 0, 0, L - x.size(3)) if name == "maps" else (0, L - x.size(3))
                out.append(torch.cat([torch.nn.functional.pad(x, pad(x), value=fill) for x in ts]))
            return AttentionTrace(*out)

        def cat(name, fill):
            ts = [getattr(p, name) for p in parts]
            if any(t is None for t in ts):
                return None
            L = max(t.size(-1) for t in ts)
            return torch.cat([torch.nn.functional.pad(t, (0, L - t.size(-1)), value=fill) for t in ts])
        return CaptionScores(torch.cat([p.log_probs for p in parts]), torch.cat([p.n_tokens for p in parts]),
                             torch.cat([p.marginal for p in parts]), cat("token_lp", 0.0), cat("token_rank", -1), cat_trace())

    def summary(self) -> Dict[str, float]:
        """nll_per_token = -sum_c mean_n log_probs / sum_c n_tokens, perplexity = exp of it, marginal_nll_per_token =
        -sum_c marginal / sum_c n_tokens; top1 / top5: the share of scored tokens of rank 0 / below 5 (with token_rank)."""
        n = float(self.n_tokens.sum().item())
        if n == 0:
            raise ValueError("no caption was scored")
        nll = -float(self.log_probs.double().mean(-1).sum().item()) / n
        out = {"n_captions": int((self.n_tokens > 0).sum().item()), "n_tokens": int(n), "nll_per_token": nll,
               "perplexity": math.exp(nll) if nll < 700 else math.inf,
               "marginal_nll_per_token": -float(self.marginal.double().sum().item()) / n}
        if self.token_rank is not None:
            scored = self.token_rank >= 0
            k = max(int(scored.sum().item()), 1)
            out["top1"] = int((self.token_rank == 0).sum().item()) / k
            out["top5"] = int((scored & (self.token_rank < 5)).sum().item()) / k
        return out


def score_captions(dec: DecodeEngine, feats: torch.Tensor, sentiment: Optional[torch.Tensor], captions: torch.Tensor, n_samples: int,
                   boundary_index: int, layout: str, eps_steps: Optional[List[torch.Tensor]] = None,
                   obj_means: Optional[torch.Tensor] = None, pad_index: int = 0, want_tokens: bool = False,
                   want_ranks: bool = False, attention: Optional[str] = None) -> CaptionScores:
    """How likely are GIVEN captions under the model: feats (nimg, R, F), sentiment (nimg,) or None, captions (nimg, C, L) int64,
    each scored under n_samples latent samples drawn from the prior (DecodeEngine.score, one library call).
    layout - required, nothing is guessed: "padded" = the training layout (the words, then pad_index; no boundary tokens; a slot
    that starts with pad_index is absent) - the END is appended here; "decoded" = what the decoders return (the words, then
    boundary_index from the caption's end on; a slot whose first entry is negative is absent) - scored as emitted: a caption that
    ran out of steps before its END has none.  The call is trimmed to the longest caption.  Ids outside the vocabulary raise
    ValueError on the host, before anything is launched.
    eps_steps: optional explicit noise per step [(nimg * C * n_samples, Z)], rows (image, caption, sample); default: a generator of
    this call's own, seeded by ONE draw of the global CPU generator (as diverse_decode draws its noise).
    obj_means (nimg, R, Z): per-region attribute means, SENTIMENT_VAE = 2 only.
    attention: None, "summary" or "full": the scores then carry the AttentionTrace of every (caption, sample) - top_region /
    top_weight / entropy (nimg, C, N, L) and, under "full", maps (nimg, C, N, L, R); zeros (region -1) after a caption's end."""
    if attention not in (None, "summary", "full"):
        raise ValueError(f'attention must be None, "summary" or "full", got {attention!r}')
    if layout not in ("padded", "decoded"):
        raise ValueError(f"layout must be 'padded' (training layout) or 'decoded' (decoder output), got {layout!r}")
    if captions.dim() != 3 or captions.size(0) != feats.size(0) or captions.size(2) < 1:
        raise ValueError(f"captions must be (nimg, C, L) with nimg = {feats.size(0)}, got {tuple(captions.shape)}")
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1")
    d = dec.dims
    dev = feats.device
    nimg, Cc, L0 = captions.shape
    caps = captions.to("cpu", torch.int64)
    end = boundary_index
    steps = torch.arange(L0 + 1).view(1, 1, -1)
    if layout == "padded":
        is_pad = caps == pad_index
        length = torch.where(is_pad.any(-1), is_pad.float().argmax(-1), torch.full((nimg, Cc), L0))   # words before the first pad
        absent = length == 0
        tg = torch.cat([caps, torch.full((nimg, Cc, 1), end, dtype=torch.int64)], -1)
        tg = torch.where(steps >= length.unsqueeze(-1), torch.full_like(tg, end), tg)
        n_scored = length + 1
    else:
        absent = caps[..., 0] < 0
        is_end = caps == end
        length = torch.where(is_end.any(-1), is_end.float().argmax(-1), torch.full((nimg, Cc), L0))
        tg = torch.where(steps[..., :L0] >= length.unsqueeze(-1), torch.full_like(caps, end), caps)
        n_scored = (length + 1).clamp(max=L0)
    live = ~absent
    if not bool(live.any()):
        raise ValueError("every caption slot is absent")
    words = tg[live]
    if bool(((words < 0) | (words >= d.V)).any()):
        bad = words[(words < 0) | (words >= d.V)]
        raise ValueError(f"caption ids outside the vocabulary [0, {d.V}): e.g. {int(bad[0])}")
    Lc = int(n_scored[live].max())
    tg = tg[..., :Lc].clone()
    tg[absent] = -1
    G = nimg * Cc * n_samples
    if eps_steps is not None:
        if len(eps_steps) < Lc:
            raise ValueError(f"eps_steps holds {len(eps_steps)} steps, the longest caption needs {Lc}")
        eps0 = eps_steps[0].to(dev, torch.float32)
        eps = torch.stack([e.to(dev, torch.float32) for e in eps_steps[1:Lc]]) if Lc > 1 else None
    else:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        eps0 = torch.randn(G, d.Z, device=dev, generator=gen)
        eps = torch.randn(max(Lc - 1, 1), G, d.Z, device=dev, generator=gen)[: Lc - 1] if Lc > 1 else None
    ctx = dec.prepare(feats, obj_means)
    sent_g = sentiment.reshape(nimg, 1).expand(nimg, Cc * n_samples).reshape(G) if sentiment is not None else None
    lps, ntok, tlp, trk, *rec = dec.score(ctx, sent_g, tg.to(dev), n_samples, end, eps0, eps, want_tokens=want_tokens,
                                          want_ranks=want_ranks, attention=attention is not None)
    lps = lps.view(nimg, Cc, n_samples)
    tr = None
    if rec:
        sel = torch.arange(G, device=dev).view(nimg, Cc, n_samples)
        tr = dec.attention(rec[0], sel, maps=attention == "full", summary=True)
    return CaptionScores(attention=tr, log_probs=lps, n_tokens=ntok, marginal=torch.logsumexp(lps, -1) - math.log(n_samples),
                         token_lp=tlp.view(nimg, Cc, n_samples, Lc) if tlp is not None else None,
                         token_rank=trk.view(nimg, Cc, n_samples, Lc) if trk is not None else None)


# ---- posterior scoring: ELBO and the importance-weighted bound -------------------------------------------------------------------------
def plan_posterior_chunks(n_words, n_samples: int, max_rows: int = 256) -> "List[Tuple[List[int], int]]":
    """The forwards of one posterior scoring call.  n_words: the words of every caption slot in slot order (image-major, flat; 0: an
    absent slot, which is dropped).  -> [(slots, length)]: the slot numbers of a chunk, in order, and its longest caption; a chunk
    runs len(slots) * n_samples rows (slot-major, then sample), at most max_rows; the samples of a caption are never split.  Pure."""
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1")
    if n_samples > max_rows:
        raise ValueError(f"n_samples ({n_samples}) exceeds max_rows ({max_rows}): the samples of a caption stay in one forward")
    per = max_rows // n_samples
    present = [i for i, n in enumerate(n_words) if int(n) > 0]
    chunks = []
    for lo in range(0, len(present), per):
        slots = present[lo: lo + per]
        chunks.append((slots, max(int(n_words[i]) for i in slots)))
    return chunks


@dataclass
class PosteriorScores:
    """What posterior_score_captions returns (K = n_samples draws z^k ~ q(z | x) per caption; include/ssc.h: ssc_train_posterior).
    (nimg, C, K): log_w = log p(x | z, image) + log p(z) - log q(z | x), nll = -log p(x | z, image), log_ratio = log p(z) - log q(z | x)
    with p(z) the prior the eval decode samples, kld = the training KL in closed form (SENTIMENT_VAE 0: against N(0, 1) whatever
    PRIOR_STD is).  (nimg, C): n_tokens (the END included; 0: an absent slot, zeros everywhere), elbo = mean_k log_w, iwae =
    logsumexp_k log_w - log K (>= elbo; Burda et al. 2016), ess = exp(2 lse(log_w) - lse(2 log_w)) in [1, K].  kl_dim (Z) float64: the
    training KL per latent dimension summed over every live (row, step), n_steps of them.  token_kl / token_ratio (nimg, C, K, L + 1)
    with want_steps: the training KL / the log-ratio of every step (0 after the caption's end)."""
    log_w: torch.Tensor
    nll: torch.Tensor
    log_ratio: torch.Tensor
    kld: torch.Tensor
    n_tokens: torch.Tensor
    elbo: torch.Tensor
    iwae: torch.Tensor
    ess: torch.Tensor
    kl_dim: torch.Tensor
    n_steps: int
    token_kl: Optional[torch.Tensor] = None
    token_ratio: Optional[torch.Tensor] = None

    @staticmethod
    def reduce(log_w: torch.Tensor, present: torch.Tensor):
        """(elbo, iwae, ess) over the last axis of log_w; zeros where `present` is False."""
        K = log_w.size(-1)
        lse = torch.logsumexp(log_w, -1)
        elbo, iwae = log_w.mean(-1), lse - math.log(K)
        ess = torch.exp(2 * lse - torch.logsumexp(2 * log_w, -1))
        zero = torch.zeros_like(elbo)
        return torch.where(present, elbo, zero), torch.where(present, iwae, zero), torch.where(present, ess, zero)

    @staticmethod
    def concat(parts: "List[PosteriorScores]") -> "PosteriorScores":
        """The scores of several calls over different images as one (token arrays padded to the longest call with 0)."""
        def cat(name):
            ts = [getattr(p, name) for p in parts]
            if any(t is None for t in ts):
                return None
            L = max(t.size(-1) for t in ts)
            return torch.cat([torch.nn.functional.pad(t, (0, L - t.size(-1))) for t in ts])
        simple = {n: torch.cat([getattr(p, n) for p in parts]) for n in ("log_w", "nll", "log_ratio", "kld", "n_tokens", "elbo", "iwae", "ess")}
        return PosteriorScores(kl_dim=sum(p.kl_dim for p in parts), n_steps=sum(p.n_steps for p in parts), token_kl=cat("token_kl"),
                               token_ratio=cat("token_ratio"), **simple)

    def summary(self, active_threshold: float = 0.01) -> Dict[str, float]:
        """Per scored token (n = sum n_tokens): elbo_nll_per_token = -sum_c elbo / n, iwae_nll_per_token = -sum_c iwae / n (<= the
        former), recon_nll_per_token = sum_c mean_k nll / n, kl_per_token = sum_c mean_k kld / n (closed form, the training KL),
        kl_mc_per_token = -sum_c mean_k log_ratio / n (one-sample estimate against the decode prior; elbo_nll = recon_nll + kl_mc);
        ess_mean over the present captions; active_units = #{j: kl_dim[j] / n_steps > active_threshold nats}."""
        n = float(self.n_tokens.sum().item())
        if n == 0:
            raise ValueError("no caption was scored")
        present = self.n_tokens > 0
        per = lambda t: float(t.double().mean(-1).sum().item()) / n
        return {"n_captions": int(present.sum().item()), "n_tokens": int(n),
                "elbo_nll_per_token": -float(self.elbo.double().sum().item()) / n,
                "iwae_nll_per_token": -float(self.iwae.double().sum().item()) / n,
                "recon_nll_per_token": per(self.nll), "kl_per_token": per(self.kld), "kl_mc_per_token": -per(self.log_ratio),
                "ess_mean": float(self.ess.double()[present].mean().item()),
                "active_units": int((self.kl_dim.double() / max(self.n_steps, 1) > active_threshold).sum().item())}


def posterior_score_captions(eng, feats: torch.Tensor, sentiment: Optional[torch.Tensor], captions: torch.Tensor, n_samples: int, *,
                             eps: Optional[torch.Tensor] = None, obj_means: Optional[torch.Tensor] = None, pad_index: int = 0,
                             max_rows: int = 256, want_steps: bool = False) -> PosteriorScores:
    """Given captions under the POSTERIOR branch of the model: eng a TrainEngine, feats (nimg, R, F), sentiment (nimg,) or None,
    captions (nimg, C, L) int64 in the "padded" layout of score_captions (the words are those before the first pad_index, what
    follows is set to pad; a slot that starts with pad_index is absent: zeros, n_tokens 0, not run).  Every present caption is run
    through TrainEngine.posterior_forward under n_samples noise draws; the rows (image, caption, sample) of the present captions are
    chunked into forwards of at most max_rows rows (plan_posterior_chunks), each trimmed to its longest caption.  The per-row image
    terms are recomputed for every row of an image.  Ids outside [0, V) raise ValueError before anything is launched.
    eps: optional explicit noise (L + 1, nimg * C * n_samples, Z) over ALL slots, rows (image, caption, sample); default: a
    generator of this call's own, seeded by ONE draw of the global CPU generator.  obj_means (nimg, R, Z): SENTIMENT_VAE = 2 only."""
    if captions.dim() != 3 or captions.size(0) != feats.size(0) or captions.size(2) < 1:
        raise ValueError(f"captions must be (nimg, C, L) with nimg = {feats.size(0)}, got {tuple(captions.shape)}")
    d = eng.dims
    nimg, Cc, L0 = captions.shape
    K = int(n_samples)
    caps = captions.to("cpu", torch.int64)
    is_pad = caps == pad_index
    length = torch.where(is_pad.any(-1), is_pad.float().argmax(-1), torch.full((nimg, Cc), L0))   # words before the first pad
    caps = torch.where(torch.arange(L0).view(1, 1, -1) >= length.unsqueeze(-1), torch.full_like(caps, pad_index), caps)
    chunks = plan_posterior_chunks(length.view(-1).tolist(), K, max_rows)
    if not chunks:
        raise ValueError("every caption slot is absent")
    words = caps[length > 0]
    bad = (words < 0) | (words >= d.V)
    if bool(bad.any()):
        raise ValueError(f"caption ids outside the vocabulary [0, {d.V}): e.g. {int(words[bad][0])}")
    dev = feats.device
    G = nimg * Cc * K
    T0 = L0 + 1
    if eps is not None:
        if tuple(eps.shape) != (T0, G, d.Z):
            raise ValueError(f"eps must be (L + 1, nimg * C * n_samples, Z) = {(T0, G, d.Z)}, got {tuple(eps.shape)}")
        eps = eps.to(dev, torch.float32)
    else:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        eps = torch.randn(T0, G, d.Z, device=dev, generator=gen)
    flat = {n: torch.zeros(nimg * Cc, K, device=dev) for n in ("log_w", "nll", "log_ratio", "kld")}
    tok = {n: torch.zeros(nimg * Cc, K, T0, device=dev) for n in (("token_kl", "token_ratio") if want_steps else ())}
    kl_dim = torch.zeros(d.Z, dtype=torch.float64)
    col = torch.empty(d.Z, device=dev)
    caps_dev = caps.view(nimg * Cc, L0).to(dev)
    for slots, Lc in chunks:
        sl = torch.tensor(slots, device=dev)
        rows = (sl.view(-1, 1) * K + torch.arange(K, device=dev).view(1, -1)).reshape(-1)   # rows of eps: (slot, sample)
        img = (sl // Cc).repeat_interleave(K)
        n = rows.numel()
        out = eng.posterior_forward(feats.index_select(0, img).to(torch.float32).contiguous(),
                                    caps_dev.index_select(0, sl).repeat_interleave(K, 0)[:, :Lc].contiguous(),
                                    sentiment.reshape(nimg).to(dev, torch.float32).index_select(0, img) if sentiment is not None else None,
                                    eps[: Lc + 1].index_select(1, rows).contiguous(),
                                    obj_means.to(dev, torch.float32).index_select(0, img) if obj_means is not None else None)
        nll, kld, log_ratio, log_w, kd, step_kl, step_ratio = out
        for name, v in (("log_w", log_w), ("nll", nll), ("log_ratio", log_ratio), ("kld", kld)):
            flat[name][sl] = v.view(-1, K)
        if want_steps:
            tok["token_kl"][sl, :, : Lc + 1] = step_kl.t().reshape(-1, K, Lc + 1)
            tok["token_ratio"][sl, :, : Lc + 1] = step_ratio.t().reshape(-1, K, Lc + 1)
        # the per-dimension total of the chunk's rows on the device, the chunks summed on the host in float64
        eng.lib.ssc_colsum(_lib.ptr(kd), d.Z, n, d.Z, None, _lib.ptr(col), 1, 0, _lib.stream_ptr())
        kl_dim += col.double().cpu()
    n_tokens = torch.where(length > 0, length + 1, torch.zeros_like(length)).to(dev)
    log_w = flat["log_w"].view(nimg, Cc, K)
    elbo, iwae, ess = PosteriorScores.reduce(log_w, n_tokens > 0)
    shape4 = lambda t: t.view(nimg, Cc, K, T0)
    return PosteriorScores(log_w=log_w, nll=flat["nll"].view(nimg, Cc, K), log_ratio=flat["log_ratio"].view(nimg, Cc, K),
                           kld=flat["kld"].view(nimg, Cc, K), n_tokens=n_tokens, elbo=elbo, iwae=iwae, ess=ess, kl_dim=kl_dim,
                           n_steps=int(n_tokens.sum().item()) * K,
                           token_kl=shape4(tok["token_kl"]) if want_steps else None,
                           token_ratio=shape4(tok["token_ratio"]) if want_steps else None)
