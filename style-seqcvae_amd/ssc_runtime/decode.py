"""Eval-mode decode step + constrained beam search over the C ABI (ssc_decode_*, ssc_beam_*).

Reference: UpDownCaptioner._decode_step eval branch (var_updown/var_updown/models/updown_captioner.py:371-455),
ConstrainedBeamSearch.search (updown-baseline/updown/modules/cbs.py:59-277).
"""
import ctypes as C
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import torch

from . import lib as _lib
from .engine import ModelDims

STATE_KEYS = ("h1", "c1", "h_encoder", "c_encoder", "h_decoder", "c_decoder")


class ImageContext:
    """Per-image terms computed once per image set (mask, avg, pv, hoisted gate term): ssc_decode_prepare."""

    def __init__(self, feats: torch.Tensor, buf: torch.Tensor, obj: Optional[torch.Tensor] = None):
        self.feats = feats
        self.buf = buf
        self.obj = obj   # SENTIMENT_VAE = 2: per-region attribute means (nimg, R, Z) of these images (updown_cell.py:160-163)
        self.nimg, self.R, _ = feats.shape
        self.att_table_ready = False   # the per-image attended-feature table is formed by the first step that uses it


class AttentionRecord(NamedTuple):
    """The attention trace a one-call decode leaves with attention=True (ssc_attn_record, include/ssc.h): hist (steps, rows, R) - step
    t's attention weights in that step's row order - and anc (rows, steps) int32 - the row of slab t behind word t of returned
    caption q, -1 where the word read nothing.  Captions are numbered as the call returns them, flattened.  Read it with
    DecodeEngine.attention."""
    hist: torch.Tensor
    anc: torch.Tensor
    rows: int
    R: int
    steps: int


class AttentionTrace(NamedTuple):
    """What DecodeEngine.attention reads from a record, per selected caption and step: maps (..., steps, R) - the word's attention
    over the regions, exact zeros where it read nothing -, top_region (..., steps) int32 (-1 there), top_weight and entropy
    (..., steps) in nats (0 there).  The parts not asked for are None."""
    maps: Optional[torch.Tensor]
    top_region: Optional[torch.Tensor]
    top_weight: Optional[torch.Tensor]
    entropy: Optional[torch.Tensor]


class DecodeEngine:
    DEFAULT_GEMM_MODE = 3

    def __init__(self, dims: ModelDims, params_struct_fn: Callable[[], "_lib.Params"], device):
        self.lib = _lib.load()
        self.dims = dims
        self.device = torch.device(device)
        self._cfg = dims.cfg()
        # numerics of the decode's products (ssc_model_cfg.gemm_mode).  Default 3: 3xBF16 everywhere except the large (>= 768
        # workgroups of 128x128) NT products - the per-step gate / vocabulary products of a 10000-row call, 80 % of its time -, which
        # take the 2xFP16 form: two fp16 pieces per fp32 operand (scaled by powers of two measured per image context), three
        # partial products instead of six on the matrix cores, 21-22 significant bits per operand instead of 24 (within 2e-6 of
        # sum|a||b| against float64, tests/test_gemm_gpu.py; the reference fixtures of the eval path hold at 1e-4 / identical
        # captions).  1 = 3xBF16 only, 2 = exact-fp32 MFMA; an engine-wide dims.gemm_mode other than 0 wins.
        if self._cfg.gemm_mode == 0:
            self._cfg.gemm_mode = self.DEFAULT_GEMM_MODE
        self._params = params_struct_fn
        self._ws = None
        self._ws_key = None
        # weights_frozen: the caller's promise that the parameters do not change between prepare() calls (an inference run over a
        # loaded checkpoint: scripts/inference.py, bench.py's decode leg).  What ssc_decode_prepare derives from the weights alone
        # (the per-token gate table) is then taken over from the previous image context instead of being formed per call.
        # Default off: the drop-in module's eval calls may be interleaved with training steps.
        self.weights_frozen = False
        self._last_ctx = None
        self._sws = None   # workspace of the one-call decodes

    def prepare(self, feats: torch.Tensor, obj_means: Optional[torch.Tensor] = None) -> ImageContext:
        """obj_means (nimg, R, Z): the per-region attribute means of SENTIMENT_VAE = 2 (kld_mode 2), else None."""
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 3 and feats.size(2) == self.dims.F
        feats = feats.contiguous()
        nimg, R, _ = feats.shape
        if self.dims.kld_mode == 2:
            if obj_means is None or tuple(obj_means.shape) != (nimg, R, self.dims.Z):
                raise ValueError(f"SENTIMENT_VAE = 2 needs the per-region attribute means obj_atts ({nimg}, {R}, {self.dims.Z}), got "
                                 f"{None if obj_means is None else tuple(obj_means.shape)}")
            obj_means = obj_means.to(self.device, torch.float32).contiguous()
        else:
            obj_means = None
        nbytes = self.lib.ssc_decode_image_bytes(C.byref(self._cfg), nimg, R)
        buf = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
        p = self._params()
        prev = self._last_ctx if self.weights_frozen else None
        self.lib.ssc_decode_prepare_from(C.byref(self._cfg), C.byref(p), _lib.ptr(feats), nimg, R, _lib.ptr(buf), buf.numel() * 4,
                                         _lib.ptr(prev.buf) if prev is not None else None, prev.nimg if prev is not None else 0,
                                         prev.R if prev is not None else 0, _lib.stream_ptr())
        ctx = ImageContext(feats, buf, obj_means)
        # (kept alive by this reference: the copy above is stream-ordered before anything that could overwrite the old buffer)
        self._last_ctx = ctx if self.weights_frozen else None
        return ctx

    # The attended-feature term of the decoder gates from a per-image table (ssc_decode_step_desc.att_table): worth its one-off
    # product per image context once a step has a few hundred rows that share their image sixteen or more at a time (C4: 5000
    # rows, 100 per image: -13 % per call); below that the K = F segment is cheaper (one image x 100 rows: 3.8 vs 4.7 ms).
    ATT_TABLE_MIN_ROWS = 512
    ATT_TABLE_MIN_ROWS_PER_IMAGE = 16

    def _att_table_fits(self, ctx: "ImageContext", G: int, rpi: int) -> bool:
        return ctx.R <= 128 and G >= self.ATT_TABLE_MIN_ROWS and rpi >= self.ATT_TABLE_MIN_ROWS_PER_IMAGE

    def _att_table_mode(self, ctx: "ImageContext", G: int, rpi: int) -> int:
        if not self._att_table_fits(ctx, G, rpi):
            return 0
        on = C.c_int(1)   # ssc_debug_set("dec_att_table", 0): A/B switch of include/ssc_debug.h
        if self.lib._raw_ssc_debug_get(b"dec_att_table", C.byref(on)) != 0 or not on.value:
            return 0
        if not ctx.att_table_ready:
            ctx.att_table_ready = True
            return 2
        return 1

    def zero_states(self, G: int) -> Dict[str, torch.Tensor]:
        return {k: torch.zeros(G, self.dims.H, dtype=torch.float32, device=self.device) for k in STATE_KEYS}

    def step(self, ctx: ImageContext, tokens: torch.Tensor, states: Optional[Dict[str, torch.Tensor]],
             sentiment: Optional[torch.Tensor], eps: torch.Tensor, want_log_probs: bool = True,
             emb_table: Optional[torch.Tensor] = None, raw_logits: bool = False, prior_mean_out: Optional[torch.Tensor] = None,
             prior_mean: Optional[torch.Tensor] = None, prior_var: Optional[torch.Tensor] = None
             ) -> Tuple[Optional[torch.Tensor], Dict[str, torch.Tensor], torch.Tensor]:
        """One eval decode step for G rows (row g -> image g // (G / nimg)).  Returns (log_probs (G,V) or None,
        new states, alpha (G,R)).  h_encoder / c_encoder are carried through untouched (updown_cell.py:176-203).
        raw_logits: return the un-normalised vocabulary logits instead (for cbs_search(raw_logits=True), which takes the
        log-sum-exp inside its selection kernel: one pass over the (G,V) matrix less per step).
        prior_mean_out (G, Z), SENTIMENT_VAE = 2 only: receives the step's pooled prior mean (what the cell returns, updown_cell.py:231).
        prior_mean / prior_var (G, Z): the caller's own prior instead of the one the configuration implies."""
        d = self.dims
        G = tokens.numel()
        assert G % ctx.nimg == 0, (G, ctx.nimg)
        rpi = G // ctx.nimg
        if states is None:
            states = self.zero_states(G)
        # "_parent" (B, S*beam) int64: set by cbs_search after a beam re-ordering - row g descends from beam parent[g] of its group;
        # beams with the same parent hold identical states (ssc_decode_step_desc.parent: their shared products are formed once)
        parent = states.get("_parent")
        # "_ungathered": the states are the previous call's outputs in ITS row order (cbs_search left out the re-ordering by
        # back-pointer because ungathered_ok() said this call reads them through the parent lists)
        ungathered = bool(states.get("_ungathered", False))
        # "_skip": (running log-probs (B,S,beam), end index) from cbs_search(skip_dead=True): rows without a finite beam and rows
        # whose beam has ended need no step (ssc_decode_step_desc.row_lp)
        skip = states.get("_skip")
        st = {k: v.contiguous() for k, v in states.items() if not k.startswith("_")}
        tokens = tokens.to(torch.int64).contiguous()
        eps = eps.to(self.device, torch.float32).contiguous()
        assert tuple(eps.shape) == (G, d.Z), eps.shape
        sent = sentiment.reshape(G).to(torch.float32).contiguous() if sentiment is not None else None
        key = (G, ctx.R)
        if self._ws_key != key:
            nbytes = self.lib.ssc_decode_step_workspace_bytes(C.byref(self._cfg), G, ctx.R)
            self._ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            self._ws_key = key
        new = {k: torch.empty_like(st[k]) for k in ("h1", "c1", "h_decoder", "c_decoder")}
        alpha = torch.empty(G, ctx.R, dtype=torch.float32, device=self.device)
        lp = torch.empty(G, d.V, dtype=torch.float32, device=self.device) if want_log_probs else None
        pm_in = prior_mean.to(self.device, torch.float32).contiguous() if prior_mean is not None else None
        pv_in = prior_var.to(self.device, torch.float32).contiguous() if prior_var is not None else None
        assert pm_in is None or tuple(pm_in.shape) == (G, d.Z)
        assert pv_in is None or tuple(pv_in.shape) == (G, d.Z)
        att_table = self._att_table_mode(ctx, G, rpi)
        has_parent = parent is not None and parent.numel() == G
        group = parent.shape[-1] if has_parent else 0
        if ungathered and not (has_parent and emb_table is None and
                               self.lib._raw_ssc_decode_ungathered_ok(C.byref(self._cfg), ctx.nimg, G, group, att_table)):
            raise ValueError("un-gathered states handed to a decode step that cannot read them through parent lists")
        desc = _lib.DecodeStepDesc(G, ctx.R, rpi, ctx.feats.data_ptr(), ctx.buf.data_ptr(), tokens.data_ptr(),
                                   sent.data_ptr() if sent is not None else None, eps.data_ptr(),
                                   st["h1"].data_ptr(), st["c1"].data_ptr(), st["h_decoder"].data_ptr(),
                                   st["c_decoder"].data_ptr(), new["h1"].data_ptr(), new["c1"].data_ptr(),
                                   new["h_decoder"].data_ptr(), new["c_decoder"].data_ptr(), alpha.data_ptr(),
                                   lp.data_ptr() if lp is not None else None, 1 if raw_logits else 0,
                                   1 if emb_table is not None else 0,
                                   parent.data_ptr() if has_parent else None, group, att_table, 1 if ungathered else 0,
                                   skip[0].data_ptr() if skip is not None else None, int(skip[1]) if skip is not None else 0,
                                   ctx.obj.data_ptr() if ctx.obj is not None else None,
                                   prior_mean_out.data_ptr() if (prior_mean_out is not None and ctx.obj is not None) else None,
                                   _lib.ptr(pm_in), _lib.ptr(pv_in))
        p = self._params()
        if emb_table is not None:  # rows of `emb_table` are the token embeddings themselves (UpDownCell.forward API)
            p.emb = emb_table.data_ptr()
            p.ld_emb = emb_table.stride(0)
        self.lib.ssc_decode_step(C.byref(self._cfg), C.byref(p), C.byref(desc), _lib.ptr(self._ws), self._ws.numel() * 4,
                                 _lib.stream_ptr())
        out_states = dict(st)
        out_states.update(new)
        return lp, out_states, alpha

    def ungathered_ok(self, ctx: ImageContext, G: int, group: int) -> bool:
        """May a step of G rows in groups of `group` beams over `ctx` take its previous states in the previous step's row order
        (states["_ungathered"], with the back-pointers in states["_parent"])?  For cbs_search(ungathered_ok=...)."""
        if G % ctx.nimg != 0:
            return False
        # (same decision as step(): the table must be in use; it has been formed by the time a search re-orders beams)
        att = 1 if self._att_table_fits(ctx, G, G // ctx.nimg) else 0
        return bool(self.lib._raw_ssc_decode_ungathered_ok(C.byref(self._cfg), ctx.nimg, G, group, att))


    def _noise(self, sentiment, eps0, eps, first_rows: int, rows: int, steps: int):
        """The caller's sentiment (first_rows), eps0 (first_rows, Z) and eps (steps - 1, rows, Z) as contiguous float32 on the device,
        shape-checked; eps is None for a one-step call."""
        dev, Z = self.device, self.dims.Z
        sent = sentiment.reshape(first_rows).to(dev, torch.float32).contiguous() if sentiment is not None else None
        eps0 = eps0.to(dev, torch.float32).contiguous()
        assert tuple(eps0.shape) == (first_rows, Z), (eps0.shape, (first_rows, Z))
        if steps <= 1:
            return sent, eps0, None
        eps = eps.to(dev, torch.float32).contiguous()
        assert tuple(eps.shape) == (steps - 1, rows, Z), (eps.shape, (steps - 1, rows, Z))
        return sent, eps0, eps

    def _workspace(self, nbytes: int):
        """-> (workspace, bytes, stream): the trailing arguments of a one-call decode; the workspace only ever grows."""
        if self._sws is None or self._sws.numel() < nbytes:
            self._sws = None   # (release before growing)
            self._sws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return _lib.ptr(self._sws), self._sws.numel(), _lib.stream_ptr()

    def _attn_record(self, steps: int, rows: int, R: int):
        """-> (AttentionRecord over fresh buffers, its ssc_attn_record): the caller keeps both alive until the call is queued."""
        rec = AttentionRecord(torch.empty(steps, rows, R, dtype=torch.float32, device=self.device),
                              torch.empty(rows, steps, dtype=torch.int32, device=self.device), rows, R, steps)
        return rec, _lib.AttnRecord(rec.hist.data_ptr(), rec.anc.data_ptr())

    def attention(self, record: AttentionRecord, sel: Optional[torch.Tensor] = None, maps: bool = True,
                  summary: bool = True) -> AttentionTrace:
        """Read an attention record (ssc_attn_gather): for every caption of `sel` - int64 indices into the call's captions in the
        order it returned them, flattened; any shape; None: all of them - and every step the attention map (maps=True) and / or its
        arg-max region, the weight there and the entropy (summary=True).  An index outside the call's captions gives a zero row.
        -> AttentionTrace with tensors of shape sel.shape + (steps,) (+ (R,) for the maps)."""
        if not (maps or summary):
            raise ValueError("DecodeEngine.attention: nothing asked for (maps and summary both off)")
        dev = self.device
        if sel is None:
            shape, n, sel_t = (record.rows,), record.rows, None
        else:
            sel_t = sel.to(dev, torch.int64).contiguous()
            shape, n = tuple(sel_t.shape), sel_t.numel()
        steps, R = record.steps, record.R
        m = torch.empty(*shape, steps, R, dtype=torch.float32, device=dev) if maps else None
        top = torch.empty(*shape, steps, dtype=torch.int32, device=dev) if summary else None
        wgt = torch.empty(*shape, steps, dtype=torch.float32, device=dev) if summary else None
        ent = torch.empty(*shape, steps, dtype=torch.float32, device=dev) if summary else None
        if n > 0:
            d = _lib.AttnGatherDesc(record.hist.data_ptr(), record.rows, R, steps, record.anc.data_ptr(), record.rows,
                                    _lib.ptr(sel_t), n, _lib.ptr(m), R, _lib.ptr(top), _lib.ptr(wgt), _lib.ptr(ent))
            self.lib.ssc_attn_gather(C.byref(d), _lib.stream_ptr())
        return AttentionTrace(m, top, wgt, ent)

    def _one_call(self, ctx, sentiment, n_samples, S, beam, per_node, max_steps, end_index, eps0, eps, early_stop, skip_dead,
                  out_shape, workspace_bytes, call, machine=None, attention=False, start=None):
        """The shared body of the one-call decodes over a search descriptor: B = ctx.nimg * n_samples batch entries of S * beam
        rows.  Fills the descriptor (machine(desc) adds a search's machine fields), checks the noise, allocates the outputs -
        predictions out_shape + (max_steps,), log-probs out_shape -, takes the pinned early-stop flag, sizes the workspace with
        workspace_bytes(cfg, desc) and issues call(params, desc, (workspace, bytes, stream)).
        -> (predictions cut to the executed steps, log_probs[, AttentionRecord over max_steps steps with attention=True]); one wait
        at the end, for the number of steps.  start: a StartState (ssc_runtime.prefix, DecodeEngine.prime) over the B entries, or
        None - the call then starts from its states and its tokens (ssc_search_desc.start) and returns the continuation."""
        B = ctx.nimg * n_samples
        dev = self.device
        sd = _lib.SearchDesc()
        if start is not None:
            sdesc, _keep_start = start.desc(dev, B, self.dims.H)
            sd.start = C.pointer(sdesc)
        sd.nimg, sd.R, sd.n_samples = ctx.nimg, ctx.R, n_samples
        sd.S, sd.beam, sd.per_node, sd.max_steps, sd.end_index = S, beam, per_node, max_steps, end_index
        sd.feats, sd.imgbuf = ctx.feats.data_ptr(), ctx.buf.data_ptr()
        sent, eps0, eps = self._noise(sentiment, eps0, eps, B, B * S * beam, max_steps)
        sd.sentiment, sd.eps0, sd.eps = _lib.ptr(sent), _lib.ptr(eps0), _lib.ptr(eps)
        sd.obj_atts = _lib.ptr(ctx.obj)
        if machine is not None:
            machine(sd)
        sd.skip_dead = 1 if skip_dead else 0
        sd.early_stop = 1 if early_stop else 0
        pred = torch.empty(*out_shape, max_steps, dtype=torch.int64, device=dev)
        lps = torch.empty(*out_shape, dtype=torch.float32, device=dev)
        ctl = torch.empty(2 + 2 * max_steps, dtype=torch.int32, device=dev)
        sd.predictions, sd.log_probs, sd.ctl = _lib.ptr(pred), _lib.ptr(lps), _lib.ptr(ctl)
        flag = None
        if early_stop:
            flag, flag_dev = _host_flag()
            if flag_dev is not None:
                sd.host_flag, sd.host_flag_host = flag_dev, C.c_void_p(flag.data_ptr())
        rec = arec = None
        if attention:
            rec, arec = self._attn_record(max_steps, B * S * beam, ctx.R)
            sd.attn = C.pointer(arec)
        ws = self._workspace(workspace_bytes(C.byref(self._cfg), C.byref(sd)))
        call(self._params(), sd, ws)
        nsteps = int(ctl[0]) if early_stop else max_steps   # (the one wait of the call: its result is about to be read anyway)
        if flag is not None:
            _HOST_FLAGS.append(flag)
        if attention:
            return pred[..., :nsteps].contiguous(), lps, rec
        return pred[..., :nsteps].contiguous(), lps

    def _guide_desc(self, guide, B: int):
        """-> (ssc_latent_guide, the tensors behind it) of a LatentGuide (ssc_runtime.guide) for a call of B entries, refused on the
        host where the library would refuse it."""
        if self.dims.kld_mode == 2:
            raise NotImplementedError("latent guides (guide=) are not implemented for SENTIMENT_VAE = 2: the pooled prior mean there also "
                                      "conditions the LSTMs")
        return guide.desc(self.device, B, self.dims.Z)

    def search(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int, max_steps: int,
               end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], fsm: Optional[torch.Tensor] = None,
               compiled: Optional["CompiledFsm"] = None, mach: Optional[torch.Tensor] = None, skip_dead: bool = False,
               early_stop: bool = True, attention: bool = False, guide=None, start=None):
        """The whole constrained beam search of one call in ONE library call (ssc_decode_search): ctx.nimg images x n_samples
        latent samples, batch entry b = (image, sample).  sentiment (B) or None; eps0 (B, Z), eps (max_steps - 1, B*S*beam, Z):
        the noise of every step, drawn by the caller.  fsm (M,S,S,V) / compiled / mach as in cbs_search.
        -> (predictions (B, S, beam, steps), log_probs (B, S, beam)); one wait at the end, for the number of steps.
        attention=True (here and on every one-call decode below): additionally an AttentionRecord of the call's captions in the
        order returned (caption q = the flattened index of the predictions' leading dimensions), for DecodeEngine.attention.
        guide: a LatentGuide (ssc_runtime.guide) over the B entries, or None - step t's latent of entry b is then drawn around
        guide.mean[t, b] instead of the prior (ssc_decode_search_guided); eps0 / eps are still the noise (unread where the guide has
        no variance).
        start: a StartState (DecodeEngine.prime), or None - the search starts from its states and tokens instead of zero states and
        @@BOUNDARY@@ and returns the CONTINUATION: the machine starts in its start state, max_steps bounds the continuation, the
        log-probs are the continuation's (here and on every decode below; ssc_runtime.prefix.join_prefix adds the prefix).  Not
        together with a guide."""
        _start_check(start, guide)
        call = lambda p, sd, ws: self.lib.ssc_decode_search(C.byref(self._cfg), C.byref(p), C.byref(sd), *ws)
        if guide is not None:
            gd, _keep = self._guide_desc(guide, ctx.nimg * n_samples)
            call = lambda p, sd, ws: self.lib.ssc_decode_search_guided(C.byref(self._cfg), C.byref(p), C.byref(sd), C.byref(gd), *ws)
        return self._search(ctx, sentiment, n_samples, beam, per_node, max_steps, end_index, eps0, eps, fsm, compiled, mach, skip_dead,
                            early_stop, attention, self.lib.ssc_decode_search_workspace_bytes, call, start=start)

    def _search(self, ctx, sentiment, n_samples, beam, per_node, max_steps, end_index, eps0, eps, fsm, compiled, mach, skip_dead,
                early_stop, attention, workspace_bytes, call, start=None):
        """The body of search(): the machine's checks and descriptor fields around _one_call, for the entry point `call` and its
        `workspace_bytes` (ssc_decode_search; ssc_decode_search_ensemble for EnsembleDecodeEngine.search)."""
        B = ctx.nimg * n_samples
        S = 1 if fsm is None else fsm.size(1)
        if fsm is not None:
            assert fsm.is_cuda and fsm.dtype == torch.uint8 and fsm.is_contiguous()
            assert mach is not None or fsm.size(0) == B
        if mach is not None:   # one machine index per BATCH ENTRY (image, sample); the kernels index the machines with it unchecked
            assert fsm is not None and mach.numel() == B, (mach.shape, B)
            lo, hi = int(mach.min()), int(mach.max())
            assert 0 <= lo and hi < fsm.size(0), (lo, hi, fsm.size(0))
            mach = mach.to(self.device, torch.int32).contiguous()
        if compiled is not None:
            assert compiled.dims.S == S and compiled.dims.P >= per_node

        def machine(sd):
            sd.fsm, sd.mach = _lib.ptr(fsm), _lib.ptr(mach)
            if compiled is not None:
                sd.tables, sd.dims = _lib.ptr(compiled.tables), compiled.dims

        return self._one_call(ctx, sentiment, n_samples, S, beam, per_node, max_steps, end_index, eps0, eps, early_stop,
                              skip_dead and (compiled is not None or fsm is None), (B, S, beam), workspace_bytes, call,
                              machine, attention=attention, start=start)

    def sample(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, max_steps: int, end_index: int,
               eps0: torch.Tensor, eps: Optional[torch.Tensor], sampler, seed: int, early_stop: bool = True,
               attention: bool = False, guide=None, logit_rules=None, skip_dead: bool = True, start=None, truncation=None,
               truncation_stats: bool = False, contrast=None, contrast_stats: bool = False, mirostat=None,
               mirostat_stats: bool = False, arithmetic=None, arithmetic_codes: bool = False):
        """The whole sampled decode of one call in ONE library call (ssc_decode_sample_opts): ctx.nimg images x n_samples latent samples,
        one row per batch entry b = (image, sample), one word per row and step drawn by `sampler` (ssc_runtime.sampling) with the
        64-bit `seed`.  sentiment (B) or None; eps0 (B, Z), eps (max_steps - 1, B, Z): the noise of every step.
        -> (predictions (B, steps) int64, log_probs (B,): each caption's summed untempered log-prob).
        guide: a LatentGuide over the B entries, or None (ssc_sample_opts.guide; see search).
        logit_rules: a sampling.LogitRules, or None - every step's raw logits are edited in front of the draw
        (ssc_sample_opts.rules: word bias, repetition / presence / frequency penalties, n-gram / length / token bans) and the
        log-probs are those under the edited distributions; None or inactive rules leave the field NULL.
        truncation: a sampling.Truncation, or None - every step's raw logits are cut between the logit rules and the draw
        (ssc_sample_opts.trunc: typical, min-p, eta or epsilon truncation of the distribution tempered by the sampler's
        temperature); None or an inactive one issues the call without it.  truncation_stats=True (with an active truncation):
        the result is followed by (entropy (B, steps) float32 in nats, kept (B, steps) int32 - the entries left finite), zero
        for ended rows and in the columns past the stop.
        contrast: a contrast.Contrast, or None - contrastive decoding (ssc_sample_opts.contrast): an amateur stream is decoded in
        lock-step with this one, fed the same words, and every step's raw logits are contrasted with the amateur's in front of the
        logit rules; None or an inactive one issues the call without it.  With start= the Contrast carries the amateur's own
        StartState (Contrast.start).  contrast_stats=True (with an active contrast): the result is followed - behind the
        truncation's statistics - by (kept (B, steps) int32 - the words left plausible -, divergence (B, steps) float32 - the KL
        of the expert's word distribution from the amateur's, in nats), zero for ended rows and in the columns past the stop.
        mirostat: a sampling.Mirostat, or None - the surprise of the drawn words is held at its target by feedback
        (ssc_decode_sample_mirostat: a cut behind the truncation with the row's running threshold mu, an update of mu behind the
        draw); None or an inactive one issues ssc_decode_sample_opts as before.  mirostat_stats=True (with an active Mirostat): the
        result is followed - behind the other statistics - by (mu (B, steps) float32 - the threshold step t cut with -, surprise
        (B, steps) float32 - the drawn word's surprise under the tempered distribution in front of the cut -, kept (B, steps) int32),
        mu and surprise in the object's unit; surprise and kept are zero for ended rows, all three in the columns past the stop.
        arithmetic: a sampling.Arithmetic, or None - the draw of every step is made by inverse CDF along a code point per row
        (ssc_decode_sample_arith), the codes a randomly shifted lattice per image that `seed` decides, or the object's own; None
        issues the call of before.  arithmetic_codes=True (with an arithmetic): the result is followed - behind the other
        statistics - by the codes (B, steps + 1) int64 holding the uint64 bits: column t is the code step t drew with, column
        t + 1 the code it left; zero past the stop.
        skip_dead (default on): ended rows are not stepped; the captions do not depend on it."""
        _start_check(start, guide)
        if arithmetic_codes and arithmetic is None:
            raise ValueError("DecodeEngine.sample: arithmetic_codes needs an arithmetic")
        if mirostat is not None and not mirostat.active:
            mirostat = None
        if mirostat_stats and mirostat is None:
            raise ValueError("DecodeEngine.sample: mirostat_stats needs an active mirostat")
        if contrast is not None and not contrast.active:
            contrast = None
        if contrast_stats and contrast is None:
            raise ValueError("DecodeEngine.sample: contrast_stats needs an active contrast")
        if truncation is not None and not truncation.active:
            truncation = None
        if truncation_stats and truncation is None:
            raise ValueError("DecodeEngine.sample: truncation_stats needs an active truncation")
        sampler.check_vocab(self.dims.V)
        sdesc = sampler.desc(seed)
        B = ctx.nimg * n_samples
        # one descriptor for the call's options; every object behind a field stays alive in `keep` until the call has returned
        opts = _lib.SampleOpts(bytes=C.sizeof(_lib.SampleOpts))
        keep = []
        if guide is not None:
            gd, _keep = self._guide_desc(guide, B)
            opts.guide = C.pointer(gd)
            keep += [gd, _keep]
        if logit_rules is not None and logit_rules.active:
            logit_rules.check(self.dims.V, end_index, max_steps, ctx.nimg)
            rd, _keep = logit_rules.desc(n_samples)
            opts.rules = C.pointer(rd)
            keep += [rd, _keep]
        ent = kept = None
        if truncation is not None:
            if truncation_stats:   # (max_steps, B) blocks; slabs of steps never queued stay zero
                ent = torch.zeros(max_steps, B, dtype=torch.float32, device=self.device)
                kept = torch.zeros(max_steps, B, dtype=torch.int32, device=self.device)
            td = truncation.desc(ent, kept)
            opts.trunc = C.pointer(td)
            keep.append(td)
        ckept = cdiv = None
        if contrast is not None:
            if contrast_stats:   # (max_steps, B) blocks; slabs of steps never queued stay zero
                ckept = torch.zeros(max_steps, B, dtype=torch.int32, device=self.device)
                cdiv = torch.zeros(max_steps, B, dtype=torch.float32, device=self.device)
            cd, _keep = contrast.desc(self, ctx, n_samples, max_steps, start is not None, ckept, cdiv)
            opts.contrast = C.pointer(cd)
            keep += [cd, _keep]
        call = lambda p, sd, ws: self.lib.ssc_decode_sample_opts(C.byref(self._cfg), C.byref(p), C.byref(sd), C.byref(sdesc),
                                                                 C.byref(opts), *ws)
        workspace_bytes = lambda cfg, sd: self.lib.ssc_decode_sample_opts_workspace_bytes(cfg, sd, C.byref(opts))
        if mirostat is not None:   # the descriptor beside the opts; mu (max_steps + 1, B); slabs of steps never queued stay zero
            mmu = torch.zeros(max_steps + 1, B, dtype=torch.float32, device=self.device)
            msur = torch.zeros(max_steps, B, dtype=torch.float32, device=self.device) if mirostat_stats else None
            mkept = torch.zeros(max_steps, B, dtype=torch.int32, device=self.device) if mirostat_stats else None
            md = mirostat.desc(mmu, msur, mkept)
            call = lambda p, sd, ws: self.lib.ssc_decode_sample_mirostat(C.byref(self._cfg), C.byref(p), C.byref(sd), C.byref(sdesc),
                                                                         C.byref(opts), C.byref(md), *ws)
            workspace_bytes = lambda cfg, sd: self.lib.ssc_decode_sample_mirostat_workspace_bytes(cfg, sd, C.byref(opts), C.byref(md))
        if arithmetic is not None:   # the descriptor beside the opts and Mirostat's (NULL when off); code (max_steps + 1, B)
            acode = torch.zeros(max_steps + 1, B, dtype=torch.int64, device=self.device)
            ad = arithmetic.desc(acode)
            mref = C.byref(md) if mirostat is not None else None
            aref = C.byref(ad) if ad is not None else None
            call = lambda p, sd, ws: self.lib.ssc_decode_sample_arith(C.byref(self._cfg), C.byref(p), C.byref(sd), C.byref(sdesc),
                                                                      C.byref(opts), mref, aref, *ws)
            workspace_bytes = lambda cfg, sd: self.lib.ssc_decode_sample_arith_workspace_bytes(cfg, sd, C.byref(opts), mref, aref)
        out = self._one_call(ctx, sentiment, n_samples, 1, 1, 1, max_steps, end_index, eps0, eps, early_stop, skip_dead,
                             (ctx.nimg * n_samples,), workspace_bytes, call, attention=attention, start=start)
        if truncation_stats:
            steps = out[0].size(-1)
            out = tuple(out) + ((ent[:steps].t().contiguous(), kept[:steps].t().contiguous()),)
        if contrast_stats:
            steps = out[0].size(-1)
            out = tuple(out) + ((ckept[:steps].t().contiguous(), cdiv[:steps].t().contiguous()),)
        if mirostat_stats:
            steps = out[0].size(-1)
            out = tuple(out) + ((mirostat.from_nats(mmu[:steps].t().contiguous()), mirostat.from_nats(msur[:steps].t().contiguous()),
                                 mkept[:steps].t().contiguous()),)
        if arithmetic_codes:
            steps = out[0].size(-1)
            out = tuple(out) + (acode[:steps + 1].t().contiguous(),)
        return out

    def score(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], targets: torch.Tensor, n_samples: int, end_index: int,
              eps0: torch.Tensor, eps: Optional[torch.Tensor], want_tokens: bool = False, want_ranks: bool = False,
              attention: bool = False, guide=None):
        """The teacher-forced decode of GIVEN captions in ONE library call (ssc_decode_score): targets (nimg, C, L) int64 - the
        caption's words, then end_index from its end on; a slot whose first entry is negative is absent - scored under n_samples
        latent samples each, row g = (image, caption, sample), G = nimg * C * n_samples.  sentiment (G) per row or None; eps0
        (G, Z), eps (L - 1, G, Z): the noise of every step.
        -> (log_probs (G,), n_tokens (nimg, C) int32, token_lp (G, L) or None, token_rank (G, L) int32 or None[, AttentionRecord
        of the G rows over L steps with attention=True]).
        guide: a LatentGuide over the G rows, or None (ssc_decode_score_guided; see search)."""
        dev = self.device
        assert targets.dim() == 3 and targets.size(0) == ctx.nimg, (targets.shape, ctx.nimg)
        _, Cc, Lc = targets.shape
        G = ctx.nimg * Cc * n_samples
        targets = targets.to(dev, torch.int64).contiguous()
        sd = _lib.ScoreDesc()
        sd.nimg, sd.R, sd.n_captions, sd.n_samples, sd.max_len, sd.end_index = ctx.nimg, ctx.R, Cc, n_samples, Lc, end_index
        sd.feats, sd.imgbuf = ctx.feats.data_ptr(), ctx.buf.data_ptr()
        sent, eps0, eps = self._noise(sentiment, eps0, eps, G, G, Lc)
        sd.sentiment, sd.obj_atts, sd.targets = _lib.ptr(sent), _lib.ptr(ctx.obj), _lib.ptr(targets)
        sd.eps0, sd.eps = _lib.ptr(eps0), _lib.ptr(eps)
        lps = torch.empty(G, dtype=torch.float32, device=dev)
        ntok = torch.empty(ctx.nimg, Cc, dtype=torch.int32, device=dev)
        tlp = torch.empty(G, Lc, dtype=torch.float32, device=dev) if want_tokens else None
        trk = torch.empty(G, Lc, dtype=torch.int32, device=dev) if want_ranks else None
        sd.log_probs, sd.n_tokens, sd.token_lp, sd.token_rank = _lib.ptr(lps), _lib.ptr(ntok), _lib.ptr(tlp), _lib.ptr(trk)
        rec = arec = None
        if attention:
            rec, arec = self._attn_record(Lc, G, ctx.R)
            sd.attn = C.pointer(arec)
        ws = self._workspace(self.lib.ssc_decode_score_workspace_bytes(C.byref(self._cfg), C.byref(sd)))
        p = self._params()
        if guide is not None:
            gd, _keep = self._guide_desc(guide, G)
            self.lib.ssc_decode_score_guided(C.byref(self._cfg), C.byref(p), C.byref(sd), C.byref(gd), *ws)
        else:
            self.lib.ssc_decode_score(C.byref(self._cfg), C.byref(p), C.byref(sd), *ws)
        if attention:
            return lps, ntok, tlp, trk, rec
        return lps, ntok, tlp, trk

    def prime(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, prefix, end_index: int, eps: torch.Tensor,
              want_tokens: bool = False):
        """Teacher-force a prefix on the B = ctx.nimg * n_samples rows of a call in ONE library call (ssc_decode_prime) and return
        the StartState (ssc_runtime.prefix) the searches and the sampled decode take as start=.  prefix: a DecodePrefix or an
        int64 tensor, (nimg, Lp) - expanded over the samples - or (B, Lp), padded with -1; a row's prefix ends at its first id
        outside [0, V) or equal to end_index.  sentiment (B) or None; eps (Lp, B, Z): the noise of the prefix's steps.  A row
        without a prefix gets the start of an unprefixed call (zero states, end_index, log-prob 0).
        want_tokens: the StartState carries token_lp (B, Lp)."""
        from .prefix import DecodePrefix, StartState
        dev, d = self.device, self.dims
        B = ctx.nimg * n_samples
        ids = prefix.ids if isinstance(prefix, DecodePrefix) else DecodePrefix(prefix).ids
        if ids.size(0) == ctx.nimg and n_samples > 1:
            ids = ids.repeat_interleave(n_samples, 0)
        if ids.size(0) != B:
            raise ValueError(f"prime: the prefix has {ids.size(0)} rows; this call has {ctx.nimg} images and {B} entries")
        ids = ids.to(dev, torch.int64).contiguous()
        Lp = ids.size(1)
        eps = eps.to(dev, torch.float32).contiguous()
        if tuple(eps.shape) != (Lp, B, d.Z):
            raise ValueError(f"prime: eps must be (Lp, B, Z) = {(Lp, B, d.Z)}, got {tuple(eps.shape)}")
        sent = sentiment.reshape(B).to(dev, torch.float32).contiguous() if sentiment is not None else None
        pd = _lib.PrimeDesc()
        pd.nimg, pd.R, pd.n_samples, pd.max_len, pd.end_index = ctx.nimg, ctx.R, n_samples, Lp, end_index
        pd.feats, pd.imgbuf = ctx.feats.data_ptr(), ctx.buf.data_ptr()
        pd.sentiment, pd.obj_atts, pd.prefix, pd.eps = _lib.ptr(sent), _lib.ptr(ctx.obj), _lib.ptr(ids), _lib.ptr(eps)
        st = [torch.empty(B, d.H, dtype=torch.float32, device=dev) for _ in range(4)]
        tok = torch.empty(B, dtype=torch.int64, device=dev)
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        lps = torch.empty(B, dtype=torch.float32, device=dev)
        tlp = torch.empty(B, Lp, dtype=torch.float32, device=dev) if want_tokens else None
        pd.h1, pd.c1, pd.hd, pd.cd = [_lib.ptr(t) for t in st]
        pd.tokens, pd.lengths, pd.log_probs, pd.token_lp = _lib.ptr(tok), _lib.ptr(lens), _lib.ptr(lps), _lib.ptr(tlp)
        ws = self._workspace(self.lib.ssc_decode_prime_workspace_bytes(C.byref(self._cfg), C.byref(pd)))
        p = self._params()
        self.lib.ssc_decode_prime(C.byref(self._cfg), C.byref(p), C.byref(pd), *ws)
        return StartState(st[0], st[1], st[2], st[3], tok, lens, lps, tlp)

    def stochastic_beam(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int,
                        max_steps: int, end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], sampler, seed: int,
                        early_stop: bool = True, skip_dead: bool = True, attention: bool = False, guide=None, start=None):
        """The whole stochastic beam search of one call in ONE library call (ssc_decode_stochastic_beam): ctx.nimg images x n_samples
        latent samples, batch entry b = (image, sample), `beam` captions per entry sampled without replacement by `sampler`
        (sampling.GumbelSampler) with the 64-bit `seed`, per_node candidates per beam.  sentiment (B) or None; eps0 (B, Z),
        eps (max_steps - 1, B*beam, Z): the noise of every step.
        -> (predictions (B, beam, steps) int64, log_probs (B, beam): summed untempered log-probs, descending)."""
        if guide is not None:
            _guide_unsupported('the stochastic beam search (stochastic_beam)')
        if not 1 <= per_node <= beam <= min(32, self.dims.V):
            raise ValueError(f"stochastic beam search needs 1 <= per_node <= beam <= min(32, V), got per_node {per_node}, beam {beam}")
        gdesc = sampler.desc(seed)
        return self._one_call(ctx, sentiment, n_samples, 1, beam, per_node, max_steps, end_index, eps0, eps, early_stop, skip_dead,
                              (ctx.nimg * n_samples, beam),
                               self.lib.ssc_decode_stochastic_beam_workspace_bytes,
                               lambda p, sd, ws: self.lib.ssc_decode_stochastic_beam(C.byref(self._cfg), C.byref(p), C.byref(sd),
                                                                                     C.byref(gdesc), *ws),
                              attention=attention, start=start)

    def sampled_beam(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int,
                     max_steps: int, end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], sampler, seed: int,
                     early_stop: bool = True, skip_dead: bool = True, attention: bool = False, guide=None, start=None):
        """The whole sampled-node beam search of one call in ONE library call (ssc_decode_sampled_beam): the reference's BeamSearch
        driven by a word sampler (ssc_runtime.sampling: multinomial / top-k / top-p) - step 0 takes the top `beam` tokens, every
        later step draws per_node candidates per beam (with or without replacement, sampler.with_replacement) with the 64-bit
        `seed` and keeps the `beam` best by summed log-prob.  ctx.nimg images x n_samples latent samples, batch entry
        b = (image, sample).  sentiment (B) or None; eps0 (B, Z), eps (max_steps - 1, B*beam, Z): the noise of every step.
        -> (predictions (B, beam, steps) int64, log_probs (B, beam): summed untempered log-probs, descending - beam 0 the best)."""
        if guide is not None:
            _guide_unsupported('the sampled-node beam search (sampled_beam)')
        V = self.dims.V
        if sampler.beam_search:
            raise ValueError("the sampled-node beam search takes a word sampler (multinomial / top-k / top-p); the Gumbel sampler "
                             "runs as DecodeEngine.stochastic_beam")
        if not (1 <= beam <= min(32, V) and 1 <= per_node <= min(32, V)):
            raise ValueError(f"sampled beam search needs 1 <= beam, per_node <= min(32, V), got beam {beam}, per_node {per_node}")
        if sampler.kind == 1 and not per_node <= sampler.k <= V:   # (beam_search.py:180-183)
            raise ValueError("k must be a postive integer no less than per_node_beam_size and no greater than vocabulary size")
        sdesc = sampler.desc(seed)
        rep = 1 if sampler.with_replacement else 0
        return self._one_call(ctx, sentiment, n_samples, 1, beam, per_node, max_steps, end_index, eps0, eps, early_stop, skip_dead,
                              (ctx.nimg * n_samples, beam),
                               self.lib.ssc_decode_sampled_beam_workspace_bytes,
                               lambda p, sd, ws: self.lib.ssc_decode_sampled_beam(C.byref(self._cfg), C.byref(p), C.byref(sd),
                                                                                  C.byref(sdesc), rep, *ws),
                              attention=attention, start=start)

    def diverse_beam(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int,
                     max_steps: int, end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], diverse,
                     early_stop: bool = True, skip_dead: bool = True, attention: bool = False, guide=None, start=None):
        """The whole diverse beam search of one call in ONE library call (ssc_decode_diverse_beam): `beam` beams per batch entry in
        diverse.groups groups (sampling.DiverseBeam), searched in order inside every step with the Hamming penalty
        diverse.strength; per_node candidates per beam.  Deterministic.  ctx.nimg images x n_samples latent samples, batch entry
        b = (image, sample).  sentiment (B) or None; eps0 (B, Z), eps (max_steps - 1, B*beam, Z): the noise of every step.
        -> (predictions (B, beam, steps) int64 group-major, log_probs (B, beam): true summed log-probs, NOT sorted across groups -
        the best caption of an entry is the arg-max)."""
        if guide is not None:
            _guide_unsupported('the diverse beam search (diverse_beam)')
        V = self.dims.V
        if not (1 <= beam <= min(32, V) and 1 <= per_node <= min(32, V)):
            raise ValueError(f"diverse beam search needs 1 <= beam, per_node <= min(32, V), got beam {beam}, per_node {per_node}")
        diverse.check_beam(beam)
        ddesc = diverse.desc()
        return self._one_call(ctx, sentiment, n_samples, 1, beam, per_node, max_steps, end_index, eps0, eps, early_stop, skip_dead,
                              (ctx.nimg * n_samples, beam),
                               lambda cfg, sd: self.lib.ssc_decode_diverse_beam_workspace_bytes(cfg, sd, C.byref(ddesc)),
                               lambda p, sd, ws: self.lib.ssc_decode_diverse_beam(C.byref(self._cfg), C.byref(p), C.byref(sd),
                                                                                  C.byref(ddesc), *ws),
                              attention=attention, start=start)

    def rules_beam(self, ctx: ImageContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int,
                   max_steps: int, end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], rules,
                   early_stop: bool = True, skip_dead: bool = True, attention: bool = False, guide=None, start=None):
        """The whole beam search under the decode rules of one call in ONE library call (ssc_decode_rules_beam): blocking of
        repeated n-grams, a minimum length, suppressed tokens and a length penalty in the ranking (sampling.DecodeRules), applied
        where the selection runs; per_node candidates per beam.  Deterministic.  ctx.nimg images x n_samples latent samples,
        batch entry b = (image, sample).  sentiment (B) or None; eps0 (B, Z), eps (max_steps - 1, B*beam, Z): the noise of every
        step.  -> (predictions (B, beam, steps) int64, log_probs (B, beam): the true summed log-probs, scores (B, beam): the sums
        over the penalty of the captions' lengths, descending - beam 0 is the best caption -, lengths (B, beam) int32: the tokens
        of every caption, the END counted)."""
        if guide is not None:
            _guide_unsupported('the beam search under decode rules (rules_beam)')
        V = self.dims.V
        if not (1 <= beam <= min(32, V) and 1 <= per_node <= min(32, V)):
            raise ValueError(f"the beam search under decode rules needs 1 <= beam, per_node <= min(32, V), got beam {beam}, "
                             f"per_node {per_node}")
        rules.check(V, end_index, max_steps)
        rdesc = rules.desc()
        B = ctx.nimg * n_samples
        scores = torch.empty(B, beam, dtype=torch.float32, device=self.device)
        lengths = torch.empty(B, beam, dtype=torch.int32, device=self.device)
        out = self._one_call(ctx, sentiment, n_samples, 1, beam, per_node, max_steps, end_index, eps0, eps, early_stop,
                             skip_dead, (B, beam), self.lib.ssc_decode_rules_beam_workspace_bytes,
                             lambda p, sd, ws: self.lib.ssc_decode_rules_beam(C.byref(self._cfg), C.byref(p), C.byref(sd),
                                                                              C.byref(rdesc), _lib.ptr(scores),
                                                                              _lib.ptr(lengths), *ws), attention=attention,
                             start=start)
        return (out[0], out[1], scores, lengths) + tuple(out[2:])

    def _step_from_embedding(self, ctx, token_embedding, states, sentiment, eps, prior_mean_out=None, prior_mean=None, prior_var=None):
        G = token_embedding.size(0)
        table = token_embedding.to(self.device, torch.float32).contiguous()
        ids = torch.arange(G, dtype=torch.int64, device=self.device)
        return self.step(ctx, ids, states, sentiment, eps, want_log_probs=False, emb_table=table, prior_mean_out=prior_mean_out,
                         prior_mean=prior_mean, prior_var=prior_var)


DecodeEngine.step_from_embedding = DecodeEngine._step_from_embedding


def _guide_unsupported(what):
    from .guide import guide_unsupported
    guide_unsupported(what)


def _start_check(start, guide):
    """A start state and a latent guide are not combined (include/ssc.h: ssc_start_state)."""
    if start is not None and guide is not None:
        raise NotImplementedError("a start state (start=) together with a latent guide (guide=) is not implemented: a guide's slab t "
                                  "is the step of a caption decoded from @@BOUNDARY@@")


ENSEMBLE_MODES = {"prob": 0, "logprob": 1}


def ensemble_weights(weights, n: int):
    """The members' weights as the library takes them: n positive finite floats, normalised to sum 1 (None: uniform).
    ValueError otherwise."""
    import math
    if weights is None:
        return [1.0 / n] * n
    w = [float(x) for x in weights]
    if len(w) != n:
        raise ValueError(f"ensemble: {len(w)} weights for {n} members")
    if any(not math.isfinite(x) or x <= 0.0 for x in w):
        raise ValueError(f"ensemble: weights must be positive and finite, got {w}")
    total = sum(w)
    return [x / total for x in w]


class EnsembleContext:
    """One ImageContext per member over the same features (EnsembleDecodeEngine.prepare)."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        self.feats, self.obj = self.ctxs[0].feats, self.ctxs[0].obj
        self.nimg, self.R = self.ctxs[0].nimg, self.ctxs[0].R


class EnsembleDecodeEngine:
    """Ensemble decoding: one beam search over several DecodeEngines of one architecture (checkpoints of one configuration), the
    members' word distributions averaged at every step (ssc_decode_search_ensemble).  mode "prob": the weighted mean of the
    members' probabilities; "logprob": the normalised weighted mean of their log-probs.  weights: positive, any scale (None:
    uniform).  Only the beam search runs over an ensemble; the other decodes name the feature they lack."""

    def __init__(self, members, weights=None, mode: str = "prob"):
        members = list(members)
        if not 1 <= len(members) <= _lib.SSC_ENSEMBLE_MAX:
            raise ValueError(f"ensemble: 1 .. {_lib.SSC_ENSEMBLE_MAX} members, got {len(members)}")
        if mode not in ENSEMBLE_MODES:
            raise ValueError(f"ensemble: unknown mode {mode!r} (one of {sorted(ENSEMBLE_MODES)})")
        for m in members[1:]:
            if m.dims != members[0].dims:
                raise ValueError(f"ensemble: members of different architecture: {m.dims} != {members[0].dims}")
            if m._cfg.gemm_mode != members[0]._cfg.gemm_mode or m.device != members[0].device:
                raise ValueError("ensemble: members differ in their numerics mode or their device")
        self.weights = ensemble_weights(weights, len(members))
        self.members = members
        self.mode = mode
        self.dims = members[0].dims
        self.device = members[0].device
        self.lib = members[0].lib
        self._cfg = members[0]._cfg

    @property
    def weights_frozen(self):
        return all(m.weights_frozen for m in self.members)

    @weights_frozen.setter
    def weights_frozen(self, on):
        for m in self.members:
            m.weights_frozen = on

    def prepare(self, feats: torch.Tensor, obj_means: Optional[torch.Tensor] = None) -> EnsembleContext:
        return EnsembleContext([m.prepare(feats, obj_means) for m in self.members])

    def search(self, ctx: EnsembleContext, sentiment: Optional[torch.Tensor], n_samples: int, beam: int, per_node: int,
               max_steps: int, end_index: int, eps0: torch.Tensor, eps: Optional[torch.Tensor], fsm: Optional[torch.Tensor] = None,
               compiled: Optional["CompiledFsm"] = None, mach: Optional[torch.Tensor] = None, skip_dead: bool = False,
               early_stop: bool = True, attention: bool = False, guide=None, start=None):
        """DecodeEngine.search over the ensemble: the same arguments (ctx from this engine's prepare), the same return value."""
        if start is not None:
            raise NotImplementedError("a start state (start=) over an ensemble (EnsembleDecodeEngine) is not implemented: every member "
                                      "would need its own primed states")
        if guide is not None:
            _guide_unsupported("an ensemble (EnsembleDecodeEngine)")
        if attention:
            raise NotImplementedError("attention traces of an ensemble are not implemented (ensemble decoding runs the beam search only)")
        if len(ctx.ctxs) != len(self.members):
            raise ValueError("ensemble: the context was not prepared by this engine")
        M = len(self.members)
        structs = [m._params() for m in self.members]   # (kept alive until the call is queued)
        params = (C.POINTER(_lib.Params) * M)(*[C.pointer(s) for s in structs])
        imgbufs = (C.c_void_p * M)(*[c.buf.data_ptr() for c in ctx.ctxs])
        weights = (C.c_float * M)(*self.weights)
        ed = _lib.EnsembleDesc(M, params, imgbufs, weights, ENSEMBLE_MODES[self.mode])
        lib, cfg = self.lib, C.byref(self._cfg)
        # member 0 runs the shared body of the search: its descriptor carries imgbufs[0], as the library asks
        return self.members[0]._search(ctx.ctxs[0], sentiment, n_samples, beam, per_node, max_steps, end_index, eps0, eps, fsm,
                                       compiled, mach, skip_dead, early_stop, False,
                                       lambda c, sd: lib.ssc_decode_search_ensemble_workspace_bytes(c, sd, C.byref(ed)),
                                       lambda p, sd, ws: lib.ssc_decode_search_ensemble(cfg, C.byref(ed), C.byref(sd), *ws))

    def _unsupported(self, what):
        raise NotImplementedError(f"{what} over an ensemble is not implemented (ensemble decoding runs the beam search only)")

    def sample(self, *a, **k):
        self._unsupported("the sampled decode (sample)")

    def score(self, *a, **k):
        self._unsupported("caption scoring (score)")

    def stochastic_beam(self, *a, **k):
        self._unsupported("the stochastic beam search (stochastic_beam)")

    def sampled_beam(self, *a, **k):
        self._unsupported("the sampled-node beam search (sampled_beam)")

    def diverse_beam(self, *a, **k):
        self._unsupported("the diverse beam search (diverse_beam)")

    def rules_beam(self, *a, **k):
        self._unsupported("the beam search under decode rules (rules_beam)")

    def attention(self, *a, **k):
        self._unsupported("the attention trace (attention)")


class CompiledFsm:
    """Machines in the compiled form of ssc_fsm_compile (include/ssc.h): per (machine, from-state) a default target set plus a
    short list of exception tokens.  `fsm` (M,S,S,V) uint8 on the device stays referenced: a from-state that does not fit the
    form (more than `max_exceptions` tokens off the default) is flagged on the device and takes the dense scans.
    fill: how many of the smallest non-exception tokens are kept per from-state (>= per-node beam size of the search)."""

    def __init__(self, fsm: torch.Tensor, max_exceptions: int = 512, fill: int = 8):
        assert fsm.is_cuda and fsm.dtype == torch.uint8 and fsm.dim() == 4 and fsm.size(1) == fsm.size(2) <= 32, fsm.shape
        self.fsm = fsm.contiguous()
        M, S, _, V = self.fsm.shape
        lib = _lib.load()
        self.dims = _lib.FsmDims(M, S, V, int(max_exceptions), int(fill))
        nbytes = lib.ssc_fsm_tables_bytes(C.byref(self.dims))
        if nbytes == 0:
            raise ValueError(f"ssc_fsm_tables_bytes: bad dims {fsm.shape}, E={max_exceptions}, P={fill}")
        self.tables = torch.empty(nbytes // 4, dtype=torch.int32, device=fsm.device)
        lib.ssc_fsm_compile(_lib.ptr(self.fsm), C.byref(self.dims), _lib.ptr(self.tables), nbytes, _lib.stream_ptr())

    def sparse_states(self) -> torch.Tensor:
        """(M, S) bool: which from-states took the compiled form (diagnostic; one device read)."""
        ms = self.dims.M * self.dims.S
        return self.tables[:ms].view(self.dims.M, self.dims.S) != 0


_HOST_FLAGS = []   # pinned words for the early-stop flag, recycled (allocating pinned memory is slow)


def _host_flag():
    """-> (pinned int32 tensor [2] holding zeros - stop flag, last completed step: ssc_beam_desc.host_flag -, its device-visible address)."""
    lib = _lib.load()
    t = _HOST_FLAGS.pop() if _HOST_FLAGS else torch.zeros(2, dtype=torch.int32).pin_memory()
    t.zero_()
    dp = C.c_void_p()
    if lib._raw_ssc_host_device_ptr(C.c_void_p(t.data_ptr()), C.byref(dp)) != 0:
        return t, None
    return t, dp


def cbs_search(start_predictions: torch.Tensor, start_state, step: Callable, fsm: Optional[torch.Tensor], end_index: int,
               max_steps: int, beam_size: int, per_node_beam_size: int, early_stop: bool = True,
               early_stop_every: int = 4, raw_logits: bool = False,
               ungathered_ok: Optional[Callable[[int, int], bool]] = None, compiled: Optional[CompiledFsm] = None,
               mach: Optional[torch.Tensor] = None, skip_dead: bool = False, compile_fsm: bool = True):
    """Constrained beam search with on-device bookkeeping (ssc_beam_first_fsm / ssc_beam_step_fsm / ssc_gather_rows /
    ssc_beam_backtrace_ctl).  `step(tokens (G,), state) -> (log_probs (G,V), state, ...)` as in cbs.py:127,170.
    Returns (predictions (B,S,beam,steps) int64, log_probs (B,S,beam)).
    fsm: (M,S,S,V) uint8 on the device, or None = the trivial one-state machine; batch entry b runs machine mach[b] (int32 (B);
    None: M = B, machine b).  compiled: the machines' compiled form (made here from `fsm` when S > 1 unless compile_fsm=False,
    which keeps the dense per-target scans): one scan per row instead of S, bit-identical selections.
    raw_logits: `step` returns un-normalised logits; the selection kernels normalise each row themselves (bit-identical
    selections and log-probs).
    early_stop: cbs.py:167 stops as soon as every beam has ended - a host sync per step in the reference.  Here the device itself
    notes the step after which all beams had ended (ssc_beam_desc.ctl) and turns every later step into a no-op, the host polls a
    pinned flag the device writes and merely stops QUEUEING steps once it sees it; the columns the reference would have produced
    are cut out at the end.  Same output for every machine, no host round trip.  early_stop_every <= 1: ask (and wait) after
    every step, as the reference does.
    skip_dead: ssc_beam_desc.skip_dead (rows without a finite beam are not scored from their logits; needs the compiled form).
    ungathered_ok(G, group) -> bool: the step function reads its previous states through the back-pointers itself
    (DecodeEngine.ungathered_ok): the states then stay in the previous step's row order, with state["_parent"] = back-pointers and
    state["_ungathered"] = True, and the re-ordering of cbs.py:236-250 (one gather per state tensor and step) is not done here."""
    lib = _lib.load()
    st = _lib.stream_ptr
    dev = start_predictions.device
    B = start_predictions.numel()
    if compiled is not None and fsm is None:
        fsm = compiled.fsm
    if fsm is None:   # the trivial one-state machine (every transition allowed): no mask is read on the device
        M, S, V = B, 1, None
    else:
        M, S, _, V = fsm.shape
        assert fsm.is_cuda and fsm.dtype == torch.uint8
        fsm = fsm.contiguous()
        assert mach is not None or M == B, (M, B)
        if compiled is None and compile_fsm and S > 1:
            compiled = CompiledFsm(fsm, fill=max(8, per_node_beam_size))
    if mach is not None:
        mach = mach.to(dev, torch.int32).contiguous()
        assert mach.numel() == B
        assert 0 <= int(mach.min()) and int(mach.max()) < M, "machine index out of range"   # (the kernels index the machines with it unchecked)
    assert not skip_dead or compiled is not None
    SB = S * beam_size
    preds = torch.empty(max_steps, B, SB, dtype=torch.int64, device=dev)
    backs = torch.empty(max(max_steps - 1, 1), B, SB, dtype=torch.int64, device=dev)
    last_lp = torch.empty(B, S, beam_size, dtype=torch.float32, device=dev)
    ctl = flag = flag_dev = None
    if early_stop:
        ctl = torch.zeros(2 + 2 * max_steps, dtype=torch.int32, device=dev)
        ctl[0] = max_steps
        flag, flag_dev = _host_flag()
    out = step(start_predictions, start_state)
    lp0, state = out[0], out[1]
    lp0 = lp0.contiguous()
    if V is None:
        V = lp0.shape[1]
    assert lp0.shape == (B, V), lp0.shape
    d = _lib.BeamDesc()
    d.raw_logits = 1 if raw_logits else 0
    d.fsm = _lib.ptr(fsm)
    d.tables = _lib.ptr(compiled.tables) if compiled is not None else None
    d.dims = compiled.dims if compiled is not None else _lib.FsmDims(M, S, V, 0, 1)
    d.mach = _lib.ptr(mach)
    d.B, d.beam, d.per_node, d.end_index = B, beam_size, per_node_beam_size, end_index
    d.skip_dead = 1 if skip_dead else 0
    d.ctl = _lib.ptr(ctl)
    d.max_steps = max_steps
    d.host_flag = flag_dev if ctl is not None else None
    d.scores, d.ld = _lib.ptr(lp0), lp0.stride(0)
    d.pred, d.lp_out = _lib.ptr(preds[0]), _lib.ptr(last_lp)
    lib.ssc_beam_first_fsm(C.byref(d), st())
    # enlarge states to (B*S*beam, *) batch-major (cbs.py:10-17,152-155)
    def enlarge(t):
        _, *rest = t.shape
        return t.view(B, 1, 1, *rest).expand(B, S, beam_size, *rest).reshape(-1, *rest).contiguous()

    state = {k: enlarge(v) for k, v in state.items() if not k.startswith("_")}
    state["_parent"] = torch.zeros(B, SB, dtype=torch.int64, device=dev)   # every beam of a group descends from the one start row
    sval = torch.empty(B * S * SB * per_node_beam_size, dtype=torch.float32, device=dev)
    sidx = torch.empty(B * S * SB * per_node_beam_size, dtype=torch.int64, device=dev)
    d.scratch_val, d.scratch_idx = _lib.ptr(sval), _lib.ptr(sidx)
    for t in range(1, max_steps):
        last = preds[t - 1].reshape(B * SB)
        if ctl is not None:
            if early_stop_every <= 1:
                if int(ctl[0]) <= t:   # (waits for the device, like the reference's `.all()`)
                    break
            elif int(flag[0]) != 0:    # a plain read of pinned host memory: nothing is queued, nothing waited for
                break
        state["_last_lp"] = last_lp
        if skip_dead:   # (for step functions that skip the rows whose logits will not be read: DecodeEngine.step)
            state["_skip"] = (last_lp, end_index)
        out = step(last, state)
        lp, state = out[0].contiguous(), out[1]
        new_lp = torch.empty_like(last_lp)
        d.scores, d.ld = _lib.ptr(lp), lp.stride(0)
        d.last_pred, d.last_lp = _lib.ptr(last), _lib.ptr(last_lp)
        d.pred, d.lp_out, d.backptr = _lib.ptr(preds[t]), _lib.ptr(new_lp), _lib.ptr(backs[t - 1])
        d.step_index = t
        lib.ssc_beam_step_fsm(C.byref(d), st())
        last_lp = new_lp
        new_state = {}
        # a step function that reads its previous states through the parent list (DecodeEngine.step at large G: `ungathered_ok`)
        # gets them as they are - the re-ordering of cbs.py:236-250 then happens inside its kernels' row lists
        leave = ungathered_ok is not None and SB > 1 and bool(ungathered_ok(B * SB, SB))
        for k, v in state.items():  # cbs.py:236-250
            if k.startswith("_"):
                continue
            if leave:
                new_state[k] = v
                continue
            v2 = v.reshape(B * SB, -1).contiguous()
            dst = torch.empty_like(v2)
            lib.ssc_gather_rows(_lib.ptr(v2), v2.stride(0), _lib.ptr(backs[t - 1]), B, SB, v2.size(1), _lib.ptr(dst), st())
            new_state[k] = dst.view_as(v)
        new_state["_parent"] = backs[t - 1]   # for the step function: which rows of a group now hold the same states
        if leave:
            new_state["_ungathered"] = True
        state = new_state
    if ctl is None:
        allp = torch.empty(B, SB, max_steps, dtype=torch.int64, device=dev)
        lib.ssc_beam_backtrace(_lib.ptr(preds), _lib.ptr(backs), max_steps, B, SB, _lib.ptr(allp), st())
        return allp.view(B, S, beam_size, max_steps), last_lp
    # a search the host stopped queueing at step t has written columns [0, t) and ctl[0] <= t; one that ran out has ctl[0] <= max_steps
    allp = torch.empty(B, SB, max_steps, dtype=torch.int64, device=dev)
    lib.ssc_beam_backtrace_ctl(_lib.ptr(preds), _lib.ptr(backs), _lib.ptr(ctl), max_steps, B, SB, end_index, _lib.ptr(allp), st())
    nsteps = int(ctl[0])   # (the one wait of the search: its result is about to be read anyway)
    _HOST_FLAGS.append(flag)
    return allp[:, :, :nsteps].contiguous().view(B, S, beam_size, nsteps), last_lp
