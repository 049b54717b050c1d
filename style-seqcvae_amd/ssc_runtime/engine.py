"""Training / decoding engine over the C ABI: flat parameter + gradient buffers, the fused
T-step forward/BPTT, clip + SGD, and the data-parallel gradient exchange.

Reference for the behaviour reproduced here: UpDownCaptioner.forward
(var_updown/var_updown/models/updown_captioner.py:228-368) and the optimiser loop of
var_updown/scripts/train.py:154-176.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import lib as _lib

P_CELL = "_updown_cell."
P_ATT = P_CELL + "_attention_lstm_cell."
P_ENC = P_CELL + "_language_lstm_cell_encoder."
P_DEC = P_CELL + "_language_lstm_cell_decoder."
P_BUTD = P_CELL + "_butd_attention."

# state_dict key -> ssc_params field
FIELD_OF = {
    "_embedding_layer.weight": "emb",
    P_ATT + "weight_ih": "att_w_ih", P_ATT + "weight_hh": "att_w_hh", P_ATT + "bias_ih": "att_b_ih", P_ATT + "bias_hh": "att_b_hh",
    P_BUTD + "_query_vector_projection_layer.weight": "wq",
    P_BUTD + "_image_features_projection_layer.weight": "wv",
    P_BUTD + "_attention_layer.weight": "wa",
    P_ENC + "weight_ih": "enc_w_ih", P_ENC + "weight_hh": "enc_w_hh", P_ENC + "bias_ih": "enc_b_ih", P_ENC + "bias_hh": "enc_b_hh",
    P_CELL + "fc_mean.weight": "fc_mean_w", P_CELL + "fc_mean.bias": "fc_mean_b",
    P_CELL + "fc_log_var.weight": "fc_lv_w", P_CELL + "fc_log_var.bias": "fc_lv_b",
    "_output_layer.weight": "out_w", "_output_layer.bias": "out_b",
    "_output_projection.0.weight": "proj_w", "_output_projection.0.bias": "proj_b",
    P_DEC + "weight_ih": "dec_w_ih", P_DEC + "weight_hh": "dec_w_hh", P_DEC + "bias_ih": "dec_b_ih", P_DEC + "bias_hh": "dec_b_hh",
}
HAS_LD = dict(_lib.PARAM_FIELDS)


class _EventWork:
    """wait() makes the compute stream wait for a collective that was issued on the communication stream (same call as the
    torch.distributed work handle's)."""

    def __init__(self, event, stream):
        self.event, self.stream = event, stream

    def wait(self):
        self.stream.wait_event(self.event)


@dataclass
class ModelDims:
    """Hot-path hyper-parameters (mirror of ssc_model_cfg)."""
    V: int
    E: int
    H: int
    A: int
    F: int
    Z: int
    S: int = 0            # conditioning columns on the language LSTMs (updown_cell.py:47-81): 0, 1 (sentiment) or, with kld_mode 2
                          # (SENTIMENT_VAE = 2: attention-pooled attribute means, Z wide), Z (LATENT_EMBEDDING "glove": all of them) or
                          # 1 ("senti_word_net": the first one, updown_cell.py:169-172)
    tied: bool = False    # E in {300,600}: frozen tied embedding (updown_captioner.py:75,112-119)
    kld_mode: int = 0     # 0: SENTIMENT_VAE == 0 formula, 1 otherwise (updown_captioner.py:298-303), 2: formula 1 with the prior
                          # mean of each step = the attention-pooled obj_atts (SENTIMENT_VAE = 2, updown_cell.py:160-163)
    pm_scale: float = 0.0  # prior_mean = pm_scale * sentiment
    prior_var: float = 1.0
    pad: int = 0
    boundary: int = 1
    gemm_mode: int = 0    # numerics of this engine's products: 0 = process default (ssc_set_gemm_mode), 1 = 3xBF16, 2 = exact-fp32 MFMA
    label_smoothing: float = 0.0   # eps of the cross-entropy (ssc_ce_fwd_smooth) in the cfg this builds; TrainEngine.forward /
                                   # train_step set the field per call from their own label_smoothing argument

    def cfg(self) -> _lib.ModelCfg:
        return _lib.ModelCfg(self.V, self.E, self.H, self.A, self.F, self.Z, self.S, int(self.tied), self.kld_mode,
                             float(self.pm_scale), float(self.prior_var), self.pad, self.boundary, int(self.gemm_mode),
                             check_label_smoothing(self.label_smoothing))

    def param_shapes(self) -> "Dict[str, Tuple[int, ...]]":
        V, E, H, A, F, Z, S = self.V, self.E, self.H, self.A, self.F, self.Z, self.S
        sh = {"_embedding_layer.weight": (V, E)}
        sh[P_ATT + "weight_ih"] = (4 * H, E + F + 2 * H)
        sh[P_ATT + "weight_hh"] = (4 * H, H)
        sh[P_ATT + "bias_ih"] = (4 * H,)
        sh[P_ATT + "bias_hh"] = (4 * H,)
        sh[P_BUTD + "_query_vector_projection_layer.weight"] = (A, H)
        sh[P_BUTD + "_image_features_projection_layer.weight"] = (A, F)
        sh[P_BUTD + "_attention_layer.weight"] = (1, A)
        sh[P_ENC + "weight_ih"] = (4 * H, S + F + 2 * H)
        sh[P_ENC + "weight_hh"] = (4 * H, H)
        sh[P_ENC + "bias_ih"] = (4 * H,)
        sh[P_ENC + "bias_hh"] = (4 * H,)
        sh[P_CELL + "fc_mean.weight"] = (Z, H)
        sh[P_CELL + "fc_log_var.weight"] = (Z, H)      # adjacent to fc_mean.weight: one (2Z,H) GEMM operand
        sh[P_CELL + "fc_mean.bias"] = (Z,)
        sh[P_CELL + "fc_log_var.bias"] = (Z,)
        if self.tied:
            sh["_output_projection.0.weight"] = (E, H)
            sh["_output_projection.0.bias"] = (E,)
        else:
            sh["_output_layer.weight"] = (V, H)
            sh["_output_layer.bias"] = (V,)
        # decoder LSTM last: one contiguous range that the freeze schedule (train.py:156-161) can skip
        sh[P_DEC + "weight_ih"] = (4 * H, S + F + 2 * H + Z)
        sh[P_DEC + "weight_hh"] = (4 * H, H)
        sh[P_DEC + "bias_ih"] = (4 * H,)
        sh[P_DEC + "bias_hh"] = (4 * H,)
        return sh


def _r4(x):
    return (x + 3) // 4 * 4


def check_label_smoothing(x, name="label_smoothing") -> float:
    """x as a float in [0, 1) (torch.nn.functional.cross_entropy's label_smoothing), else a ValueError that names `name`."""
    try:
        v = float(x)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(x, bool) or not 0.0 <= v < 1.0:
        raise ValueError(f"{name} must be a number in [0, 1); found {x!r}")
    return v


def check_sched_sampling(prob, sampler=None, seed=0) -> "Optional[_lib.SchedSampling]":
    """ssc_sched_sampling for a forward, or None for prob 0 (teacher forcing: the call is then the one without it).  prob in [0, 1];
    sampler: None (multinomial at temperature 1) or (kind, top_k, top_p, temperature) as ssc_sampler_desc has them - an object with
    a word sampler of ssc_runtime/sampling.py (kind, k, p, temperature) will do -; seed: the one 64-bit seed of the decisions and the draws."""
    try:
        v = float(prob)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(prob, bool) or not 0.0 <= v <= 1.0:
        raise ValueError(f"ss_prob must be a number in [0, 1]; found {prob!r}")
    if sampler is None:
        sampler = (0, 0, 1.0, 1.0)
    if not isinstance(sampler, (tuple, list)):
        sampler = (sampler.kind, getattr(sampler, "k", 0), getattr(sampler, "p", 1.0), sampler.temperature)
    kind, top_k, top_p, temperature = int(sampler[0]), int(sampler[1]), float(sampler[2]), float(sampler[3])
    if kind not in (0, 1, 2) or not 0.0 < temperature < float("inf") or not 0.0 <= top_p <= 1.0 or (kind == 1 and top_k < 1):
        raise ValueError(f"ss_sampler must be (kind 0 | 1 | 2, top_k >= 1 for kind 1, top_p in [0, 1], temperature > 0); found {sampler!r}")
    if v == 0.0:
        return None
    return _lib.SchedSampling(v, _lib.SamplerDesc(kind, top_k, top_p, temperature, int(seed) & ((1 << 64) - 1)))


def check_distill(alpha, temperature=1.0) -> Tuple[float, float]:
    """(alpha in [0, 1], temperature > 0 and finite) as floats - the mixing weight and the temperature of ssc_distill (include/ssc.h)
    -, else a ValueError that names distill_alpha / distill_temperature."""
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        a = float("nan")
    if isinstance(alpha, bool) or not 0.0 <= a <= 1.0:
        raise ValueError(f"distill_alpha must be a number in [0, 1]; found {alpha!r}")
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        t = float("nan")
    if isinstance(temperature, bool) or not 0.0 < t < float("inf"):
        raise ValueError(f"distill_temperature must be a finite number > 0; found {temperature!r}")
    return a, t


@dataclass
class Distill:
    """The soft targets of ONE forward (TrainEngine.forward / train_step: `distill=`): scores (T*B, >= V) float32 on the engine's
    device - a teacher's raw logits or log-probs of the same rows, time-major, leading dimension ld (DistillTeacher.scores makes
    them) -, the mixing weight alpha and the temperature.  alpha 0 = off: the forward is the one without it."""
    scores: torch.Tensor
    ld: int
    alpha: float
    temperature: float = 1.0

    def __post_init__(self):
        self.alpha, self.temperature = check_distill(self.alpha, self.temperature)
        self.ld = int(self.ld)


def check_distill_sampling(alpha, ss_prob):
    """Distillation and scheduled sampling do not compose (the student would be fed its own words while the teacher was fed the
    ground truth: the two rows would describe different histories): a ValueError that names both."""
    if float(alpha) > 0.0 and float(ss_prob) > 0.0:
        raise ValueError(f"distillation (distill_alpha = {alpha}) and scheduled sampling (ss_prob = {ss_prob}) cannot be used "
                         "in one forward: the teacher's rows are those of the ground-truth inputs")


def check_unlikelihood(alpha, min_one_minus=1e-5) -> Tuple[float, float]:
    """(alpha a finite number >= 0, min_one_minus in (0, 1)) as floats - the weight and the clamp of ssc_unlikelihood (include/ssc.h)
    -, else a ValueError that names unlikelihood / unlikelihood_clamp."""
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        a = float("nan")
    if isinstance(alpha, bool) or not 0.0 <= a < float("inf"):
        raise ValueError(f"unlikelihood must be a finite number >= 0; found {alpha!r}")
    try:
        d = float(min_one_minus)
    except (TypeError, ValueError):
        d = float("nan")
    if isinstance(min_one_minus, bool) or not 0.0 < d < 1.0:
        raise ValueError(f"unlikelihood_clamp must be a number in (0, 1); found {min_one_minus!r}")
    return a, d


def check_unlikelihood_distill(unlikelihood, distill_alpha):
    """Unlikelihood training and distillation do not compose (include/ssc.h: ssc_train_fwd_unlike): a ValueError that names both."""
    if float(unlikelihood) > 0.0 and float(distill_alpha) > 0.0:
        raise ValueError(f"unlikelihood training (unlikelihood = {unlikelihood}) and distillation (distill_alpha = {distill_alpha}) "
                         "cannot be used in one forward")


UNLIKELIHOOD_MAX_STEPS = 256   # ssc_ce_fwd_unlike: one lane of a workgroup per context position


FREE_BITS_MODES = {"element": 1, "step": 2, "dim": 3}   # ssc_free_bits.mode / ssc_train_opts.free_bits_mode


def check_free_bits(x, mode="dim", name="free_bits") -> Tuple[float, int]:
    """(lambda as a finite float >= 0, the mode's number in include/ssc.h), else a ValueError that names `name` / `name`_mode.
    The mode is checked whatever lambda is: a misspelt mode does not wait for the day the floor is switched on."""
    try:
        v = float(x)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(x, bool) or not 0.0 <= v < float("inf"):
        raise ValueError(f"{name} must be a finite number >= 0 (nats); found {x!r}")
    if mode not in FREE_BITS_MODES:
        raise ValueError(f"{name}_mode must be one of {' | '.join(FREE_BITS_MODES)}; found {mode!r}")
    return v, FREE_BITS_MODES[mode]


class _FwdOpts(NamedTuple):
    """The ssc_train_opts of one forward (c) and what it points into - the ssc_sched_sampling, the ssc_distill and the teacher's
    scores tensor -, and the ssc_unlikelihood that travels beside it; each None where the option is off, referenced until the last
    backward of that forward."""
    c: _lib.TrainOpts
    sched: Optional[_lib.SchedSampling]
    distill: Optional[_lib.Distill]
    scores: Optional[Distill]
    unlikelihood: Optional[_lib.Unlikelihood] = None


OPTIM_KINDS = ("sgd", "adam", "adamw")


@dataclass
class OptimSpec:
    """Which optimiser follows the clip in a fused step (train_step, backward_update, SelfCritical.step, scst_step: `optim=`).
    kind: "sgd" (momentum, L2) | "adam" (L2 folded into the gradient) | "adamw" (decoupled decay).  momentum / weight_decay left at
    None take the call's own momentum / weight_decay arguments (OPTIM.MOMENTUM, OPTIM.WEIGHT_DECAY are shared by the kinds)."""
    kind: str = "sgd"
    momentum: Optional[float] = None
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: Optional[float] = None

    def __post_init__(self):
        if self.kind not in OPTIM_KINDS:
            raise ValueError(f"optimiser kind must be one of {list(OPTIM_KINDS)}, got {self.kind!r}")
        self.betas = (float(self.betas[0]), float(self.betas[1]))

    @property
    def is_adam(self) -> bool:
        return self.kind != "sgd"

    def resolve(self, momentum, weight_decay):
        """(momentum, weight_decay) of a call that passes these two next to this spec: the spec's own where it sets them."""
        return (momentum if self.momentum is None else self.momentum,
                weight_decay if self.weight_decay is None else self.weight_decay)


def range_step_count(counts) -> int:
    """The one Adam step count of a range of the flat layout from its parameters' counts.  A parameter with count 0 next to others
    that agree never received a gradient under torch.optim (no state entry): it joins the range with zero moments, as a torch
    SGD checkpoint's parameter without a momentum buffer does.  Two different non-zero counts cannot be carried by one counter."""
    nonzero = sorted({int(c) for c in counts if c})
    if len(nonzero) > 1:
        raise ValueError(f"Adam state: the step counts {nonzero} differ within one range of the flat layout (the fused step keeps one "
                         "count for the decoder LSTM and one for the rest); scripts/train.py --reset-optimizer starts without the state")
    return nonzero[0] if nonzero else 0


def optimizer_state_kind(sd: dict) -> Optional[str]:
    """"sgd" / "adam" from the per-parameter entries of an optimiser state_dict (momentum_buffer versus exp_avg; Adam and AdamW
    keep the same state), else from its param group, else None (nothing in it says)."""
    for st in sd.get("state", {}).values():
        if "exp_avg" in st:
            return "adam"
        if "momentum_buffer" in st:
            return "sgd"
    for grp in sd.get("param_groups", []):
        if "betas" in grp:
            return "adam"
        if "momentum" in grp:
            return "sgd"
    return None


def check_optimizer_state_kind(sd: dict, want: str):
    """ValueError if `sd` holds the other optimiser family's state than `want` ("sgd" | "adam" | "adamw")."""
    have = optimizer_state_kind(sd)
    fam = "sgd" if want == "sgd" else "adam"
    if have is not None and have != fam:
        raise ValueError(f"the optimiser state is of kind {have!r} ({'exp_avg' if have == 'adam' else 'momentum_buffer'} entries) but the "
                         f"optimiser is {want!r}: state of one kind cannot continue the other (scripts/train.py: --reset-optimizer "
                         "drops it and starts at iteration 1)")


def _unpadded(flat, offsets, shapes, name):
    """The un-padded view of tensor `name` inside a flat buffer laid out as FlatStore lays it out."""
    o, cnt = offsets[name]
    shp = shapes[name]
    if len(shp) == 2 and shp[0] > 1:
        return flat[o:o + cnt].view(shp[0], _r4(shp[1]))[:, :shp[1]]
    return flat[o:o + shp[-1]].view(*shp)


def pack_adam_state(names, offsets, shapes, exp_avg, exp_avg_sq, steps, lr, spec: OptimSpec, weight_decay, iteration) -> dict:
    """Flat moment buffers + a step count per name -> torch.optim.Adam's state_dict layout (`step` a float32 scalar tensor,
    exp_avg / exp_avg_sq in the parameters' own shapes, indexed in `names` order); a name whose count is 0 has no entry.  Pure
    tensor work: runs on any device."""
    state = {}
    for i, n in enumerate(names):
        if steps.get(n, 0) > 0:
            state[i] = {"step": torch.tensor(float(steps[n]), dtype=torch.float32),
                        "exp_avg": _unpadded(exp_avg, offsets, shapes, n).detach().clone().contiguous(),
                        "exp_avg_sq": _unpadded(exp_avg_sq, offsets, shapes, n).detach().clone().contiguous()}
    group = {"lr": float(lr), "betas": tuple(spec.betas), "eps": float(spec.eps), "weight_decay": float(weight_decay),
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": spec.kind == "adamw", "params": list(range(len(names)))}
    return {"state": state, "param_groups": [group], "iteration": int(iteration)}


def unpack_adam_state(names, offsets, shapes, exp_avg, exp_avg_sq, sd: dict) -> "Dict[str, int]":
    """Inverse of pack_adam_state (also reads what torch.optim.Adam / AdamW wrote): fills the flat buffers in place (zero where a
    parameter has no entry) and returns the step count per name."""
    check_optimizer_state_kind(sd, "adam")
    exp_avg.zero_()
    exp_avg_sq.zero_()
    steps = {n: 0 for n in names}
    for i, st in sd.get("state", {}).items():
        n = names[int(i)]
        if "exp_avg" not in st:
            continue
        for flat, key in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            dst = _unpadded(flat, offsets, shapes, n)
            dst.copy_(st[key].to(dst.device, torch.float32).view_as(dst))
        steps[n] = int(round(float(st["step"])))
    return steps


class FlatStore:
    """One flat fp32 device buffer holding every tensor of `shapes` (16-B aligned offsets, rows of 2-D
    weights padded to a multiple of 4 floats so that 16 B/lane loads stay legal), exposed as views."""

    def __init__(self, shapes: "Dict[str, Tuple[int, ...]]", device, zero=True):
        self.shapes = dict(shapes)
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for name, shp in shapes.items():
            n = shp[0] * _r4(shp[1]) if len(shp) == 2 and shp[0] > 1 else _r4(shp[-1])
            self.offsets[name] = (off, n)
            off += n  # n is a multiple of 4 floats: every tensor starts 16-B aligned, neighbours stay adjacent
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=device) if zero else torch.empty(
            off, dtype=torch.float32, device=device)
        self.views: Dict[str, torch.Tensor] = {}
        for name, shp in shapes.items():
            o, n = self.offsets[name]
            if len(shp) == 2 and shp[0] > 1:
                ld = _r4(shp[1])
                self.views[name] = self.flat[o:o + n].view(shp[0], ld)[:, :shp[1]]
            else:
                self.views[name] = self.flat[o:o + shp[-1]].view(*shp)

    def range_of(self, names: Sequence[str]) -> Tuple[int, int]:
        """[lo, hi) flat range covering `names` (must be laid out consecutively)."""
        lo = min(self.offsets[n][0] for n in names)
        hi = max(self.offsets[n][0] + self.offsets[n][1] for n in names)
        return lo, hi

    def c_struct(self, only: Optional[Sequence[str]] = None) -> _lib.Params:
        s = _lib.Params()
        for name, view in self.views.items():
            if only is not None and name not in only:
                continue
            f = FIELD_OF[name]
            setattr(s, f, view.data_ptr())
            if HAS_LD[f]:
                setattr(s, "ld_" + f, view.stride(0))
        return s


def params_struct(tensors: "Dict[str, torch.Tensor]") -> _lib.Params:
    """ssc_params over arbitrary (row-major, unit inner stride) tensors."""
    s = _lib.Params()
    for name, t in tensors.items():
        if name not in FIELD_OF:
            continue
        f = FIELD_OF[name]
        if t.dim() == 2 and t.stride(1) != 1 and t.size(0) > 1:
            raise ValueError(f"{name}: inner stride must be 1")
        setattr(s, f, t.data_ptr())
        if HAS_LD[f]:
            setattr(s, "ld_" + f, t.stride(0) if t.size(0) > 1 else t.size(1))
    return s


class TrainEngine:
    """Owns parameters, gradients and the activation workspace of one model replica on one GPU."""

    def __init__(self, dims: ModelDims, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("TrainEngine needs a ROCm GPU (no CPU fallback)")
        self.dims = dims
        self.device = torch.device(device if device is not None else "cuda")
        shapes = dims.param_shapes()
        self.params = FlatStore(shapes, self.device)
        self.grads = FlatStore(shapes, self.device)
        self.momentum = None
        self.exp_avg = None           # Adam / AdamW moments, flat as the parameters, zeroed on first use (clip_adam_step)
        self.exp_avg_sq = None
        self.adam_steps = [0, 0]      # updates taken so far by [everything but the decoder LSTM, the decoder LSTM]
        self._ws = None
        self._ws_key = None
        self._cfg = dims.cfg()
        self._keep = None
        self._kld = None              # the kld tensor the last forward returned (kld_raw() without a floor)
        self._opts = _FwdOpts(_lib.TrainOpts(), None, None, None)   # the options of the last forward: every backward of it is given the same
        self._kd_scratch = None       # 3*T*B + B floats: the descriptor's rows blocks and kd_b
        self._ul_scratch = None       # 2*T*B + B floats: ssc_unlikelihood's rows blocks and ul_b
        self._post_ws = None          # posterior_forward's own workspace: the training forward's activations are never overwritten
        self._post_ws_key = None
        self._post = None
        self._scratch = torch.zeros(1024 + 16, dtype=torch.float32, device=self.device)
        names = list(shapes)
        self.decoder_names = [n for n in names if n.startswith(P_DEC)]
        self.frozen_names = ["_embedding_layer.weight"] if dims.tied else []
        self.steps_done = 0
        self.fwd_version = 0
        self.dp_buckets = 1
        self.dp_overlap = True
        self.dp_force = False         # take the phased / overlapped path in a one-rank group too (tests: the real RCCL backend on one GPU)
        self.dp_autograd = False      # the autograd path (UpDownCaptioner.forward + loss.backward()) all-reduces the flat
                                      # gradient buffer inside backward (scripts/train.py without --fused-optimizer)
        self.dp_profile = False       # record the exposed all-reduce time of every overlapped backward (bench.py --gpus N)
        self.dp_exposure_events = []  # [(bwd kernels done, gradients reduced)] torch.cuda.Event pairs
        # gradient exchange of the overlapped backward: "rccl" = torch.distributed all-reduce (RCCL rings / trees); "xgmi" = the
        # direct reduce-scatter + all-gather over hipIpc peer mappings (ssc_runtime/xgmi.py, csrc/collective.hip: all xGMI links
        # at once); "auto" = map the peers, verify the direct path against torch.distributed, time both on the real
        # gradient buffer and keep the faster - falling back to "rccl" whenever the direct path cannot be set up on every rank
        self.dp_algo = "rccl"
        self.dp_choice = None         # what "auto" / "xgmi" resolved to: {"algo": ..., "rccl_ms": ..., "xgmi_ms": ..., "why": ...}
        self._xgmi = None
        self._comm_stream = None

    def adopt(self, named: "Dict[str, torch.nn.Parameter]"):
        """Re-home nn.Parameters into the flat store (copy once, then `param.data` IS the view).  Cheap when they
        already live there; re-adopts after .to()/.cuda() or any external re-binding of param.data."""
        for name, p in named.items():
            view = self.params.views[name]
            if p.data_ptr() != view.data_ptr() or p.stride() != view.stride() or p.device != view.device:
                with torch.no_grad():
                    view.copy_(p.data.to(self.device, torch.float32))
                p.data = view

    def param_version(self):
        return (self.params.flat._version, self.steps_done)

    # ---- parameters --------------------------------------------------------------------------------
    def load_state_dict(self, sd: "Dict[str, torch.Tensor]"):
        for name, view in self.params.views.items():
            src = sd[name]
            view.copy_(src.to(self.device, torch.float32).view_as(view))

    def state_dict(self) -> "Dict[str, torch.Tensor]":
        out = {k: v.detach().clone().contiguous() for k, v in self.params.views.items()}
        if self.dims.tied:
            out["_output_layer.weight"] = out["_embedding_layer.weight"]
        return out

    def grad_dict(self) -> "Dict[str, torch.Tensor]":
        return {k: v.detach().clone().contiguous() for k, v in self.grads.views.items()}

    # ---- fused forward / backward ----------------------------------------------------------------------
    def _workspace(self, B, R, L):
        key = (B, R, L)
        if self._ws_key != key:
            nbytes = self.lib.ssc_train_workspace_bytes(C.byref(self._cfg), B, R, L)
            self._ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            self._ws_key = key
        return self._ws

    def _batch(self, feats, caps, sentiment, eps, obj_atts=None):
        B, R, F = feats.shape
        L = caps.shape[1]
        assert F == self.dims.F and feats.is_contiguous() and caps.is_contiguous() and eps.is_contiguous()
        assert caps.dtype == torch.int64 and feats.dtype == torch.float32 and eps.dtype == torch.float32
        assert tuple(eps.shape) == (L + 1, B, self.dims.Z), eps.shape
        sent = None
        if sentiment is not None:
            sent = sentiment.reshape(B).to(torch.float32).contiguous()
        if self.dims.kld_mode == 2:
            assert obj_atts is not None and tuple(obj_atts.shape) == (B, R, self.dims.Z), "SENTIMENT_VAE = 2 needs obj_atts (B,R,Z)"
            obj_atts = obj_atts.to(torch.float32).contiguous()
        else:
            obj_atts = None
        bt = _lib.Batch(B, R, L, feats.data_ptr(), caps.data_ptr(), sent.data_ptr() if sent is not None else None,
                        eps.data_ptr(), obj_atts.data_ptr() if obj_atts is not None else None)
        return bt, (sent, obj_atts)

    def forward(self, feats, caps, sentiment, eps, obj_atts=None, label_smoothing=0.0, free_bits=0.0, free_bits_mode="dim",
                ss_prob=0.0, ss_sampler=None, ss_seed=0, distill: "Optional[Distill]" = None, unlikelihood=0.0, unlikelihood_clamp=1e-5):
        """-> (loss (B,), kld (B,)); keeps activations for backward().  obj_atts (B,R,S): per-region attribute means, kld_mode 2 only.
        label_smoothing: eps of THIS call's cross-entropy (ssc_ce_fwd_smooth; 0 = the plain masked NLL, the kernels as they are
        without it).  It stays in the engine's cfg until the next forward, so every backward of this forward - the phased one of
        the data-parallel path included - differentiates the loss that was returned.  nll() is the unsmoothed loss either way.
        free_bits (nats) / free_bits_mode ("element" | "step" | "dim"): a floor on the KL of THIS call (include/ssc.h:
        ssc_free_bits) - kld is then the floored KL, a term at or below the floor has no gradient in the backward, kld_raw() is the
        KL without the floor.  0 = off: the kernels as they are without it.  "dim" floors the mean over the B rows of this call
        of each latent dimension (under data parallelism: this rank's rows).  Kept beside the cfg until the next forward likewise.
        ss_prob / ss_sampler / ss_seed: scheduled sampling of THIS call (include/ssc.h: ssc_sched_sampling; check_sched_sampling) -
        with probability ss_prob an eligible position is fed the word the model draws from its own logits of the previous step.
        0 = off: teacher forcing as before.  input_tokens() / fed_mask() read what was fed; the engine remembers, until the next
        forward, that every backward of this forward scatters the embedding gradient by the fed ids.
        distill: the soft targets of THIS call (Distill; include/ssc.h: ssc_distill) - loss is then (1 - alpha) * the (smoothed)
        hard loss + alpha * tau^2 KL(teacher || student) per row, kd() the KL term alone, nll() unchanged.  None or alpha 0 = off:
        the cross-entropy as before.  Kept beside the cfg until the next forward, as the options above are.  Not together with
        ss_prob > 0 (ValueError).
        unlikelihood / unlikelihood_clamp: token-level unlikelihood training of THIS call (include/ssc.h: ssc_unlikelihood) - each row
        adds unlikelihood * (- sum over the caption's earlier words c, the row's own target left out, of log max(1 - p[c],
        unlikelihood_clamp)) to its (smoothed) loss; ul() is that term alone, nll() unchanged.  0 = off: the cross-entropy as before.
        Kept beside the cfg until the next forward, as the options above are.  Composes with everything but distill (ValueError)."""
        check_distill_sampling(distill.alpha if distill is not None else 0.0, ss_prob)
        ul_alpha, ul_clamp = check_unlikelihood(unlikelihood, unlikelihood_clamp)
        check_unlikelihood_distill(ul_alpha, distill.alpha if distill is not None else 0.0)
        self._cfg.label_smoothing = check_label_smoothing(label_smoothing)
        fb = check_free_bits(free_bits, free_bits_mode)
        ss = check_sched_sampling(ss_prob, ss_sampler, ss_seed)
        bt, sent = self._batch(feats, caps, sentiment, eps, obj_atts)
        kd = self._distill_desc(distill, (bt.L + 1) * bt.B, bt.B)
        ul = self._unlikelihood_desc(ul_alpha, ul_clamp, bt.L + 1, bt.B)
        self._opts = _FwdOpts(_lib.TrainOpts(*fb, C.pointer(ss) if ss is not None else None, C.pointer(kd) if kd is not None else None),
                              ss, kd, distill, ul)
        ws = self._workspace(bt.B, bt.R, bt.L)
        loss = torch.empty(bt.B, dtype=torch.float32, device=self.device)
        kld = torch.empty(bt.B, dtype=torch.float32, device=self.device)
        p = self.params.c_struct()
        if ul is not None:   # (the descriptor travels beside the opts: include/ssc.h, ssc_train_fwd_unlike)
            self.lib.ssc_train_fwd_unlike(C.byref(self._cfg), C.byref(p), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(loss),
                                          _lib.ptr(kld), C.byref(self._opts.c), C.byref(ul), _lib.stream_ptr())
        else:
            self.lib.ssc_train_fwd_opts(C.byref(self._cfg), C.byref(p), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(loss),
                                        _lib.ptr(kld), C.byref(self._opts.c), _lib.stream_ptr())
        self._keep = (bt, feats, caps, sent, eps)
        self._kld = kld
        self.fwd_version += 1
        return loss, kld

    def _distill_desc(self, distill, rows, B) -> "Optional[_lib.Distill]":
        """ssc_distill of a forward over `rows` = T*B rows, or None where it does not distil; the scratch is the engine's."""
        if distill is None or distill.alpha == 0.0:
            return None
        t = distill.scores
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.params.flat.device):
            raise ValueError("distill.scores must be a float32 tensor on the engine's device")
        have = t.untyped_storage().nbytes() // 4 - t.storage_offset()   # (scores may be a view of padded rows: what lies behind its first element)
        if distill.ld < self.dims.V or have < (rows - 1) * distill.ld + self.dims.V:
            raise ValueError(f"distill.scores holds {have} floats at ld {distill.ld}: fewer than the {rows} rows of V = {self.dims.V} of this forward")
        n = 3 * rows + B
        if self._kd_scratch is None or self._kd_scratch.numel() != n:
            self._kd_scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        sc = self._kd_scratch
        return _lib.Distill(t.data_ptr(), distill.ld, distill.alpha, distill.temperature, sc.data_ptr(), sc[3 * rows:].data_ptr())

    def kd(self):
        """(B,) kd_b of the last forward - n_b sum_t w tau^2 KL(teacher || student) / (n_b + 1e-13), not weighted by alpha -: a view of
        the engine's scratch, valid until the next distilled forward; zeros when the last forward did not distil."""
        B = self._keep[0].B
        if self._opts.distill is None:
            return torch.zeros(B, dtype=torch.float32, device=self.device)
        return self._kd_scratch[self._kd_scratch.numel() - B:]

    def _unlikelihood_desc(self, alpha, clamp, T, B) -> "Optional[_lib.Unlikelihood]":
        """ssc_unlikelihood of a forward over T steps of B captions, or None where the term is off; the scratch is the engine's."""
        if alpha == 0.0:
            return None
        if T > UNLIKELIHOOD_MAX_STEPS:
            raise ValueError(f"unlikelihood training handles captions of at most {UNLIKELIHOOD_MAX_STEPS} steps; found {T}")
        rows = T * B
        n = 2 * rows + B
        if self._ul_scratch is None or self._ul_scratch.numel() != n:
            self._ul_scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        sc = self._ul_scratch
        return _lib.Unlikelihood(alpha, clamp, sc.data_ptr(), sc[2 * rows:].data_ptr())

    def ul(self):
        """(B,) ul_b of the last forward - n_b sum_t w ul_row / (n_b + 1e-13), not weighted by alpha -: a view of the engine's
        scratch, valid until the next forward with the term on; zeros when the last forward had it off."""
        B = self._keep[0].B
        if self._opts.unlikelihood is None:
            return torch.zeros(B, dtype=torch.float32, device=self.device)
        return self._ul_scratch[self._ul_scratch.numel() - B:]

    def _bwd_phases(self, p, bt, ws, gl, gk, g, mask):
        """One ssc_train_bwd_opts call of the last forward (mask 15: its whole backward), with the cfg and the options of that forward
        (ssc_train_bwd_unlike where that forward had the unlikelihood term on)."""
        ul = self._opts.unlikelihood
        if ul is not None:
            self.lib.ssc_train_bwd_unlike(C.byref(self._cfg), C.byref(p), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(gl),
                                          _lib.ptr(gk), C.byref(g), mask, C.byref(self._opts.c), C.byref(ul), _lib.stream_ptr())
            return
        self.lib.ssc_train_bwd_opts(C.byref(self._cfg), C.byref(p), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(gl),
                                    _lib.ptr(gk), C.byref(g), mask, C.byref(self._opts.c), _lib.stream_ptr())

    def posterior_forward(self, feats, caps, sentiment, eps, obj_atts=None):
        """The posterior branch's view of given captions (include/ssc.h: ssc_train_posterior) -> (nll (B,), kld (B,), log_ratio (B,),
        log_w (B,), kl_dim (B, Z), step_kl (T, B), step_ratio (T, B)): one ssc_train_fwd (label_smoothing 0; that entry has no free-bits floor) on a workspace of
        this method's own and a copy of the cfg, then the log-density ratio log p(z) - log q(z | x) at the sampled z, the KL per
        latent dimension and per step, and log_w = log_ratio - nll.  Nothing a later backward() reads is touched - _keep, the
        training workspace, the cfg's label_smoothing, fwd_version: backward() after this call still differentiates the forward
        the caller ran before it.  posterior_view(which) reads this forward's activations."""
        cfg = _lib.ModelCfg.from_buffer_copy(self._cfg)
        cfg.label_smoothing = 0.0
        bt, keep = self._batch(feats, caps, sentiment, eps, obj_atts)
        B, T, Z = bt.B, bt.L + 1, self.dims.Z
        key = (B, bt.R, bt.L)
        if self._post_ws_key != key:
            nbytes = self.lib.ssc_train_workspace_bytes(C.byref(cfg), B, bt.R, bt.L)
            self._post_ws = None   # (the old one is released before the new one is taken)
            self._post_ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            self._post_ws_key = key
        ws = self._post_ws
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        nll, kld, log_ratio, log_w, kl = new(B), new(B), new(B), new(B), new(B)
        kl_dim, step_kl, step_ratio = new(B, Z), new(T, B), new(T, B)
        p = self.params.c_struct()
        st = _lib.stream_ptr()
        self.lib.ssc_train_fwd(C.byref(cfg), C.byref(p), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(nll), _lib.ptr(kld), st)
        self.lib.ssc_train_posterior(C.byref(cfg), C.byref(bt), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(log_w), _lib.ptr(log_ratio),
                                     _lib.ptr(kl), _lib.ptr(kl_dim), Z, _lib.ptr(step_kl), _lib.ptr(step_ratio), st)
        self._post = (bt, feats, caps, keep, eps, cfg)
        return nll, kld, log_ratio, log_w, kl_dim, step_kl, step_ratio

    def posterior_view(self, which):
        """Activations of the last posterior_forward (test hook): "z" (T, B, Z) as the forward stored it, "pm" (T, B, Z) the pooled
        prior means of kld_mode 2, "w" (T, B) the step weights (ssc_train_posterior_view); an int: workspace_view's numbering."""
        bt, cfg, ws = self._post[0], self._post[5], self._post_ws
        if isinstance(which, int):
            return self._view(ws, bt, cfg, which)
        ld = C.c_int(0)
        p = self.lib.ssc_train_posterior_view(C.byref(cfg), bt.B, bt.R, bt.L, _lib.ptr(ws), {"z": 0, "pm": 1, "w": 2}[which], C.byref(ld))
        if not p:
            raise ValueError(which)
        off = (p - ws.data_ptr()) // 4
        T, B = bt.L + 1, bt.B
        if which == "w":
            return ws[off:off + T * B].view(T, B)
        return ws[off:off + T * B * ld.value].view(T, B, ld.value)[:, :, :self.dims.Z]

    # gradient ranges that are final after each backward phase (flat layout order: emb | att LSTM | attention |
    # enc LSTM | fc | output head | dec LSTM)
    def phase_ranges(self):
        names = list(self.grads.views)
        head = [n for n in names if n.startswith("_output_")]
        dec = self.decoder_names
        emb = [n for n in names if n.startswith("_embedding")]
        first = [n for n in names if n.startswith(P_ATT) or n.startswith(P_BUTD)]
        mid = [n for n in names if n.startswith(P_ENC) or n.startswith(P_CELL + "fc_")]
        # (mask, range final after it): the head's gradients travel under the whole BPTT loop, which finishes no range itself;
        # the three weight-gradient phases are independent of each other - the two lighter ones run first so that the first
        # large all-reduce starts ~0.2 ms earlier and the heaviest phase computes under two reductions
        # the embedding gradient (one product + a scatter, 40 MB at C2) goes first: its range travels under all other phases, and
        # the last range - what stays exposed - is the attention LSTM's alone (five ranges: VERDICT r2 next-4a)
        return [(16, self.grads.range_of(head)), (32, None), (64, self.grads.range_of(emb)), (8, self.grads.range_of(dec)),
                (4, self.grads.range_of(mid)), (128, self.grads.range_of(first))]

    def backward_overlapped(self, gl, gk, skip: Sequence[str] = (), group=None):
        """Backward in four phases; the sum all-reduce of each finished gradient range is issued asynchronously
        (RCCL runs it on its own stream) while the next phase's GEMMs run.  Returns the world size."""
        import torch.distributed as dist

        bt = self._keep[0]
        ws = self._workspace(bt.B, bt.R, bt.L)
        skipset = set(skip) | set(self.frozen_names)
        only = [n for n in self.grads.views if n not in skipset]
        p = self.params.c_struct()
        g = self.grads.c_struct(only=only)
        gl = gl.to(torch.float32).contiguous()
        gk = gk.to(torch.float32).contiguous()
        world = dist.get_world_size(group)
        works = []
        xg = self._resolve_dp_algo(group) if world > 1 else None
        cur = torch.cuda.current_stream(self.device)
        # only what the update will read travels: a frozen decoder LSTM / tied embedding keeps its (stale) gradient range at home
        t_lo, t_hi = self.trainable_range(bool(set(self.decoder_names) & skipset))
        for mask, rng in self.phase_ranges():
            self._bwd_phases(p, bt, ws, gl, gk, g, mask)
            if rng is not None:
                lo, hi = max(rng[0], t_lo), min(rng[1], t_hi)
                if hi > lo and xg is not None:
                    # direct path: the collective's kernels run on the communication stream behind this phase; the compute
                    # stream goes on with the next phase and waits for the `done` event before it reads the range
                    ready = torch.cuda.Event()
                    ready.record(cur)
                    self._comm_stream.wait_event(ready)
                    xg.allreduce(lo, hi, stream=self._comm_stream)
                    done = torch.cuda.Event()
                    done.record(self._comm_stream)
                    works.append((_EventWork(done, cur), (lo, hi)))
                elif hi > lo:
                    works.append((dist.all_reduce(self.grads.flat[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True), (lo, hi)))
        if xg is not None:
            xg.poll(self._comm_stream)   # a bounded wait that gave up leaves the gradients un-summed: reported one step later at most
        if self.dp_profile:   # exposure = time the compute stream sits between its last backward kernel and the reduced gradients
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        # the squared norm of every range is summed as soon as that range has arrived, under the reductions still in flight:
        # behind the last one only its own range's norm and the update are left
        n_parts = 0
        for w, (lo, hi) in works:
            w.wait()
            self.lib.ssc_sq_norm(_lib.ptr(self.grads.flat[lo:hi]), hi - lo, _lib.ptr(self._scratch),
                                 _lib.ptr(self._scratch[1026 + n_parts:1027 + n_parts]), _lib.stream_ptr())
            n_parts += 1
        self._sq_parts = self._scratch[1026:1026 + n_parts].sum(dim=0, keepdim=True) if n_parts else None
        if self.dp_profile:
            e1.record()
            self.dp_exposure_events.append((e0, e1))
        return world

    def _resolve_dp_algo(self, group):
        """The XgmiAllReduce to use for this group, or None for torch.distributed (see dp_algo).  Collective on first use."""
        if self.dp_algo == "rccl":
            return None
        if self.dp_choice is not None:
            return self._xgmi if self.dp_choice["algo"] == "xgmi" else None
        import sys

        import torch.distributed as dist

        from . import xgmi
        rank = dist.get_rank(group)
        log = (lambda m: print("[ssc dp]", m, file=sys.stderr, flush=True)) if rank == 0 else None
        self._comm_stream = torch.cuda.Stream(device=self.device)
        obj = xgmi.try_create(self.grads.flat, group=group, log=log)
        choice = {"algo": "rccl", "rccl_ms": None, "xgmi_ms": None, "why": "direct path unavailable"}
        if obj is not None and self.dp_algo == "xgmi":
            choice.update(algo="xgmi", why="requested")
        elif obj is not None:   # auto: time both on the whole gradient buffer (contents are scratch between steps)
            def timed(fn):
                torch.cuda.synchronize(self.device)
                dist.barrier(group=group)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()   # warm-up
                e0.record()
                for _ in range(3):
                    fn()
                e1.record()
                torch.cuda.synchronize(self.device)
                t = torch.tensor([e0.elapsed_time(e1) / 3], dtype=torch.float64,
                                 device=self.device if dist.get_backend(group) == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
                return float(t.item())
            # the start-up self-test over the WHOLE gradient buffer (the construction's own covers 64 K floats): ordering / visibility
            # problems of a 446 MB exchange do not show on a buffer that fits the caches
            try:
                obj.self_test(self.grads.flat.numel())
                full_ok = True
            except Exception as e:   # noqa: BLE001 - XgmiError is raised on every rank or on none
                full_ok = False
                if log:
                    log(f"direct path failed its full-buffer self-test ({e}): using torch.distributed")
            self.grads.flat.zero_()
            r_ms = timed(lambda: dist.all_reduce(self.grads.flat, op=dist.ReduceOp.SUM, group=group))
            x_ms = timed(lambda: obj.allreduce(0, self.grads.flat.numel()))
            try:
                obj.check()
                healthy = True
            except Exception:   # noqa: BLE001 - a bounded wait gave up on this rank
                healthy = False
            healthy = obj._agree(healthy and full_ok)   # collective: every rank takes the same path
            choice.update(rccl_ms=r_ms, xgmi_ms=x_ms)
            if not healthy:
                choice.update(why="a rank timed out in the direct path")
            elif x_ms < r_ms:
                choice.update(algo="xgmi", why="faster than torch.distributed on this node")
            else:
                choice.update(why="torch.distributed is faster on this node")
        self._xgmi = obj
        self.dp_choice = choice
        if log:
            log(f"gradient exchange: {choice}")
        return obj if choice["algo"] == "xgmi" else None

    def dp_exposure_ms(self):
        """Exposed all-reduce time per overlapped backward since the last call (synchronises)."""
        torch.cuda.synchronize()
        out = [a.elapsed_time(b) for a, b in self.dp_exposure_events]
        self.dp_exposure_events = []
        return out

    def backward_phased(self, gl, gk, masks: Sequence[int], skip: Sequence[str] = ()):
        """The backward as a given sequence of ssc_train_bwd_phases calls, no collective (tests: every legal order of the phases
        leaves the gradients of the one-call backward)."""
        bt = self._keep[0]
        ws = self._workspace(bt.B, bt.R, bt.L)
        skipset = set(skip) | set(self.frozen_names)
        p = self.params.c_struct()
        g = self.grads.c_struct(only=[n for n in self.grads.views if n not in skipset])
        gl = gl.to(torch.float32).contiguous()
        gk = gk.to(torch.float32).contiguous()
        for mask in masks:
            self._bwd_phases(p, bt, ws, gl, gk, g, mask)

    def backward(self, gl, gk, skip: Sequence[str] = ()):
        """Writes d(sum_b gl_b loss_b + gk_b kld_b)/dparam into self.grads for every parameter not in `skip`
        (nor frozen)."""
        bt = self._keep[0]
        ws = self._workspace(bt.B, bt.R, bt.L)
        skipset = set(skip) | set(self.frozen_names)
        only = [n for n in self.grads.views if n not in skipset]
        p = self.params.c_struct()
        g = self.grads.c_struct(only=only)
        gl = gl.to(torch.float32).contiguous()
        gk = gk.to(torch.float32).contiguous()
        self._bwd_phases(p, bt, ws, gl, gk, g, 15)

    def nll(self):
        """(B,) unsmoothed loss_b of the last forward (= its loss when that ran with label_smoothing 0): a view of the workspace,
        valid until the next forward."""
        return self.workspace_view(12)

    def input_tokens(self):
        """(T, B) int64: the ids the last forward fed to the attention LSTM - with scheduled sampling the fed ids block of the
        workspace (a view, valid until the next forward), else the ground-truth inputs tok[:-1]."""
        bt = self._keep[0]
        T, B = bt.L + 1, bt.B
        ws = self._workspace(bt.B, bt.R, bt.L)
        fed = self._opts.sched is not None
        view = self.lib.ssc_train_sched_view if fed else self.lib.ssc_train_workspace_view
        p = view(C.byref(self._cfg), bt.B, bt.R, bt.L, _lib.ptr(ws), 13 if fed else 10, None)
        off = (p - ws.data_ptr()) // 4
        return ws[off:off + 2 * T * B].view(torch.int64).view(T, B)

    def fed_mask(self):
        """(T, B) bool: where the last forward fed the model's own word (all False without scheduled sampling)."""
        bt = self._keep[0]
        T, B = bt.L + 1, bt.B
        if self._opts.sched is None:
            return torch.zeros(T, B, dtype=torch.bool, device=self.device)
        ws = self._workspace(bt.B, bt.R, bt.L)
        p = self.lib.ssc_train_sched_view(C.byref(self._cfg), bt.B, bt.R, bt.L, _lib.ptr(ws), 14, None)
        off = (p - ws.data_ptr()) // 4
        return ws[off:off + T * B].view(T, B) != 0

    def kld_raw(self):
        """(B,) KL of the last forward without the free-bits floor: a view of the workspace, valid until the next forward - or,
        when that forward ran with free_bits 0, the kld it returned."""
        return self.free_bits_view("raw") if self._opts.c.free_bits > 0 else self._kld

    def free_bits_view(self, which):
        """Of the last forward with free_bits > 0 (ssc_train_free_bits_view): "raw" (B,) the KL without the floor, "kdim" (Z,) the
        minibatch means K_j and "gate_dim" (Z,) their gates (mode "dim"), "gate_step" (T, B) the step gates (mode "step"); gates
        are 1.0 / 0.0.  Views of the workspace, valid until the next forward."""
        bt = self._keep[0]
        ws = self._workspace(bt.B, bt.R, bt.L)
        ld = C.c_int(0)
        p = self.lib.ssc_train_free_bits_view(C.byref(self._cfg), bt.B, bt.R, bt.L, _lib.ptr(ws),
                                              {"raw": 0, "kdim": 1, "gate_step": 2, "gate_dim": 3}[which], C.byref(ld))
        off = (p - ws.data_ptr()) // 4
        T, B = bt.L + 1, bt.B
        if which == "raw":
            return ws[off:off + B]
        if which == "gate_step":
            return ws[off:off + T * B].view(T, B)
        return ws[off:off + self.dims.Z]

    def workspace_view(self, which, T1=None):
        """Saved activations of the last forward (test hook; see ssc_train_workspace_view)."""
        bt = self._keep[0]
        return self._view(self._workspace(bt.B, bt.R, bt.L), bt, self._cfg, which)

    def _view(self, ws, bt, cfg, which):
        ld = C.c_int(0)
        p = self.lib.ssc_train_workspace_view(C.byref(cfg), bt.B, bt.R, bt.L, _lib.ptr(ws), which, C.byref(ld))
        off = (p - ws.data_ptr()) // 4
        T, B = bt.L + 1, bt.B
        d = self.dims
        if which <= 5:
            return ws[off:off + (T + 1) * B * ld.value].view(T + 1, B, ld.value)[:, :, :d.H]
        if which == 6:
            return ws[off:off + T * B * bt.R].view(T, B, bt.R)
        if which in (7, 8):
            return ws[off:off + T * B * ld.value].view(T, B, ld.value)[:, :, :d.Z]
        if which == 9:
            return ws[off:off + T * B * ld.value].view(T, B, ld.value)[:, :, :d.V]
        if which == 11:
            return ws[off:off + T * B * ld.value].view(T, B, ld.value)[:, :, :d.F]
        if which == 12:
            return ws[off:off + B]
        raise ValueError(which)

    # ---- optimiser (train.py:126-134,173-176) ---------------------------------------------------------
    def trainable_range(self, decoder_frozen: bool) -> Tuple[int, int]:
        """The flat layout is [frozen tied embedding | always-trainable | decoder LSTM], so the trainable part is
        one contiguous range whatever the freeze schedule (train.py:156-161) says."""
        lo, hi = 0, self.params.numel
        if self.frozen_names:
            lo = self.params.range_of(self.frozen_names)[1]
        if decoder_frozen:
            hi = self.params.range_of(self.decoder_names)[0]
        return lo, hi

    def clip_sgd_step(self, lr, momentum=0.9, weight_decay=0.001, max_norm=12.5, decoder_frozen=False, gscale=1.0, sq_norm=None):
        """clip_grad_norm_(max_norm) + SGD(momentum, weight_decay) on the flat buffers, skipping frozen ranges
        (torch>=2 semantics: parameters without a gradient are not touched).  Momentum buffers start at zero,
        which reproduces torch's lazily created buffer (first step: buf = d_p).  Returns the squared grad norm."""
        if self.momentum is None:
            self.momentum = torch.zeros_like(self.params.flat)
        lo, hi = self.trainable_range(decoder_frozen)
        st = _lib.stream_ptr()
        if sq_norm is not None:   # already summed range by range (backward_overlapped)
            sq = sq_norm
        else:
            sq = self._scratch[1024:1025]
            self.lib.ssc_sq_norm(_lib.ptr(self.grads.flat[lo:hi]), hi - lo, _lib.ptr(self._scratch), _lib.ptr(sq), st)
        self.lib.ssc_sgd_step(_lib.ptr(self.params.flat[lo:hi]), _lib.ptr(self.grads.flat[lo:hi]),
                              _lib.ptr(self.momentum[lo:hi]), hi - lo, _lib.ptr(sq), float(gscale), float(max_norm),
                              float(lr), float(momentum), float(weight_decay), 0, st)
        self.steps_done += 1
        return sq

    def _adam_buffers(self):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params.flat)
            self.exp_avg_sq = torch.zeros_like(self.params.flat)

    def clip_adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=12.5,
                       decoder_frozen=False, gscale=1.0, sq_norm=None):
        """clip_grad_norm_(max_norm) + torch.optim.Adam (decoupled: AdamW) on the flat buffers: the twin of clip_sgd_step, same
        ranges, same sq_norm / gscale, same return value.  torch counts the steps per parameter and does not count one for a
        parameter without a gradient, so under the freeze schedule the decoder LSTM's count lags: two counters (adam_steps), one
        ssc_adam_step call when they agree after this step's increments, else two split at the decoder range, both reading the
        same squared norm.  The moments start at zero (torch's lazily created state)."""
        self._adam_buffers()
        lo, hi = self.trainable_range(decoder_frozen)
        st = _lib.stream_ptr()
        if sq_norm is not None:   # already summed range by range (backward_overlapped)
            sq = sq_norm
        else:
            sq = self._scratch[1024:1025]
            self.lib.ssc_sq_norm(_lib.ptr(self.grads.flat[lo:hi]), hi - lo, _lib.ptr(self._scratch), _lib.ptr(sq), st)
        self.adam_steps[0] += 1
        if not decoder_frozen:
            self.adam_steps[1] += 1
        if decoder_frozen or self.adam_steps[0] == self.adam_steps[1]:
            calls = [(lo, hi, self.adam_steps[0])]
        else:
            mid = self.params.range_of(self.decoder_names)[0]
            calls = [(lo, mid, self.adam_steps[0]), (mid, hi, self.adam_steps[1])]
        for a, b, step in calls:
            self.lib.ssc_adam_step(_lib.ptr(self.params.flat[a:b]), _lib.ptr(self.grads.flat[a:b]), _lib.ptr(self.exp_avg[a:b]),
                                   _lib.ptr(self.exp_avg_sq[a:b]), b - a, _lib.ptr(sq), float(gscale), float(max_norm), float(lr),
                                   float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)), step, st)
        self.steps_done += 1
        return sq

    def _adam_step_counts(self, names) -> "Dict[str, int]":
        dec, frozen = set(self.decoder_names), set(self.frozen_names)
        return {n: 0 if n in frozen else self.adam_steps[1 if n in dec else 0] for n in names}

    def optimizer_state_dict(self, named_parameters, lr, momentum, weight_decay, iteration, optim: Optional[OptimSpec] = None) -> dict:
        """The fused optimiser's state in torch.optim.SGD's state_dict layout (one momentum_buffer per parameter, indexed
        in `named_parameters` order = model.parameters() order), so that a checkpoint written on either path of
        scripts/train.py resumes on the other and `optimizer.load_state_dict` of the reference's train.py:142-151 accepts
        it.  `iteration` rides along inside this entry: the reference loads every OTHER top-level key into the model.
        optim of an Adam kind: torch.optim.Adam's layout instead (pack_adam_state; a parameter that never took a step - the
        frozen tied embedding, the decoder LSTM before its first update - has no entry)."""
        names = [n for n, _ in named_parameters]
        if optim is not None and optim.is_adam:
            self._adam_buffers()
            wd = optim.resolve(momentum, weight_decay)[1]
            return pack_adam_state(names, self.params.offsets, self.params.shapes, self.exp_avg, self.exp_avg_sq,
                                   self._adam_step_counts(names), lr, optim, wd, iteration)
        if optim is not None:
            momentum, weight_decay = optim.resolve(momentum, weight_decay)
        state = {}
        if self.momentum is not None:
            for i, n in enumerate(names):
                o, cnt = self.params.offsets[n]
                shp = self.params.shapes[n]
                if len(shp) == 2 and shp[0] > 1:
                    buf = self.momentum[o:o + cnt].view(shp[0], _r4(shp[1]))[:, :shp[1]]
                else:
                    buf = self.momentum[o:o + shp[-1]].view(*shp)
                state[i] = {"momentum_buffer": buf.detach().clone().contiguous()}
        group = {"lr": float(lr), "momentum": float(momentum), "dampening": 0, "weight_decay": float(weight_decay),
                 "nesterov": False, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
                 "params": list(range(len(names)))}
        return {"state": state, "param_groups": [group], "iteration": int(iteration)}

    def load_optimizer_state_dict(self, named_parameters, sd: dict, optim: Optional[OptimSpec] = None):
        """Inverse of optimizer_state_dict; also accepts a torch.optim.SGD state_dict (parameters without a buffer - never
        updated so far - start from zero, torch's lazily created buffer) or, with optim of an Adam kind, torch.optim.Adam's /
        AdamW's.  State of the other kind than `optim` (default: SGD) is a ValueError that names both."""
        names = [n for n, _ in named_parameters]
        if optim is not None and optim.is_adam:
            check_optimizer_state_kind(sd, optim.kind)
            self._adam_buffers()
            steps = unpack_adam_state(names, self.params.offsets, self.params.shapes, self.exp_avg, self.exp_avg_sq, sd)
            dec, frozen = set(self.decoder_names), set(self.frozen_names)
            for which, group in ((1, [n for n in names if n in dec]), (0, [n for n in names if n not in dec and n not in frozen])):
                self.adam_steps[which] = range_step_count(steps[n] for n in group)
            return
        check_optimizer_state_kind(sd, "sgd")
        if self.momentum is None:
            self.momentum = torch.zeros_like(self.params.flat)
        self.momentum.zero_()
        for i, st in sd.get("state", {}).items():
            buf = st.get("momentum_buffer")
            if buf is None:
                continue
            n = names[int(i)]
            o, cnt = self.params.offsets[n]
            shp = self.params.shapes[n]
            if len(shp) == 2 and shp[0] > 1:
                dst = self.momentum[o:o + cnt].view(shp[0], _r4(shp[1]))[:, :shp[1]]
            else:
                dst = self.momentum[o:o + shp[-1]].view(*shp)
            dst.copy_(buf.to(self.device, torch.float32).view_as(dst))

    # ---- data parallel -----------------------------------------------------------------------------------
    def allreduce_grads(self, group=None):
        """One RCCL all-reduce (sum) over the flat gradient buffer; the 1/world_size is folded into the SGD kernel."""
        from . import dp

        return dp.allreduce_flat(self.grads.flat, group=group, n_buckets=self.dp_buckets)

    def train_step(self, feats, caps, sentiment, eps, lr, kld_weight=750.0, momentum=0.9, weight_decay=0.001,
                   max_norm=12.5, decoder_frozen=False, group=None, obj_atts=None, optim: Optional[OptimSpec] = None,
                   label_smoothing=0.0, kl_beta=1.0, free_bits=0.0, free_bits_mode="dim", ss_prob=0.0, ss_sampler=None, ss_seed=0,
                   distill: "Optional[Distill]" = None, unlikelihood=0.0, unlikelihood_clamp=1e-5):
        """fwd + bwd + (all-reduce) + clip + SGD: one iteration of train.py:154-176.  Returns (loss, kld) per row.
        optim: another optimiser behind the clip (OptimSpec); None = SGD with the arguments above.
        label_smoothing: as forward(); loss is then the smoothed one, nll() the unsmoothed.
        kl_beta: the annealing weight of this iteration (ssc_runtime/schedule.py) - the objective is mean loss + kl_beta * mean kld /
        kld_weight, so the upstream of kld_b is kl_beta / (B * kld_weight); 0 is legal: no KL gradient at all.
        free_bits / free_bits_mode: as forward(); kld is then the floored KL, kld_raw() the raw one.
        ss_prob / ss_sampler / ss_seed: scheduled sampling, as forward().
        distill: soft targets, as forward(); loss is then the mixed one, kd() the KL term, nll() the hard loss.
        unlikelihood / unlikelihood_clamp: as forward(); loss then carries the weighted term, ul() the term alone."""
        kl_beta = float(kl_beta)
        if not 0.0 <= kl_beta < float("inf"):
            raise ValueError(f"kl_beta must be a finite number >= 0; found {kl_beta!r}")
        loss, kld = self.forward(feats, caps, sentiment, eps, obj_atts, label_smoothing, free_bits, free_bits_mode, ss_prob, ss_sampler,
                                 ss_seed, distill, unlikelihood, unlikelihood_clamp)
        B = loss.numel()
        key = (B, float(kld_weight))
        if getattr(self, "_upstream_key", None) != key:   # d(mean loss + beta mean kld / KLD_WEIGHT) / d(loss_b, kld_b): two (B,) buffers per (B, weight)
            self._upstream = (torch.full((B,), 1.0 / B, dtype=torch.float32, device=self.device),
                              torch.full((B,), 1.0 / (B * kld_weight), dtype=torch.float32, device=self.device))
            self._upstream_key = key
            self._upstream_beta = 1.0
        gl, gk = self._upstream
        if kl_beta != self._upstream_beta:   # a schedule moves beta every iteration: refill the same buffer (one launch, no allocation, no sync)
            gk.fill_(kl_beta / (B * kld_weight))
            self._upstream_beta = kl_beta
        self.backward_update(gl, gk, lr, momentum, weight_decay, max_norm, decoder_frozen, group, optim)
        return loss, kld

    def backward_update(self, gl, gk, lr, momentum=0.9, weight_decay=0.001, max_norm=12.5, decoder_frozen=False, group=None,
                        optim: Optional[OptimSpec] = None):
        """What follows the forward in one iteration: the backward of the last forward() with the per-row upstream gradients
        gl / gk (B,), the gradient all-reduce, clip + SGD.  train_step passes the constant vectors of the mean objective, the
        self-critical step (ssc_runtime/scst.py) the advantage-weighted ones: one path for both."""
        import torch.distributed as dist

        skip = self.decoder_names if decoder_frozen else ()
        if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or self.dp_force) and self.dp_overlap:
            world = self.backward_overlapped(gl, gk, skip=skip, group=group)
            sq_parts = self._sq_parts
        else:
            self.backward(gl, gk, skip=skip)
            world = self.allreduce_grads(group)
            sq_parts = None
        if optim is None:
            self.clip_sgd_step(lr, momentum, weight_decay, max_norm, decoder_frozen, gscale=1.0 / world, sq_norm=sq_parts)
            return
        momentum, weight_decay = optim.resolve(momentum, weight_decay)
        if optim.is_adam:
            self.clip_adam_step(lr, optim.betas, optim.eps, weight_decay, optim.kind == "adamw", max_norm, decoder_frozen,
                                gscale=1.0 / world, sq_norm=sq_parts)
        else:
            self.clip_sgd_step(lr, momentum, weight_decay, max_norm, decoder_frozen, gscale=1.0 / world, sq_norm=sq_parts)
