"""Knowledge distillation: the teacher side of TrainEngine.forward(..., distill=) (include/ssc.h: ssc_distill).

A DistillTeacher holds 1..8 frozen TrainEngines of the student's architecture.  scores() runs each member's plain teacher-forced
forward on the student's minibatch - the same captions and the same noise eps, so each teacher decodes its own posterior sample of
the same noise - and returns the (T*B, V) matrix the student's cross-entropy is trained against: one member's raw logits as they
stand in its workspace, or ssc_ensemble_combine_rows over several members' logits (log-probs of the weighted mixture, mode "prob"
or "logprob" as in ensemble decoding).  The temperature is applied by the student's loss, to that matrix."""
import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import lib as _lib
from .decode import ENSEMBLE_MODES, ensemble_weights
from .engine import Distill, ModelDims, TrainEngine, check_distill

ARCH_FIELDS = ("V", "E", "H", "A", "F", "Z", "S", "tied", "kld_mode", "pm_scale", "prior_var", "pad", "boundary")


def same_architecture(a: ModelDims, b: ModelDims) -> bool:
    """Whether two ModelDims describe one architecture and vocabulary (the numerics mode and the smoothing are per engine / per call)."""
    return all(getattr(a, f) == getattr(b, f) for f in ARCH_FIELDS)


class DistillTeacher:
    """members: 1..8 TrainEngines, or (state_dict, ModelDims) pairs (an engine is then built and loaded on first use, on `device`).
    weights: positive, any scale (None: uniform); mode "prob" | "logprob": how several members are combined (ssc_ensemble_combine_rows).
    student_dims: the student's ModelDims - every member must be of its architecture and vocabulary (ValueError otherwise)."""

    def __init__(self, members, weights=None, mode: str = "prob", student_dims: Optional[ModelDims] = None, device=None):
        members = list(members)
        if not 1 <= len(members) <= _lib.SSC_ENSEMBLE_MAX:
            raise ValueError(f"distillation: 1 .. {_lib.SSC_ENSEMBLE_MAX} teachers, got {len(members)}")
        if mode not in ENSEMBLE_MODES:
            raise ValueError(f"distillation: unknown mode {mode!r} (one of {sorted(ENSEMBLE_MODES)})")
        dims = []
        for i, m in enumerate(members):
            if isinstance(m, TrainEngine):
                dims.append(m.dims)
            elif isinstance(m, (tuple, list)) and len(m) == 2 and isinstance(m[0], dict) and isinstance(m[1], ModelDims):
                dims.append(m[1])
            else:
                raise ValueError(f"distillation: teacher {i} is neither a TrainEngine nor a (state_dict, ModelDims) pair: {type(m).__name__}")
        lead = student_dims if student_dims is not None else dims[0]
        for i, d in enumerate(dims):
            if not same_architecture(d, lead):
                raise ValueError(f"distillation: teacher {i} has another architecture or vocabulary than "
                                 f"{'the student' if student_dims is not None else 'teacher 0'}: {d} != {lead}")
        self.weights = ensemble_weights(weights, len(members))
        self.mode = mode
        self.dims = dims[0]
        self._members = members
        self._device = device
        self._engines: Optional[Sequence[TrainEngine]] = None
        self._out = None

    def check_student(self, dims: ModelDims):
        if not same_architecture(self.dims, dims):
            raise ValueError(f"distillation: the teachers have another architecture or vocabulary than the student: {self.dims} != {dims}")

    @property
    def engines(self):
        """The members as TrainEngines (built from their state dicts on first use; frozen: nothing here ever updates them)."""
        if self._engines is None:
            engs = []
            for m in self._members:
                if not isinstance(m, TrainEngine):
                    sd, dims = m
                    m = TrainEngine(dims, self._device)
                    m.load_state_dict(sd)
                engs.append(m)
            if any(e.params.flat.device != engs[0].params.flat.device for e in engs[1:]):
                raise ValueError("distillation: the teachers live on different devices")
            self._engines = engs
        return self._engines

    def scores(self, feats, caps, sentiment, eps, obj_atts=None):
        """-> (scores, ld): the (T*B, >= V) float32 matrix of the teachers' per-word scores for this minibatch, time-major as the
        train step's rows, and its leading dimension.  One member: its workspace's logits block itself (raw logits, no copy);
        several: one ssc_ensemble_combine_rows over the members' blocks into a buffer of this object (log-probs of the mixture).
        Rows without a target (w = 0) hold whatever they hold: nobody reads them.  Valid until the next scores() call - the
        student's forward AND its backward read it."""
        engs = self.engines
        views = []
        for e in engs:
            e.forward(feats, caps, sentiment, eps, obj_atts)      # plain: label smoothing 0, no floor, no sampling
            views.append(e.workspace_view(9))
        ld = views[0].stride(1)
        if len(engs) == 1:
            return views[0], ld
        T, B, V = views[0].shape
        if self._out is None or self._out.numel() != T * B * ld:
            self._out = torch.empty(T * B * ld, dtype=torch.float32, device=engs[0].device)
        M = len(engs)
        ptrs = (_lib.vp * M)(*[v.data_ptr() for v in views])
        logw = (C.c_float * M)(*[math.log(w) for w in self.weights])
        d = _lib.EnsembleRowsDesc(M, ptrs, ld, logw, ENSEMBLE_MODES[self.mode])
        engs[0].lib.ssc_ensemble_combine_rows(C.byref(d), T * B, V, None, None, 0, _lib.ptr(self._out), ld, _lib.stream_ptr())
        return self._out.view(T, B, ld)[:, :, :V], ld

    def distill(self, feats, caps, sentiment, eps, alpha, temperature=1.0, obj_atts=None) -> Optional[Distill]:
        """The `distill=` argument of the student's forward on this minibatch; None for alpha 0 (no teacher forward is run)."""
        alpha, temperature = check_distill(alpha, temperature)
        if alpha == 0.0:
            return None
        t, ld = self.scores(feats, caps, sentiment, eps, obj_atts)
        return Distill(t, ld, alpha, temperature)
