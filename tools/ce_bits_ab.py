#!/usr/bin/env python3
"""Bit-equality of two builds of libssc_hip.so on the vocabulary cross-entropy of the train step - the A/B behind a change of
csrc/cross_entropy.hip that must not move a bit: the same seeded inputs through the in-tree library and through a variant
(tools/build_variant.py, e.g. of the parent commit), each in a child process of its own, every output tensor compared on its int32
view (the driver of tools/cut_bits_ab.py).
Kernel inputs: every (V, ld, offset) of tests/test_label_smoothing_gpu.py, test_distill_gpu.py and test_unlikelihood_gpu.py at T = 5,
B = 3 with captions of 5, 3 and 2 steps and one more weightless step inside the first - a row without a weight holds NaN, the
teacher's too -, pad columns and the floats around the block poisoned.  ssc_ce_fwd / ssc_ce_bwd; the smoothed pair at eps 0 and 0.1;
the distilled pair over test_distill_gpu.COMBOS with the teacher laid out as the student and otherwise; the unlikelihood pair at
alpha 0.5 and 2.0 x eps 0 and 0.1, and once at T = 70 (candidate lanes in two waves).  Kept: lse with its [w*row] blocks, the
descriptors' rows, loss, nll, kd / ul and the whole logits block after the backward, pad columns included.
One-call inputs on the small model of tools/cut_bits_ab.py: one train step each with label smoothing 0.1, distillation, unlikelihood
and nothing (loss, kld, nll, kd, ul, every gradient).
    python tools/ce_bits_ab.py <variant dir under style-seqcvae_amd, e.g. _base>
Prints one JSON line: the tensors compared and the names of those that differ; exit code 1 if any does."""
import ctypes as C
import sys

from cut_bits_ab import PKG, ROOT, main

SHAPES = [(37, 37, 0), (451, 452, 0), (451, 452, 1), (777, 780, 0), (1024, 1024, 0), (1024, 1028, 1), (2003, 2004, 0), (90, 92, 1),
          (10000, 10000, 0)]
T_, B_ = 5, 3
LENGTHS = (5, 3, 2)
COMBOS = [(alpha, tau, eps) for alpha in (0.3, 1.0) for tau in (1.0, 2.0, 4.0) for eps in (0.0, 0.1)]   # test_distill_gpu.COMBOS
POISON = -7.5e8


def dump(path):
    sys.path[:0] = [ROOT, PKG]
    import torch
    from ssc_runtime import lib as L
    from ssc_runtime.engine import Distill
    from ssc_runtime.vocab import Vocabulary
    from var_updown.models import UpDownCaptioner
    lib = L.load()
    dev = "cuda"
    st = L.stream_ptr()
    out = {}

    def keep(name, t):
        assert name not in out, name
        out[name] = t.detach().cpu().contiguous().view(-1).view(torch.int32).clone()

    def block(m, w, ld, off):
        """the (T, B, V) matrix m as the device sees it: rows of ld floats from `off` on, weightless rows NaN, poison elsewhere"""
        rows, V = m.shape[0] * m.shape[1], m.shape[2]
        md = m.clone()
        md[w == 0] = float("nan")
        buf = torch.full((rows * ld + 8,), POISON)
        buf[off:off + rows * ld].view(rows, ld)[:, :V] = md.view(rows, V)
        return buf.to(dev)

    def case(V, T, B, lengths, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(T, B, V, generator=g) * 2.0
        x[1, 0] = torch.rand(V, generator=g) * 160.0 - 80.0      # spread over +-80: the running maximum moves
        s = torch.randn(T, B, V, generator=g) * 2.0
        s[0, 0, 1] = s[1, 1, V // 3] = float("-inf")
        w = torch.tensor([[1.0 if t < lengths[b] else 0.0 for b in range(B)] for t in range(T)])
        w[2, 0] = 0.0                                            # a weightless step inside a caption
        y = torch.randint(0, V, (T, B), generator=g)
        y[3, 0], y[4, 0], y[2, 1] = y[0, 0], y[1, 0], y[0, 1]    # repeats: unlikelihood candidates
        gl = torch.tensor([0.7, -1.3, 0.0] + [0.25] * (B - 3))[:B]
        return x, s, w, y, gl

    def pair(tag, fwd, bwd, xb, rows, B, extra):
        """fwd(lse, loss, nll) and bwd(lse) on the block xb; `extra`: name -> tensor the descriptor's calls wrote"""
        lse = torch.full((3 * rows,), -7.0, device=dev)
        loss = torch.full((B,), -7.0, device=dev)
        nll = torch.full_like(loss, -7.0)
        rc = (fwd(lse, loss, nll), bwd(lse))
        torch.cuda.synchronize()
        assert rc == (0, 0), (tag, rc)
        for name, t in dict(lse=lse, loss=loss, nll=nll, logits=xb, **extra).items():
            keep(f"{tag}/{name}", t)

    def kernels(V, ld, off, T, B, lengths, seed, what):
        x, s, w, y, gl = case(V, T, B, lengths, seed)
        rows = T * B
        yd, wd, nv, gld = y.to(dev), w.to(dev), w.sum(0).to(dev), gl.to(dev)
        common = lambda xb: (L.ptr(xb[off:]), ld, L.ptr(yd), L.ptr(wd), L.ptr(nv))
        shape = f"V{V}+{off}" + ("" if T == T_ else f"/T{T}")
        if "plain" in what:
            xb = block(x, w, ld, off)
            pair(f"plain/{shape}", lambda lse, loss, nll: lib._raw_ssc_ce_fwd(*common(xb), T, B, V, L.ptr(lse), L.ptr(loss), st),
                 lambda lse: lib._raw_ssc_ce_bwd(*common(xb), L.ptr(lse), L.ptr(gld), T, B, V, st), xb, rows, B, {})
        if "smooth" in what:
            for eps in (0.0, 0.1):
                xb = block(x, w, ld, off)
                pair(f"smooth/{shape}/eps{eps}",
                     lambda lse, loss, nll: lib._raw_ssc_ce_fwd_smooth(*common(xb), T, B, V, eps, L.ptr(lse), L.ptr(loss), L.ptr(nll), st),
                     lambda lse: lib._raw_ssc_ce_bwd_smooth(*common(xb), L.ptr(lse), L.ptr(gld), T, B, V, eps, st), xb, rows, B, {})
        if "distill" in what:
            for layout, (ldt, offt) in (("same", (ld, off)), ("other", (V + 3, (off + 2) % 4))):   # test_distill_gpu.teacher_layout
                for alpha, tau, eps in COMBOS:
                    xb, sb = block(x, w, ld, off), block(s, w, ldt, offt)
                    trows = torch.full((3 * rows,), -7.0, device=dev)
                    kdb = torch.full((B,), -7.0, device=dev)
                    d = L.Distill(sb[offt:].data_ptr(), ldt, alpha, tau, trows.data_ptr(), kdb.data_ptr())
                    pair(f"distill/{shape}/{layout}/a{alpha}/tau{tau}/eps{eps}",
                         lambda lse, loss, nll: lib._raw_ssc_ce_fwd_distill(*common(xb), T, B, V, eps, C.byref(d), L.ptr(lse), L.ptr(loss),
                                                                            L.ptr(nll), st),
                         lambda lse: lib._raw_ssc_ce_bwd_distill(*common(xb), L.ptr(lse), L.ptr(gld), T, B, V, eps, C.byref(d), st),
                         xb, rows, B, dict(rows=trows, kd=kdb, teacher=sb))
        if "unlike" in what:
            for alpha in (0.5, 2.0):
                for eps in (0.0, 0.1):
                    xb = block(x, w, ld, off)
                    trows = torch.full((2 * rows,), -7.0, device=dev)
                    ulb = torch.full((B,), -7.0, device=dev)
                    d = L.Unlikelihood(alpha, 1e-5, trows.data_ptr(), ulb.data_ptr())
                    pair(f"unlike/{shape}/a{alpha}/eps{eps}",
                         lambda lse, loss, nll: lib._raw_ssc_ce_fwd_unlike(*common(xb), T, B, V, eps, C.byref(d), L.ptr(lse), L.ptr(loss),
                                                                           L.ptr(nll), st),
                         lambda lse: lib._raw_ssc_ce_bwd_unlike(*common(xb), L.ptr(lse), L.ptr(gld), T, B, V, eps, C.byref(d), st),
                         xb, rows, B, dict(rows=trows, ul=ulb))

    for V, ld, off in SHAPES:
        kernels(V, ld, off, T_, B_, LENGTHS, 3000 + V + ld + off, ("plain", "smooth", "distill", "unlike"))
    kernels(451, 452, 1, 70, 3, (70, 40, 66), 77, ("unlike",))   # words first seen at a step >= 64: candidates of the second wave
    # ---- one train step each on a small model -----------------------------------------------------------------------------------------
    torch.manual_seed(0)
    V, F, E, H, A, Z, Lc = 1200, 64, 40, 48, 32, 16, 8
    model = UpDownCaptioner(Vocabulary.synthetic(V), F, E, H, A, max_caption_length=Lc, beam_size=1, z_space=Z, sentiment_vae=1,
                            senti_prior_multip=0.5, device=torch.device(dev)).to(dev)
    eng = model._engine()
    g = torch.Generator().manual_seed(5)
    Bt, R = 6, 6
    caps = torch.zeros(Bt, Lc, dtype=torch.long)
    for b in range(Bt):
        n = 3 + b % 5
        caps[b, :n] = torch.randint(2, 40, (n,), generator=g)    # a small range: words repeat inside a caption
    tf = torch.randn(Bt, R, F, generator=g).to(dev)
    senti = torch.randint(-1, 2, (Bt, 1), generator=g).float().to(dev)
    teps = torch.randn(Lc + 1, Bt, Z, generator=g).to(dev)
    scores = (torch.randn((Lc + 1) * Bt, V, generator=g) * 2.0).to(dev)
    for name, kw in (("plain", {}), ("smooth", dict(label_smoothing=0.1)),
                     ("distill", dict(label_smoothing=0.1, distill=Distill(scores, V, 0.5, 2.0))),
                     ("unlike", dict(label_smoothing=0.1, unlikelihood=0.5))):
        loss, kld = eng.forward(tf, caps.to(dev), senti, teps, **kw)
        for k, t in dict(loss=loss, kld=kld, nll=eng.nll(), kd=eng.kd(), ul=eng.ul()).items():
            keep(f"train_{name}/{k}", t)
        eng.backward(torch.full((Bt,), 1.0 / Bt, device=dev), torch.full((Bt,), 1.0 / (Bt * 750.0), device=dev))
        for k, t in sorted(eng.grad_dict().items()):
            keep(f"train_{name}/grad/{k}", t)
    torch.cuda.synchronize()
    torch.save(out, path)


if __name__ == "__main__":
    main(dump)
