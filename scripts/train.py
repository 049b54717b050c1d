#!/usr/bin/env python3
"""Train a Style-SeqCVAE captioner on MI355X - counterpart of the reference's var_updown/scripts/train.py:26-188 with
the same flags, config keys, seeds, optimiser (SGD momentum/weight-decay, LambdaLR linear decay; OPTIM.OPTIMIZER adam / adamw:
Adam or AdamW behind the same clip and decay, on all three paths), decoder-LSTM freeze
schedule, clip_grad_norm, scalar names and checkpoint layout ({"model": state_dict, "optimizer": ...}).

One process per GPU: `python scripts/train.py --config cfg.yaml --gpu-ids 0` or, for N GPUs,
`python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 scripts/train.py ... --gpu-ids 0 1 ...`
(the reference's nn.DataParallel path crashes for training: SURVEY §2.1).  OPTIM.BATCH_SIZE is the GLOBAL batch.
Data: --train-tensors file.pt (see ssc_runtime/data.py) or --synthetic N (random features / captions).
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL across processes (before HIP loads)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssc_runtime.config import Config  # noqa: E402
from ssc_runtime.data import SyntheticCaptionData, TensorFileData, cycle  # noqa: E402
from ssc_runtime.vocab import Vocabulary  # noqa: E402
from var_updown.models import UpDownCaptioner  # noqa: E402

parser = argparse.ArgumentParser("Train a Style-SeqCVAE UpDown captioner (MI355X).")
parser.add_argument("--config", required=True)
parser.add_argument("--config-override", default=[], nargs="*")
parser.add_argument("--gpu-ids", required=True, nargs="+", type=int)
parser.add_argument("--cpu-workers", type=int, default=0)
parser.add_argument("--in-memory", action="store_true")
parser.add_argument("--skip-validation", action="store_true", help="no validation pass even with --val-tensors")
parser.add_argument("--val-tensors", default="",
                    help="held-out .pt file (as --train-tensors, dense image_features): its captions are scored under the model "
                         "(teacher forcing, UpDownCaptioner.score_captions) and val_* scalars are appended to scalars.jsonl")
parser.add_argument("--val-every", type=int, default=1000, help="with --val-tensors: validate every K iterations and at the last one")
parser.add_argument("--val-samples", type=int, default=1, help="with --val-tensors: latent samples per caption")
parser.add_argument("--val-images", type=int, default=0, help="with --val-tensors: score the first M images (0: all)")
# (absent from the namespace unless given, as --reset-optimizer: off, and today's output unchanged)
parser.add_argument("--val-posterior-samples", type=int, default=argparse.SUPPRESS,
                    help="with --val-tensors: also score the held-out captions under the POSTERIOR branch with K noise draws each "
                         "(UpDownCaptioner.posterior_score_captions) and append val_elbo_nll_per_token, val_iwae_nll_per_token, "
                         "val_kl_per_token, val_active_units; 0: off")
parser.add_argument("--val-reconstruction", action="store_true", default=argparse.SUPPRESS,
                    help="with --val-tensors: also decode every held-out caption back from its own posterior latent path "
                         "(UpDownCaptioner.reconstruct_captions, beam search under a latent guide) and append val_recon_token_accuracy, "
                         "val_recon_exact_rate, val_recon_wer: how much of a caption its latents carry")
parser.add_argument("--serialization-dir", default="checkpoints/experiment")
parser.add_argument("--checkpoint-every", default=10000, type=int)
parser.add_argument("--start-from-checkpoint", default="")
parser.add_argument("--train-tensors", default="", help=".pt file with image_features / caption_tokens / sentiment")
parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images (BASELINE.md §4)")
parser.add_argument("--vocab-size", type=int, default=10000, help="vocabulary size for --synthetic")
parser.add_argument("--num-boxes", type=int, default=36)
parser.add_argument("--eps-source", default="device", choices=["cpu", "device"],
                    help="cpu: the reference's CPU randn stream per step; device: GPU RNG, no host traffic")
parser.add_argument("--zero-eps", action="store_true", help="testing: eps = 0 (deterministic z = mean)")
parser.add_argument("--stop-after", type=int, default=0, help="testing: stop after this iteration (NUM_ITERATIONS keeps defining the schedule)")
parser.add_argument("--attribute-table", default="",
                    help="SENTIMENT_VAE 2: json {attribute word: [Z_SPACE floats]} - the table the reference builds from its sentiment-GloVe / "
                         "SentiWordNet files (updown_captioner.py:79-93); only needed when obj_atts arrive as attribute strings")
parser.add_argument("--fused-optimizer", action="store_true",
                    help="clip + SGD (OPTIM.OPTIMIZER adam / adamw: clip + Adam / AdamW) in one HIP pass on the flat buffers instead of "
                         "torch.optim")
# (absent from the namespace unless given: the namespace of a command line without it is what it was before the flag existed)
parser.add_argument("--reset-optimizer", action="store_true", default=argparse.SUPPRESS,
                    help="with --start-from-checkpoint: load the model only, drop the checkpoint's optimiser state and start at "
                         "iteration 1 (the hand-over from cross-entropy training under SGD to self-critical training under Adam)")
parser.add_argument("--scst-references", default="",
                    help="train with self-critical steps (ssc_runtime/scst.py) instead of cross-entropy ones: sampled captions rewarded "
                         'against these references - COCO annotations {"annotations": [{"image_id", "caption"}]} or {image_id: [captions]}, '
                         "as scripts/evaluate.py reads them; with --synthetic any value: the synthetic captions are the references.  "
                         "Implies the fused optimiser; OPTIM.BATCH_SIZE counts images")
parser.add_argument("--scst-samples", type=int, default=5, help="with --scst-references: captions sampled per image")
parser.add_argument("--scst-baseline", default="loo", choices=["loo", "greedy", "none"],
                    help="loo: the mean reward of the image's other samples; greedy: the reward of the arg-max caption at zero noise")
parser.add_argument("--scst-sampler", default="multinomial", choices=["multinomial", "top-k", "top-p"],
                    help="the word sampler of the rollout (MODEL.DECODE_SAMPLER's names)")
parser.add_argument("--scst-temperature", type=float, default=1.0)
parser.add_argument("--scst-top-k", type=int, default=40)
parser.add_argument("--scst-top-p", type=float, default=0.9)
parser.add_argument("--scst-reward", default="0,0,0,0,0,1", help="reward weights B1,B2,B3,B4,R,C (default: CIDEr-D alone)")
parser.add_argument("--scst-max-steps", type=int, default=20, help="with --scst-references: longest sampled caption")
# (absent from the namespace unless given, as --reset-optimizer)
parser.add_argument("--distill-checkpoints", nargs="+", default=argparse.SUPPRESS,
                    help="knowledge distillation: 1..8 teacher checkpoints of this configuration (as this script writes them); the "
                         "cross-entropy steps then train against their per-word distributions with OPTIM.DISTILL_ALPHA (> 0) at "
                         "OPTIM.DISTILL_TEMPERATURE, several teachers combined as OPTIM.DISTILL_MODE says.  Loaded once, frozen")
parser.add_argument("--distill-weights", nargs="+", type=float, default=argparse.SUPPRESS,
                    help="with --distill-checkpoints: one positive weight per teacher (default: uniform)")


VAL_IMAGES_PER_CALL = 100


def validate(model, val, n_images, n_samples, seed, iteration, device):
    """Held-out likelihood of the captions of `val` under the model as it stands.  The noise comes from a generator of this pass's
    own seeded by (seed, iteration) and the model's mode is left alone: neither the global random state nor anything the
    training step reads is touched, so a run with validation trains exactly as the same run without it."""
    from ssc_runtime.inference import CaptionScores
    gen = torch.Generator(device=device)
    gen.manual_seed((int(seed) * 1000003 + int(iteration)) % (2 ** 63))
    Z = model.z_space
    parts = []
    for lo in range(0, n_images, VAL_IMAGES_PER_CALL):
        hi = min(lo + VAL_IMAGES_PER_CALL, n_images)
        caps = val.caps[lo:hi]
        G = (hi - lo) * n_samples
        eps = [torch.randn(G, Z, device=device, generator=gen) for _ in range(caps.size(1) + 1)]
        feats = val.feats[lo:hi].to(device)
        obj = val.obj[lo:hi, : feats.size(1)].to(device) if val.obj is not None else None
        parts.append(model.score_captions(feats, caps, sentiment=val.senti[lo:hi, 0].to(device), obj_atts=obj, n_samples=n_samples,
                                          want_ranks=True, eps_steps=eps))
    s = CaptionScores.concat(parts).summary()
    return {"val_nll_per_token": s["nll_per_token"], "val_perplexity": s["perplexity"],
            "val_marginal_nll_per_token": s["marginal_nll_per_token"], "val_top1": s["top1"]}


POSTERIOR_TAG = 0x706F7374   # keeps the posterior pass's noise apart from the prior pass's of the same (seed, iteration)


def validate_posterior(model, val, n_images, n_samples, seed, iteration, device):
    """ELBO, importance-weighted bound and KL diagnostics of the captions of `val` under the posterior branch of the model as it
    stands.  As validate(): a generator of this pass's own seeded by (seed, iteration) plus a tag, the model's mode left alone, a
    forward on a workspace of its own - a run with it trains exactly as the same run without it."""
    from ssc_runtime.inference import PosteriorScores
    gen = torch.Generator(device=device)
    gen.manual_seed(((int(seed) * 1000003 + int(iteration)) * 1000003 + POSTERIOR_TAG) % (2 ** 63))
    Z = model.z_space
    parts = []
    for lo in range(0, n_images, VAL_IMAGES_PER_CALL):
        hi = min(lo + VAL_IMAGES_PER_CALL, n_images)
        caps = val.caps[lo:hi]
        eps = torch.randn(caps.size(1) + 1, (hi - lo) * n_samples, Z, device=device, generator=gen)
        feats = val.feats[lo:hi].to(device)
        obj = val.obj[lo:hi, : feats.size(1)].to(device) if val.obj is not None else None
        parts.append(model.posterior_score_captions(feats, caps, sentiment=val.senti[lo:hi, 0].to(device), obj_atts=obj,
                                                    n_samples=n_samples, eps=eps))
    s = PosteriorScores.concat(parts).summary()
    return {"val_elbo_nll_per_token": s["elbo_nll_per_token"], "val_iwae_nll_per_token": s["iwae_nll_per_token"],
            "val_kl_per_token": s["kl_per_token"], "val_active_units": s["active_units"]}


def scst_sampler(args):
    """The word sampler the --scst-sampler / --scst-temperature / --scst-top-k / --scst-top-p flags describe."""
    from ssc_runtime import sampling
    if args.scst_sampler == "top-k":
        return sampling.TopKSampler(k=args.scst_top_k, temperature=args.scst_temperature)
    if args.scst_sampler == "top-p":
        return sampling.TopPSampler(p=args.scst_top_p, temperature=args.scst_temperature)
    return sampling.MultinomialSampler(temperature=args.scst_temperature)


def scst_references(args, data, vocabulary):
    """{image_id: [captions]} of --scst-references; with --synthetic the synthetic captions, spelled with the vocabulary's words."""
    from ssc_runtime.evaluation import load_references
    if not args.synthetic:
        return load_references(args.scst_references)
    refs = {}
    for iid, cap in zip(data.image_id.tolist(), data.caps.tolist()):
        refs.setdefault(iid, []).append(" ".join(vocabulary.get_token_from_index(t) for t in cap if t != 0))
    return refs


def distill_plan(_A, _C):
    """(checkpoint paths, weights or None, alpha, temperature, mode) of a distilling run, None for one that does not distil; the
    flags' and keys' errors as SystemExit, before anything is loaded."""
    paths = getattr(_A, "distill_checkpoints", None)
    weights = getattr(_A, "distill_weights", None)
    alpha = _C.OPTIM.DISTILL_ALPHA
    if paths is None:
        if weights is not None:
            raise SystemExit("--distill-weights needs --distill-checkpoints")
        if alpha > 0:
            raise SystemExit(f"OPTIM.DISTILL_ALPHA {alpha} needs teachers: pass --distill-checkpoints")
        return None
    if not 1 <= len(paths) <= 8:
        raise SystemExit(f"--distill-checkpoints takes 1 to 8 checkpoints; found {len(paths)}")
    if weights is not None and (len(weights) != len(paths) or any(not 0.0 < w < float("inf") for w in weights)):
        raise SystemExit(f"--distill-weights takes one positive finite weight per teacher ({len(paths)}); found {weights}")
    if not alpha > 0:
        raise SystemExit("--distill-checkpoints needs OPTIM.DISTILL_ALPHA > 0 (the weight of the teachers' term in the loss)")
    if _C.OPTIM.SCHEDULED_SAMPLING_START >= 0:
        raise SystemExit("--distill-checkpoints (distillation) cannot be combined with a configured scheduled sampling "
                         "(OPTIM.SCHEDULED_SAMPLING_START >= 0): the teachers' distributions are those of the ground-truth inputs")
    return list(paths), (list(weights) if weights is not None else None), alpha, _C.OPTIM.DISTILL_TEMPERATURE, _C.OPTIM.DISTILL_MODE


def validate_reconstruction(model, val, n_images, device):
    """Reconstruction of the captions of `val` through z with the model as it stands: the mean path of the posterior branch (no
    noise), the beam search under it, the words compared on the device.  Deterministic; draws nothing from any random stream, the
    model's mode left alone, a forward on a workspace of its own - a run with it trains exactly as the same run without it."""
    from ssc_runtime.guide import match_summary
    parts = []
    for lo in range(0, n_images, VAL_IMAGES_PER_CALL):
        hi = min(lo + VAL_IMAGES_PER_CALL, n_images)
        caps = val.caps[lo:hi]
        caps = caps[:, 0] if caps.dim() == 3 else caps   # (the first caption of every image)
        rec = model.reconstruct_captions(val.feats[lo:hi].to(device), caps, sentiment=val.senti[lo:hi, 0].to(device), prior_samples=0)
        parts.append(rec.match)
    s = match_summary(torch.cat(parts))
    return {"val_recon_token_accuracy": s["token_accuracy"], "val_recon_exact_rate": s["exact_rate"], "val_recon_wer": s["wer"]}


def main():
    _A = parser.parse_args()
    _C = Config(_A.config, _A.config_override)
    plan = distill_plan(_A, _C)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    validating = bool(_A.val_tensors) and not _A.skip_validation
    if validating and world > 1:
        # a pass on one rank alone stalls the peers' gradient exchange (ssc_runtime/xgmi.py); sharding it is not built
        raise SystemExit("--val-tensors runs on one GPU only (WORLD_SIZE = 1): a validation pass on rank 0 alone would stall the "
                         "other ranks' gradient exchange; train on several GPUs with --skip-validation and score checkpoints apart")
    if validating and (_A.val_samples < 1 or _A.val_images < 0):
        raise SystemExit("--val-samples must be at least 1 and --val-images at least 0")
    posterior_samples = getattr(_A, "val_posterior_samples", 0)
    if posterior_samples < 0:
        raise SystemExit("--val-posterior-samples must be at least 0")
    reconstruction = getattr(_A, "val_reconstruction", False)
    if reconstruction and not _A.val_tensors:
        raise SystemExit("--val-reconstruction needs --val-tensors")
    if -1 in _A.gpu_ids:
        raise SystemExit("--gpu-ids -1 (CPU) is not available: this build has no CPU path")
    gpu = _A.gpu_ids[local % len(_A.gpu_ids)]
    torch.cuda.set_device(gpu)
    device = torch.device("cuda", gpu)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
    if rank == 0:
        print(_C)
        os.makedirs(_A.serialization_dir, exist_ok=True)
        _C.dump(os.path.join(_A.serialization_dir, "config.yml"))

    random.seed(_C.RANDOM_SEED)
    np.random.seed(_C.RANDOM_SEED)
    torch.manual_seed(_C.RANDOM_SEED)

    if _A.synthetic:
        vocabulary = Vocabulary.synthetic(_A.vocab_size)
        sv2 = _C.MODEL.SENTIMENT_VAE == 2 and not _C.MODEL.SIMPLE_VAE
        data = SyntheticCaptionData(_A.synthetic, _A.num_boxes, _C.MODEL.IMAGE_FEATURE_SIZE, _C.DATA.MAX_CAPTION_LENGTH,
                                    _A.vocab_size, seed=1234, obj_dim=_C.MODEL.Z_SPACE if sv2 else 0)
    else:
        vocabulary = Vocabulary.from_files(_C.DATA.VOCABULARY)
        if not _A.train_tensors:
            raise SystemExit("the h5 / nltk dataset readers are not built (h5py, nltk are not installable here): pass "
                             "--train-tensors file.pt (ssc_runtime/data.py: dense or ragged region features) or --synthetic N")
        data = TensorFileData(_A.train_tensors)
    val = None
    if validating:
        val = TensorFileData(_A.val_tensors)
        if val.feats is None:
            raise SystemExit("--val-tensors needs dense image_features (N, R, F)")
    if _C.OPTIM.BATCH_SIZE % world:
        raise SystemExit("OPTIM.BATCH_SIZE (global) must be divisible by the number of ranks")

    extra = {}
    if _C.MODEL.SENTIMENT_VAE == 2:
        # the attribute table (word -> Z_SPACE floats) the reference reads from hard-coded pickle paths (updown_captioner.py:79-86).
        # Needed only for obj_atts given as attribute STRINGS; the tensor files / the synthetic source carry the per-region means.
        extra["mean_choice"] = {k: np.asarray(v) for k, v in json.load(open(_A.attribute_table)).items()} if _A.attribute_table else {}
    model = UpDownCaptioner.from_config(_C, vocabulary=vocabulary, cbs_simple=_C.MODEL.CBS_SIMPLE, device=device, **extra).to(device)
    model.eps_source = _A.eps_source
    model.train()
    eng = model._engine()
    smoothing = model.label_smoothing   # OPTIM.LABEL_SMOOTHING: the cross-entropy steps; nll (the unsmoothed loss) is then logged too
    if smoothing > 0 and _A.scst_references and rank == 0:
        print(f"OPTIM.LABEL_SMOOTHING {smoothing} is ignored by the self-critical steps (--scst-references): the advantage-weighted "
              "loss is no likelihood target")
    # OPTIM.KL_ANNEAL* / OPTIM.FREE_BITS*: the cross-entropy steps.  beta of iteration i (counted from 1) is kl_beta(i - 1, ...), a
    # function of the iteration number alone, so a resumed run continues the schedule.  The floored KL enters the objective,
    # 2kld_loss stays the raw KL of the same forward
    from ssc_runtime.schedule import kl_beta_from_config
    free_bits, free_bits_mode = model.free_bits, model.free_bits_mode
    if (free_bits > 0 or _C.OPTIM.KL_ANNEAL != "none") and _A.scst_references and rank == 0:
        print(f"OPTIM.KL_ANNEAL {_C.OPTIM.KL_ANNEAL} / OPTIM.FREE_BITS {free_bits} are ignored by the self-critical steps "
              "(--scst-references): they take the KL as it is, with the constant MODEL.KLD_WEIGHT")
    # OPTIM.SCHEDULED_SAMPLING_*: the cross-entropy steps, on the fused and the autograd path.  The probability of iteration i
    # (counted from 1) is ss_prob(i - 1, ...), as beta is; decisions and draws are seeded by (RANDOM_SEED, iteration, rank), so a
    # resumed run draws what the uninterrupted run would have drawn
    from ssc_runtime.schedule import ss_prob_from_config, ss_sampler_from_config, ss_seed
    ss_configured = _C.OPTIM.SCHEDULED_SAMPLING_START >= 0
    ss_sampler = ss_sampler_from_config(_C.OPTIM)
    if ss_configured and _A.scst_references and rank == 0:
        print(f"OPTIM.SCHEDULED_SAMPLING_START {_C.OPTIM.SCHEDULED_SAMPLING_START} is ignored by the self-critical steps "
              "(--scst-references): their rollout already feeds the model its own words")
    # --distill-checkpoints / OPTIM.DISTILL_*: the cross-entropy steps, on the fused and the autograd path.  One set of frozen
    # teachers per rank, loaded once; every step they run their forwards on the step's minibatch and noise ahead of the student's
    teacher = None
    if plan is not None and _A.scst_references:
        if rank == 0:
            print(f"--distill-checkpoints / OPTIM.DISTILL_ALPHA {plan[2]} are ignored by the self-critical steps (--scst-references): "
                  "the advantage-weighted loss is no likelihood target")
    elif plan is not None:
        from ssc_runtime.distill import DistillTeacher
        paths, weights, kd_alpha, kd_tau, kd_mode = plan
        members = []
        for path in paths:
            sd = torch.load(path, map_location=device, weights_only=True)["model"]
            members.append(({k: v for k, v in sd.items()}, eng.dims))
        teacher = DistillTeacher(members, weights, kd_mode, student_dims=eng.dims, device=device)
        model.distill(teacher, kd_alpha, kd_tau)   # (the autograd path; the fused path passes distill= itself)
    # OPTIM.UNLIKELIHOOD_ALPHA: the cross-entropy steps, on the fused and the autograd path (the module carries it there); ul, the
    # unweighted term of the same forward, is then logged beside nll
    unlikelihood = model.unlikelihood
    if unlikelihood > 0 and _A.scst_references and rank == 0:
        print(f"OPTIM.UNLIKELIHOOD_ALPHA {unlikelihood} is ignored by the self-critical steps (--scst-references): the "
              "advantage-weighted loss is no likelihood target")
    from ssc_runtime.engine import OptimSpec, check_optimizer_state_kind
    kind = _C.OPTIM.OPTIMIZER
    spec = None   # the fused paths' optimiser; None: SGD with OPTIM.MOMENTUM / WEIGHT_DECAY, as before the key existed
    if kind == "sgd":
        optimizer = torch.optim.SGD(model.parameters(), lr=_C.OPTIM.LR, momentum=_C.OPTIM.MOMENTUM,
                                    weight_decay=_C.OPTIM.WEIGHT_DECAY)
    else:
        spec = OptimSpec(kind=kind, betas=tuple(_C.OPTIM.ADAM_BETAS), eps=_C.OPTIM.ADAM_EPS)
        optimizer = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(
            model.parameters(), lr=_C.OPTIM.LR, betas=spec.betas, eps=spec.eps, weight_decay=_C.OPTIM.WEIGHT_DECAY)
    # Learning rate: the reference's LambdaLR(1 - it / NUM_ITERATIONS) stepped once per iteration (train.py:132-134,176) gives
    # iteration i the rate LR * (1 - (i - 1) / N).  It is computed from the iteration number on BOTH paths, so a resumed run
    # continues the decay where it stopped (a fresh LambdaLR would restart at LR).
    eng.dp_autograd = world > 1 and not (_A.fused_optimizer or _A.scst_references)
    named = list(model.named_parameters())
    start_iteration = 1
    if _A.start_from_checkpoint:
        # Layout {"model": state_dict, "optimizer": SGD (or Adam / AdamW) state_dict} as written by the reference's CheckpointManager
        # (updown-baseline/updown/utils/checkpointing.py:81-112); the iteration rides inside the optimizer entry
        # (the reference's train.py:143-149 loads every other top-level key into the model).
        ckpt = torch.load(_A.start_from_checkpoint, map_location=device, weights_only=True)
        model.load_state_dict(ckpt["model"])
        osd = None if getattr(_A, "reset_optimizer", False) else ckpt.get("optimizer")
        if osd is not None:
            check_optimizer_state_kind(osd, kind)   # SGD state under an Adam kind (or the reverse): stop, naming both
            if _A.fused_optimizer or _A.scst_references:
                eng.load_optimizer_state_dict(named, osd, spec)
            else:
                for st in osd["state"].values():   # torch.optim.Adam keeps its step counts on the host
                    if "step" in st:
                        st["step"] = st["step"].cpu()
                optimizer.load_state_dict({"state": osd["state"], "param_groups": osd["param_groups"]})
            start_iteration = int(osd.get("iteration", 0)) + 1   # correct resume (the reference restarts at 1: train.py:149)
    # batch i of a run is a function of (seed, i): a resumed run continues the data order where it stopped
    scst = None
    if _A.scst_references:
        from ssc_runtime.evaluation import CaptionReferences
        from ssc_runtime.scst import SelfCritical, parse_reward_weights, scst_seed
        scst = SelfCritical(eng, model._dec, CaptionReferences(scst_references(_A, data, vocabulary), device=device), vocabulary,
                            n_samples=_A.scst_samples, sampler=scst_sampler(_A), baseline=_A.scst_baseline,
                            reward_weights=parse_reward_weights(_A.scst_reward), max_steps=_A.scst_max_steps)
    loader = cycle(data, _C.OPTIM.BATCH_SIZE // world, device, rank, world, seed=_C.RANDOM_SEED, start_batch=start_iteration - 1)
    log = open(os.path.join(_A.serialization_dir, "scalars.jsonl"), "a") if rank == 0 else None

    t0 = time.time()
    for iteration in range(start_iteration, _C.OPTIM.NUM_ITERATIONS + 1):
        train_decoder = (iteration > _C.OPTIM.EPOCH_START_DECODER_TRAINING
                         or iteration % _C.OPTIM.BEFORE_UPDATE_DECODER_EVERY == 0)   # train.py:156-161
        for p in model._updown_cell._language_lstm_cell_decoder.parameters():
            p.requires_grad = train_decoder
        if _A.stop_after and iteration > _A.stop_after:
            break
        batch = next(loader)
        lr = _C.OPTIM.LR * (1 - (iteration - 1) / _C.OPTIM.NUM_ITERATIONS)
        if _A.zero_eps:
            Bz, Lz = batch["caption_tokens"].shape
            model._eps_override = torch.zeros(Lz + 1, Bz, _C.MODEL.Z_SPACE, device=device)
        scst_stats = None
        beta = 1.0 if scst is not None else kl_beta_from_config(_C.OPTIM, iteration - 1)
        kld_free = None   # the floored KL that entered the objective (OPTIM.FREE_BITS > 0)
        ss_p = ss_prob_from_config(_C.OPTIM, iteration - 1) if scst is None else 0.0
        ss_args = dict(ss_prob=ss_p, ss_sampler=ss_sampler, ss_seed=ss_seed(_C.RANDOM_SEED, iteration, rank)) if ss_p > 0 else {}
        if scst is not None:
            # rollout noise and word draws are a function of (RANDOM_SEED, iteration, rank): a resumed run draws what this one would
            loss_b, kld_b, scst_stats = scst.step(batch["image_features"], batch["image_id"].tolist(), batch["sentiment"], lr=lr,
                                                  kld_weight=_C.MODEL.KLD_WEIGHT, momentum=_C.OPTIM.MOMENTUM,
                                                  weight_decay=_C.OPTIM.WEIGHT_DECAY, max_norm=_C.OPTIM.CLIP_GRADIENTS,
                                                  decoder_frozen=not train_decoder, seed=scst_seed(_C.RANDOM_SEED, iteration, rank),
                                                  obj_atts=batch.get("obj_atts"), optim=spec)
            reconstr_loss, kld_loss = loss_b.mean(), kld_b.mean()
            loss = reconstr_loss + kld_loss / _C.MODEL.KLD_WEIGHT
        elif _A.fused_optimizer:
            B, L = batch["caption_tokens"].shape
            eps = model._draw_eps(L + 1, B, device)
            kd_args = {}
            if teacher is not None:
                kd_args["distill"] = teacher.distill(batch["image_features"], batch["caption_tokens"], batch["sentiment"], eps, kd_alpha,
                                                     kd_tau, batch.get("obj_atts"))
            loss_b, kld_b = eng.train_step(batch["image_features"], batch["caption_tokens"], batch["sentiment"], eps, lr=lr,
                                           kld_weight=_C.MODEL.KLD_WEIGHT, momentum=_C.OPTIM.MOMENTUM,
                                           weight_decay=_C.OPTIM.WEIGHT_DECAY, max_norm=_C.OPTIM.CLIP_GRADIENTS,
                                           decoder_frozen=not train_decoder, obj_atts=batch.get("obj_atts"), optim=spec,
                                           label_smoothing=smoothing, kl_beta=beta, free_bits=free_bits,
                                           free_bits_mode=free_bits_mode, unlikelihood=unlikelihood,
                                           unlikelihood_clamp=model.unlikelihood_clamp, **ss_args, **kd_args)
            reconstr_loss, kld_loss = loss_b.mean(), eng.kld_raw().mean()
            kld_free = kld_b.mean() if free_bits > 0 else None
            loss = reconstr_loss + beta * kld_b.mean() / _C.MODEL.KLD_WEIGHT
        else:
            optimizer.zero_grad()
            if ss_configured:
                model.scheduled_sampling(ss_p, ss_args.get("ss_seed", 0), ss_sampler)
            out = model(batch["image_features"], batch.get("obj_atts"), None, batch["caption_tokens"], batch["sentiment"])
            reconstr_loss, kld_loss = out["loss"].mean(), eng.kld_raw().mean()
            kld_free = out["kld"].mean() if free_bits > 0 else None
            loss = reconstr_loss + beta * out["kld"].mean() / _C.MODEL.KLD_WEIGHT
            for group in optimizer.param_groups:
                group["lr"] = lr
            loss.backward()   # world > 1: the flat gradient buffer is all-reduced once inside backward (eng.dp_autograd)
            torch.nn.utils.clip_grad_norm_(model.parameters(), _C.OPTIM.CLIP_GRADIENTS)
            optimizer.step()
        if rank == 0 and (iteration % 100 == 0 or iteration == start_iteration or _C.OPTIM.NUM_ITERATIONS <= 100):
            rec = {"iteration": iteration, "1reconstr_loss": float(reconstr_loss), "2kld_loss": float(kld_loss),
                   "3loss": float(loss), "4learning_rate": lr, "elapsed_s": time.time() - t0}
            if teacher is not None:
                rec["kd"] = float(eng.kd().mean())     # tau^2 KL(teacher || student) of the same forward (this rank's rows)
            if unlikelihood > 0 and scst is None:
                rec["ul"] = float(eng.ul().mean())     # - sum log(1 - p[repeated word]) of the same forward (this rank's rows), unweighted
            if (smoothing > 0 or teacher is not None or unlikelihood > 0) and scst is None:
                rec["nll"] = float(eng.nll().mean())   # the unsmoothed loss of the same forward (this rank's rows)
            if scst is None:
                rec["kl_beta"] = beta
                if kld_free is not None:
                    rec["kld_free"] = float(kld_free)
                    if free_bits_mode == "dim":   # latent dimensions whose minibatch mean KL is above the floor (this rank's rows)
                        rec["active_dims"] = int(eng.free_bits_view("gate_dim").sum())
            if ss_configured and scst is None:
                rec["ss_prob"] = ss_p
                # the share of the weighted positions (this rank's rows) the model's own word was fed at: read back here only
                n_weighted = int((batch["caption_tokens"] != 0).sum()) + batch["caption_tokens"].size(0)
                rec["ss_fed_share"] = float(eng.fed_mask().sum()) / max(n_weighted, 1)
            if scst_stats is not None:
                st = scst_stats.tolist()
                rec.update({"5reward": st[0], "6baseline": st[1], "7abs_advantage": st[2], "8no_end_share": st[3]})
            log.write(json.dumps(rec) + "\n")
            log.flush()
            if iteration % 2000 == 0 or iteration == start_iteration:
                print("{:6f}    {:6f}    {:6f}".format(rec["3loss"], rec["1reconstr_loss"], rec["2kld_loss"]))
        last = iteration == _C.OPTIM.NUM_ITERATIONS or (_A.stop_after and iteration == _A.stop_after)
        if val is not None and rank == 0 and (last or (_A.val_every > 0 and iteration % _A.val_every == 0)):
            rec = {"iteration": iteration}
            n_val = min(_A.val_images or len(val), len(val))
            rec.update(validate(model, val, n_val, _A.val_samples, _C.RANDOM_SEED, iteration, device))
            if posterior_samples > 0:
                rec.update(validate_posterior(model, val, n_val, posterior_samples, _C.RANDOM_SEED, iteration, device))
            if reconstruction:
                rec.update(validate_reconstruction(model, val, n_val, device))
            log.write(json.dumps(rec) + "\n")
            log.flush()
        if rank == 0 and iteration % _A.checkpoint_every == 0:
            if _A.fused_optimizer or scst is not None:
                osd = eng.optimizer_state_dict(named, lr, _C.OPTIM.MOMENTUM, _C.OPTIM.WEIGHT_DECAY, iteration, spec)
            else:
                osd = optimizer.state_dict()
                osd["iteration"] = iteration
            torch.save({"model": model.state_dict(), "optimizer": osd},
                       os.path.join(_A.serialization_dir, f"checkpoint_{iteration}.pth"))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
