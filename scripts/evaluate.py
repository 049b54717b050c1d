#!/usr/bin/env python3
"""Diverse-caption evaluation on MI355X - counterpart of the reference's eval/eval.py: oracle and mean BLEU-1..4, ROUGE-L and
CIDEr-D over the N captions per image of a predictions JSON (what scripts/inference.py writes), Div-1 / Div-2 over all captions
and over the top 5 by CIDEr, and style precision / recall against a wordforms TSV.  METEOR is not computed.  --set-diversity adds the caption-set numbers
(each image's N captions against each other): mBLEU-1..4, Self-CIDEr and the share of distinct captions.  --consensus-bank adds best-1 after
consensus re-ranking: every image's pick by mean CIDEr-D against the captions of its nearest bank images (features from --query-tensors).
--select-k K keeps K captions per image that are good and different from each other (MBR / MMR / greedy DPP on the caption kernel with the
bank's document frequencies, the consensus scores as quality: no test reference is involved) and reports that subset's own numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

import torch  # noqa: E402

from ssc_runtime.evaluation import (CaptionReferences, format_summary, load_predictions, load_references,  # noqa: E402
                                    style_words_from_tsv)

parser = argparse.ArgumentParser("Score diverse captions (oracle / mean BLEU, ROUGE-L, CIDEr-D, Div-n, style) on the GPU.")
parser.add_argument("--predictions", required=True, help='[{"image_id", "caption"}, ...]: N captions per image, in file order')
parser.add_argument("--references", required=True,
                    help='COCO annotations {"annotations": [{"image_id", "caption"}, ...]} or {image_id: [captions]}')
parser.add_argument("--style-wordforms", default="", help="wordforms TSV whose words are the style words (senti_prec / senti_rec)")
parser.add_argument("--gpu-ids", default=[0], nargs="+", type=int)
parser.add_argument("--output-json", default="", help="write the summary here")
parser.add_argument("--set-diversity", action="store_true",
                    help="also compare each image's captions with each other: mBLEU-1..4 (lower = more diverse), Self-CIDEr, unique")
parser.add_argument("--top5-output", default="", help="write the 5 captions per image of highest CIDEr-D here (eval.py's filtered list)")
parser.add_argument("--consensus-bank", default="", help="a bank of training images (scripts/build_consensus_bank.py): adds the consensus lines")
parser.add_argument("--query-tensors", default="",
                    help="with --consensus-bank: a tensor file (image_features or features + num_boxes, image_id) with the region "
                         "features of every prediction image")
parser.add_argument("--consensus-k", type=int, default=60, help="nearest bank images per prediction image")
parser.add_argument("--consensus-output", default="", help="write the consensus pick of every image here")
parser.add_argument("--select-k", type=int, default=0,
                    help="with --consensus-bank: keep K captions per image that are good and different from each other; adds the "
                         "'select subset' lines")
parser.add_argument("--select-method", default="dpp", choices=["dpp", "mmr", "mbr"],
                    help="greedy DPP MAP (quality x diversity), maximal marginal relevance, or minimum Bayes risk under the caption kernel")
parser.add_argument("--select-quality", default="consensus", choices=["consensus", "logprob"],
                    help="the per-caption quality: the consensus scores (a predictions file holds no log-probs: logprob is "
                         "scripts/inference.py's)")
parser.add_argument("--select-lambda", type=float, default=0.5, help="mmr: weight of the quality against the similarity to a pick")
parser.add_argument("--select-theta", type=float, default=1.0, help="dpp: weight of the quality")
parser.add_argument("--select-output", default="", help="write the K captions per image here, in pick order (a predictions file)")


def consensus_of(a, preds, device):
    from ssc_runtime.data import TensorFileData
    from ssc_runtime.evaluation import ConsensusBank, pool_rows
    if not a.query_tensors:
        raise SystemExit("--consensus-bank needs --query-tensors (the prediction images' region features)")
    data = TensorFileData(a.query_tensors)
    row = {}
    for r, iid in enumerate(data.image_id.tolist()):
        row.setdefault(iid, r)
    for iid in preds:
        if iid not in row:
            raise SystemExit(f"--query-tensors holds no features for prediction image {iid!r}")
    bank = ConsensusBank.load(a.consensus_bank, device=device)
    pooled = pool_rows(data, [row[iid] for iid in preds], device)
    # an image that is itself in the bank is not its own neighbour
    return bank, bank.rerank_captions(preds, pooled, k=a.consensus_k, exclude_ids=list(preds))


def main():
    a = parser.parse_args()
    device = torch.device("cuda", a.gpu_ids[0])
    torch.cuda.set_device(device)
    style = style_words_from_tsv(a.style_wordforms) if a.style_wordforms else None
    refs = CaptionReferences(load_references(a.references), style_words=style, device=device)
    preds = load_predictions(a.predictions)
    if a.consensus_output and not a.consensus_bank:
        raise SystemExit("--consensus-output needs --consensus-bank")
    if a.select_k < 0 or (a.select_output and not a.select_k):
        raise SystemExit("--select-output needs --select-k K (K >= 1)")
    if a.select_k and a.select_quality == "logprob":
        raise SystemExit("--select-quality logprob: a predictions file holds no log-probs (scripts/inference.py --select-k has them)")
    if a.select_k and not a.consensus_bank:
        raise SystemExit("--select-quality consensus needs --consensus-bank")
    bank, cons = consensus_of(a, preds, device) if a.consensus_bank else (None, None)
    result = refs.score_captions(preds, set_diversity=a.set_diversity, consensus=cons)
    selection = None
    if a.select_k:
        selection = bank.select_captions(preds, quality="consensus", consensus=cons, k=a.select_k, method=a.select_method,
                                         lam=a.select_lambda, theta=a.select_theta)
    print("input:", a.predictions)
    print("Total ref sentences:", sum(len(refs.tokens[i]) for i in result.image_ids))
    s = result.summary()
    if selection is not None:
        s.update(result.subset_summary(selection, "select"))
    for line in format_summary(s):
        print(line)
    if result.empty_images:
        print(f"{result.empty_images} image(s) with only empty captions: Div-n 0")
    if result.degenerate_sets:
        print(f"{result.degenerate_sets} image(s) whose captions hold no weighted n-gram: Self-CIDEr 0")
    if a.output_json:
        json.dump(s, open(a.output_json, "w"), indent=1)
    if a.top5_output:
        out = [{"image_id": iid, "caption": preds[iid][int(n)]} for iid, row in zip(result.image_ids, result.top5) for n in row]
        json.dump(out, open(a.top5_output, "w"))
    if a.consensus_output:
        out = [{"image_id": iid, "caption": caps[int(n)]} for (iid, caps), n in zip(preds.items(), cons.pick)]
        json.dump(out, open(a.consensus_output, "w"))
    if a.select_output:
        out = [{"image_id": iid, "caption": c} for iid, caps in selection.captions(preds).items() for c in caps]
        json.dump(out, open(a.select_output, "w"))


if __name__ == "__main__":
    main()
