#!/usr/bin/env python3
"""Builds the bank of training images that consensus re-ranking searches (ssc_runtime.evaluation.ConsensusBank): every distinct
image of a training tensor file with its pooled region features (the masked mean over regions, on the device) and all its captions as
words.  scripts/inference.py --consensus-bank and scripts/evaluate.py --consensus-bank read the file."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

import torch  # noqa: E402

from ssc_runtime.data import TensorFileData  # noqa: E402
from ssc_runtime.evaluation import ConsensusBank, pool_rows  # noqa: E402
from ssc_runtime.vocab import Vocabulary  # noqa: E402

parser = argparse.ArgumentParser("Build a consensus re-ranking bank from a training tensor file (MI355X).")
parser.add_argument("--train-tensors", required=True,
                    help="tensor file: caption_tokens (N, L), image_id (N,), image_features (N, R, F) or features + num_boxes")
parser.add_argument("--vocabulary", required=True, help="vocabulary directory (tokens.txt) the caption ids index")
parser.add_argument("--output", required=True, help="the bank file to write")
parser.add_argument("--gpu-ids", default=[0], nargs="+", type=int)


def main():
    a = parser.parse_args()
    device = torch.device("cuda", a.gpu_ids[0])
    torch.cuda.set_device(device)
    vocabulary = Vocabulary.from_files(a.vocabulary)
    boundary = vocabulary.get_token_index("@@BOUNDARY@@")
    V = vocabulary.get_vocab_size()
    data = TensorFileData(a.train_tensors)
    first, captions = {}, {}
    for r, (iid, cap) in enumerate(zip(data.image_id.tolist(), data.caps.tolist())):
        first.setdefault(iid, r)
        ids = [t for t in cap if t != 0 and t != boundary]   # id 0 is padding (and @@UNKNOWN@@, which matches nothing anyway)
        if any(t < 0 or t >= V for t in ids):
            raise SystemExit(f"row {r}: a caption id outside the vocabulary of {V} words")
        if ids:
            captions.setdefault(iid, []).append(" ".join(vocabulary.get_token_from_index(t) for t in ids))
    ids = list(first)
    for iid in ids:
        if iid not in captions:
            raise SystemExit(f"image {iid!r} has no caption")
    pooled = pool_rows(data, [first[i] for i in ids], device)
    ConsensusBank.write_file(a.output, pooled, ids, [captions[i] for i in ids])
    print(f"wrote {len(ids)} images, {sum(len(captions[i]) for i in ids)} captions, {pooled.size(1)} features to {a.output}")


if __name__ == "__main__":
    main()
