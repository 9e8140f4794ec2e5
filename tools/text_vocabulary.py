"""Turn a list of class names into a test vocabulary with the CLIP text encoder (BS/bsgal/predictor.py:15-23):

    python tools/text_vocabulary.py --weights clip_text.pth --bpe bpe_simple_vocab_16e6.txt.gz --names cat,dog,"traffic light" --out v.npy

writes the (C, 512) .npy that MODEL.ROI_BOX_HEAD.ZEROSHOT_WEIGHT_PATH / MODEL.TEST_CLASSIFIERS read.  --weights is the text encoder's
state dict (clip's ViT-B/32 state dict; `visual.*` and the scalar entries are ignored), --bpe clip's merges file: neither is fetched.
--names-file takes one name per line instead of --names.  Needs the GPU: the encoder runs on libdgx."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--bpe", required=True)
    ap.add_argument("--names", default="")
    ap.add_argument("--names-file", default="")
    ap.add_argument("--prompt", default="a ")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    names = [n.strip() for n in args.names.split(",") if n.strip()]
    if args.names_file:
        names += [ln.strip() for ln in open(args.names_file) if ln.strip()]
    if not names:
        ap.error("give --names a,b,c or --names-file")
    from divergen_amd.modeling.text import build_text_encoder
    from divergen_amd.modeling.utils import text_vocabulary
    enc = build_text_encoder(args.weights, args.bpe).to(args.device)
    emb = text_vocabulary(enc, names, args.prompt)
    np.save(args.out, emb.numpy())
    print("wrote %s: %d x %d" % (args.out, emb.shape[0], emb.shape[1]))


if __name__ == "__main__":
    main()
