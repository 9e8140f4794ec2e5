"""Generate tests/golden/text_encoder.npz: the reference's own CLIPTEXT (DG/divergen/modeling/text/text_encoder.py) on token rows.
Run in the authoring container only:

    python tests/golden/make_golden_caption.py

Two small configurations of the reference's class after its own initialize_parameters under a fixed seed -- 'a': width 64, 1 head,
2 layers; 'b': width 128, 2 heads, 1 layer; both vocab 96, embed 32, context 77 -- and the token rows of
tests/_text_ref64.token_rows (end token at positions 1, 40 and 76; a row without an end token whose maximum occurs twice; a full-length
row).  Tokens go straight into the reference's encode_text; its tokenizer is the import-time stand-in of _refload (`clip` is not
installed here).  The four large matrices of every block are rounded to bf16 in place BEFORE the reference runs and stored as their
16-bit patterns (keys ending in ':bf16'): half the bytes, and the features are still the reference's own function of the stored
weights.  Data only is stored: weights, tokens, features.  Fixed zip timestamps: two runs give identical bytes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refload as R  # noqa: E402
import _text_ref64 as T  # noqa: E402
from make_golden_blend import save_deterministic  # noqa: E402

BIG = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def main():
    R.install()
    R._ns("divergen.modeling.text", R.DG + "/modeling/text")
    te = R.ref("divergen.modeling.text.text_encoder")
    out = {}
    for i, name in enumerate(("a", "b")):
        width, heads, layers, vocab, embed = T.GEOMETRIES[name]
        torch.manual_seed(4100 + i)
        m = te.CLIPTEXT(embed_dim=embed, context_length=T.CONTEXT, vocab_size=vocab, transformer_width=width, transformer_heads=heads,
                        transformer_layers=layers).eval()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if k.endswith(BIG):
                    v.copy_(v.to(torch.bfloat16).float())
        tokens = T.token_rows(vocab, 77 + i)
        with torch.no_grad():
            feats = m.encode_text(tokens)
        for k, v in m.state_dict().items():
            if k.endswith(BIG):
                out["%s/%s:bf16" % (name, k)] = v.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            else:
                out["%s/%s" % (name, k)] = v.numpy()
        out[name + "/tokens"] = tokens.numpy()
        out[name + "/features"] = feats.numpy()
        out[name + "/geometry"] = np.asarray(T.GEOMETRIES[name], dtype=np.int64)
    save_deterministic(os.path.join(HERE, "text_encoder.npz"), out)


if __name__ == "__main__":
    main()
