"""Host tests of the CLIP text encoder: the float64 restatement (tests/_text_ref64.py) against the reference's own features, the
emulation tables behind the GPU bounds, the tokenizer, the module's state-dict names and the library's new symbols.  (The emulation-table
and bound tests pin the constants recorded in _text_ref64 to what it computes; the golden, module, symbol and GPU tests are the ones
that need the library.)"""
import gzip
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _text_ref64 as T  # noqa: E402

NEW_SYMBOLS = ("dgx_text_embed", "dgx_causal_attention_fwd", "dgx_quick_gelu", "dgx_text_eot_project")


@pytest.mark.parametrize("name", ["a", "b"])
def test_float64_restatement_equals_the_reference_features(name):
    """The reference ran in fp32: the bound is its own summation error, 1e-5 max|ref| + 1e-6."""
    sd, tokens, feats, heads = T.load_golden(name)
    assert tuple(int(v) for v in np.load(os.path.join(HERE, "golden", "text_encoder.npz"))[name + "/geometry"]) == T.GEOMETRIES[name]
    assert torch.equal(tokens, T.token_rows(T.GEOMETRIES[name][3], 77 + "ab".index(name)))
    assert tokens.argmax(-1).tolist() == [1, 40, 76, 10, 61]
    ref = T.encode(sd, tokens, heads)
    assert float((ref - feats.double()).abs().max()) <= 1e-5 * float(feats.abs().max()) + 1e-6


def test_attention_emulation_table_holds():
    ratios = [T.attn_emu_ratio(T.ordinary_inputs(B, L, nH), B, L, nH) for B, L, nH in T.ATTN_SHAPES]
    assert all(2 * r <= T.M_ATTN for r in ratios), ratios
    assert T.attn_m(ratios) == T.M_ATTN
    for B, L, nH in T.ATTN_SHAPES[1:4]:                                     # the hard inputs stay inside the same bound
        qkv = T.hard_inputs(B, L, nH)
        r = T.attn_ref64(qkv, B, L, nH)
        assert T.worst_ratio(T.attn_emu(qkv, B, L, nH), r["out"], T.attn_bound(r)) <= 1.0
        q, k, _ = T._heads(qkv, B, L, nH)
        s = T._logits(q, k)
        assert float(s[..., 1:L - 1, 0].min() - s[..., 1:L - 1, 1:].max()) > 30          # key 0 dominates
        assert float(s[..., L - 1, :].abs().max()) == 0.0                                # the last query: all logits equal


@pytest.mark.parametrize("geom,seeds", [("a", range(T.ENC_SEEDS)), ("b", range(T.ENC_SEEDS)), ("real", range(2))])
def test_encoder_bound_is_twice_the_emulation_deviation(geom, seeds):
    worst = max(T.enc_deviation(geom, s) for s in seeds)
    assert 2 * worst <= T.ENC_BOUND[geom] * (1 + 1e-3), (geom, worst)
    if len(seeds) == T.ENC_SEEDS:
        assert 2 * worst >= T.ENC_BOUND[geom] * (1 - 1e-3), (geom, worst)           # the recorded bound is this figure, not a wider one


def test_causality_and_argmax_in_the_restatement():
    sd = T.init_sd(64, 1, 1, 96, 32, 5)
    tok = T.token_rows(96, 9)
    f = T.encode(sd, tok, 1)
    t2 = tok.clone()
    t2[0, 2:] = 7                                                           # behind the end token at position 1
    assert torch.equal(T.encode(sd, t2, 1)[0], f[0])
    t3 = tok.clone()
    t3[3, 30] -= 1                                                          # the second maximum gone: the first won before, and wins now
    assert int(tok[3].argmax()) == int(t3[3].argmax()) == 10 and torch.equal(T.encode(sd, t3, 1)[3], f[3])


# ---------------------------------------------------------------------------------------------- tokenizer
MERGES = ["#version: test", "l o", "lo w</w>", "e r</w>", "n e", "ne w", "new er</w>"]


@pytest.fixture(scope="module")
def bpe_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("bpe") / "merges.txt.gz"
    with gzip.open(p, "wb") as f:
        f.write("\n".join(MERGES).encode("utf-8"))
    return str(p)


def test_tokenizer_hand_worked_bpe(bpe_path):
    from divergen_amd.modeling.text import SimpleTokenizer
    tk = SimpleTokenizer(bpe_path)
    assert len(tk.encoder) == 256 + 256 + 6 + 2
    assert tk.encoder["<|startoftext|>"] == 518 and tk.encoder["<|endoftext|>"] == 519
    assert tk.encoder["!"] == 0 and tk.encoder["w"] == 86 and tk.encoder["!</w>"] == 256 and tk.encoder[",</w>"] == 267
    assert tk.bpe("low") == "low</w>"                       # l o -> lo, lo w</w> -> low</w>
    assert tk.bpe("lower") == "lo w er</w>"                 # e r</w> merges; 'lo w' is no merge ('lo w</w>' is another pair)
    assert tk.bpe("newer") == "newer</w>"                   # e r</w> (learnt before n e), n e, ne w, new er</w>
    assert tk.encode("Low  lower, NEWER!") == [513, 512, 86, 514, 267, 517, 256]
    assert tk.encode("it's") == [tk.encoder["i"], tk.encoder["t</w>"], tk.encoder["'"], tk.encoder["s</w>"]]
    assert tk.encode("a&amp;b") == tk.encode("a&b")         # html entities are unescaped
    assert tk.encode("é") == [tk.encoder[tk.byte_encoder[0xC3]], tk.encoder[tk.byte_encoder[0xA9] + "</w>"]]      # bytes, not characters
    assert tk.decode(tk.encode("low lower")) == "low lower "
    with pytest.raises(ValueError, match="bpe_path"):
        SimpleTokenizer("")


def test_tokenize_pads_and_crops_with_the_reference_draws(bpe_path):
    from divergen_amd.modeling.text import CLIPTEXT
    m = CLIPTEXT(embed_dim=8, context_length=8, vocab_size=520, transformer_width=64, transformer_heads=1, transformer_layers=1,
                 bpe_path=bpe_path)
    long_a, short, long_b = "low lower, newer!", "low", "newer newer newer newer newer newer newer newer newer low"
    full_a = [518, 513, 512, 86, 514, 267, 517, 256, 519]
    full_b = [518] + [517] * 9 + [513, 519]
    torch.manual_seed(123)
    got = m.tokenize([long_a, short, long_b], context_length=8)
    torch.manual_seed(123)                                   # one draw per over-long caption, in order; the short one draws nothing
    st_a = torch.randint(len(full_a) - 8 + 1, (1,))[0].item()
    st_b = torch.randint(len(full_b) - 8 + 1, (1,))[0].item()
    assert got.dtype == torch.int64 and got.shape == (3, 8)
    assert got[0].tolist() == full_a[st_a:st_a + 8]
    assert got[1].tolist() == [518, 513, 519, 0, 0, 0, 0, 0]
    assert got[2].tolist() == full_b[st_b:st_b + 8]
    assert m.tokenize("low", context_length=8).shape == (1, 8)


# ---------------------------------------------------------------------------------------------- module and library
def test_state_dict_names_equal_the_reference(tmp_path):
    from divergen_amd.modeling.text import CLIPTEXT, build_text_encoder
    for name in ("a", "b"):
        sd, _, _, heads = T.load_golden(name)
        width, _, layers, vocab, embed = T.GEOMETRIES[name]
        m = CLIPTEXT(embed_dim=embed, context_length=T.CONTEXT, vocab_size=vocab, transformer_width=width, transformer_heads=heads,
                     transformer_layers=layers)
        assert sorted(m.state_dict()) == sorted(sd)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
        m.load_state_dict(sd, strict=True)
        assert all(not p.requires_grad for p in m.parameters())
    d = CLIPTEXT()
    assert (d.context_length, d.vocab_size, d.embed_dim, d.transformer.width, d.transformer.heads, d.transformer.layers) == (77, 49408, 512, 512, 8, 12)
    # a clip state dict as the reference leaves it, and one that still has the deleted entries
    full = dict(d.state_dict())
    full.update({"visual.conv1.weight": torch.zeros(2), "logit_scale": torch.zeros(()), "input_resolution": torch.zeros(()),
                 "context_length": torch.zeros(()), "vocab_size": torch.zeros(())})
    p = str(tmp_path / "clip_text.pth")
    torch.save(full, p)
    e = build_text_encoder(p)
    assert torch.equal(e.text_projection, d.text_projection) and not e.training
    torch.save({k: v for k, v in d.state_dict().items() if k != "ln_final.bias"}, p)
    with pytest.raises(RuntimeError, match="ln_final.bias"):
        build_text_encoder(p)
    with pytest.raises(ValueError, match="weights_path"):
        build_text_encoder("")
    with pytest.raises(ValueError, match="heads of 64"):
        CLIPTEXT(transformer_width=512, transformer_heads=16)
    with pytest.raises(ValueError, match="context_length"):
        CLIPTEXT(context_length=97)


def test_no_cpu_path():
    from divergen_amd import _lib
    from divergen_amd.layers import text_ops
    from divergen_amd.modeling.text import CLIPTEXT
    sd, tokens, _, heads = T.load_golden("a")
    m = CLIPTEXT(32, T.CONTEXT, 96, 64, 1, 2)
    m.load_state_dict(sd)
    with pytest.raises(_lib.DgxError):
        m.encode_text(tokens)
    with pytest.raises(_lib.DgxError):
        text_ops.quick_gelu(torch.zeros(8, dtype=torch.bfloat16))


def test_text_vocabulary_rows_and_chunks():
    from divergen_amd.modeling.utils import text_vocabulary
    calls = []

    def enc(texts):
        calls.append(list(texts))
        return torch.tensor([[float(len(t)), 1.0] for t in texts])
    emb = text_vocabulary(enc, ["cat", "traffic light", "ox"], prompt="a ", chunk=2)
    assert calls == [["a cat", "a traffic light"], ["a ox"]]
    assert emb.dtype == torch.float32 and emb.tolist() == [[5.0, 1.0], [15.0, 1.0], [4.0, 1.0]]
    with pytest.raises(ValueError):
        text_vocabulary(enc, [])


def test_library_exports_the_new_symbols():
    from divergen_amd import _lib
    from divergen_amd.csrc.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "divergen_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = _lib.lib()
    assert "text_encoder.hip" in SOURCES
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES and ("int %s(" % s) in hdr and s in integ, s
    assert "#define DGX_TEXT_MAX_L 96" in hdr
    from divergen_amd.layers import text_ops
    assert text_ops.MAX_L == 96
    # the host-side checks of the entry points need no GPU: nothing is launched on a refused call
    tok = (np.arange(6, dtype=np.int64) % 3).reshape(2, 3)
    tok[1, 2] = 5
    p = tok.ctypes.data
    assert L.dgx_text_embed(p, p, p, p, 2, 3, 4, 5, p, p, None) == -1          # token 5 outside [0, 5)
    assert L.dgx_causal_attention_fwd(p, p, 1, 97, 1, None) == -1 and L.dgx_causal_attention_fwd(p, p, 1, 0, 1, None) == -1
