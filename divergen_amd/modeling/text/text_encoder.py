"""CLIP's text transformer as the reference holds it (DG/divergen/modeling/text/text_encoder.py): `CLIPTEXT` with the reference's
constructor arguments and state-dict names, run forward-only on libdgx (layers/text_ops.encode_text), and a restatement of
clip.simple_tokenizer.SimpleTokenizer that reads the BPE merges file the user supplies (clip's bpe_simple_vocab_16e6.txt.gz).

The encoder is frozen everywhere the reference uses it (custom_rcnn.py:58-62, predictor.py:15-23): every parameter has
requires_grad False, there is no backward, and the GEMM operands are a bf16 image built once after the weights are loaded
(`prepare`).  This build never fetches: `build_text_encoder` loads a state dict in the form the reference leaves clip's
(`visual.*` and the four scalars deleted, text_encoder.py:180-187) from a path.
"""
import gzip
import html
from collections import OrderedDict
from functools import lru_cache

import torch
from torch import nn

from ...layers import text_ops

BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------- tokenizer
@lru_cache()
def bytes_to_unicode():
    """byte -> a printable unicode character (the byte-level BPE alphabet of clip/simple_tokenizer.py)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2 ** 8):
        if b not in bs:
            bs.append(b)
            cs.append(2 ** 8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def get_pairs(word):
    """The set of adjacent symbol pairs of a word (a tuple of symbols)."""
    return set(zip(word[:-1], word[1:]))


def basic_clean(text):
    try:                                    # ftfy repairs mojibake when it is installed; without it the text is taken as it is
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    return html.unescape(html.unescape(text)).strip()


def whitespace_clean(text):
    return " ".join(text.split()).strip()


class SimpleTokenizer:
    """clip.simple_tokenizer.SimpleTokenizer over the merges file at `bpe_path` (gzip or plain text; the first line is a header).
    Vocabulary: the 256 byte symbols, the same with '</w>', one token per merge, then <|startoftext|> and <|endoftext|>."""

    MAX_MERGES = 49152 - 256 - 2

    def __init__(self, bpe_path):
        import regex
        if not bpe_path:
            raise ValueError("bpe_path is empty: the tokenizer reads clip's bpe_simple_vocab_16e6.txt.gz from it")
        opener = gzip.open if str(bpe_path).endswith(".gz") else open
        with opener(bpe_path, "rb") as f:
            lines = f.read().decode("utf-8").split("\n")
        merges = [tuple(m.split()) for m in lines[1:self.MAX_MERGES + 1] if len(m.split()) == 2]
        self.byte_encoder = bytes_to_unicode()
        self.byte_decoder = {v: k for k, v in self.byte_encoder.items()}
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab]
        vocab.extend("".join(m) for m in merges)
        vocab.extend(["<|startoftext|>", "<|endoftext|>"])
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {"<|startoftext|>": "<|startoftext|>", "<|endoftext|>": "<|endoftext|>"}
        self.pat = regex.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
                                 regex.IGNORECASE)

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        pairs = get_pairs(word)
        if not pairs:
            return token + "</w>"
        while True:
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))      # the merge learnt first
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new_word, i = [], 0
            while i < len(word):
                if word[i] == first and i + 1 < len(word) and word[i + 1] == second:
                    new_word.append(first + second)
                    i += 2
                else:
                    new_word.append(word[i])
                    i += 1
            word = tuple(new_word)
            if len(word) == 1:
                break
            pairs = get_pairs(word)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        import regex
        tokens = []
        text = whitespace_clean(basic_clean(text)).lower()
        for token in regex.findall(self.pat, text):
            token = "".join(self.byte_encoder[b] for b in token.encode("utf-8"))
            tokens.extend(self.encoder[t] for t in self.bpe(token).split(" "))
        return tokens

    def decode(self, tokens):
        text = "".join(self.decoder[t] for t in tokens)
        return bytearray(self.byte_decoder[c] for c in text).decode("utf-8", errors="replace").replace("</w>", " ")


# ---------------------------------------------------------------------------------------------- the module
class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    """Holds one block's parameters under the reference's names; the arithmetic is layers/text_ops.encode_text."""

    def __init__(self, d_model, n_head):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)


class Transformer(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads) for _ in range(layers)])


class _BlockOperands:
    pass


class TextOperands:
    """The frozen weights as the kernels read them, on one device: bf16 GEMM weights (as stored: (out, in)) and biases (the GEMM's bias operand is bf16), fp32 LayerNorm
    parameters, embedding tables and projection."""

    def __init__(self, model, device):
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()      # noqa: E731
        b16 = lambda t: t.detach().to(device=device, dtype=torch.float32).to(BF16).contiguous()      # noqa: E731
        self.heads = model.transformer.heads
        self.token_embedding = f32(model.token_embedding.weight)
        self.positional_embedding = f32(model.positional_embedding)
        self.ln_final_w, self.ln_final_b = f32(model.ln_final.weight), f32(model.ln_final.bias)
        self.text_projection = f32(model.text_projection)
        self.blocks = []
        for blk in model.transformer.resblocks:
            o = _BlockOperands()
            o.ln_1_w, o.ln_1_b, o.ln_2_w, o.ln_2_b = f32(blk.ln_1.weight), f32(blk.ln_1.bias), f32(blk.ln_2.weight), f32(blk.ln_2.bias)
            o.in_proj_w, o.in_proj_b = b16(blk.attn.in_proj_weight), b16(blk.attn.in_proj_bias)
            o.out_proj_w, o.out_proj_b = b16(blk.attn.out_proj.weight), b16(blk.attn.out_proj.bias)
            o.c_fc_w, o.c_fc_b = b16(blk.mlp.c_fc.weight), b16(blk.mlp.c_fc.bias)
            o.c_proj_w, o.c_proj_b = b16(blk.mlp.c_proj.weight), b16(blk.mlp.c_proj.bias)
            self.blocks.append(o)


class CLIPTEXT(nn.Module):
    def __init__(self, embed_dim=512, context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                 transformer_layers=12, bpe_path=None):
        super().__init__()
        if transformer_width != transformer_heads * text_ops.HEAD_DIM:
            raise ValueError("CLIPTEXT: the attention kernel has heads of %d: width %d with %d heads is not supported"
                             % (text_ops.HEAD_DIM, transformer_width, transformer_heads))
        if context_length > text_ops.MAX_L:
            raise ValueError("CLIPTEXT: context_length %d above the attention kernel's %d" % (context_length, text_ops.MAX_L))
        self.bpe_path = bpe_path
        self._tok = None
        self.context_length = context_length
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads)
        self.vocab_size = vocab_size
        self.embed_dim = embed_dim
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.initialize_parameters()
        for p in self.parameters():
            p.requires_grad_(False)
        self._image, self._image_stamp = None, None

    def initialize_parameters(self):
        """The reference's initial scales (text_encoder.py:99-113)."""
        width, layers = self.transformer.width, self.transformer.layers
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std, attn_std, fc_std = (width ** -0.5) * ((2 * layers) ** -0.5), width ** -0.5, (2 * width) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=width ** -0.5)

    @property
    def device(self):
        return self.text_projection.device

    @property
    def dtype(self):
        return self.text_projection.dtype

    @property
    def _tokenizer(self):
        if self._tok is None:
            self._tok = SimpleTokenizer(self.bpe_path)
        return self._tok

    def _stamp(self):
        """Storage and in-place version of every parameter: changes when weights are loaded (through this module or a parent's
        load_state_dict, which copies in place), written in place, cast or moved."""
        return tuple((p.data_ptr(), p._version, p.dtype) for p in self.parameters())

    def prepare(self):
        """The operand image on the parameters' device, built once and rebuilt whenever a parameter has changed since (`_stamp`)."""
        stamp = self._stamp()
        if self._image is None or self._image_stamp != stamp:
            self._image = TextOperands(self, self.device)
            self._image_stamp = stamp
        return self._image

    def tokenize(self, texts, context_length=77):
        """The reference's tokenize (text_encoder.py:131-152): <start> + BPE + <end>, zero-padded to context_length; an over-long caption
        is cropped to a window drawn with torch.randint, one draw per such caption in order."""
        if isinstance(texts, str):
            texts = [texts]
        sot, eot = self._tokenizer.encoder["<|startoftext|>"], self._tokenizer.encoder["<|endoftext|>"]
        all_tokens = [[sot] + self._tokenizer.encode(text) + [eot] for text in texts]
        result = torch.zeros(len(all_tokens), context_length, dtype=torch.long)
        for i, tokens in enumerate(all_tokens):
            if len(tokens) > context_length:
                st = torch.randint(len(tokens) - context_length + 1, (1,))[0].item()
                tokens = tokens[st: st + context_length]
            result[i, :len(tokens)] = torch.tensor(tokens)
        return result

    @torch.no_grad()
    def encode_text(self, text):
        """tokens i64 (B, context_length) in host memory -> features f32 (B, embed_dim) on the module's device."""
        if text.shape[1] != self.context_length:
            raise ValueError("encode_text: rows of %d tokens, context_length is %d" % (text.shape[1], self.context_length))
        return text_ops.encode_text(self.prepare(), text.cpu())

    def forward(self, captions):
        return self.encode_text(self.tokenize(captions, self.context_length))


_DROPPED = ("logit_scale", "input_resolution", "context_length", "vocab_size")


def state_dict_geometry(sd):
    """CLIPTEXT's constructor arguments read from the shapes of a text state dict: vocabulary, width, layers, context, embed dim;
    heads = width / 64 (the attention kernel's head)."""
    vocab, width = sd["token_embedding.weight"].shape
    blocks = set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks."))
    return dict(embed_dim=int(sd["text_projection"].shape[1]), context_length=int(sd["positional_embedding"].shape[0]),
                vocab_size=int(vocab), transformer_width=int(width), transformer_heads=int(width) // text_ops.HEAD_DIM,
                transformer_layers=len(blocks))


def build_text_encoder(weights_path, bpe_path=None, geometry_from_weights=False, **kwargs):
    """CLIPTEXT with the state dict at `weights_path` loaded strictly: clip's ViT-B/32 state dict with
    `visual.*` and the four scalars deleted, as the reference leaves it (keys still present are dropped the same way).
    geometry_from_weights: the constructor arguments come from the state dict's shapes (state_dict_geometry) instead of the ViT-B/32
    defaults -- the model's own encoder (MODEL.TEXT_ENCODER_WEIGHTS) is built this way."""
    if not weights_path:
        raise ValueError("weights_path is empty: this build never downloads CLIP; give the path of the text encoder's "
                         "state dict")
    sd = torch.load(weights_path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
    sd = {k: v for k, v in sd.items() if k not in _DROPPED and not k.startswith("visual.")}
    if geometry_from_weights:
        kwargs = dict(state_dict_geometry(sd), **kwargs)
    model = CLIPTEXT(bpe_path=bpe_path, **kwargs)
    model.load_state_dict(sd)
    return model.eval()
