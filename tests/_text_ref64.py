"""float64 restatement of CLIPTEXT.encode_text (DG/divergen/modeling/text/text_encoder.py:154-163), a CPU emulation of the rounding
points of csrc/text_encoder.hip + layers/text_ops.encode_text, and the bounds the GPU tests hold them to.  Host only, plain torch.

Layouts: qkv (B, L, 3 * nH * 64) bf16 = nn.MultiheadAttention's in_proj output (q | k | v, each split into heads of 64), batch-major
rows; a state dict `sd` with the reference's names, float32 tensors.

The contract.  Residual stream fp32.  ln_1 / ln_2: fp32 statistics, bf16 result.  Every GEMM: bf16 operands (weight and bias rounded once
when the operand image is built), fp32 accumulation, the bf16 bias added in fp32, ONE bf16 rounding of the result -- the projections' results
are rounded before they join the fp32 stream.  Attention: bf16 q, k, v; logits, softmax statistics and sums fp32; the un-normalised
P = exp(s - max) rounded to bf16 where it feeds the MFMA, normalised behind it; one final bf16 rounding.  QuickGELU: bf16 in and out,
fp32 arithmetic.  ln_final of the end-token row and text_projection: fp32 throughout, fp32 features.

Attention bound per element (`attn_bound`; the three terms of tests/_attn_ref64.py):

    |got - ref| <= 2^-9 |ref|                      final bf16 rounding
                 + m 2^-9 abs_X                    bf16 rounding of P (abs_X = P @ |v|)
                 + 1e-5 max|ref| + 1e-6            fp32 summation order

m: the largest ratio (|emu - ref| - 2^-9 |ref| - floor) / (2^-9 abs_X) of `attn_emu` against `attn_ref64` over ATTN_SHAPES with
`ordinary_inputs` (randn * 1.5), m = ceil(2 * ratio), at least 1.  `python tests/_text_ref64.py` prints:

    shape (B, L, nH)   ratio
    (1, 1, 1)          -1.01
    (2, 16, 1)         1.18
    (2, 17, 2)         1.37
    (1, 33, 1)         1.42
    (3, 64, 2)         1.98
    (2, 77, 8)         1.71
    (5, 77, 1)         1.56
    (1, 96, 2)         1.55
    worst              1.98
    m                  4

(test_host_caption.py asserts 2 * ratio <= m at every shape.)

Whole encoder.  Judged on the L2-normalised feature rows, which is what the classifier consumes: the bound on max |got_n - ref_n| is
twice the worst deviation of `encode(emu=True)` from `encode(emu=False)` over ENC_SEEDS seeds (weights at the reference's initial
scales from `init_sd`, token rows from `token_rows`); the factor covers summation order and the statistics' fp32 on the device.  Same run:

    geometry (width, heads, layers, vocab, embed)   worst deviation   bound       bound / 2^-9
    (64, 1, 2, 96, 32)                              5.626e-03         1.125e-02   5.8
    (128, 2, 1, 96, 32)                             4.303e-03         8.607e-03   4.4
    (512, 8, 12, 1000, 512)                         1.257e-03         2.514e-03   1.3

(2^-9 relative is the rounding a classifier image gets anyway when its normalised row is rounded to bf16.)
"""
import math

import torch

U = 2.0 ** -9
M_ATTN = 4
ATTN_SHAPES = [(1, 1, 1), (2, 16, 1), (2, 17, 2), (1, 33, 1), (3, 64, 2), (2, 77, 8), (5, 77, 1), (1, 96, 2)]     # (B, L, nH); 96 = DGX_TEXT_MAX_L
HD = 64
GEOMETRIES = {"a": (64, 1, 2, 96, 32), "b": (128, 2, 1, 96, 32), "real": (512, 8, 12, 1000, 512)}     # width, heads, layers, vocab, embed
ENC_BOUND = {"a": 1.125e-2, "b": 8.607e-3, "real": 2.514e-3}
ENC_SEEDS = 6
CONTEXT = 77


def _bf(x):
    return x.to(torch.bfloat16).double()


def _f32(x):
    return x.float().double()


def _heads(qkv, B, L, nH):
    return qkv.double().reshape(B, L, 3, nH, HD).permute(2, 0, 3, 1, 4)          # 3 x (B, nH, L, 64)


def _unheads(x):
    B, nH, L, _ = x.shape
    return x.transpose(1, 2).reshape(B, L, nH * HD)


def _logits(q, k):
    L = q.shape[-2]
    s = (q @ k.transpose(-2, -1)) * (HD ** -0.5)
    return s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))


def attn_ref64(qkv, B, L, nH):
    """float64 causal attention of the bf16 inputs: dict out (B, L, nH * 64), abs_out (the same product with |v|)."""
    q, k, v = _heads(qkv, B, L, nH)
    P = torch.softmax(_logits(q, k), -1)
    return {"out": _unheads(P @ v), "abs_out": _unheads(P @ v.abs())}


def attn_emu(qkv, B, L, nH):
    """The kernel's contract in float64: P rounded un-normalised, one final rounding."""
    q, k, v = _heads(qkv, B, L, nH)
    s = _logits(q, k)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return _unheads(_bf((_bf(e) @ v) / e.sum(-1, keepdim=True)))


def _floor(ref):
    return 1e-5 * float(ref.abs().max()) + 1e-6


def attn_bound(r):
    return U * r["out"].abs() + M_ATTN * U * r["abs_out"] + _floor(r["out"])


def worst_ratio(got, ref, bnd):
    """max over elements of |got - ref| / bound (inf for a non-finite result): <= 1 passes."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bnd).max())


def ordinary_inputs(B, L, nH, seed=None):
    g = torch.Generator().manual_seed(700000 + B * 1000 + L * 10 + nH if seed is None else seed)
    return (torch.randn(B, L, 3 * nH * HD, generator=g) * 1.5).to(torch.bfloat16)


def hard_inputs(B, L, nH, seed=None):
    """Ordinary inputs with, in every (sample, head): key 0 dominating every later query by about 60 in the logit (k[0] = 6 * sign
    pattern, every q with the same pattern at ~1.25: 64 * 6 * 1.25 / 8 = 60), except the LAST query, which is zero: all its logits equal."""
    qkv = ordinary_inputs(B, L, nH, seed).reshape(B, L, 3, nH, HD).clone()
    g = torch.Generator().manual_seed(31 + L)
    sign = (torch.randint(0, 2, (HD,), generator=g) * 2 - 1).to(torch.bfloat16)
    qkv[:, 0, 1] = 6.0 * sign
    qkv[:, :, 0] = 1.25 * sign + 0.25 * qkv[:, :, 0]
    qkv[:, L - 1, 0] = 0
    return qkv.reshape(B, L, 3 * nH * HD)


def attn_emu_ratio(qkv, B, L, nH):
    r = attn_ref64(qkv, B, L, nH)
    e = attn_emu(qkv, B, L, nH)
    num = (e - r["out"]).abs() - U * r["out"].abs() - _floor(r["out"])
    return float((num / (U * r["abs_out"]).clamp_min(1e-300)).max())


def attn_m(ratios):
    return max(1, math.ceil(2 * max(ratios)))


# ---------------------------------------------------------------------------------------------- the whole encoder
def quick_gelu64(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def n_layers(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))


def encode(sd, tokens, heads, emu=False):
    """encode_text in float64 (emu=False), or with the contract's roundings (emu=True): features (B, E) float64."""
    rb = _bf if emu else (lambda t: t)
    rs = _f32 if emu else (lambda t: t)
    B, L = tokens.shape
    x = rs(sd["token_embedding.weight"].double()[tokens] + sd["positional_embedding"].double()[:L])
    for i in range(n_layers(sd)):
        p = "transformer.resblocks.%d." % i

        def lin(h, name):
            return rb(h @ rb(sd[p + name + ("_weight" if name == "attn.in_proj" else ".weight")].double()).t()
                      + rb(sd[p + name + ("_bias" if name == "attn.in_proj" else ".bias")].double()))
        h = rb(_ln(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]))
        qkv = lin(h, "attn.in_proj")
        a = attn_emu(qkv, B, L, heads) if emu else attn_ref64(qkv, B, L, heads)["out"]
        x = rs(x + lin(a, "attn.out_proj"))
        h = rb(_ln(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]))
        f = lin(h, "mlp.c_fc")
        x = rs(x + lin(rb(quick_gelu64(f)), "mlp.c_proj"))
    eot = tokens.argmax(-1)
    y = _ln(x[torch.arange(B), eot], sd["ln_final.weight"], sd["ln_final.bias"]) @ sd["text_projection"].double()
    return rs(y)


def normalized(f):
    f = f.double()
    return f / f.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def init_sd(width, heads, layers, vocab, embed, seed, context=CONTEXT):
    """A state dict with the reference's names at the reference's initial scales (text_encoder.py:99-113); biases and LayerNorm
    parameters perturbed so that every one of them is exercised."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std      # noqa: E731
    proj_std, attn_std, fc_std = (width ** -0.5) * ((2 * layers) ** -0.5), width ** -0.5, (2 * width) ** -0.5
    sd = {"token_embedding.weight": rn(vocab, width, std=0.02), "positional_embedding": rn(context, width, std=0.01),
          "ln_final.weight": 1 + rn(width, std=0.1), "ln_final.bias": rn(width, std=0.05), "text_projection": rn(width, embed, std=width ** -0.5)}
    for i in range(layers):
        p = "transformer.resblocks.%d." % i
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = rn(3 * width, width, std=attn_std), rn(3 * width, std=0.02)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(width, width, std=proj_std), rn(width, std=0.02)
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = 1 + rn(width, std=0.1), rn(width, std=0.05)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = rn(4 * width, width, std=fc_std), rn(4 * width, std=0.02)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = rn(width, 4 * width, std=proj_std), rn(width, std=0.02)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = 1 + rn(width, std=0.1), rn(width, std=0.05)
    return sd


def token_rows(vocab, seed, context=CONTEXT):
    """Five rows: the end token (vocab - 1) at positions 1, 40 and 76 with zeros behind it; a row with no end token whose maximum
    occurs twice (argmax = the first); a full-length row without an end token."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for p in (1, 40, 76):
        r = torch.zeros(context, dtype=torch.int64)
        r[:p] = torch.randint(1, vocab - 8, (p,), generator=g)
        r[p] = vocab - 1
        rows.append(r)
    r = torch.zeros(context, dtype=torch.int64)
    r[:50] = torch.randint(1, vocab - 8, (50,), generator=g)
    r[10] = r[30] = vocab - 5
    rows.append(r)
    r = torch.randint(1, vocab - 8, (context,), generator=g)
    r[61] = vocab - 3
    rows.append(r)
    return torch.stack(rows)


def load_golden(name, path=None):
    """Configuration 'a' / 'b' of tests/golden/text_encoder.npz: (state dict of float32 tensors under the reference's names, tokens,
    the reference's features, heads)."""
    import os

    import numpy as np
    z = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_encoder.npz"))
    sd = {}
    for k in z.files:
        if not k.startswith(name + "/") or k.split("/", 1)[1] in ("tokens", "features", "geometry"):
            continue
        key = k.split("/", 1)[1]
        if key.endswith(":bf16"):
            sd[key[:-5]] = torch.from_numpy(z[k].view(np.int16).copy()).view(torch.bfloat16).float()
        else:
            sd[key] = torch.from_numpy(z[k])
    return sd, torch.from_numpy(z[name + "/tokens"]), torch.from_numpy(z[name + "/features"]), int(z[name + "/geometry"][1])


def enc_deviation(geom, seed):
    width, heads, layers, vocab, embed = GEOMETRIES[geom]
    sd = init_sd(width, heads, layers, vocab, embed, 9000 + seed)
    tok = token_rows(vocab, 100 + seed)
    if geom == "real":
        tok = tok[[0, 1, 4]]
    return float((normalized(encode(sd, tok, heads, emu=True)) - normalized(encode(sd, tok, heads))).abs().max())


if __name__ == "__main__":
    ratios = []
    print("    shape (B, L, nH)   ratio")
    for B, L, nH in ATTN_SHAPES:
        ratios.append(attn_emu_ratio(ordinary_inputs(B, L, nH), B, L, nH))
        print("    %-18s %.2f" % ((B, L, nH), ratios[-1]))
    print("    worst              %.2f\n    m                  %d" % (max(ratios), attn_m(ratios)))
    for geom in GEOMETRIES:
        worst = max(enc_deviation(geom, s) for s in range(ENC_SEEDS))
        print("    %-47s %.3e         %.3e   %.1f" % (GEOMETRIES[geom], worst, 2 * worst, 2 * worst / U))
