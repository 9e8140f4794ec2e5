"""GPU tests of the CLIP text encoder (csrc/text_encoder.hip, layers/text_ops.py, modeling/text/text_encoder.py): every kernel
against float64 within the a-priori bounds of tests/_text_ref64.py, the exact properties of the causal attention, and the whole
encoder against the reference's own features (tests/golden/text_encoder.npz) and against float64 at the real geometry."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _text_ref64 as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
_IDS = ["B%d-L%d-h%d" % s for s in T.ATTN_SHAPES]


def _attn(qkv, B, L, nH):
    from divergen_amd.layers.text_ops import causal_attention
    out = causal_attention(qkv.reshape(B * L, -1).to(DEV).contiguous(), B, L, nH)
    torch.cuda.synchronize()
    return out.cpu().reshape(B, L, nH * T.HD)


@pytest.mark.parametrize("kind", ["ordinary", "hard"])
@pytest.mark.parametrize("B,L,nH", T.ATTN_SHAPES, ids=_IDS)
def test_causal_attention_within_the_bound(B, L, nH, kind):
    qkv = T.ordinary_inputs(B, L, nH) if kind == "ordinary" else T.hard_inputs(B, L, nH)
    got = _attn(qkv, B, L, nH)
    r = T.attn_ref64(qkv, B, L, nH)
    ratio = T.worst_ratio(got, r["out"], T.attn_bound(r))
    print("attention %s %s: worst |got - ref| / bound = %.3f" % ((B, L, nH), kind, ratio))
    assert ratio <= 1.0
    # row 0 of every head sees one key: P = 1, the output is v[0] bit for bit
    v0 = qkv.reshape(B, L, 3, nH * T.HD)[:, 0, 2]
    assert torch.equal(got[:, 0].view(torch.int16), v0.view(torch.int16))
    again = _attn(qkv, B, L, nH)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))


@pytest.mark.parametrize("B,L,nH", [s for s in T.ATTN_SHAPES if s[1] > 1], ids=[i for i, s in zip(_IDS, T.ATTN_SHAPES) if s[1] > 1])
def test_causal_attention_later_tokens_are_invisible(B, L, nH):
    qkv = T.ordinary_inputs(B, L, nH)
    base = _attn(qkv, B, L, nH)
    g = torch.Generator().manual_seed(L)
    for p in sorted({0, (L - 1) // 2, min(15, L - 2), min(16, L - 2), L - 2}):
        x = qkv.clone()
        sign = torch.randint(0, 2, x[:, p + 1:].shape, generator=g) * 2 - 1
        x[:, p + 1:] = (1e30 * sign).to(BF16)                    # large, finite
        got = _attn(x, B, L, nH)
        assert torch.equal(got[:, :p + 1].view(torch.int16), base[:, :p + 1].view(torch.int16)), p


def test_causal_attention_refuses_a_longer_row():
    from divergen_amd import _lib as L
    from divergen_amd.layers import text_ops
    cap = text_ops.MAX_L
    assert cap >= 77 and cap == T.ATTN_SHAPES[-1][1]
    qkv = torch.zeros(cap + 1, 3 * T.HD, dtype=BF16, device=DEV)
    out = torch.full((cap + 1, T.HD), 7.0, dtype=BF16, device=DEV)
    for bad in (cap + 1, 0):
        assert L.lib().dgx_causal_attention_fwd(L.ptr(qkv), L.ptr(out), 1, bad, 1, L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                             # nothing was launched
    with pytest.raises(L.DgxError):
        text_ops.causal_attention(qkv, 1, cap + 1, 1)


def test_text_embed_exact_and_argmax_rule():
    from divergen_amd import _lib as L
    from divergen_amd.layers.text_ops import text_embed
    g = torch.Generator().manual_seed(5)
    vocab, W = 96, 72
    te, pe = torch.randn(vocab, W, generator=g), torch.randn(T.CONTEXT, W, generator=g)
    tok = T.token_rows(vocab, 3)
    x, eot = text_embed(tok, te.to(DEV), pe.to(DEV))
    assert torch.equal(x.cpu(), te[tok] + pe[None])
    assert eot.cpu().tolist() == tok.argmax(-1).tolist() == [1, 40, 76, 10, 61]
    short = tok[:, :9].contiguous()                              # a shorter row uses the first positions
    x, eot = text_embed(short, te.to(DEV), pe.to(DEV))
    assert torch.equal(x.cpu(), te[short] + pe[None, :9]) and eot.cpu().tolist() == short.argmax(-1).tolist()
    for bad in (vocab, -1, 1 << 40):
        t2 = tok.clone()
        t2[2, 5] = bad
        with pytest.raises(L.DgxError):
            text_embed(t2, te.to(DEV), pe.to(DEV))
    with pytest.raises(L.DgxError):
        text_embed(tok.to(DEV), te.to(DEV), pe.to(DEV))
    # the kernel's own guard: a device copy that differs from the checked host copy cannot read outside the table -- the row is zeros
    bad_dev = tok.clone()
    bad_dev[1, 3], bad_dev[4, 0] = vocab + 5, -7
    ted, ped, bd = te.to(DEV), pe.to(DEV), bad_dev.to(DEV)
    x = torch.full((5, T.CONTEXT, W), 3.0, device=DEV)
    eot = torch.zeros(5, dtype=torch.int32, device=DEV)
    L.check(L.lib().dgx_text_embed(tok.data_ptr(), L.ptr(bd), L.ptr(ted), L.ptr(ped), 5, T.CONTEXT, W, vocab, L.ptr(x), L.ptr(eot), L.stream()), "embed")
    want = te[tok] + pe[None]
    want[1, 3] = 0.0
    want[4, 0] = 0.0
    assert torch.equal(x.cpu(), want) and eot.cpu().tolist() == bad_dev.argmax(-1).tolist()


def test_quick_gelu_per_element():
    """|got - float64| <= 2^-8 |ref| (the bf16 rounding of the result: unit roundoff 2^-8) + 1e-5 |ref| (fp32 arithmetic: the product
    1.702 x carries 2^-24 relative, which exp turns into |1.702 x| 2^-24 <= 3.1e-6 at |x| = 30, plus a few ulps of exp, divide and
    multiply) + 1e-37."""
    from divergen_amd.layers.text_ops import quick_gelu
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.linspace(-30, 30, 4001), torch.randn(5000, generator=g) * 3, torch.zeros(3), torch.tensor([30.0, -30.0])]).to(BF16)
    for n in (x.numel(), 8, 5, 1):                               # a length that is no multiple of 8, and tails only
        xi = x[-n:].contiguous()
        got = quick_gelu(xi.to(DEV)).cpu().double()
        ref = T.quick_gelu64(xi)
        bound = (2.0 ** -8 + 1e-5) * ref.abs() + 1e-37
        assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
    assert float(quick_gelu(torch.zeros(8, dtype=BF16, device=DEV)).abs().max()) == 0.0


@pytest.mark.parametrize("B,L,W,E", [(3, 77, 512, 512), (5, 9, 72, 33), (1, 1, 64, 8)])
def test_eot_project_per_element(B, L, W, E):
    """fp32 throughout.  With A_c = (|x_c| + mean|x|) rstd |gamma_c| + |beta_c| >= |ln_c|: the statistics are fp32 sums of W terms
    (error <= W 2^-24 of the terms' absolute sum) and so is the projection: |got - ref| <= (W + 8) 2^-23 sum_c A_c |proj_ce| + 1e-30."""
    from divergen_amd.layers.text_ops import eot_project
    g = torch.Generator().manual_seed(B * 100 + W)
    x = torch.randn(B, L, W, generator=g) * 3
    x[0, :, ::7] = 30.0
    x[0, :, 1::7] = -30.0
    if B > 1:
        x[1] = 0.0                                              # a zero row: the result is beta @ proj
    eot = torch.randint(0, L, (B,), generator=g, dtype=torch.int32)
    gam, bet = 1 + 0.2 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)
    proj = torch.randn(W, E, generator=g) * W ** -0.5
    got = eot_project(x.to(DEV), eot.to(DEV), gam.to(DEV), bet.to(DEV), proj.to(DEV)).cpu().double()
    row = x[torch.arange(B), eot.long()].double()
    ref = T._ln(row, gam, bet) @ proj.double()
    mu = row.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((row - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    A = (row.abs() + row.abs().mean(-1, keepdim=True)) * rstd * gam.double().abs() + bet.double().abs()
    bound = (W + 8) * 2.0 ** -23 * (A @ proj.double().abs()) + 1e-30
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())


def _module(sd, heads, vocab, embed):
    from divergen_amd.modeling.text import CLIPTEXT
    width = sd["token_embedding.weight"].shape[1]
    m = CLIPTEXT(embed_dim=embed, context_length=T.CONTEXT, vocab_size=vocab, transformer_width=width, transformer_heads=heads,
                 transformer_layers=T.n_layers(sd))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", ["a", "b"])
def test_encoder_against_the_reference_features(name):
    sd, tokens, feats, heads = T.load_golden(name)
    _, _, _, vocab, embed = T.GEOMETRIES[name]
    m = _module(sd, heads, vocab, embed)
    got = m.encode_text(tokens).cpu()
    assert got.dtype == torch.float32 and got.shape == feats.shape
    dev = float((T.normalized(got) - T.normalized(feats)).abs().max())
    print("encoder %s: max |got_n - ref_n| = %.3e, bound %.3e" % (name, dev, T.ENC_BOUND[name]))
    assert dev <= T.ENC_BOUND[name]
    assert torch.equal(got, m.encode_text(tokens).cpu())       # two runs: the same bits
    assert all(not p.requires_grad for p in m.parameters())


def test_encoder_real_geometry_against_float64():
    width, heads, layers, vocab, embed = T.GEOMETRIES["real"]
    sd = T.init_sd(width, heads, layers, vocab, embed, 9100)
    tokens = T.token_rows(vocab, 200)[[0, 1, 4]]
    m = _module(sd, heads, vocab, embed)
    got = m.encode_text(tokens).cpu()
    ref = T.encode(sd, tokens, heads)
    dev = float((T.normalized(got) - T.normalized(ref)).abs().max())
    print("encoder real geometry: max |got_n - ref_n| = %.3e, bound %.3e" % (dev, T.ENC_BOUND["real"]))
    assert dev <= T.ENC_BOUND["real"]
    # causality end to end: what stands behind the end token does not reach the feature
    t2 = tokens.clone()
    t2[0, 2:] = torch.randint(1, vocab - 8, (T.CONTEXT - 2,), generator=torch.Generator().manual_seed(1))
    assert torch.equal(m.encode_text(t2).cpu()[0], got[0])


def test_operand_image_follows_the_parameters():
    """The bf16 operand image is rebuilt when weights arrive by any road: an in-place write, and a PARENT module's strict
    load_state_dict (which never calls the child's own)."""
    sd, tokens, feats, heads = T.load_golden("a")
    _, _, _, vocab, embed = T.GEOMETRIES["a"]
    m = _module(T.init_sd(64, 1, 2, vocab, embed, 1), heads, vocab, embed)
    other = m.encode_text(tokens).cpu()
    holder = torch.nn.Module()
    holder.text_encoder = m
    holder.load_state_dict({"text_encoder." + k: v for k, v in sd.items()}, strict=True)
    got = m.encode_text(tokens).cpu()
    assert not torch.equal(got, other)
    assert float((T.normalized(got) - T.normalized(feats)).abs().max()) <= T.ENC_BOUND["a"]
    with torch.no_grad():
        m.text_projection.mul_(2.0)
    assert torch.equal(m.encode_text(tokens).cpu(), got * 2.0)
    img = m.prepare()
    assert m.prepare() is img                                   # unchanged parameters: the image is kept
