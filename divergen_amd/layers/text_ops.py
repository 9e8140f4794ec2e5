"""CLIP text encoder ops over libdgx (csrc/text_encoder.hip): embedding gather, causal attention, QuickGELU and the fp32
end-token projection; `encode_text` strings them together with the library's GEMM and LayerNorm.
Forward only: the encoder is frozen wherever the reference uses it (DG custom_rcnn.py:58-62).  No CPU path exists."""
import torch

from .. import _lib as L
from .gemm_ops import gemm_bias_residual, gemm_nt
from .linear_ops import BF16

MAX_L = 96          # DGX_TEXT_MAX_L (include/divergen_hip.h)
HEAD_DIM = 64


def text_embed(tokens, token_embedding, positional_embedding):
    """tokens i64 (B, L) on the HOST (the tokenizer's output) -> x f32 (B, L, W) = token_embedding[tok] + positional_embedding[l] and
    eot i32 (B) = tokens.argmax(-1), both on the tables' device (dgx_text_embed).  A token outside the vocabulary raises: the library
    checks the host copy before it launches."""
    if tokens.is_cuda or tokens.dtype != torch.int64 or tokens.dim() != 2:
        raise L.DgxError("text_embed takes the tokenizer's int64 (B, L) tensor in host memory")
    tokens = tokens.contiguous()
    B, Lc = tokens.shape
    vocab, W = token_embedding.shape
    if positional_embedding.shape[0] < Lc or positional_embedding.shape[1] != W:
        raise L.DgxError("text_embed: %d tokens per row, positional_embedding %s" % (Lc, tuple(positional_embedding.shape)))
    dev = token_embedding.device
    tok_d = tokens.to(dev)
    x = torch.empty(B, Lc, W, dtype=torch.float32, device=dev)
    eot = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.lib().dgx_text_embed(tokens.data_ptr(), L.ptr(tok_d), L.ptr(token_embedding), L.ptr(positional_embedding), B, Lc, W, vocab,
                                   L.ptr(x), L.ptr(eot), L.stream()), "dgx_text_embed")
    return x, eot


def causal_attention(qkv, B, Lc, nH):
    """qkv bf16 (B * L, 3 * nH * 64) (in_proj's output, batch-major rows) -> bf16 (B * L, nH * 64) (dgx_causal_attention_fwd)."""
    if qkv.dtype != BF16 or qkv.numel() != B * Lc * 3 * nH * HEAD_DIM:
        raise L.DgxError("causal_attention: qkv bf16 (B, L, 3, nH, 64); got %s %s" % (tuple(qkv.shape), qkv.dtype))
    out = torch.empty(B * Lc, nH * HEAD_DIM, dtype=BF16, device=qkv.device)
    L.check(L.lib().dgx_causal_attention_fwd(L.ptr(qkv), L.ptr(out), B, Lc, nH, L.stream()), "dgx_causal_attention_fwd")
    return out


def quick_gelu(x):
    """bf16 x * sigmoid(1.702 x) (dgx_quick_gelu)."""
    if x.dtype != BF16:
        raise L.DgxError("quick_gelu takes bfloat16")
    y = torch.empty_like(x)
    L.check(L.lib().dgx_quick_gelu(L.ptr(x), L.ptr(y), x.numel(), L.stream()), "dgx_quick_gelu")
    return y


def eot_project(x, eot, ln_weight, ln_bias, projection, eps=1e-5):
    """x f32 (B, L, W), eot i32 (B) -> f32 (B, E) = ln_final(x[b, eot[b]]) @ projection (W, E), all fp32 (dgx_text_eot_project)."""
    B, Lc, W = x.shape
    E = projection.shape[1]
    if x.dtype != torch.float32 or projection.dtype != torch.float32 or eot.dtype != torch.int32 or projection.shape[0] != W:
        raise L.DgxError("eot_project: x f32 (B, L, W), eot i32 (B), projection f32 (W, E)")
    out = torch.empty(B, E, dtype=torch.float32, device=x.device)
    L.check(L.lib().dgx_text_eot_project(L.ptr(x), L.ptr(eot), L.ptr(ln_weight), L.ptr(ln_bias), L.ptr(projection), B, Lc, W, E, float(eps),
                                         L.ptr(out), L.stream()), "dgx_text_eot_project")
    return out


def _layernorm_rows(x, weight, bias, eps, scratch):
    """bf16 LayerNorm of the f32 rows x (T, C) in token order (dgx_layernorm_fwd, no window gather); scratch f32 (2, T): mean, rstd."""
    T, C = x.shape
    y = torch.empty(T, C, dtype=BF16, device=x.device)
    L.check(L.lib().dgx_layernorm_fwd(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(y), L.ptr(scratch[0]), L.ptr(scratch[1]), T, C, float(eps),
                                      1, T, 1, 0, 0, L.DGX_F32, L.stream()), "dgx_layernorm_fwd")
    return y


def encode_text(image, tokens):
    """CLIPTEXT.encode_text (text_encoder.py:154-163) of host tokens i64 (B, L) -> features f32 (B, E).  `image` is the operand image of
    the frozen weights (modeling/text/text_encoder.py: TextOperands).  The residual stream is fp32; every GEMM takes bf16 operands and
    rounds its result to bf16 once before it joins the stream (out_proj and c_proj
    use the GEMM's bias + residual tail in token order: its (B, H, W) geometry is (B, L, 1), no window map, no DropPath scale); ln_final and the projection of the end-token row are fp32."""
    x, eot = text_embed(tokens, image.token_embedding, image.positional_embedding)
    B, Lc, W = x.shape
    T = B * Lc
    x = x.view(T, W)
    scratch = torch.empty(2, T, dtype=torch.float32, device=x.device)
    for blk in image.blocks:
        h = _layernorm_rows(x, blk.ln_1_w, blk.ln_1_b, 1e-5, scratch)
        qkv = gemm_nt(h, blk.in_proj_w, blk.in_proj_b)
        a = causal_attention(qkv, B, Lc, image.heads)
        x = gemm_bias_residual(a, blk.out_proj_w, blk.out_proj_b, x, None, B, Lc, 1, 0, 0).view(T, W)
        h = _layernorm_rows(x, blk.ln_2_w, blk.ln_2_b, 1e-5, scratch)
        f = quick_gelu(gemm_nt(h, blk.c_fc_w, blk.c_fc_b))
        x = gemm_bias_residual(f, blk.c_proj_w, blk.c_proj_b, x, None, B, Lc, 1, 0, 0).view(T, W)
    return eot_project(x.view(B, Lc, W), eot, image.ln_final_w, image.ln_final_b, image.text_projection)
