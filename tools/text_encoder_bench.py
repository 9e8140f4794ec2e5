"""Time the CLIP text encoder on libdgx at the real geometry (width 512, 8 heads, 12 layers, context 77, seeded weights):

    python tools/text_encoder_bench.py --batches 4,32 [--iters 50]

prints ms per encode_text call and the time of each kind of launch alone (back-to-back launches on fixed operands between two events,
so a launch's own latency is hidden by the queue: these are the kernels' device times), with the bytes and FLOP each must move."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args(argv)
    from divergen_amd.layers import text_ops as O
    from divergen_amd.layers.gemm_ops import gemm_bias_residual, gemm_nt
    from divergen_amd.modeling.text import CLIPTEXT
    torch.manual_seed(0)
    m = CLIPTEXT().cuda().eval()
    im = m.prepare()
    W, L, nH, E, layers = 512, 77, 8, 512, 12
    for B in [int(v) for v in args.batches.split(",")]:
        tok = torch.randint(1, 49000, (B, L))
        tok[:, 20] = 49407
        T = B * L
        print("B = %d (%d token rows)" % (B, T))
        print("  encode_text, whole call            %9.1f us   (%d launches)" % (_time(lambda: m.encode_text(tok), args.iters), 9 * layers + 2))
        blk = im.blocks[0]
        x, eot = O.text_embed(tok, im.token_embedding, im.positional_embedding)
        x = x.view(T, W)
        scr = torch.empty(2, T, device="cuda")
        h = O._layernorm_rows(x, blk.ln_1_w, blk.ln_1_b, 1e-5, scr)
        qkv = gemm_nt(h, blk.in_proj_w, blk.in_proj_b)
        a = O.causal_attention(qkv, B, L, nH)
        f = gemm_nt(h, blk.c_fc_w, blk.c_fc_b)
        g = O.quick_gelu(f)
        rows = [
            ("dgx_text_embed (+ token copy)", lambda: O.text_embed(tok, im.token_embedding, im.positional_embedding), 1, T * W * 12, T * W),
            ("dgx_layernorm_fwd", lambda: O._layernorm_rows(x, blk.ln_1_w, blk.ln_1_b, 1e-5, scr), 2 * layers, T * W * 6, 8 * T * W),
            ("gemm in_proj (bias)", lambda: gemm_nt(h, blk.in_proj_w, blk.in_proj_b), layers, 2 * (T * W + 3 * W * W + 3 * T * W), 6 * T * W * W),
            ("dgx_causal_attention_fwd", lambda: O.causal_attention(qkv, B, L, nH), layers, 2 * 4 * T * W, 2 * 2 * B * nH * L * (L + 1) // 2 * 64),
            ("gemm out_proj (bias + residual)", lambda: gemm_bias_residual(a, blk.out_proj_w, blk.out_proj_b, x, None, B, L, 1, 0, 0), layers,
             2 * (T * W + W * W) + 8 * T * W, 2 * T * W * W),
            ("gemm c_fc (bias)", lambda: gemm_nt(h, blk.c_fc_w, blk.c_fc_b), layers, 2 * (T * W + 4 * W * W + 4 * T * W), 8 * T * W * W),
            ("dgx_quick_gelu", lambda: O.quick_gelu(f), layers, 2 * 2 * 4 * T * W, 4 * 4 * T * W),
            ("gemm c_proj (bias + residual)", lambda: gemm_bias_residual(g, blk.c_proj_w, blk.c_proj_b, x, None, B, L, 1, 0, 0), layers,
             2 * (4 * T * W + 4 * W * W) + 8 * T * W, 8 * T * W * W),
            ("dgx_text_eot_project", lambda: O.eot_project(x.view(B, L, W), eot, im.ln_final_w, im.ln_final_b, im.text_projection), 1,
             4 * (B * W + W * E + B * E), 2 * B * W * E),
        ]
        total = 0.0
        print("  %-34s %9s  x per call   %10s %10s" % ("launch", "us", "KB", "MFLOP"))
        for name, fn, count, nbytes, flop in rows:
            us = _time(fn, args.iters)
            total += us * count
            print("  %-34s %9.1f  x %-9d %10.1f %10.1f" % (name, us, count, nbytes / 1e3, flop / 1e6))
        print("  sum of the launches' own times     %9.1f us" % total)


if __name__ == "__main__":
    main()
