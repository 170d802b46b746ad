"""Kernel-level timing of decode attention (ops/csrc/decode_attention.hip)
against the sdpa path the models ran before it (bias build + GQA expand +
torch sdpa over the whole static cache).

Usage (GPU box): python tools/decode_attn_bench.py [--max-len 4096]
                     [--filled 128 1024 4096] [--step-timeout 120]

For each (shape, filled length) both paths are timed in the same process,
alternating, with device events around ``--iters`` calls, ``--repeats``
times; the median is reported in us together with the achieved GB/s of the
K+V bytes the step actually needs, 2*B*Hkv*(p+1)*D*2.  K/V rotate over
several buffers (>= 1 GB in total) so that no call finds its operands in the
256 MiB L3 left there by the previous one.

Every shape runs in a child process of its own under ``--step-timeout``; the
parent never opens the GPU and stops at the first child that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (B, H, Hkv, D, alibi)
SHAPES = {
    "bloom-560m": (8, 16, 16, 64, True),
    "bloom-7b1": (8, 32, 32, 128, True),
    "gqa-32q8kv": (8, 32, 8, 128, False),
}


def needed_bytes(B, Hkv, D, p):
    return 2 * B * Hkv * (p + 1) * D * 2


def sdpa_path(q, k, v, slopes, scale, pos_t, kpos, alibi):
    """What BloomAttention / LlamaAttention run in graph mode without the
    kernel, op for op."""
    import torch
    import torch.nn.functional as TF
    G = q.size(1) // k.size(1)
    if alibi:
        rel = (kpos - pos_t).float()
        bias = slopes[:, None, None] * rel
        bias = bias.masked_fill(kpos > pos_t, float("-inf")).to(q.dtype)[None]
    else:
        bias = torch.zeros(1, 1, 1, k.size(2), device=q.device, dtype=q.dtype)
        bias = bias.masked_fill((kpos > pos_t)[None, None, None],
                                float("-inf"))
    ke = k.repeat_interleave(G, dim=1) if G > 1 else k
    ve = v.repeat_interleave(G, dim=1) if G > 1 else v
    return TF.scaled_dot_product_attention(q, ke, ve, attn_mask=bias,
                                           scale=scale)


def run_shape(name, max_len, filled, iters, repeats, warmup, forced):
    import torch
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.decode_attention import decode_attention_reference

    assert torch.cuda.is_available(), "decode_attn_bench needs a GPU"
    ext = get_extension(required=True)
    B, H, Hkv, D, alibi = SHAPES[name]
    dev = "cuda"
    torch.manual_seed(0)
    scale = D ** -0.5
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    kv_bytes = 2 * B * Hkv * max_len * D * 2
    n_buf = max(2, min(8, -(-(1 << 30) // kv_bytes)))
    q = torch.randn(B, H, 1, D, device=dev).bfloat16()
    ks = [torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
          for _ in range(n_buf)]
    vs = [torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
          for _ in range(n_buf)]
    kpos = torch.arange(max_len, device=dev)
    pos_t = torch.zeros(1, dtype=torch.long, device=dev)
    n_splits, chunk = ext.decode_attn_plan(B, Hkv, max_len, D)

    def kernel(i, n=0):
        return ext.decode_attn(q, ks[i % n_buf], vs[i % n_buf], slopes, scale,
                               pos_t, n)

    def sdpa(i):
        return sdpa_path(q, ks[i % n_buf], vs[i % n_buf], slopes, scale,
                         pos_t, kpos, alibi)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters      # us per call

    for length in filled:
        p = length - 1
        pos_t.fill_(p)
        # results must agree before a time means anything
        ref = decode_attention_reference(
            q.double(), ks[0].double(), vs[0].double(), slopes.double(),
            scale, pos_t)
        vmax = vs[0].double().abs().max().item()
        errs = {}
        for label, fn in (("kernel", kernel), ("sdpa", sdpa)):
            errs[label] = ((fn(0).double() - ref).abs().max() / vmax).item()
        for i in range(warmup):
            kernel(i), sdpa(i)
        torch.cuda.synchronize()
        t_k, t_s = [], []
        for _ in range(repeats):                       # alternate the two
            t_k.append(timed(kernel))
            t_s.append(timed(sdpa))
        # other plans, for tuning the auto rule (not part of the A/B)
        t_forced = {}
        for n in forced:
            fn = lambda i, n=n: kernel(i, n)
            timed(fn)
            t_forced[n] = round(statistics.median(
                timed(fn) for _ in range(repeats)), 2)
        need = needed_bytes(B, Hkv, D, p)
        us_k, us_s = statistics.median(t_k), statistics.median(t_s)
        print(json.dumps({
            "shape": name, "B": B, "H": H, "Hkv": Hkv, "D": D,
            "max_len": max_len, "filled": length, "n_splits": n_splits,
            "chunk": chunk, "kv_buffers": n_buf, "needed_MB": need / 1e6,
            "kernel_us": round(us_k, 2), "sdpa_us": round(us_s, 2),
            "kernel_us_all": [round(t, 2) for t in t_k],
            "sdpa_us_all": [round(t, 2) for t in t_s],
            "kernel_GBps": round(need / us_k / 1e3, 1),
            "sdpa_GBps": round(need / us_s / 1e3, 1),
            "speedup": round(us_s / us_k, 2),
            "kernel_us_forced_n_splits": t_forced,
            "kernel_err_over_vmax": errs["kernel"],
            "sdpa_err_over_vmax": errs["sdpa"],
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--filled", type=int, nargs="+",
                    default=[128, 1024, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--also-n-splits", type=int, nargs="*", default=[],
                    help="also time the kernel with these forced plans")
    ap.add_argument("--step-timeout", type=int, default=120,
                    help="seconds allowed to each shape's child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert all(1 <= f <= args.max_len for f in args.filled)

    if args.child:
        run_shape(args.child, args.max_len, args.filled, args.iters,
                  args.repeats, args.warmup, args.also_n_splits)
        return
    for name in args.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--max-len", str(args.max_len), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--filled", *map(str, args.filled),
               "--also-n-splits", *map(str, args.also_n_splits)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
