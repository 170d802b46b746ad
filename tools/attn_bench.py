"""Microbenchmark: hand-written attn kernels vs the sdpa-with-mask fallback.

Usage (GPU box):  python tools/attn_bench.py
Prints us/call for fwd and fwd+bwd on the bench shapes.

`--work-order` instead times the v2 kernels alone, once under the causal mask
and once fully visible, to show how evenly a causal launch's tiles are spread
over the GPU (see work_order_shape).
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pipegoose_amd.ops import get_extension  # noqa: E402


def bench(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def run_shape(B, H, S, D):
    ext = get_extension(required=True)
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    do = torch.randn_like(q)
    slopes = (torch.rand(H, device="cuda") * 0.5).float()
    scale = D ** -0.5

    t_fwd = bench(lambda: ext.attn_fwd(q, k, v, slopes, scale, 0))
    o, lse = ext.attn_fwd(q, k, v, slopes, scale, 0)
    t_bwd = bench(lambda: ext.attn_bwd(do, q, k, v, o, lse, slopes, scale, 0))

    # sdpa-with-mask fallback (what the model used before the kernel)
    pos = torch.arange(S, device="cuda")
    rel = (pos[None, :] - pos[:, None]).float()
    bias = (slopes[:, None, None] * rel[None]
            + torch.triu(torch.full((S, S), float("-inf"), device="cuda"), 1)[None]
            ).to(torch.bfloat16)[None]
    qg = q.clone().requires_grad_(True)
    kg = k.clone().requires_grad_(True)
    vg = v.clone().requires_grad_(True)

    def sdpa_fwd():
        return torch.nn.functional.scaled_dot_product_attention(
            q, k, v, attn_mask=bias, scale=scale)

    t_sdpa_fwd = bench(sdpa_fwd)

    def sdpa_fwdbwd():
        out = torch.nn.functional.scaled_dot_product_attention(
            qg, kg, vg, attn_mask=bias, scale=scale)
        out.backward(do)
        qg.grad = kg.grad = vg.grad = None

    t_sdpa_fb = bench(sdpa_fwdbwd)

    flops_fwd = 2 * B * H * S * S * D * 2 / 2  # causal half
    print(f"B{B} H{H} S{S} D{D}: "
          f"ours fwd {t_fwd:8.1f}us ({flops_fwd / t_fwd / 1e6:6.1f} TF)  "
          f"bwd {t_bwd:8.1f}us | "
          f"sdpa fwd {t_sdpa_fwd:8.1f}us ({flops_fwd / t_sdpa_fwd / 1e6:6.1f} TF)  "
          f"fwd+bwd {t_sdpa_fb:8.1f}us")


BENCH_SHAPES = ((8, 16, 2048, 64),     # bloom-560m
                (8, 32, 2048, 128))    # bloom-7b1


def event_us(fn, iters, reps, warmup=5):
    """us per call from device events around `iters` back-to-back calls,
    `reps` times: (median, min, max)."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e3 / iters)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def work_order_shape(B, H, S, D, masks, iters, reps, digest):
    """The v2 kernels under a causal (kv_off 0) and a fully visible
    (kv_off -S) launch of the same grid.  Causal does 36/64 of the tiles at
    S=2048 with 256-row blocks, so a causal/full time ratio near 0.56 says
    the tiles are spread evenly over the CUs, and one near 1.0 that the
    launch waits for its most loaded XCD.  `fwd` is attn_fwd_v2 alone; `bwd`
    is delta + dq_v2 + dkdv_v2 (split them by name with
    `rocprofv3 --kernel-trace --stats -- python tools/attn_bench.py
    --work-order --mask causal`, and again with `--mask full`)."""
    ext = get_extension(required=True)
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    do = torch.randn_like(q)
    slopes = (torch.rand(H, device="cuda") * 0.5).float()
    scale = D ** -0.5
    res = {"shape": f"B{B} H{H} S{S} D{D}",
           "variant": list(ext.attn_variant(S, D))}
    for mask in masks:
        kv_off = 0 if mask == "causal" else -S
        o, lse = ext.attn_fwd(q, k, v, slopes, scale, kv_off)
        fwd = event_us(lambda: ext.attn_fwd(q, k, v, slopes, scale, kv_off),
                       iters, reps)
        bwd = event_us(lambda: ext.attn_bwd(do, q, k, v, o, lse, slopes,
                                            scale, kv_off), iters, reps)
        res[mask] = {"fwd_us": [round(x, 1) for x in fwd],
                     "bwd_us": [round(x, 1) for x in bwd]}
        if digest:
            grads = ext.attn_bwd(do, q, k, v, o, lse, slopes, scale, kv_off)
            res[mask]["sha256"] = {"fwd": _digest(o, lse),
                                   "dq": _digest(grads[0]),
                                   "dkdv": _digest(grads[1], grads[2])}
    if len(masks) == 2:
        res["causal_over_full"] = {
            key: round(res["causal"][f"{key}_us"][0]
                       / res["full"][f"{key}_us"][0], 3)
            for key in ("fwd", "bwd")}
    print(json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--work-order", action="store_true",
                   help="time the v2 kernels causal and fully visible at the "
                        "bench shapes (device events), one JSON line each")
    p.add_argument("--mask", choices=("causal", "full", "both"),
                   default="both")
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--digest", action="store_true",
                   help="add a sha256 prefix of the raw outputs on the seeded "
                        "inputs, to compare two builds bit for bit")
    args = p.parse_args()
    if not args.work_order:
        for shape in BENCH_SHAPES:
            run_shape(*shape)
        return
    masks = ("causal", "full") if args.mask == "both" else (args.mask,)
    for shape in BENCH_SHAPES:
        work_order_shape(*shape, masks, args.iters, args.reps, args.digest)


if __name__ == "__main__":
    main()
