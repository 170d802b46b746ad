"""Timing of ragged-batch paged attention
(ops/csrc/paged_varlen_attention.hip) against the paths that served the same
rows before it, in the style of tools/paged_prefill_attn_bench.py: same
timing method, every comparison alternated in one process.

Usage (GPU box): python tools/paged_varlen_attn_bench.py [--mode ragged equal decode]
                     [--context 0 1024] [--page 16]
                 python tools/paged_varlen_attn_bench.py --mode e2e
                 python tools/paged_varlen_attn_bench.py --kv fp8 [--mode ragged | e2e]

Three head shapes: bloom-560m (H16, D64, ALiBi), llama-7b (H32, D128) and a
GQA shape (H32 over 8 kv heads, D128); 8 sequences; every sequence's rows sit
at ``start = context``.  Timed with device events around ``--iters`` calls,
``--repeats`` times, median in us, with the spread (max - min over the median)
of both paths next to every ratio:

  ragged   8 prompts of 64..1024 new tokens: ONE ``paged_varlen_attn`` launch
           against the loop of eight B = 1 ``paged_prefill_attn`` launches
  equal    8 x 512 new tokens: ``paged_varlen_attn`` against ONE
           ``paged_prefill_attn`` launch (B = 8) — what sharing the staged
           K/V tile among the heads of a GQA group buys
  decode   8 x 1 new token: ``paged_varlen_attn`` against
           ``paged_decode_attn``; a decode row fills gp of a tile's 64 rows

K/V rotate over several pools (>= 1 GB in total) so that no call finds its
operands in the 256 MiB L3.  Before timing, both paths' results must agree to
bf16 accuracy.

End to end (``--mode e2e``): bloom-560m, the 8 ragged prompts through
``PagedDecoder.generate`` to the first token, with and without
``batched_prefill``, host clock around a device synchronise.

fp8 caches (``--kv fp8``, ops/csrc/paged_fp8_varlen_attention.hip): the
ragged rows over e4m3fn pools with per-row scales, ONE
``paged_varlen_attn_fp8`` launch against the loop of eight B = 1
``paged_prefill_attn_fp8`` launches and against the bf16 ``paged_varlen_attn``
on the same rows, all three alternated; bloom-7b1's heads (H32, D128, ALiBi)
stand where llama-7b's do.  ``--mode e2e`` then builds both decoders with
``kv_dtype=torch.float8_e4m3fn``.

Every shape runs in a child process of its own under ``--step-timeout``; the
parent never opens the GPU and stops at the first child that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {                       # H, Hkv, D, alibi
    "bloom-560m": (16, 16, 64, True),
    "llama-7b": (32, 32, 128, False),
    "bloom-7b1": (32, 32, 128, True),
    "gqa-32q8kv": (32, 8, 128, False),
}
LENS = {"ragged": [64, 128, 200, 333, 512, 700, 900, 1024],
        "equal": [512] * 8, "decode": [1] * 8}


def summary(times):
    """median us, spread in % of it, per path."""
    med = {k: statistics.median(t) for k, t in times.items()}
    return ({k: round(m, 1) for k, m in med.items()},
            {k: round(100 * (max(t) - min(t)) / med[k], 1)
             for k, t in times.items()})


def alternate(paths, warmup, repeats, timed):
    """``repeats`` timings of every path, the paths taking turns."""
    import torch
    for i in range(warmup):
        for fn in paths.values():
            fn(i)
    torch.cuda.synchronize()
    times = {label: [] for label in paths}
    for _ in range(repeats):
        for label, fn in paths.items():
            times[label].append(timed(fn))
    return times


def run_shape(name, modes, contexts, page, iters, repeats, warmup, kv):
    import torch
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.paged_attention import quantize_rows_fp8

    assert torch.cuda.is_available(), "paged_varlen_attn_bench needs a GPU"
    ext = get_extension(required=True)
    H, Hkv, D, alibi = SHAPES[name]
    B, dev, scale = 8, "cuda", D ** -0.5
    torch.manual_seed(0)
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    max_len = -(-(max(contexts) + 1024) // page) * page
    max_pages = max_len // page
    n_pages = B * max_pages + 1                         # + the null page
    n_buf = max(2, min(8, -(-(1 << 30) // (2 * B * Hkv * max_len * D * 2))))
    table = (torch.randperm(n_pages - 1, device=dev) + 1).view(
        B, max_pages).to(torch.int32)
    kps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
           for _ in range(n_buf)]
    vps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
           for _ in range(n_buf)]

    # the same pools as the fp8 cache holds them: bytes and per-row scales
    k8s, v8s = ([quantize_rows_fp8(p) for p in pools] if kv == "fp8" else []
                for pools in (kps, vps))

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters      # us per call

    for mode in modes:
        lens = LENS[mode]
        T = sum(lens)
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        cu_q = torch.tensor(cu, dtype=torch.int32, device=dev)
        q = torch.randn(T, H, D, device=dev).bfloat16()
        # the same rows as the older kernels take them: [1 or B, H, Sq, D]
        # views of [.., Sq, H, D] memory
        per_seq = [q[cu[b]:cu[b + 1]].transpose(0, 1)[None] for b in range(B)]
        batch = q.view(B, lens[0], H, D).transpose(1, 2) \
            if mode != "ragged" else None
        for context in contexts:
            start = torch.full((B,), context, dtype=torch.long, device=dev)
            starts = [start[b:b + 1] for b in range(B)]
            tables = [table[b:b + 1] for b in range(B)]

            def varlen(i):
                return ext.paged_varlen_attn(q, kps[i % n_buf], vps[i % n_buf],
                                             table, slopes, scale, cu_q, start)

            def prefill_loop(i):
                return torch.cat([
                    ext.paged_prefill_attn(
                        per_seq[b], kps[i % n_buf], vps[i % n_buf], tables[b],
                        slopes, scale, starts[b])[0].transpose(0, 1)
                    for b in range(B)])

            def prefill_loop_timed(i):      # the launches alone, no cat
                for b in range(B):
                    ext.paged_prefill_attn(
                        per_seq[b], kps[i % n_buf], vps[i % n_buf], tables[b],
                        slopes, scale, starts[b])

            def prefill_batch(i):
                return ext.paged_prefill_attn(
                    batch, kps[i % n_buf], vps[i % n_buf], table, slopes,
                    scale, start)

            def decode(i):
                return ext.paged_decode_attn(
                    batch, kps[i % n_buf], vps[i % n_buf], table, slopes,
                    scale, start, 0)

            def varlen_fp8(i):
                (k8, ks), (v8, vs) = k8s[i % n_buf], v8s[i % n_buf]
                return ext.paged_varlen_attn_fp8(q, k8, v8, ks, vs, table,
                                                 slopes, scale, cu_q, start)

            def prefill_fp8_loop(i):        # the launches alone, no cat
                (k8, ks), (v8, vs) = k8s[i % n_buf], v8s[i % n_buf]
                return [ext.paged_prefill_attn_fp8(
                    per_seq[b], k8, v8, ks, vs, tables[b], slopes, scale,
                    starts[b]) for b in range(B)]

            if kv == "fp8":
                paths = {"varlen_fp8": varlen_fp8,
                         "prefill_fp8_x8": prefill_fp8_loop, "varlen": varlen}
                want = torch.cat([o[0].transpose(0, 1)
                                  for o in prefill_fp8_loop(0)]).float()
                err = (varlen_fp8(0).float() - want).abs().max().item()
                assert err <= 2.0 ** -5 * max(1.0, want.abs().max().item()), \
                    f"varlen_fp8 differs from prefill_fp8_x8 by {err} at " \
                    f"{context}"
                times = alternate(paths, warmup, repeats, timed)
                med, spread = summary(times)
                print(json.dumps({
                    "shape": name, "mode": mode, "kv": kv, "H": H, "Hkv": Hkv,
                    "D": D, "page": page, "lens": lens, "context": context,
                    "kv_buffers": n_buf, "us": med, "spread_pct": spread,
                    "us_all": {k: [round(x, 1) for x in t]
                               for k, t in times.items()},
                    "fp8_over_prefill_x8": round(
                        med["varlen_fp8"] / med["prefill_fp8_x8"], 3),
                    "fp8_over_bf16": round(med["varlen_fp8"] / med["varlen"],
                                           3),
                    "max_abs_diff": round(err, 5)}), flush=True)
                continue

            old_name, old, old_check = {
                "ragged": ("prefill_x8", prefill_loop_timed, prefill_loop),
                "equal": ("prefill_b8", prefill_batch, lambda i:
                          prefill_batch(i).transpose(1, 2).reshape(T, H, D)),
                "decode": ("decode", decode, lambda i:
                           decode(i).transpose(1, 2).reshape(T, H, D)),
            }[mode]
            paths = {"varlen": varlen, old_name: old}

            # results must agree before a time means anything
            want, got = old_check(0).float(), varlen(0).float()
            err = (got - want).abs().max().item()
            assert err <= 2.0 ** -5 * max(1.0, want.abs().max().item()), \
                f"varlen differs from {old_name} by {err} at {mode}/{context}"

            times = alternate(paths, warmup, repeats, timed)
            med, spread = summary(times)
            pairs = sum(n * context + n * (n + 1) // 2 for n in lens)
            print(json.dumps({
                "shape": name, "mode": mode, "H": H, "Hkv": Hkv, "D": D,
                "page": page, "lens": lens, "context": context,
                "kv_buffers": n_buf, "us": med, "spread_pct": spread,
                "us_all": {k: [round(x, 1) for x in t]
                           for k, t in times.items()},
                "varlen_TFLOPs": round(4 * H * D * pairs / med["varlen"] / 1e6,
                                       1),
                "varlen_over_old": round(med["varlen"] / med[old_name], 3),
                "max_abs_diff": round(err, 5)}), flush=True)


def run_e2e(repeats, kv):
    """bloom-560m through PagedDecoder: time to the first tokens of the 8
    ragged prompts (one new token, so no decode step runs)."""
    import torch
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
    from pipegoose_amd.models.paged_decode import PagedDecoder

    assert torch.cuda.is_available(), "paged_varlen_attn_bench needs a GPU"
    for name, value in (("RANK", "0"), ("LOCAL_RANK", "0"),
                        ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                        ("MASTER_PORT", "29898")):
        os.environ.setdefault(name, value)
    ctx = ParallelContext.from_torch()
    torch.manual_seed(0)
    cfg = BloomConfig(vocab_size=250880, hidden_size=1024, n_layer=24,
                      n_head=16)
    model = BloomForCausalLM(cfg, ctx).to("cuda", torch.bfloat16).eval()
    page, lens = 16, LENS["ragged"]
    prompts = [torch.randint(0, cfg.vocab_size, (n,), device="cuda")
               for n in lens]
    n_pages = sum(-(-(n + 1) // page) for n in lens) + 1
    decs = {label: PagedDecoder(model, max_seqs=8, n_pages=n_pages,
                                page_size=page, max_len=max(lens) + page,
                                use_graph=False, batched_prefill=flag,
                                kv_dtype=torch.float8_e4m3fn
                                if kv == "fp8" else None)
            for label, flag in (("per_prompt", False), ("batched", True))}
    first = {}
    for label, dec in decs.items():                     # warm-up
        first[label] = torch.cat(dec.generate(prompts, 1)).tolist()
    torch.cuda.synchronize()
    times = {label: [] for label in decs}
    for _ in range(repeats):                            # alternate
        for label, dec in decs.items():
            t0 = time.perf_counter()
            dec.generate(prompts, 1)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) * 1e3)
    med, spread = summary(times)
    print(json.dumps({
        "model": "bloom-560m", "kv": kv, "prompts": lens, "page": page, "ms": med,
        "spread_pct": spread,
        "ms_all": {k: [round(x, 2) for x in t] for k, t in times.items()},
        "batched_over_per_prompt": round(med["batched"] / med["per_prompt"],
                                         3),
        "same_first_tokens": first["batched"] == first["per_prompt"],
    }), flush=True)
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=list(SHAPES),
                    help="default: bloom-560m, llama-7b (bloom-7b1 with "
                    "--kv fp8) and gqa-32q8kv")
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"],
                    help="cache dtype; fp8 takes --mode ragged or e2e")
    ap.add_argument("--mode", nargs="+",
                    choices=["ragged", "equal", "decode", "e2e"])
    ap.add_argument("--context", type=int, nargs="+", default=[0, 1024])
    ap.add_argument("--page", type=int, default=16, choices=[16, 32, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    fp8 = args.kv == "fp8"
    args.mode = args.mode or (["ragged"] if fp8
                              else ["ragged", "equal", "decode"])
    args.shapes = args.shapes or [
        "bloom-560m", "bloom-7b1" if fp8 else "llama-7b", "gqa-32q8kv"]
    assert not fp8 or args.mode in (["ragged"], ["e2e"]), \
        "--kv fp8 takes --mode ragged or --mode e2e"

    if args.child == "e2e":
        run_e2e(args.repeats, args.kv)
        return
    if args.child:
        run_shape(args.child, args.mode, args.context, args.page, args.iters,
                  args.repeats, args.warmup, args.kv)
        return
    if "e2e" in args.mode:
        assert args.mode == ["e2e"], "--mode e2e runs on its own"
        jobs = ["e2e"]
    else:
        jobs = args.shapes
    for name in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--mode", *args.mode, "--context", *map(str, args.context),
               "--page", str(args.page), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--kv", args.kv]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
