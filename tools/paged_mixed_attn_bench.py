"""Timing of split-KV ragged paged attention
(ops/csrc/paged_varlen_split_attention.hip) against the kernels that served
the same rows before it, on the pattern of tools/paged_varlen_attn_bench.py:
same shapes, same timing method (device events around ``--iters`` calls,
``--repeats`` times, median in us with the spread (max - min over the median)
of every path), every comparison alternated in one process, K/V rotating over
pools of >= 1 GB in total.

Usage (GPU box): python tools/paged_mixed_attn_bench.py [--mode decode mixed prefill]
                     [--context 0 128 1024 4096] [--page 16]
                 python tools/paged_mixed_attn_bench.py --mode e2e

  decode   8 x 1 new token behind ``--context``: the new kernel at auto and
           forced 1 / 4 / 16 splits, with the short-tile body and with the
           shared-tile body alone, against ``paged_decode_attn`` (auto) and
           ``paged_varlen_attn``
  mixed    one 512-token piece plus 8 / 32 / 64 decode rows, all at context
           1024: ONE new launch against the pair it replaces
           (``paged_varlen_attn`` for the piece + ``paged_decode_attn`` for
           the rows)
  prefill  the 8 ragged prompts of the varlen profile at the auto plan
           (which must be 1 split) against ``paged_varlen_attn``
  e2e      bloom-560m, 32 ragged prompts: ``generate_continuous`` with
           ``max_seqs=8`` against four ``generate(batched_prefill=True)``
           calls of 8 prompts; total time and mean time to first token

``--kv fp8`` (ops/csrc/paged_fp8_varlen_split_attention.hip) runs the same
modes over e4m3fn pools with per-row scales: ``split*`` is
``paged_varlen_split_attn_fp8``, ``varlen`` is ``paged_varlen_attn_fp8`` (the
route it replaces), ``decode`` is ``paged_decode_attn_fp8``, and
``bf16_split0`` is the bf16 split kernel on the unquantised pools.

Every shape runs in a child process of its own under ``--step-timeout``; the
parent never opens the GPU and stops at the first child that fails.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.paged_varlen_attn_bench import (LENS, SHAPES, alternate,  # noqa: E402
                                           summary)

NEW = 32                        # tokens per prompt of the e2e run


def run_shape(name, modes, contexts, page, iters, repeats, warmup, kv):
    import torch
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.paged_attention import quantize_rows_fp8

    assert torch.cuda.is_available(), "paged_mixed_attn_bench needs a GPU"
    ext = get_extension(required=True)
    H, Hkv, D, alibi = SHAPES[name]
    B, dev, scale = 72, "cuda", D ** -0.5       # a piece + up to 64 rows
    torch.manual_seed(0)
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    max_len = -(-(max(contexts + [1024]) + 1024) // page) * page
    max_pages = max_len // page
    live = 8                                    # sequences with pages
    n_pages = live * max_pages + 1              # + the null page
    n_buf = max(2, min(8, -(-(1 << 30) // (2 * live * Hkv * max_len * D * 2))))
    # decode rows beyond the 8th share the 8 sequences' pages: the bytes read
    # per row are the same, the pools stay at the varlen profile's size
    table = (torch.randperm(n_pages - 1, device=dev) + 1).view(
        live, max_pages).to(torch.int32).repeat(B // live, 1)
    kps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
           for _ in range(n_buf)]
    vps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
           for _ in range(n_buf)]
    # the same pools as the fp8 cache holds them: bytes and per-row scales
    fp8 = kv == "fp8"
    k8s, v8s = ([quantize_rows_fp8(p) for p in pools] if fp8 else []
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

    def problem(lens, starts):
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        return (torch.randn(cu[-1], H, D, device=dev).bfloat16(),
                torch.tensor(cu, dtype=torch.int32, device=dev),
                torch.tensor(starts, dtype=torch.long, device=dev),
                table[:len(lens)])

    def split_bf16(q, cu_q, start, tab, n, short=True):
        return lambda i: ext.paged_varlen_split_attn(
            q, kps[i % n_buf], vps[i % n_buf], tab, slopes, scale, cu_q,
            start, n, short)

    def cache8(i):
        (k8, ks), (v8, vs) = k8s[i % n_buf], v8s[i % n_buf]
        return k8, v8, ks, vs

    def split(q, cu_q, start, tab, n, short=True):
        if not fp8:
            return split_bf16(q, cu_q, start, tab, n, short)
        return lambda i: ext.paged_varlen_split_attn_fp8(
            q, *cache8(i), tab, slopes, scale, cu_q, start, n, short)

    def varlen(q, cu_q, start, tab):
        if fp8:
            return lambda i: ext.paged_varlen_attn_fp8(
                q, *cache8(i), tab, slopes, scale, cu_q, start)
        return lambda i: ext.paged_varlen_attn(
            q, kps[i % n_buf], vps[i % n_buf], tab, slopes, scale, cu_q, start)

    def decode(q, start, tab):                  # q [n, H, D] as [n, H, 1, D]
        qd = q[:, None].transpose(1, 2)
        if fp8:
            return lambda i: ext.paged_decode_attn_fp8(
                qd, *cache8(i), tab, slopes, scale, start, 0)
        return lambda i: ext.paged_decode_attn(
            qd, kps[i % n_buf], vps[i % n_buf], tab, slopes, scale, start, 0)

    def report(mode, paths, want, extra, prob):
        got = {k: fn(0).float() for k, fn in paths.items()
               if k.startswith("split")}
        if fp8:     # the bf16 split kernel on the unquantised pools, a column
            paths["bf16_split0"] = split_bf16(*prob, 0)
        err = max((g - want).abs().max().item() for g in got.values())
        assert err <= 2.0 ** -5 * max(1.0, want.abs().max().item()), \
            f"{mode}: the new kernel differs from the old by {err}: {extra}"
        times = alternate(paths, warmup, repeats, timed)
        med, spread = summary(times)
        print(json.dumps(dict(
            extra, shape=name, mode=mode, kv=kv, H=H, Hkv=Hkv, D=D, page=page,
            kv_buffers=n_buf, us=med, spread_pct=spread,
            us_all={k: [round(x, 1) for x in t] for k, t in times.items()},
            max_abs_diff=round(err, 5))), flush=True)
        return med

    for mode in modes:
        if mode == "decode":
            for context in contexts:
                q, cu_q, start, tab = problem([1] * 8, [context] * 8)
                paths = {"decode": decode(q, start, tab),
                         "varlen": varlen(q, cu_q, start, tab)}
                for n in (0, 1, 4, 16):
                    paths[f"split{n}"] = split(q, cu_q, start, tab, n)
                    paths[f"split{n}_shared"] = split(q, cu_q, start, tab, n,
                                                      False)
                report(mode, paths, paths["varlen"](0).float(), {
                    "context": context, "auto_plan": ext.paged_varlen_split_plan(
                        8, 8, H, Hkv, max_len)[0]}, (q, cu_q, start, tab))
        elif mode == "mixed":
            for rows in (8, 32, 64):
                lens, starts = [512] + [1] * rows, [1024] * (rows + 1)
                q, cu_q, start, tab = problem(lens, starts)
                piece = varlen(q[:512], cu_q[:2], start[:1], tab[:1])
                dec = decode(q[512:], start[1:], tab[1:])
                paths = {"pair": lambda i: (piece(i), dec(i)),
                         "split0": split(q, cu_q, start, tab, 0),
                         "split0_shared": split(q, cu_q, start, tab, 0, False),
                         "varlen": varlen(q, cu_q, start, tab)}
                report(mode, paths, paths["varlen"](0).float(), {
                    "decode_rows": rows, "context": 1024,
                    "auto_plan": ext.paged_varlen_split_plan(
                        len(q), rows + 1, H, Hkv, max_len)[0]},
                    (q, cu_q, start, tab))
        else:
            for context in contexts:
                lens = LENS["ragged"]
                q, cu_q, start, tab = problem(lens, [context] * 8)
                plan = ext.paged_varlen_split_plan(len(q), 8, H, Hkv, max_len)
                paths = {"varlen": varlen(q, cu_q, start, tab),
                         "split0": split(q, cu_q, start, tab, 0)}
                report(mode, paths, paths["varlen"](0).float(), {
                    "lens": lens, "context": context, "auto_plan": plan[0]},
                    (q, cu_q, start, tab))


def run_e2e(repeats, kv):
    """bloom-560m, 32 ragged prompts, NEW tokens each.  With an fp8 cache a
    third path, ``continuous_unsplit``, is ``generate_continuous`` with its
    attention sent to ``paged_varlen_attn_fp8``, the route it took before the
    fp8 split kernel."""
    import torch
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
    from pipegoose_amd.models.paged_decode import PagedDecoder
    from pipegoose_amd.ops import get_extension

    assert torch.cuda.is_available(), "paged_mixed_attn_bench needs a GPU"
    for name, value in (("RANK", "0"), ("LOCAL_RANK", "0"),
                        ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                        ("MASTER_PORT", "29899")):
        os.environ.setdefault(name, value)
    ctx = ParallelContext.from_torch()
    torch.manual_seed(0)
    cfg = BloomConfig(vocab_size=250880, hidden_size=1024, n_layer=24,
                      n_head=16)
    model = BloomForCausalLM(cfg, ctx).to("cuda", torch.bfloat16).eval()
    page, chunk = 16, 512
    lens = [LENS["ragged"][(5 * i) % 8] for i in range(32)]
    prompts = [torch.randint(0, cfg.vocab_size, (n,), device="cuda")
               for n in lens]
    n_pages = 8 * -(-(max(lens) + NEW) // page) + 1
    args = (model, 8, n_pages, page, max(lens) + NEW + page)
    kw = dict(prefill_chunk=chunk,
              kv_dtype=torch.float8_e4m3fn if kv == "fp8" else None)
    batched = PagedDecoder(*args, batched_prefill=True, **kw)
    cont = PagedDecoder(*args, **kw)

    budget = 8 * chunk

    def batched_x4():
        for lo in range(0, 32, 8):
            batched.generate(prompts[lo:lo + 8], NEW)

    def continuous():
        cont.generate_continuous(prompts, NEW, token_budget=budget)

    def total_ms(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def forward_ends(fn):
        """ms from the start to the end of every EAGER model forward (a
        synchronise in a forward hook; graph replays run no hook)."""
        ends, t0 = [], time.perf_counter()

        def stamp(*_):
            torch.cuda.synchronize()
            ends.append((time.perf_counter() - t0) * 1e3)
        hook = model.register_forward_hook(stamp)
        fn()
        hook.remove()
        return ends

    def continuous_unsplit():
        ext = get_extension(required=True)
        new = ext.paged_varlen_split_attn_fp8
        ext.paged_varlen_split_attn_fp8 = \
            lambda *a: ext.paged_varlen_attn_fp8(*a[:-1])   # drops n_splits
        try:
            continuous()
        finally:
            ext.paged_varlen_split_attn_fp8 = new

    paths = {"batched_x4": batched_x4, "continuous": continuous}
    if kv == "fp8":
        paths["continuous_unsplit"] = continuous_unsplit
    for fn in paths.values():                  # warm-up, graph capture
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            times[k].append(total_ms(fn))
    med, spread = summary(times)

    # time to first token: the forward that ends prompt i, by schedule.
    # batched: the graphs exist, so the eager forwards of a call are its
    # prefill rounds, and prompt i ends in round ceil(len / chunk) - 1
    ends = forward_ends(batched_x4)
    rounds = [-(-max(lens[lo:lo + 8]) // chunk) for lo in range(0, 32, 8)]
    assert len(ends) == sum(rounds), (len(ends), rounds)
    ttft_b = [ends[sum(rounds[:i // 8]) + -(-lens[i] // chunk) - 1]
              for i in range(32)]
    ends = forward_ends(continuous)
    first = first_token_steps(lens, 8, chunk, budget, NEW)
    assert len(ends) == first.pop(), "schedule and decoder disagree"
    ttft_c = [ends[s] for s in first]
    print(json.dumps({
        "model": "bloom-560m", "kv": kv, "prompts": lens, "new_tokens": NEW,
        "max_seqs": 8, "page": page, "prefill_chunk": chunk,
        "total_ms": med, "spread_pct": spread,
        "ms_all": {k: [round(x, 1) for x in t] for k, t in times.items()},
        "continuous_over_batched": round(med["continuous"]
                                         / med["batched_x4"], 3),
        "mean_ttft_ms": {"batched_x4": round(sum(ttft_b) / 32, 1),
                         "continuous": round(sum(ttft_c) / 32, 1)},
        "continuous_steps": len(ends),
    }), flush=True)
    ctx.destroy()


def first_token_steps(lens, max_seqs, chunk, budget, new):
    """The forward (0-based) of ``generate_continuous`` that yields each
    prompt's first token when pages never run short, then the number of
    forwards in all."""
    waiting, flight, step = list(range(len(lens))), [], 0
    left, held, first = list(lens), [0] * len(lens), [0] * len(lens)
    while waiting or flight:
        while waiting and len(flight) < max_seqs:
            flight.append(waiting.pop(0))
        sampled = [i for i in flight if left[i] == 0]
        room = budget - len(sampled)
        for i in flight:
            if left[i] and room:
                k = min(left[i], chunk, room)
                left[i], room = left[i] - k, room - k
                if left[i] == 0:
                    sampled.append(i)
                    first[i] = step
        for i in sampled:
            held[i] += 1
        flight = [i for i in flight if held[i] < new]
        step += 1
    return first + [step]
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=list(SHAPES),
                    default=["bloom-560m", "llama-7b", "gqa-32q8kv"])
    ap.add_argument("--mode", nargs="+", default=["decode", "mixed", "prefill"],
                    choices=["decode", "mixed", "prefill", "e2e"])
    ap.add_argument("--context", type=int, nargs="+",
                    default=[0, 128, 1024, 4096])
    ap.add_argument("--kv", default="bf16", choices=["bf16", "fp8"],
                    help="cache dtype; fp8 times paged_varlen_split_attn_fp8 "
                    "against the fp8 kernels, the bf16 split kernel a column")
    ap.add_argument("--page", type=int, default=16, choices=[16, 32, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()

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
               "--kv", args.kv, "--page", str(args.page),
               "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
