"""Timing of the fused rope + paged cache write (``paged_rope_write``,
ops/csrc/paged_rope_write.hip) against the sequence it replaces
(``PG_PAGED_ROPE=0``: rope_at_position(q), rope_at_position(k),
paged_kv_write), following the method of tools/paged_decode_attn_bench.py.

Usage (GPU box): python tools/paged_rope_write_bench.py [--cases ...]
                     [--decoder]

Kernel level: for each case (shape, B, S) and cache type (bf16, fp8) the two
paths are timed in the same process, alternating, with device events around
``--iters`` calls, ``--repeats`` times; the median and the spread
((max - min) / median) are reported in us per call.  q, k and v are
transposed views of [B, S, heads * D] buffers, as the models pass them; they
are a few hundred KB at most and stay in cache, as they do behind the
projection GEMMs.  Before timing, the two paths must agree: the pools within
one bf16 / e4m3 step of each other (the fused angle is more accurate), q_rot
likewise.

``--decoder``: ms/step of ``PagedDecoder`` on llama-1b (the llama config of
tools/decode_bench.py), graph and eager, fused and unfused: the difference of
a long and a short generate() over the difference in steps, so that prefill
and capture cancel.

Every case runs in a child process of its own under ``--step-timeout``; the
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

# name: (B, H, Hkv, D, S)
CASES = {
    "llama-7b-B1": (1, 32, 32, 128, 1),
    "llama-7b-B8": (8, 32, 32, 128, 1),
    "gqa-32q8kv-B1": (1, 32, 8, 128, 1),
    "gqa-32q8kv-B8": (8, 32, 8, 128, 1),
    "llama-7b-B1-S512": (1, 32, 32, 128, 512),
}
PAGE, MAX_LEN, THETA = 16, 4096, 1e4


def _summary(times):
    med = statistics.median(times)
    return {"us": round(med, 2),
            "spread": round((max(times) - min(times)) / med, 3)}


def run_case(name, iters, repeats, warmup):
    import torch
    from pipegoose_amd.ops.paged_attention import (paged_rope_write,
                                                   quantize_rows_fp8)

    assert torch.cuda.is_available(), "paged_rope_write_bench needs a GPU"
    B, H, Hkv, D, S = CASES[name]
    dev = "cuda"
    torch.manual_seed(0)
    max_pages = MAX_LEN // PAGE
    n_pages = B * max_pages + 1                         # + the null page
    table = (torch.randperm(n_pages - 1, device=dev) + 1).view(
        B, max_pages).to(torch.int32)
    start = (torch.arange(B, device=dev) * 37 + 1000) % (MAX_LEN - S)
    mk = lambda h: torch.randn(B, S, h * D, device=dev).bfloat16().view(
        B, S, h, D).transpose(1, 2)
    q, k, v = mk(H), mk(Hkv), mk(Hkv)

    def cache(fp8):
        pool = torch.randn(n_pages, Hkv, PAGE, D, device=dev).bfloat16()
        if not fp8:
            return [pool, pool.clone()], []
        b8, sc = quantize_rows_fp8(pool)
        return [b8, b8.clone()], [sc, sc.clone()]

    def timed(fn):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / iters            # us per call

    for kind in ("bf16", "fp8"):
        base = cache(kind == "fp8")                    # both start the same
        caches = {label: [[t.clone() for t in part] for part in base]
                  for label in ("fused", "unfused")}

        def call(label):
            pools, scales = caches[label]
            return paged_rope_write(q, k, v, *pools, table, start, THETA,
                                    *scales)

        def select(label):                  # read by the dispatcher per call
            os.environ["PG_PAGED_ROPE"] = "1" if label == "fused" else "0"
            return label

        # results must agree before a time means anything
        qa = call(select("fused")).float()
        qb = call(select("unfused")).float()
        assert (qa - qb).abs().max() <= 2.0 ** -6 * qb.abs().max()
        for a, b in zip(sum(caches["fused"], []), sum(caches["unfused"], [])):
            assert (a.float() - b.float()).abs().max() \
                <= 2.0 ** -3 * b.float().abs().max(), kind
        for _ in range(warmup):
            for label in caches:
                call(select(label))
        torch.cuda.synchronize()
        times = {label: [] for label in caches}
        for _ in range(repeats):                       # alternate the paths
            for label in caches:
                select(label)
                times[label].append(timed(lambda: call(label)))
        res = {label: _summary(t) for label, t in times.items()}
        print(json.dumps({
            "case": name, "cache": kind, "B": B, "H": H, "Hkv": Hkv, "D": D,
            "S": S, "page": PAGE, **res,
            "fused_over_unfused": round(
                res["fused"]["us"] / res["unfused"]["us"], 3)}), flush=True)


def run_decoder(kv, repeats):
    import torch
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models import llama as L
    from pipegoose_amd.models.paged_decode import PagedDecoder

    assert torch.cuda.is_available(), "paged_rope_write_bench needs a GPU"
    for name, value in (("RANK", "0"), ("LOCAL_RANK", "0"),
                        ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                        ("MASTER_PORT", "29877")):
        os.environ.setdefault(name, value)
    ctx = ParallelContext.from_torch()
    torch.manual_seed(0)
    cfg = L.llama_1b()
    model = L.LlamaForCausalLM(cfg, ctx).to("cuda", torch.bfloat16).eval()
    B, P, short, long_ = 8, 512, 8, 72
    prompts = [torch.randint(0, cfg.vocab_size, (P,), device="cuda")
               for _ in range(B)]
    n_pages = B * (-(-(P + long_) // PAGE)) + 1
    kv_dtype = torch.float8_e4m3fn if kv == "fp8" else None
    decs = {}
    for mode in ("graph", "eager"):
        for fused in ("1", "0"):
            os.environ["PG_PAGED_ROPE"] = fused        # held by a capture
            dec = PagedDecoder(model, B, n_pages, PAGE, P + long_,
                               use_graph=mode == "graph", kv_dtype=kv_dtype)
            dec.generate(prompts, short)               # warmup (+ capture)
            assert (dec._graph is not None) == (mode == "graph")
            decs[(mode, fused)] = dec
    times = {key: [] for key in decs}
    for _ in range(repeats):                           # alternate the paths
        for (mode, fused), dec in decs.items():
            os.environ["PG_PAGED_ROPE"] = fused
            t = []
            for n in (short, long_):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.generate(prompts, n)
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
            times[(mode, fused)].append((t[1] - t[0]) / (long_ - short) * 1e3)
    print(json.dumps({
        "decoder": "llama-1b", "cache": kv, "B": B, "prompt": P, "page": PAGE,
        "ms_per_step": {
            f"{mode}-{'fused' if fused == '1' else 'unfused'}": {
                "ms": round(statistics.median(t), 4),
                "spread": round((max(t) - min(t)) / statistics.median(t), 3)}
            for (mode, fused), t in times.items()}}), flush=True)
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES),
                    choices=list(CASES))
    ap.add_argument("--decoder", action="store_true",
                    help="time PagedDecoder steps instead of the op")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=120,
                    help="seconds allowed to each child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child:
        if args.decoder:
            run_decoder(args.child, args.repeats)
        else:
            run_case(args.child, args.iters, args.repeats, args.warmup)
        return
    for name in (("bf16", "fp8") if args.decoder else args.cases):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--iters", str(args.iters), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup)] \
            + (["--decoder"] if args.decoder else [])
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
