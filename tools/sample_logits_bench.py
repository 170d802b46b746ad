"""Timing of the HIP sampler (``sample_logits``, ops/csrc/sampling.hip) against
the torch sequence it replaces, following the method of
tools/paged_rope_write_bench.py.

Usage (GPU box): python tools/sample_logits_bench.py [--cases ...] [--decoder]

Kernel level: for each case (R rows, vocabulary V) and parameter set
(temperature only, top-k 50, top-k 50 + top-p 0.9) three paths are timed in
the same process, alternating, with device events around ``--iters`` calls,
``--repeats`` times: the kernel with the auto plan, the kernel with
``splits=1``, and ``torch``: the body of the former ``generation._sample``
on the bf16 row (cast to fp32, divide, ``topk`` + ``masked_fill``, ``softmax``,
``multinomial``) with a sort-based top-p before the softmax where top-p is on.
The median and the spread ((max - min) / median) are reported in us per call.
The logits are at most 32 MB and stay in the last-level cache, as they do
behind the LM-head GEMM.

``--decoder``: ms/step of ``PagedDecoder`` on bloom-560m under a graph, 8
rows: greedy twice (two decoders, alternating: their difference is the
run-to-run spread of the unchanged greedy step) and sampled (temperature 0.8,
top-k 50, top-p 0.9): the difference of a long and a short generate() over
the difference in steps, so that prefill and capture cancel.

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

CASES = {f"R{R}-V{V}": (R, V) for R in (1, 8, 64)
         for V in (32000, 128256, 250880)}
# name: (temperature, top_k, top_p)
PARAMS = {"T": (0.8, 0, 1.0), "T+k50": (0.8, 50, 1.0),
          "T+k50+p0.9": (0.8, 50, 0.9)}


def _summary(times):
    med = statistics.median(times)
    return {"us": round(med, 2),
            "spread": round((max(times) - min(times)) / med, 3)}


def torch_sample(logits, temperature, top_k, top_p):
    import torch
    logits = logits.float() / temperature
    if top_k > 0:
        kth = logits.topk(top_k, dim=-1).values[..., -1, None]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1:
        srt, idx = logits.sort(dim=-1, descending=True)
        cum = torch.softmax(srt, dim=-1).cumsum(-1)
        drop = cum - torch.softmax(srt, dim=-1) >= top_p
        logits = logits.masked_fill(
            torch.zeros_like(drop).scatter(-1, idx, drop), float("-inf"))
    return torch.multinomial(torch.softmax(logits, dim=-1), 1).squeeze(-1)


def run_case(name, iters, repeats, warmup):
    import torch
    from pipegoose_amd.ops.sampling import sample_logits

    assert torch.cuda.is_available(), "sample_logits_bench needs a GPU"
    R, V = CASES[name]
    torch.manual_seed(0)
    logits = (4 * torch.randn(R, V, device="cuda")).bfloat16()
    u = torch.rand(R, device="cuda")

    def timed(fn):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / iters            # us per call

    for pname, (T, k, p) in PARAMS.items():
        Tt = torch.full((R,), T, device="cuda")
        kt = torch.full((R,), k, device="cuda", dtype=torch.int32)
        pt = torch.full((R,), p, device="cuda")
        paths = {
            "auto": lambda: sample_logits(logits, u, Tt, kt, pt),
            "splits1": lambda: sample_logits(logits, u, Tt, kt, pt, splits=1),
            "torch": lambda: torch_sample(logits, T, k, p),
        }
        # the plans must agree before a time means anything
        assert torch.equal(paths["auto"](), paths["splits1"]())
        for _ in range(warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        times = {label: [] for label in paths}
        for _ in range(repeats):                       # alternate the paths
            for label, fn in paths.items():
                times[label].append(timed(fn))
        res = {label: _summary(t) for label, t in times.items()}
        print(json.dumps({
            "case": name, "params": pname, "R": R, "V": V, **res,
            "auto_over_torch": round(res["auto"]["us"] / res["torch"]["us"],
                                     3),
            "auto_over_splits1": round(
                res["auto"]["us"] / res["splits1"]["us"], 3)}), flush=True)


def run_decoder(repeats):
    import torch
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models import bloom as B_
    from pipegoose_amd.models.paged_decode import PagedDecoder

    assert torch.cuda.is_available(), "sample_logits_bench needs a GPU"
    for name, value in (("RANK", "0"), ("LOCAL_RANK", "0"),
                        ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                        ("MASTER_PORT", "29878")):
        os.environ.setdefault(name, value)
    ctx = ParallelContext.from_torch()
    torch.manual_seed(0)
    cfg = B_.bloom_560m()
    model = B_.BloomForCausalLM(cfg, ctx).to("cuda", torch.bfloat16).eval()
    B, P, short, long_, page = 8, 512, 8, 72, 16
    prompts = [torch.randint(0, cfg.vocab_size, (P,), device="cuda")
               for _ in range(B)]
    n_pages = B * (-(-(P + long_) // page)) + 1
    sampled = dict(temperature=0.8, top_k=50, top_p=0.9)
    runs = {"greedy": {}, "greedy-again": {}, "sampled": sampled}
    decs = {}
    for label, kwargs in runs.items():
        dec = PagedDecoder(model, B, n_pages, page, P + long_)
        dec.generate(prompts, short, **kwargs)         # warmup + capture
        assert dec._graph is not None
        decs[label] = dec
    times = {label: [] for label in decs}
    for _ in range(repeats):                           # alternate the paths
        for label, dec in decs.items():
            t = []
            for n in (short, long_):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.generate(prompts, n, **runs[label])
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
            times[label].append((t[1] - t[0]) / (long_ - short) * 1e3)
    print(json.dumps({
        "decoder": "bloom-560m", "B": B, "prompt": P, "page": page,
        "ms_per_step": {
            label: {"ms": round(statistics.median(t), 4),
                    "spread": round((max(t) - min(t)) / statistics.median(t),
                                    3)}
            for label, t in times.items()}}), flush=True)
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES),
                    choices=list(CASES))
    ap.add_argument("--decoder", action="store_true",
                    help="time PagedDecoder steps instead of the op")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=120,
                    help="seconds allowed to each child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child:
        if args.decoder:
            run_decoder(args.repeats)
        else:
            run_case(args.child, args.iters, args.repeats, args.warmup)
        return
    for name in (("bloom-560m",) if args.decoder else args.cases):
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
