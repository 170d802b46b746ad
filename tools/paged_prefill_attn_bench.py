"""Timing of paged PREFILL attention (ops/csrc/paged_prefill_attention.hip),
the sibling of tools/paged_decode_attn_bench.py: same three shapes, same
timing method.

Usage (GPU box): python tools/paged_prefill_attn_bench.py
                     [--sq 128 512] [--context 0 1024 3584] [--pages 16 64]
                 python tools/paged_prefill_attn_bench.py --e2e

Kernel level.  For each (shape, Sq, context) the chunk of ``Sq`` query rows
sits at ``start = context`` and sees ``context + Sq`` keys.  Timed in the same
process, alternating, with device events around ``--iters`` calls,
``--repeats`` times, median in us:

  paged{PAGE}   the kernel at every page size; pools hold exactly the pages
                of the batch plus the null page, dealt by a random permutation
  gather+sdpa   ``paged_gather`` of the ``context + Sq`` visible rows, kv heads
                expanded for GQA, torch sdpa in bf16 with the causal(+ALiBi)
                bias [H, Sq, keys]: the job without the kernel (the bias is
                built once, outside the timed window)
  attn_fwd      context 0 only, for orientation: the training forward on
                contiguous tensors (no table, no pools)

K/V rotate over several pools (>= 1 GB in total) so that no call finds its
operands in the 256 MiB L3.  Before timing, the kernel's result must agree
with gather+sdpa to bf16 accuracy.

End to end (``--e2e``): bloom-560m, a 2048-token prompt through PagedDecoder —
time to first token whole against ``prefill_chunk=512``, and two prompts that
share 1536 tokens with and without ``share_prefix``.

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

from tools.decode_attn_bench import SHAPES  # noqa: E402


def attn_flops(B, H, D, Sq, context):
    """QK^T and PV over the visible (row, key) pairs."""
    pairs = Sq * context + Sq * (Sq + 1) // 2
    return 4 * B * H * D * pairs


def run_shape(name, sqs, contexts, pages, iters, repeats, warmup):
    import torch
    import torch.nn.functional as TF
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.paged_attention import paged_gather

    assert torch.cuda.is_available(), "paged_prefill_attn_bench needs a GPU"
    ext = get_extension(required=True)
    B, H, Hkv, D, alibi = SHAPES[name]
    G = H // Hkv
    dev = "cuda"
    torch.manual_seed(0)
    scale = D ** -0.5
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    max_len = max(contexts) + max(sqs)
    max_len = -(-max_len // max(pages)) * max(pages)
    kv_bytes = 2 * B * Hkv * max_len * D * 2
    n_buf = max(2, min(8, -(-(1 << 30) // kv_bytes)))
    start_t = torch.zeros(1, dtype=torch.long, device=dev)

    pools = {}
    for page in pages:
        max_pages = max_len // page
        n_pages = B * max_pages + 1                     # + the null page
        perm = torch.randperm(n_pages - 1, device=dev) + 1
        table = perm.view(B, max_pages).to(torch.int32)
        kps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
               for _ in range(n_buf)]
        vps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
               for _ in range(n_buf)]
        pools[page] = (kps, vps, table)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters      # us per call

    for Sq in sqs:
        # the models' layout: [B, Sq, H, D] in memory
        q = torch.randn(B, Sq, H, D, device=dev).bfloat16().transpose(1, 2)
        for context in contexts:
            keys = context + Sq
            start_t.fill_(context)
            rel = torch.arange(keys, device=dev)[None, :] \
                - (context + torch.arange(Sq, device=dev))[:, None]
            bias = (slopes[:, None, None] * rel).masked_fill(
                rel > 0, float("-inf")).bfloat16()[None]   # [1, H, Sq, keys]

            paths = {}
            for page in pages:
                kps, vps, table = pools[page]

                def paged(i, kps=kps, vps=vps, table=table):
                    return ext.paged_prefill_attn(
                        q, kps[i % n_buf], vps[i % n_buf], table, slopes,
                        scale, start_t)
                paths[f"paged{page}"] = paged
            kps, vps, table = pools[pages[0]]

            def gather_sdpa(i, kps=kps, vps=vps, table=table):
                k = paged_gather(kps[i % n_buf], table, keys)
                v = paged_gather(vps[i % n_buf], table, keys)
                if G > 1:
                    k = k.repeat_interleave(G, dim=1)
                    v = v.repeat_interleave(G, dim=1)
                return TF.scaled_dot_product_attention(
                    q, k, v, attn_mask=bias, scale=scale)
            paths["gather+sdpa"] = gather_sdpa
            if context == 0 and Sq % 64 == 0:
                kc = [torch.randn(B, Sq, Hkv, D, device=dev).bfloat16()
                      .transpose(1, 2) for _ in range(n_buf)]
                vc = [torch.randn(B, Sq, Hkv, D, device=dev).bfloat16()
                      .transpose(1, 2) for _ in range(n_buf)]
                paths["attn_fwd"] = lambda i: ext.attn_fwd(
                    q, kc[i % n_buf], vc[i % n_buf], slopes, scale, 0)

            # results must agree before a time means anything
            want = gather_sdpa(0).float()
            got = paths[f"paged{pages[0]}"](0).float()
            err = (got - want).abs().max().item()
            assert err <= 2.0 ** -5 * max(1.0, want.abs().max().item()), \
                f"kernel differs from gather+sdpa by {err} at {Sq}/{context}"

            for i in range(warmup):
                for fn in paths.values():
                    fn(i)
            torch.cuda.synchronize()
            times = {label: [] for label in paths}
            for _ in range(repeats):                   # alternate the paths
                for label, fn in paths.items():
                    times[label].append(timed(fn))
            med = {label: statistics.median(t) for label, t in times.items()}
            flops = attn_flops(B, H, D, Sq, context)
            print(json.dumps({
                "shape": name, "B": B, "H": H, "Hkv": Hkv, "D": D,
                "Sq": Sq, "context": context, "kv_buffers": n_buf,
                "GFLOP": round(flops / 1e9, 2),
                "us": {label: round(t, 1) for label, t in med.items()},
                "us_all": {label: [round(x, 1) for x in t]
                           for label, t in times.items()},
                "TFLOPs": {label: round(flops / t / 1e6, 1)
                           for label, t in med.items()
                           if label.startswith("paged")},
                "kernel_over_fallback": {
                    label: round(t / med["gather+sdpa"], 3)
                    for label, t in med.items() if label.startswith("paged")},
            }), flush=True)


def run_e2e(prompt_len, chunk, shared, repeats):
    """bloom-560m through PagedDecoder: time to first token (one new token,
    so no decode step runs), host clock around a device synchronise."""
    import torch
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.models.bloom import BloomConfig, BloomForCausalLM
    from pipegoose_amd.models.paged_decode import PagedDecoder

    assert torch.cuda.is_available(), "paged_prefill_attn_bench needs a GPU"
    for name, value in (("RANK", "0"), ("LOCAL_RANK", "0"),
                        ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"),
                        ("MASTER_PORT", "29897")):
        os.environ.setdefault(name, value)
    ctx = ParallelContext.from_torch()
    torch.manual_seed(0)
    cfg = BloomConfig(vocab_size=250880, hidden_size=1024, n_layer=24,
                      n_head=16)
    model = BloomForCausalLM(cfg, ctx).to("cuda", torch.bfloat16).eval()
    page = 16
    prompt = torch.randint(0, cfg.vocab_size, (prompt_len,), device="cuda")
    second = torch.cat([prompt[:shared], torch.randint(
        0, cfg.vocab_size, (prompt_len - shared,), device="cuda")])
    n_pages = 2 * (-(-(prompt_len + 1) // page)) + 1

    def ttft(prompts, **kwargs):
        chunked = kwargs.pop("prefill_chunk", None)
        dec = PagedDecoder(model, max_seqs=2, n_pages=n_pages, page_size=page,
                           max_len=prompt_len + page, use_graph=False,
                           prefill_chunk=chunked)
        dec.generate(prompts, 1, **kwargs)              # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            dec.generate(prompts, 1, **kwargs)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"ms": round(statistics.median(times), 2),
                "ms_all": [round(t, 2) for t in times],
                "peak_MB": round(torch.cuda.max_memory_allocated() / 1e6)}

    print(json.dumps({
        "model": "bloom-560m", "prompt": prompt_len, "page": page,
        "whole": ttft([prompt]),
        f"prefill_chunk={chunk}": ttft([prompt], prefill_chunk=chunk),
        f"two prompts sharing {shared}, share_prefix=False":
            ttft([prompt, second]),
        f"two prompts sharing {shared}, share_prefix=True":
            ttft([prompt, second], share_prefix=True),
    }), flush=True)
    ctx.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--sq", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--context", type=int, nargs="+",
                    default=[0, 1024, 3584])
    ap.add_argument("--pages", type=int, nargs="+", default=[16, 64],
                    choices=[16, 32, 64, 128])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", action="store_true",
                    help="the end-to-end PagedDecoder timings instead")
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--shared", type=int, default=1536)
    ap.add_argument("--step-timeout", type=int, default=240,
                    help="seconds allowed to each child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child == "e2e":
        run_e2e(args.prompt, args.chunk, args.shared, args.repeats)
        return
    if args.child:
        run_shape(args.child, args.sq, args.context, args.pages, args.iters,
                  args.repeats, args.warmup)
        return
    common = ["--iters", str(args.iters), "--repeats", str(args.repeats),
              "--warmup", str(args.warmup)]
    if args.e2e:
        jobs = {"e2e": ["--prompt", str(args.prompt), "--chunk",
                        str(args.chunk), "--shared", str(args.shared)]}
    else:
        jobs = {name: ["--sq", *map(str, args.sq), "--context",
                       *map(str, args.context), "--pages",
                       *map(str, args.pages)] for name in args.shapes}
    for name, extra in jobs.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               *common, *extra]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
