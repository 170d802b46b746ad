"""Kernel-level timing of PAGED decode attention against the contiguous
decode kernel (both in ops/csrc/decode_attention.hip), the sibling of
tools/decode_attn_bench.py: same three shapes, same filled lengths, same
timing method.

Usage (GPU box): python tools/paged_decode_attn_bench.py [--max-len 4096]
                     [--filled 128 1024 4096] [--pages 16 64]

For each (shape, filled length) the contiguous kernel and the paged kernel
at every page size are timed in the same process, alternating, with device
events around ``--iters`` calls, ``--repeats`` times; the median is reported
in us.  K/V rotate over several buffers (>= 1 GB in total per path) so that
no call finds its operands in the 256 MiB L3.  The pools hold exactly the
pages of the batch plus the null page, dealt to the sequences by a random
permutation, so consecutive logical pages are scattered over the pool.  Before
timing, the paged result must equal the contiguous kernel's on the gathered
cache bit for bit.

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

from tools.decode_attn_bench import SHAPES, needed_bytes  # noqa: E402


def run_shape(name, max_len, filled, pages, iters, repeats, warmup):
    import torch
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.paged_attention import paged_gather

    assert torch.cuda.is_available(), "paged_decode_attn_bench needs a GPU"
    ext = get_extension(required=True)
    B, H, Hkv, D, alibi = SHAPES[name]
    dev = "cuda"
    torch.manual_seed(0)
    scale = D ** -0.5
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    kv_bytes = 2 * B * Hkv * max_len * D * 2
    n_buf = max(2, min(8, -(-(1 << 30) // kv_bytes)))
    q = torch.randn(B, H, 1, D, device=dev).bfloat16()
    pos_t = torch.zeros(1, dtype=torch.long, device=dev)
    n_splits, chunk = ext.decode_attn_plan(B, Hkv, max_len, D)

    ks = [torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
          for _ in range(n_buf)]
    vs = [torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
          for _ in range(n_buf)]
    paths = {"contiguous": lambda i: ext.decode_attn(
        q, ks[i % n_buf], vs[i % n_buf], slopes, scale, pos_t, 0)}
    checks = {}
    for page in pages:
        assert max_len % page == 0
        max_pages = max_len // page
        n_pages = B * max_pages + 1                     # + the null page
        perm = torch.randperm(n_pages - 1, device=dev) + 1
        table = perm.view(B, max_pages).to(torch.int32)
        kps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
               for _ in range(n_buf)]
        vps = [torch.randn(n_pages, Hkv, page, D, device=dev).bfloat16()
               for _ in range(n_buf)]

        def paged(i, kps=kps, vps=vps, table=table):
            return ext.paged_decode_attn(q, kps[i % n_buf], vps[i % n_buf],
                                         table, slopes, scale, pos_t, 0)
        paths[f"paged{page}"] = paged
        checks[f"paged{page}"] = (kps[0], vps[0], table)

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
        for label, (kp, vp, table) in checks.items():
            flat = ext.decode_attn(
                q, paged_gather(kp, table, max_len).contiguous(),
                paged_gather(vp, table, max_len).contiguous(), slopes, scale,
                pos_t, 0)
            assert torch.equal(paths[label](0), flat), \
                f"{label} differs from the contiguous kernel at {length}"
        for i in range(warmup):
            for fn in paths.values():
                fn(i)
        torch.cuda.synchronize()
        times = {label: [] for label in paths}
        for _ in range(repeats):                       # alternate the paths
            for label, fn in paths.items():
                times[label].append(timed(fn))
        need = needed_bytes(B, Hkv, D, p)
        med = {label: statistics.median(t) for label, t in times.items()}
        print(json.dumps({
            "shape": name, "B": B, "H": H, "Hkv": Hkv, "D": D,
            "max_len": max_len, "filled": length, "n_splits": n_splits,
            "chunk": chunk, "kv_buffers": n_buf, "needed_MB": need / 1e6,
            "us": {label: round(t, 2) for label, t in med.items()},
            "us_all": {label: [round(x, 2) for x in t]
                       for label, t in times.items()},
            "GBps": {label: round(need / t / 1e3, 1)
                     for label, t in med.items()},
            "paged_over_contiguous": {
                label: round(t / med["contiguous"], 3)
                for label, t in med.items() if label != "contiguous"},
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--filled", type=int, nargs="+",
                    default=[128, 1024, 4096])
    ap.add_argument("--pages", type=int, nargs="+", default=[16, 64],
                    choices=[16, 32, 64, 128])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=120,
                    help="seconds allowed to each shape's child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert all(1 <= f <= args.max_len for f in args.filled)

    if args.child:
        run_shape(args.child, args.max_len, args.filled, args.pages,
                  args.iters, args.repeats, args.warmup)
        return
    for name in args.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--max-len", str(args.max_len), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--filled", *map(str, args.filled),
               "--pages", *map(str, args.pages)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
