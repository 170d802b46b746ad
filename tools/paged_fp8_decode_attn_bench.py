"""Kernel-level timing of the fp8 paged cache kernels
(ops/csrc/paged_fp8_attention.hip) against their bf16 twins
(ops/csrc/decode_attention.hip), with the method and shapes of
tools/paged_decode_attn_bench.py.

Usage (GPU box): python tools/paged_fp8_decode_attn_bench.py [--max-len 4096]
                     [--filled 128 1024 4096] [--pages 16 64] [--s-new 1 512]

Decode: for each (shape, page size, filled length) ``paged_decode_attn`` and
``paged_decode_attn_fp8`` are timed in the same process, alternating, with
device events around ``--iters`` calls, ``--repeats`` times; median and
spread ((max - min) / median) are reported in us.  Pools (and scales) rotate
over several buffers, >= 1 GB in total per path, so that no call finds its
operands in the 256 MiB L3; the pages of the batch are dealt by a random
permutation.  The fp8 pools are filled by the write kernel from the bf16
rows, and before timing the fp8 result must lie within the tests' bound of
the fp64 reference on the dequantised gather.  ``needed_MB`` counts the K+V
bytes (and, for fp8, the scale bytes) of the live rows.

Write: ``paged_kv_write`` against ``paged_kv_write_fp8`` at ``--s-new`` new
rows per sequence, same alternation and statistics.

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


def _stats(times):
    med = statistics.median(times)
    return round(med, 2), round((max(times) - min(times)) / med, 3)


def run_shape(name, max_len, filled, pages, s_news, iters, repeats, warmup):
    import torch
    from pipegoose_amd.models.bloom import alibi_slopes
    from pipegoose_amd.ops import get_extension
    from pipegoose_amd.ops.paged_attention import (
        paged_decode_attention_reference, paged_gather_dequant)

    assert torch.cuda.is_available(), "paged_fp8_decode_attn_bench needs a GPU"
    ext = get_extension(required=True)
    B, H, Hkv, D, alibi = SHAPES[name]
    dev = "cuda"
    torch.manual_seed(0)
    scale = D ** -0.5
    slopes = (alibi_slopes(H) if alibi else torch.zeros(H)).to(dev).float()
    kv_bytes = 2 * B * Hkv * max_len * D       # the fp8 path, the smaller one
    n_buf = max(2, min(16, -(-(1 << 30) // kv_bytes)))
    q = torch.randn(B, H, 1, D, device=dev).bfloat16()
    pos_t = torch.zeros(1, dtype=torch.long, device=dev)
    zero = torch.zeros(1, dtype=torch.long, device=dev)

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / iters      # us per call

    def compare(paths):
        for i in range(warmup):
            for fn in paths.values():
                fn(i)
        torch.cuda.synchronize()
        times = {label: [] for label in paths}
        for _ in range(repeats):                       # alternate the paths
            for label, fn in paths.items():
                times[label].append(timed(fn))
        return times

    for page in pages:
        assert max_len % page == 0
        max_pages = max_len // page
        n_pages = B * max_pages + 1                     # + the null page
        table = (torch.randperm(n_pages - 1, device=dev) + 1).view(
            B, max_pages).to(torch.int32)
        pool = lambda dt: torch.zeros(n_pages, Hkv, page, D, device=dev,
                                      dtype=dt)
        sc = lambda: torch.zeros(n_pages, Hkv, page, device=dev)
        kps, vps, k8s, v8s, kss, vss = [], [], [], [], [], []
        for _ in range(n_buf):
            k = torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
            v = torch.randn(B, Hkv, max_len, D, device=dev).bfloat16()
            kps.append(pool(torch.bfloat16)), vps.append(pool(torch.bfloat16))
            k8s.append(pool(torch.float8_e4m3fn))
            v8s.append(pool(torch.float8_e4m3fn))
            kss.append(sc()), vss.append(sc())
            ext.paged_kv_write(k, v, kps[-1], vps[-1], table, zero)
            ext.paged_kv_write_fp8(k, v, k8s[-1], v8s[-1], kss[-1], vss[-1],
                                   table, zero)
        paths = {
            "bf16": lambda i: ext.paged_decode_attn(
                q, kps[i % n_buf], vps[i % n_buf], table, slopes, scale,
                pos_t, 0),
            "fp8": lambda i: ext.paged_decode_attn_fp8(
                q, k8s[i % n_buf], v8s[i % n_buf], kss[i % n_buf],
                vss[i % n_buf], table, slopes, scale, pos_t, 0)}
        for length in filled:
            p = length - 1
            pos_t.fill_(p)
            # the result must be right before a time means anything
            ref = paged_decode_attention_reference(
                q.double(), k8s[0], v8s[0], table, slopes.double(), scale,
                pos_t, kss[0], vss[0])
            vmax = paged_gather_dequant(v8s[0], vss[0], table, length,
                                        torch.float64).abs().max()
            err = (paths["fp8"](0).double() - ref).abs()
            assert (err <= 2.0 ** -7 * ref.abs() + 2.0 ** -7 * vmax).all(), \
                f"fp8 kernel outside the bound at page {page}, {length}"
            times = compare(paths)
            need = {"bf16": needed_bytes(B, Hkv, D, p),
                    "fp8": needed_bytes(B, Hkv, D, p) // 2
                    + 2 * B * Hkv * length * 4}
            med = {label: _stats(t) for label, t in times.items()}
            print(json.dumps({
                "op": "decode", "shape": name, "B": B, "H": H, "Hkv": Hkv,
                "D": D, "page": page, "max_len": max_len, "filled": length,
                "kv_buffers": n_buf,
                "needed_MB": {k: v / 1e6 for k, v in need.items()},
                "us": {k: m for k, (m, _) in med.items()},
                "spread": {k: s for k, (_, s) in med.items()},
                "us_all": {k: [round(x, 2) for x in t]
                           for k, t in times.items()},
                "GBps": {k: round(need[k] / med[k][0] / 1e3, 1) for k in med},
                "fp8_over_bf16": round(med["fp8"][0] / med["bf16"][0], 3),
            }), flush=True)
        for s_new in s_news:
            k = torch.randn(B, Hkv, s_new, D, device=dev).bfloat16()
            v = torch.randn(B, Hkv, s_new, D, device=dev).bfloat16()
            times = compare({
                "bf16": lambda i: ext.paged_kv_write(
                    k, v, kps[i % n_buf], vps[i % n_buf], table, zero),
                "fp8": lambda i: ext.paged_kv_write_fp8(
                    k, v, k8s[i % n_buf], v8s[i % n_buf], kss[i % n_buf],
                    vss[i % n_buf], table, zero)})
            med = {label: _stats(t) for label, t in times.items()}
            print(json.dumps({
                "op": "write", "shape": name, "B": B, "Hkv": Hkv, "D": D,
                "page": page, "S_new": s_new,
                "us": {k: m for k, (m, _) in med.items()},
                "spread": {k: s for k, (_, s) in med.items()},
                "us_all": {k: [round(x, 2) for x in t]
                           for k, t in times.items()},
                "fp8_over_bf16": round(med["fp8"][0] / med["bf16"][0], 3),
            }), flush=True)
        del kps, vps, k8s, v8s, kss, vss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES),
                    choices=list(SHAPES))
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--filled", type=int, nargs="+",
                    default=[128, 1024, 4096])
    ap.add_argument("--pages", type=int, nargs="+", default=[16, 64],
                    choices=[16, 32, 64, 128])
    ap.add_argument("--s-new", type=int, nargs="+", default=[1, 512])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=180,
                    help="seconds allowed to each shape's child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert all(1 <= f <= args.max_len for f in args.filled)
    assert all(1 <= s <= args.max_len for s in args.s_new)

    if args.child:
        run_shape(args.child, args.max_len, args.filled, args.pages,
                  args.s_new, args.iters, args.repeats, args.warmup)
        return
    for name in args.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
               "--max-len", str(args.max_len), "--iters", str(args.iters),
               "--repeats", str(args.repeats), "--warmup", str(args.warmup),
               "--filled", *map(str, args.filled),
               "--pages", *map(str, args.pages),
               "--s-new", *map(str, args.s_new)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {args.step_timeout} s; "
                     "stopping")
        if rc != 0:
            sys.exit(f"{name}: child exited with {rc}; stopping")


if __name__ == "__main__":
    main()
