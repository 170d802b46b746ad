"""MoE routing-plan / permute / combine kernels vs the eager torch they replace.

Usage (GPU box): python tools/moe_permute_bench.py [--markdown] [--quick]

Shape: the bloom-1b7 MoE bank (N=16384 tokens, H=2048, E=8) with router
fan-out k = 1 and 2 and three routes: balanced and skewed with every slot
kept (M = S = N*k), and `dropped`, the balanced route with about 25 % of
the kept weights zeroed (capacity drops: M < S, so the kernels also
zero-fill dead rows while the eager path works on M rows).  For each of the
five kernels of csrc/moe_permute.hip it times

  hip    the kernel (the plan is its three launches)
  torch  the exact eager sequence of Experts._forward_local_grouped (and
         of its autograd) that the kernel replaces, host syncs included

alternated inside each round; the table reports the median over rounds with
the min..max spread of device-event times of `iters` back-to-back calls, and
the useful GB/s: the bytes that must move (every distinct live input row
read once, every live output row written once; zero-filled dead rows do
not count) divided by the median time.
The summary is committed under profiles/moe_grouped_gemm.md.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pipegoose_amd.ops import get_extension  # noqa: E402

N, H, E = 16384, 2048, 8
SKEW = [8192, 4096, 2048, 1024, 512, 256, 128, 128]


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def make_route(kind, k, gen):
    if kind in ("balanced", "dropped"):
        s = torch.arange(N * k, device="cuda")
        return (s % E).reshape(N, k)
    p = torch.tensor(SKEW, dtype=torch.float32, device="cuda")
    return torch.multinomial(p.expand(N, E), k, replacement=False,
                             generator=gen)


def make_contenders(ext, order, weight, x, ys, dxs, dout):
    """{kernel: (useful bytes, {impl: callable})}"""
    k = order.size(1)
    S = N * k
    off, ros, sor = ext.moe_route_plan(order, weight, 0, E)
    gates = weight.gather(1, order).reshape(-1).float()
    row_b = H * 2
    M = off[-1].item()                                   # kept slots
    n_in = (ros.view(N, k) >= 0).any(1).sum().item()     # tokens with any

    # the eager dispatch state of _forward_local_grouped
    def torch_plan():
        tok = torch.arange(N, device="cuda").repeat_interleave(k)
        ridx = order.reshape(-1)
        keep = (ridx >= 0) & (ridx < E)
        wvals = weight[tok, ridx]
        keep = keep & (wvals > 0)
        tok, ridx = tok[keep], ridx[keep]
        perm = torch.argsort(ridx, stable=True)
        tok, ridx = tok[perm], ridx[perm]
        counts = torch.bincount(ridx, minlength=E)
        offsets = torch.zeros(E + 1, device="cuda", dtype=torch.int32)
        offsets[1:] = torch.cumsum(counts, 0)
        return tok, wvals[keep][perm], offsets

    tok, wsorted, _ = torch_plan()
    wcol = wsorted.unsqueeze(-1).to(torch.bfloat16)
    ys_m, dxs_m = ys[:M], dxs[:M]       # the eager buffers have M rows

    def torch_permute_bwd():
        return torch.zeros_like(x).index_put_((tok,), dxs_m, accumulate=True)

    def torch_combine_fwd():
        eo = ys_m * wcol
        if k == 1:
            return torch.zeros_like(x).index_put((tok,), eo)
        out32 = torch.zeros(x.shape, device="cuda", dtype=torch.float32)
        return out32.index_put((tok,), eo.float(),
                               accumulate=True).to(torch.bfloat16)

    def torch_combine_bwd():
        if k == 1:
            d = dout[tok]
        else:
            d = dout.float()[tok].to(torch.bfloat16)
        return d * wcol, (d * ys_m).sum(-1)

    return {
        "route_plan": (S * (8 + 2 + 8), {
            "hip": lambda: ext.moe_route_plan(order, weight, 0, E),
            "torch": torch_plan}),
        "permute_fwd": ((n_in + M) * row_b, {
            "hip": lambda: ext.moe_permute_fwd(x, sor, k),
            "torch": lambda: x[tok]}),
        "permute_bwd": ((N + M) * row_b, {
            "hip": lambda: ext.moe_permute_bwd(dxs, ros, N, k),
            "torch": torch_permute_bwd}),
        "combine_fwd": ((N + M) * row_b, {
            "hip": lambda: ext.moe_combine_fwd(ys, gates, ros, N, k),
            "torch": torch_combine_fwd}),
        "combine_bwd": ((n_in + 2 * M) * row_b, {
            "hip": lambda: ext.moe_combine_bwd(dout, ys, gates, sor, k, True),
            "torch": torch_combine_bwd}),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--quick", action="store_true",
                    help="fewer rounds (smoke-testing the tool)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ext = get_extension(required=True)
    rounds, iters = (2, 3) if args.quick else (7, 10)

    rows = []
    for k in (1, 2):
        for kind in ("balanced", "skewed", "dropped"):
            gen = torch.Generator(device="cuda").manual_seed(0)
            rnd = lambda *s: (torch.rand(*s, device="cuda", generator=gen)  # noqa: E731
                              * 2 - 1).bfloat16()
            order = make_route(kind, k, gen)
            weight = (torch.rand(N, E, device="cuda", generator=gen)
                      + 0.1).bfloat16()
            if kind == "dropped":
                weight = weight * (torch.rand(N, E, device="cuda",
                                              generator=gen) >= 0.25)
            x, dout = rnd(N, H), rnd(N, H)
            ys, dxs = rnd(N * k, H), rnd(N * k, H)
            for name, (nbytes, impls) in make_contenders(
                    ext, order, weight, x, ys, dxs, dout).items():
                for f in impls.values():        # warm every shape
                    time_ms(f, 2)
                samples = {i: [] for i in impls}
                for _ in range(rounds):         # alternate the contenders
                    for i, f in impls.items():
                        samples[i].append(time_ms(f, iters))
                rows.append((k, kind, name, nbytes, samples))
            del x, dout, ys, dxs
            torch.cuda.empty_cache()

    def cell(v):
        return (f"{statistics.median(v):.4f} "
                f"({min(v):.4f}..{max(v):.4f})")

    if args.markdown:
        print("| k | route | kernel | hip ms | torch ms | hip GB/s | "
              "torch GB/s | torch/hip |")
        print("|---" * 8 + "|")
    for k, kind, name, nbytes, s in rows:
        med = {i: statistics.median(v) for i, v in s.items()}
        gbs = {i: nbytes / (m * 1e-3) / 1e9 for i, m in med.items()}
        cols = [str(k), kind, name, cell(s["hip"]), cell(s["torch"]),
                f"{gbs['hip']:.0f}", f"{gbs['torch']:.0f}",
                f"{med['torch'] / med['hip']:.2f}x"]
        print("| " + " | ".join(cols) + " |" if args.markdown
              else "  ".join(cols))


if __name__ == "__main__":
    main()
