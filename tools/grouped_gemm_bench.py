"""Grouped expert GEMM kernels vs the per-expert loop and the padded bmm bank.

Usage (GPU box): python tools/grouped_gemm_bench.py [--markdown] [--quick]

Shapes are the bloom-1b7 MoE bank (T=16384 tokens, H=2048, I=8192, E=8),
both linears (up: K=H, N=I; down: K=I, N=H), with one balanced and one
skewed count vector.  For each of the three passes it times

  hip   csrc/grouped_gemm.hip (one launch, ragged, weights in place)
  loop  E separate hipBLASLt GEMMs on the segment slices (what the
        per-expert loop pays for the GEMMs alone: no mask/gather/scatter)
  bmm   the PG_MOE_GROUPED=1 arithmetic: pad to the largest segment, stack
        the weights, contiguous transposed copies, torch.bmm, unpad

The three are alternated inside each round and the table reports the median
over rounds with the min..max spread; times are device-event times of
`iters` back-to-back calls.  TF/s counts the useful 2*T*N*K flops only.
The summary is committed under profiles/moe_grouped_gemm.md.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pipegoose_amd.ops import get_extension  # noqa: E402

T, H, I, E = 16384, 2048, 8192, 8
COUNTS = {
    "balanced": [T // E] * E,
    "skewed": [8192, 4096, 2048, 1024, 512, 256, 128, 128],
}


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def pad(x, counts):
    out = torch.zeros(len(counts), max(counts), x.size(1), device=x.device,
                      dtype=x.dtype)
    s = 0
    for e, c in enumerate(counts):
        out[e, :c] = x[s:s + c]
        s += c
    return out


def unpad(y, counts):
    return torch.cat([y[e, :c] for e, c in enumerate(counts) if c])


def make_passes(ext, x, dy, ws, counts):
    """{pass: {impl: callable}}; every callable returns the pass's result
    in the hip layout so the three can be compared."""
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)),
                       dtype=torch.int32, device="cuda")
    n_exp = len(counts)
    bounds, s = [], 0
    for c in counts:
        bounds.append((s, s + c))
        s += c

    def loop_fwd():
        return torch.cat([x[a:b] @ ws[e].t()
                          for e, (a, b) in enumerate(bounds)])

    def loop_dgrad():
        return torch.cat([dy[a:b] @ ws[e]
                          for e, (a, b) in enumerate(bounds)])

    def loop_wgrad():
        return torch.stack([dy[a:b].t() @ x[a:b] for (a, b) in bounds])

    def bmm_fwd():
        W = torch.stack(ws)
        return unpad(torch.bmm(pad(x, counts),
                               W.transpose(1, 2).contiguous()), counts)

    def bmm_dgrad():
        W = torch.stack(ws)
        return unpad(torch.bmm(pad(dy, counts), W.contiguous()), counts)

    def bmm_wgrad():
        return torch.bmm(pad(dy, counts).transpose(1, 2).contiguous(),
                         pad(x, counts))

    return {
        "fwd": {"hip": lambda: ext.grouped_gemm_fwd(x, ws, off, None),
                "loop": loop_fwd, "bmm": bmm_fwd},
        "dgrad": {"hip": lambda: ext.grouped_gemm_dgrad(dy, ws, off),
                  "loop": loop_dgrad, "bmm": bmm_dgrad},
        "wgrad": {"hip": lambda: ext.grouped_gemm_wgrad(
                      dy, x, off, n_exp, True)[0],
                  "loop": loop_wgrad, "bmm": bmm_wgrad},
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
    for lin, K, N in (("up", H, I), ("down", I, H)):
        for cname, counts in COUNTS.items():
            gen = torch.Generator(device="cuda").manual_seed(0)
            rnd = lambda *s: (torch.rand(*s, device="cuda", generator=gen)  # noqa: E731
                              * 2 - 1).bfloat16()
            x, dy = rnd(T, K), rnd(T, N)
            ws = [rnd(N, K) for _ in range(E)]
            passes = make_passes(ext, x, dy, ws, counts)
            flops = 2.0 * T * N * K
            for pname, impls in passes.items():
                ref = impls["loop"]().float()
                scale = max(ref.abs().max().item(), 1.0)
                relerr = {k: (f().float() - ref).abs().max().item() / scale
                          for k, f in impls.items() if k != "loop"}
                del ref
                for f in impls.values():        # warm every shape
                    time_ms(f, 2)
                samples = {k: [] for k in impls}
                for _ in range(rounds):         # alternate the contenders
                    for k, f in impls.items():
                        samples[k].append(time_ms(f, iters))
                rows.append((lin, cname, pname, flops, samples, relerr))
            del x, dy, ws, passes
            torch.cuda.empty_cache()

    def cell(v):
        med = statistics.median(v)
        return f"{med:.3f} ({min(v):.3f}..{max(v):.3f})"

    if args.markdown:
        print("| linear | counts | pass | hip ms | loop ms | bmm ms | hip TF/s "
              "| loop TF/s | hip relerr | bmm relerr |")
        print("|---" * 10 + "|")
    for lin, cname, pname, flops, s, relerr in rows:
        tf = {k: flops / (statistics.median(v) * 1e-3) / 1e12
              for k, v in s.items()}
        cols = [lin, cname, pname, cell(s["hip"]), cell(s["loop"]),
                cell(s["bmm"]), f"{tf['hip']:.0f}", f"{tf['loop']:.0f}",
                f"{relerr['hip']:.1e}", f"{relerr['bmm']:.1e}"]
        print("| " + " | ".join(cols) + " |" if args.markdown
              else "  ".join(cols))


if __name__ == "__main__":
    main()
