"""Gated (SwiGLU) expert bank: fused GLU kernels vs the composed route vs
per-expert hipBLASLt GEMMs, and the Experts layer in every PG_MOE_GROUPED
mode that runs gated experts.

Usage (GPU box): python tools/moe_glu_bench.py [--markdown] [--quick]
                                               [--skip-layer]

Kernels alone, T=16384 rows, K=2048, I=8192, E=8, balanced and skewed
counts (those of tools/grouped_gemm_bench.py):

  forward  fused     grouped_glu_fwd (one launch: g, u, h from one X read)
           composed  two grouped_gemm_fwd + silu_mul_fwd
           loop      E x 2 hipBLASLt GEMMs on the segment slices + silu_mul
  dgrad    fused     grouped_glu_dgrad (one launch, one accumulator)
           composed  two grouped_gemm_dgrad + a bf16 add

Layer: Experts with 8 GatedExpertMLP(2048, 8192), N=16384 tokens, top-1 and
top-2, forward + backward: the default loop, PG_MOE_GROUPED=2 (grouped_glu
on its default route), and =3 with grouped_glu fused and composed.

Contenders are alternated inside each round; the tables report the median
over rounds with the min..max spread of device-event times of `iters`
back-to-back calls.  TF/s counts the useful 2*T*2I*K flops only.  "extra
MB" is what the composed route moves through HBM that the fused one does
not, from the shapes: forward a second read of X and the silu_mul pass's
reads of g and u; dgrad two partial dX written and read back.
The summary is committed under profiles/moe_grouped_gemm.md §5.
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


def race(impls, rounds, iters):
    """{name: [ms per round]} with the contenders alternated in a round."""
    for f in impls.values():            # warm every shape
        time_ms(f, 2)
    samples = {k: [] for k in impls}
    for _ in range(rounds):
        for k, f in impls.items():
            samples[k].append(time_ms(f, iters))
    return samples


def cell(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}..{max(v):.3f})"


def verdict(samples, fused="fused"):
    """The project's match-or-fallback rule: the fused kernel wins only if
    its slowest run beats the fastest run of every other contender."""
    others = min(min(v) for k, v in samples.items() if k != fused)
    return "fused" if max(samples[fused]) < others else "composed"


def kernel_tables(ext, rounds, iters, markdown):
    rows = []
    for cname, counts in COUNTS.items():
        gen = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda *s: (torch.rand(*s, device="cuda", generator=gen)  # noqa: E731
                          * 2 - 1).bfloat16()
        x, dg, du = rnd(T, H), rnd(T, I), rnd(T, I)
        wg = [rnd(I, H) for _ in range(E)]
        wu = [rnd(I, H) for _ in range(E)]
        off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)),
                           dtype=torch.int32, device="cuda")
        bounds, s = [], 0
        for c in counts:
            bounds.append((s, s + c))
            s += c
        g_buf = torch.empty(T, I, device="cuda", dtype=torch.bfloat16)
        u_buf = torch.empty(T, I, device="cuda", dtype=torch.bfloat16)

        def composed_fwd():
            g = ext.grouped_gemm_fwd(x, wg, off, None)
            u = ext.grouped_gemm_fwd(x, wu, off, None)
            return ext.silu_mul_fwd(g, u)

        def loop_fwd():
            for e, (a, b) in enumerate(bounds):
                torch.mm(x[a:b], wg[e].t(), out=g_buf[a:b])
                torch.mm(x[a:b], wu[e].t(), out=u_buf[a:b])
            return ext.silu_mul_fwd(g_buf, u_buf)

        def composed_dgrad():
            return ext.grouped_gemm_dgrad(dg, wg, off) \
                + ext.grouped_gemm_dgrad(du, wu, off)

        fwd = {"fused": lambda: ext.grouped_glu_fwd(x, wg, wu, off, True)[0],
               "composed": composed_fwd, "loop": loop_fwd}
        dgrad = {"fused": lambda: ext.grouped_glu_dgrad(dg, du, wg, wu, off),
                 "composed": composed_dgrad}
        flops = 2.0 * T * 2 * I * H
        extra = {"fwd": (T * H + 2 * T * I) * 2 / 1e6,
                 "dgrad": 4 * T * H * 2 / 1e6}
        for pname, impls in (("fwd", fwd), ("dgrad", dgrad)):
            ref = impls["composed"]().float()
            scale = max(ref.abs().max().item(), 1.0)
            relerr = (impls["fused"]().float() - ref).abs().max().item() \
                / scale
            del ref
            rows.append((cname, pname, flops, race(impls, rounds, iters),
                         relerr, extra[pname]))
        del x, dg, du, wg, wu, g_buf, u_buf
        torch.cuda.empty_cache()

    if markdown:
        print("| counts | pass | fused ms | composed ms | loop ms | fused TF/s "
              "| composed TF/s | extra MB | fused vs composed relerr "
              "| default |")
        print("|---" * 10 + "|")
    for cname, pname, flops, s, relerr, extra in rows:
        tf = {k: flops / (statistics.median(v) * 1e-3) / 1e12
              for k, v in s.items()}
        cols = [cname, pname, cell(s["fused"]), cell(s["composed"]),
                cell(s["loop"]) if "loop" in s else "-",
                f"{tf['fused']:.0f}", f"{tf['composed']:.0f}",
                f"{extra:.0f}", f"{relerr:.1e}", verdict(s)]
        print("| " + " | ".join(cols) + " |" if markdown
              else "  ".join(cols))


def layer_table(rounds, iters, markdown):
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29896")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    from pipegoose_amd import ParallelContext
    from pipegoose_amd.nn.expert_parallel import GatedExpertMLP
    from pipegoose_amd.nn.expert_parallel.experts import Experts
    import pipegoose_amd.ops.grouped_gemm as gg

    ctx = ParallelContext.from_torch()
    rows = []
    try:
        torch.manual_seed(0)
        mod = Experts(E, GatedExpertMLP(H, I), enable_tensor_parallel=False,
                      parallel_context=ctx).to("cuda", torch.bfloat16)
        defaults = (gg.FUSED_FWD_DEFAULT, gg.FUSED_DGRAD_DEFAULT)
        for topk in (1, 2):
            x = torch.randn(T, H, device="cuda", dtype=torch.bfloat16,
                            requires_grad=True)
            route = torch.rand(T, E, device="cuda").topk(topk, dim=1).indices
            weight = torch.zeros(T, E, device="cuda").scatter_(
                1, route, torch.rand(T, topk, device="cuda") + 0.1
            ).bfloat16().requires_grad_(True)
            g = torch.randn(T, H, device="cuda", dtype=torch.bfloat16)
            assert mod._fused_applies(x, weight)

            def step(mode, fused):
                def run():
                    if mode is None:
                        os.environ.pop("PG_MOE_GROUPED", None)
                    else:
                        os.environ["PG_MOE_GROUPED"] = mode
                    if fused is not None:
                        gg.FUSED_FWD_DEFAULT = gg.FUSED_DGRAD_DEFAULT = fused
                    try:
                        mod(x, route, weight).backward(g)
                    finally:
                        os.environ.pop("PG_MOE_GROUPED", None)
                        gg.FUSED_FWD_DEFAULT, gg.FUSED_DGRAD_DEFAULT = \
                            defaults
                return run

            impls = {"loop": step(None, None), "=2": step("2", None),
                     "=3 fused": step("3", True),
                     "=3 composed": step("3", False)}
            rows.append((topk, race(impls, rounds, iters)))
    finally:
        ctx.destroy()

    names = ["loop", "=2", "=3 fused", "=3 composed"]
    if markdown:
        print("| top-k | " + " | ".join(f"{n} ms" for n in names)
              + " | =3 fused beats loop beyond the spread |")
        print("|---" * (len(names) + 2) + "|")
    for topk, s in rows:
        clear = max(s["=3 fused"]) < min(s["loop"])
        cols = [str(topk)] + [cell(s[n]) for n in names] \
            + ["yes" if clear else "no"]
        print("| " + " | ".join(cols) + " |" if markdown
              else "  ".join(cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--quick", action="store_true",
                    help="fewer rounds (smoke-testing the tool)")
    ap.add_argument("--skip-layer", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ext = get_extension(required=True)
    rounds, iters = (2, 3) if args.quick else (7, 10)
    kernel_tables(ext, rounds, iters, args.markdown)
    if not args.skip_layer:
        print()
        layer_table(rounds, iters, args.markdown)


if __name__ == "__main__":
    main()
