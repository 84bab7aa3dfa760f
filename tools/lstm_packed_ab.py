"""A/B: dense masked BiLSTM layer (`lstm_bilayer2`) against the packed one
(`lstm_bilayer2_packed`), forward + backward of ONE layer at the benchmark's
shape: B = 64 140 sequences, T = 100, H = 256, bf16.

Case (a): the benchmark batch's length histogram, rebuilt from its recorded
          figures (survival counts at t = 0, 10, ..., 70 and percentiles; see
          profiles/PROFILES.md, "Packed BiLSTM") — 37 % of the rows are live.
Case (b): every length = T — the packed path has nothing to skip and must
          not be slower than the dense one beyond the dense path's own
          run-to-run spread.

Dense and packed runs alternate; each figure is a host clock around work
that ends in a device synchronise.  Prints median and min-max per variant.

Run on a GPU box:  python tools/lstm_packed_ab.py [--rounds 7] [--batch 64140]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

from nerrf_amd.ops.lstm_seq import (  # noqa: E402
    build_seq_plan, lstm_bilayer2, lstm_bilayer2_packed,
)
from nerrf_amd.ops.native import load_extension  # noqa: E402
from nerrf_amd.perf import enable_tuned_gemms  # noqa: E402

T, H = 100, 256

# cumulative distribution of the bench batch's lengths: (length, P(len <= length))
# from the survival counts (alive at t means len > t) and the percentiles
_CDF = [
    (1, 0.0), (10, 82 / 64140), (20, 221 / 64140), (30, 8120 / 64140),
    (33, 0.25), (37, 0.50), (40, 44642 / 64140), (41, 0.75), (45, 0.90),
    (50, 62796 / 64140), (52, 0.99), (60, 64121 / 64140), (67, 1.0),
]


def bench_lengths(batch: int) -> np.ndarray:
    q = (np.arange(batch) + 0.5) / batch
    ls, fs = zip(*_CDF)
    ln = np.ceil(np.interp(q, fs, ls)).astype(np.int64)
    rng = np.random.default_rng(0)
    return rng.permutation(np.clip(ln, 2, 67))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64140)
    args = ap.parse_args()
    enable_tuned_gemms()
    load_extension(required=True)
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    b, gd = args.batch, 4 * H
    g = torch.Generator(device=dev).manual_seed(0)

    def rn(*shape, scale):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(dt)

    weights = [rn(gd, H, scale=0.05), rn(gd, scale=0.5), rn(gd, H, scale=0.05),
               rn(gd, scale=0.5)]
    for w in weights:
        w.requires_grad_(True)
    xg2 = rn(T, b, 2 * gd, scale=0.4).requires_grad_(True)
    g_out = rn(T, b, 2 * H, scale=1.0)
    h0 = torch.zeros(b, H, device=dev, dtype=dt)
    c0 = torch.zeros(b, H, device=dev, dtype=dt)

    for case, lengths in (("a: bench histogram", bench_lengths(b)),
                          ("b: all lengths = T", np.full(b, T, dtype=np.int64))):
        plan = build_seq_plan(lengths, T, dev)
        n = plan.n_rows
        ln_dev = torch.from_numpy(lengths).to(dev)
        mask = (torch.arange(T, device=dev)[:, None] < ln_dev[None, :]).float()
        xg2p = xg2.detach().reshape(T * b, 2 * gd)[:n].clone().requires_grad_(True)
        g_out_p = g_out.reshape(T * b, 2 * H)[:n].clone()
        print(f"case {case}: mean length {lengths.mean():.2f}, max {lengths.max()}, "
              f"live rows {n} of {T * b} = {n / (T * b):.3f}, T_live {plan.t_live}")

        def dense():
            lstm_bilayer2(xg2, h0, c0, *weights, mask).backward(g_out)

        def packed():
            lstm_bilayer2_packed(xg2p, plan, *weights).backward(g_out_p)

        def timed(fn):
            for x in (xg2, xg2p, *weights):
                x.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        timed(dense), timed(packed)  # warm-up: code objects, GEMM algorithms
        td, tp = [], []
        for _ in range(args.rounds):
            td.append(timed(dense))
            tp.append(timed(packed))
        for name, ts in (("dense ", td), ("packed", tp)):
            print(f"  {name} fwd+bwd: median {statistics.median(ts):8.2f} ms "
                  f"(min {min(ts):.2f} - max {max(ts):.2f}, {len(ts)} runs)")
        print(f"  packed / dense (medians): "
              f"{statistics.median(tp) / statistics.median(td):.3f}")
        del xg2p, g_out_p, mask, plan


if __name__ == "__main__":
    main()
