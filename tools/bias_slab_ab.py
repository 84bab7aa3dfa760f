"""Interleaved A/B of the backward pointwise kernel with and without the
bias-gradient slab, at production shapes (B=64140, H=256, bf16).

What the slab costs per launch is set against what it removes: the four
whole-history gg.sum(0) reductions per step, spread over 400 launches.

Usage: python tools/bias_slab_ab.py [B] [P ...]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerrf_amd.ops.native import load_extension

ext = load_extension(required=True)
dev = "cuda:0"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64140
PS = [int(a) for a in sys.argv[2:]] or [512, 1024, 2048, 4096, 8192]
H = 256
G = 4 * H
torch.manual_seed(0)


def rn(*shape):
    return (torch.randn(*shape, device=dev) * 0.2).to(torch.bfloat16)


gh, gout, gc, c = rn(B, H), rn(B, H), rn(B, H), rn(B, H)
gacts = torch.sigmoid(torch.randn(B, G, device=dev)).to(torch.bfloat16)
mask = (torch.rand(B, device=dev) > 0.1).float()
# grad_gates as the production layout: one 4H slab of a [B, 2*4H] buffer
gg = torch.empty(B, 2 * G, device=dev, dtype=torch.bfloat16)[:, :G]
gcp, ghp = torch.empty_like(c), torch.empty_like(c)
empty = torch.empty(0, device=dev)

variants = {"none": empty}
for p in PS:
    variants[f"P={p}"] = torch.zeros(p, G, device=dev, dtype=torch.float32)


def launch(accum):
    return ext.lstm_pointwise_bwd(gh, gout, gc, gacts, c, mask, gg, gcp, ghp, accum)


def timed(accum, n=50):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        launch(accum)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n * 1e3  # us per launch


for accum in variants.values():  # warm-up: code objects, clocks
    for _ in range(30):
        launch(accum)
torch.cuda.synchronize()

samples = {k: [] for k in variants}
for _ in range(15):  # interleaved rounds
    for k, accum in variants.items():
        samples[k].append(timed(accum))

base = statistics.median(samples["none"])
for k, s in samples.items():
    med = statistics.median(s)
    print(f"{k:>8}: median {med:7.2f} us  min {min(s):7.2f}  max {max(s):7.2f}"
          f"  delta vs none {med - base:+6.2f} us  (x400 = {(med - base) * 0.4:+.2f} ms/step)")

# the slab really holds the column sums of what was stored
slab = torch.zeros(PS[0], G, device=dev, dtype=torch.float32)
assert launch(slab)
ref = gg.double().sum(0)
err = (slab.double().sum(0) - ref).abs().max().item()
print(f"check: max |slab.sum(0) - gg.sum(0)| = {err:.3e}")
