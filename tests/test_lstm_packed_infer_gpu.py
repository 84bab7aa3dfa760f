"""Packed BiLSTM inference through lstm_rec_packed.hip against the CPU packed
reference in float64 on the same bf16-rounded values.

Tolerance: atol = rtol = 3e-2, the project's bf16 tolerance
(test_lstm_packed_gpu.py).  |h| < 1 and the state is rounded to bf16 at most
9 times, so the rounding the reference does not do stays an order of
magnitude inside it.

The first lengths set gives n_t = 147, 130, 130, 130, 70, 70, 65, 3, 3, so the
reverse direction meets (k, n) = (0, 3) zero state, (3, 3), (3, 65) k inside
block 0 and a one-row block wholly past k, (65, 70) k straddling the 64-row
block boundary, (70, 130), (130, 147) k in the last partial block; the
forward direction meets ragged n with k == n.
"""
import copy
import functools

import pytest
import torch

from nerrf_amd.models.lstm import BiLSTMDetector, LSTMConfig
from nerrf_amd.ops.lstm_seq import build_infer_plan, lstm_bilayer2_packed_infer

pytestmark = pytest.mark.gpu

T, E, H = 12, 16, 256
TOL = 3e-2
LENGTHS = {
    "ragged": [9] * 3 + [7] * 62 + [6] * 5 + [4] * 60 + [1] * 17 + [0] * 3,
    "one-full-block": [5] * 64,
    "single": [1],
}
BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(name):
    """(lengths, bf16 model, bf16 feats, per-layer float64 inputs and
    reference outputs), computed once per lengths set and only read."""
    g = torch.Generator().manual_seed(11)
    ln = torch.tensor(LENGTHS[name])
    ln = ln[torch.randperm(ln.numel(), generator=g)]
    b = ln.numel()
    with torch.random.fork_rng():
        torch.manual_seed(5)
        model = BiLSTMDetector(LSTMConfig(in_dim=E, hidden=H, layers=2)).to(BF)
    feats = torch.rand(b, T, E, generator=g)
    feats[..., :10] = torch.nn.functional.one_hot(
        torch.randint(0, 10, (b, T), generator=g), 10).float()
    feats = feats.to(BF)
    plan = build_infer_plan(ln, T)
    if name == "ragged":
        assert plan.batch_sizes == [147, 130, 130, 130, 70, 70, 65, 3, 3]
    m64 = copy.deepcopy(model).double()
    (f1, r1), (f2, r2) = m64.dirs[0], m64.dirs[1]
    with torch.no_grad():
        ref1 = lstm_bilayer2_packed_infer(
            plan, f1.w_hh, f1.b, r1.w_hh, r1.b,
            feats=feats.double(), w_ih_f=f1.w_ih, w_ih_b=r1.w_ih)
        # layer 2 alone: its input is the reference projection rounded to bf16
        xg2p = (ref1.to(BF).double() @ torch.cat([f2.w_ih, r2.w_ih]).t()).to(BF)
        ref2 = lstm_bilayer2_packed_infer(
            plan, f2.w_hh, f2.b, r2.w_hh, r2.b, xg2p=xg2p.double())
    return ln, model, feats, xg2p, (ref1, ref2)


def _layer_args(name, layer, dev):
    _, model, feats, xg2p, _ = _case(name)
    f, r = copy.deepcopy(model.dirs[layer]).to(dev)
    w = (f.w_hh.detach(), f.b.detach(), r.w_hh.detach(), r.b.detach())
    if layer == 0:
        return w, dict(feats=feats.to(dev), w_ih_f=f.w_ih.detach(),
                       w_ih_b=r.w_ih.detach())
    return w, dict(xg2p=xg2p.to(dev))


@pytest.mark.parametrize("layer", [0, 1], ids=["xproj", "xg"])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_op_matches_fp64_reference(gpu_device, name, layer):
    ln = _case(name)[0]
    ref = _case(name)[4][layer]
    plan = build_infer_plan(ln, T, gpu_device)
    w, kw = _layer_args(name, layer, gpu_device)
    with torch.no_grad():
        got = lstm_bilayer2_packed_infer(plan, *w, **kw)
    assert got.shape == ref.shape and got.dtype == BF
    got = got.double().cpu()
    print(f"{name} layer {layer + 1}: max abs err {(got - ref).abs().max().item():.3e}")
    assert torch.allclose(got, ref, atol=TOL, rtol=TOL)


@pytest.mark.parametrize("layer", [0, 1], ids=["xproj", "xg"])
def test_rows_and_k_alone_decide_what_is_read(gpu_device, layer):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    dev = gpu_device
    plan = build_infer_plan(_case("ragged")[0], T, dev)
    w, kw = _layer_args("ragged", layer, dev)
    none = torch.empty(0, device=dev, dtype=BF)

    def run(fill):
        h2p = torch.full((plan.n_rows, 2 * H), fill, device=dev, dtype=BF)
        c = torch.full((plan.batch_sizes[0], H), fill, device=dev, dtype=BF)
        for rev in (False, True):
            ext.lstm_packed_infer_dir(
                h2p[:, rev * H:(rev + 1) * H], w[2 * rev], w[2 * rev + 1], c,
                kw["xg2p"][:, rev * 4 * H:(rev + 1) * 4 * H] if layer else none,
                none if layer else kw["feats"],
                none if layer else plan.perm_dev,
                none if layer else kw["w_ih_b" if rev else "w_ih_f"],
                plan.batch_sizes, plan.offsets, rev)
        return h2p

    poisoned, clean = run(float("nan")), run(0.0)
    assert bool(torch.isfinite(poisoned).all())
    assert torch.equal(poisoned, clean)


def test_model_matches_fp64_dense_and_flag_off_is_dense(gpu_device, monkeypatch):
    ln, model, feats, _, _ = _case("ragged")
    with torch.no_grad():
        want = copy.deepcopy(model).double()._forward_dense(feats.double(), ln)
        gpu = copy.deepcopy(model).to(gpu_device)
        f_dev, ln_dev = feats.to(gpu_device), ln.to(gpu_device)
        got = gpu(f_dev, ln_dev)
        with_plan = gpu(f_dev, ln_dev, build_infer_plan(ln, T, gpu_device))
        monkeypatch.setenv("NERRF_LSTM_PACKED_INFER", "0")
        off = gpu(f_dev, ln_dev)
        dense = gpu._forward_dense(f_dev, ln_dev)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"model logits: max abs err {err:.3e}; "
          f"dense path {(dense.double().cpu() - want).abs().max().item():.3e}")
    assert torch.allclose(got.double().cpu(), want, atol=TOL, rtol=TOL)
    assert torch.equal(with_plan, got)
    # a 0-length sequence sees zero final states: the head's bias alone
    assert int((ln == 0).sum()) == 3
    assert bool((got[ln_dev == 0] == gpu.head.bias).all())
    assert torch.equal(off, dense)
