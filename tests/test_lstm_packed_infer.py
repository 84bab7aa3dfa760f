"""Packed BiLSTM inference on the CPU: the O(B + T) plan against the full
plan, and the inference op against the packed training op's forward."""
import numpy as np
import pytest
import torch

from nerrf_amd.ops.lstm_seq import (
    build_infer_plan,
    build_seq_plan,
    lstm_bilayer2_packed,
    lstm_bilayer2_packed_infer,
)

LENGTHS = [
    pytest.param([3, 0, 7, 7, 1, 9, 4, 0, 12, 4], id="mixed-with-empty"),
    pytest.param([5] * 4, id="uniform"),
    pytest.param([1], id="single"),
    pytest.param([0, 0], id="all-empty"),
]


@pytest.mark.parametrize("lengths", LENGTHS)
def test_infer_plan_agrees_with_full_plan(lengths):
    t_max = 9  # clamps the 12
    full = build_seq_plan(np.array(lengths), t_max)
    plan = build_infer_plan(torch.tensor(lengths), t_max)
    assert np.array_equal(plan.perm, full.perm)
    assert np.array_equal(plan.inv_perm, full.inv_perm)
    assert plan.batch_sizes == full.batch_sizes and plan.offsets == full.offsets
    assert (plan.n_seq, plan.t_max, plan.has_empty) == (full.n_seq, full.t_max, full.has_empty)
    assert torch.equal(plan.fin_idx, full.fin_idx) and torch.equal(plan.live, full.live)
    assert plan.perm_dev.dtype == torch.int32
    assert np.array_equal(plan.perm_dev.numpy(), full.perm)
    assert plan.pack_idx.numel() == 0 and plan.hin_idx.numel() == 0


def _layer(seed, e, hd):
    g = torch.Generator().manual_seed(seed)
    gd = 4 * hd
    w = [torch.randn(gd, hd, generator=g) * 0.2, torch.randn(gd, generator=g) * 0.5,
         torch.randn(gd, hd, generator=g) * 0.2, torch.randn(gd, generator=g) * 0.5]
    w_ih = [torch.randn(gd, e, generator=g) * 0.3, torch.randn(gd, e, generator=g) * 0.3]
    return g, w, w_ih


@pytest.mark.parametrize("lengths", LENGTHS)
def test_infer_op_equals_packed_op_forward(lengths):
    t_max, e, hd = 9, 5, 8
    b = len(lengths)
    full = build_seq_plan(np.array(lengths), t_max)
    plan = build_infer_plan(np.array(lengths), t_max)
    g, w, w_ih = _layer(3, e, hd)
    feats = torch.randn(b, t_max, e, generator=g)
    xg2p = feats.reshape(b * t_max, e)[full.pack_idx] @ torch.cat(w_ih).t()
    with torch.no_grad():
        want = lstm_bilayer2_packed(xg2p, full, *w)
    assert torch.equal(lstm_bilayer2_packed_infer(plan, *w, xg2p=xg2p), want)
    got = lstm_bilayer2_packed_infer(full, *w, feats=feats, w_ih_f=w_ih[0], w_ih_b=w_ih[1])
    assert torch.equal(got, want)


def test_infer_op_refuses_gradients():
    plan = build_infer_plan(np.array([2, 1]), 2)
    _, w, _ = _layer(4, 5, 8)
    xg2p = torch.randn(3, 64)
    w[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        lstm_bilayer2_packed_infer(plan, *w, xg2p=xg2p)
    with torch.no_grad():  # grad mode off: the same inputs are fine
        assert lstm_bilayer2_packed_infer(plan, *w, xg2p=xg2p).shape == (3, 16)
    with pytest.raises(ValueError):
        lstm_bilayer2_packed_infer(plan, *w)
