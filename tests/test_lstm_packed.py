"""Packed (length-sorted) BiLSTM training path against the dense masked
path, on the CPU reference implementations in f32.

atol=1e-5 is the tolerance of the existing variable-length and bilayer tests
(test_models.py::test_lstm_variable_lengths, test_lstm_bilayer2_matches_bilayer):
both paths evaluate the same f32 expressions, only the GEMM row counts and
the summation order of the weight gradients differ.
"""
import numpy as np
import pytest
import torch

from nerrf_amd.models.lstm import BiLSTMDetector, LSTMConfig
from nerrf_amd.ops.lstm_seq import SeqPlan, build_seq_plan

ATOL = 1e-5
LENGTHS = [12, 1, 7, 7, 3, 12, 2, 9, 5]  # ties, length 1, full length


def _model(seed=0):
    torch.manual_seed(seed)
    return BiLSTMDetector(LSTMConfig(in_dim=16, hidden=32, layers=2))


def _run(model, feats, lengths, monkeypatch, packed):
    monkeypatch.setenv("NERRF_LSTM_PACKED", "1" if packed else "0")
    model.zero_grad(set_to_none=True)
    logits = model(feats, lengths)
    g = torch.Generator().manual_seed(3)
    (logits * torch.randn(logits.shape, generator=g)).sum().backward()
    return logits.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize(
    "lengths,t",
    [
        pytest.param(LENGTHS, 12, id="ties-len1-full"),
        pytest.param([6, 1, 4, 4, 2, 6, 3, 5, 1], 12, id="maxlen6-below-T"),
        # equal lengths: the weight grads take the shifted-view path
        pytest.param([12] * 5, 12, id="uniform-full"),
        pytest.param([5] * 4, 12, id="uniform-5"),
        pytest.param([1] * 3, 12, id="uniform-1"),
    ],
)
def test_packed_model_matches_dense(monkeypatch, lengths, t):
    b = len(lengths)
    model = _model()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(b, t, 16, generator=g)
    ln = torch.tensor(lengths)
    want, want_g = _run(model, feats, ln, monkeypatch, packed=False)
    got, got_g = _run(model, feats, ln, monkeypatch, packed=True)
    assert got.shape == (b,)
    assert torch.allclose(got, want, atol=ATOL)
    assert set(got_g) == set(want_g)
    for k in want_g:
        err = (got_g[k] - want_g[k]).abs().max().item()
        assert torch.allclose(got_g[k], want_g[k], atol=ATOL), (k, err)
    # the comparison is not between two zero gradients (a recurrent weight
    # has a zero gradient only when no sequence has a second step)
    for k, v in want_g.items():
        assert bool(v.abs().max() > 0) or ("w_hh" in k and max(lengths) == 1), k


def test_packed_padding_invariance(monkeypatch):
    monkeypatch.setenv("NERRF_LSTM_PACKED", "1")
    model = _model()
    b, t = len(LENGTHS), 12
    feats = torch.randn(b, t, 16)
    ln = torch.tensor(LENGTHS)
    out = model(feats, ln)
    feats2 = feats.clone()
    for i, n in enumerate(LENGTHS):
        feats2[i, n:] = 123.0  # garbage in padding
    out2 = model(feats2, ln)
    assert out.requires_grad  # the packed path ran
    assert torch.allclose(out, out2, atol=ATOL)


def test_packed_batch_permutation(monkeypatch):
    monkeypatch.setenv("NERRF_LSTM_PACKED", "1")
    model = _model()
    b, t = len(LENGTHS), 12
    feats = torch.randn(b, t, 16)
    ln = torch.tensor(LENGTHS)
    p = torch.randperm(b, generator=torch.Generator().manual_seed(4))
    out = model(feats, ln)
    out_p = model(feats[p], ln[p])
    assert torch.allclose(out_p, out[p], atol=ATOL)


def test_packed_length_zero_gives_head_of_zero(monkeypatch):
    monkeypatch.setenv("NERRF_LSTM_PACKED", "1")
    model = _model()
    feats = torch.randn(4, 5, 16)
    ln = torch.tensor([3, 0, 5, 0])
    out = model(feats, ln)
    head0 = model.head(torch.zeros(1, 64)).squeeze()
    assert torch.allclose(out[1], head0, atol=ATOL)
    assert torch.allclose(out[3], head0, atol=ATOL)
    assert not torch.allclose(out[0], head0, atol=ATOL)
    out.sum().backward()  # and the backward runs with the empty rows
    # every sequence empty
    out0 = model(feats, torch.zeros(4, dtype=torch.long))
    assert torch.allclose(out0, head0.expand(4), atol=ATOL)


def _same_plan(a: SeqPlan, b: SeqPlan):
    assert (a.n_seq, a.t_max, a.has_empty) == (b.n_seq, b.t_max, b.has_empty)
    assert np.array_equal(a.perm, b.perm) and np.array_equal(a.inv_perm, b.inv_perm)
    assert a.batch_sizes == b.batch_sizes and a.offsets == b.offsets
    for name in ("pack_idx", "hin_idx", "fin_idx", "live"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_plan_layout_and_builders():
    from nerrf_amd.data.dataset import synth_window_batches

    # hand-checked layout: stable sort, prefix property, clamping to T
    plan = build_seq_plan(np.array([2, 9, 0, 2, 3]), 4)
    assert plan.perm.tolist() == [1, 4, 0, 3, 2]  # 9 -> 4; ties keep order
    assert plan.inv_perm.tolist() == [2, 0, 4, 3, 1]
    assert plan.batch_sizes == [4, 4, 2, 1]
    assert plan.offsets == [0, 4, 8, 10, 11]
    assert plan.n_rows == 11 and plan.t_live == 4 and plan.has_empty
    # packed row (t, r) is feats[perm[r], t]
    assert plan.pack_idx[:4].tolist() == [1 * 4, 4 * 4, 0, 3 * 4]
    assert plan.pack_idx[10].item() == 1 * 4 + 3
    assert plan.steps(False) == [(0, 4, 0, 0), (4, 4, 0, 4), (8, 2, 4, 2), (10, 1, 8, 1)]
    assert plan.steps(True) == [(10, 1, 11, 0), (8, 2, 10, 1), (4, 4, 8, 2), (0, 4, 4, 4)]

    # the plan to_torch builds from the numpy lengths == the one built from
    # the lengths tensor it also returns
    wb = synth_window_batches(n_scenarios=1, duration_s=31.0, benign_rate_hz=100.0)[0]
    tb = wb.to_torch()
    t = tb["seq_feats"].shape[1]
    _same_plan(tb["seq_plan"], build_seq_plan(tb["seq_lengths"], t))
    assert tb["seq_plan"].n_rows == int(np.clip(wb.seq_lengths, 0, t).sum())
