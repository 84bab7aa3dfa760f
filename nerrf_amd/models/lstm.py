"""BiLSTM sequence model (2 layers x 256 hidden, bidirectional).

Spec (reference docs architecture.mdx:55-59): bidirectional, 256 hidden,
2 layers, input = last 100 events per file, F1 >= 0.95 target.

MI355X-first structure: the input projection for ALL timesteps is one large
GEMM (hipBLASLt via torch.matmul — a plain library GEMM), and the
recurrence of a whole layer, both directions, goes through
`nerrf_amd.ops.lstm_seq.lstm_bilayer2`, the sequence op backed by the
hand-written CDNA4 HIP step kernels on GPU.

Variable lengths.  Training (gradients needed) packs the batch to its live
rows: sequences are sorted by length once per batch (`SeqPlan`, built on the
host with the batch or from `lengths`), every LSTM tensor holds only the
sum(lengths) live (timestep, sequence) rows, and the recurrence runs
max(lengths) steps through `lstm_bilayer2_packed`.  NERRF_LSTM_PACKED=0
(docs/flags.md) selects the dense path there too.  Inference keeps the whole
batch dense with masked state updates (`lstm_bilayer2`, the rec-fused step
kernel).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from ..ops import lstm_sequence
from ..ops.lstm_seq import (
    SeqPlan,
    build_seq_plan,
    lstm_bilayer2,
    lstm_bilayer2_packed,
)


@dataclass
class LSTMConfig:
    in_dim: int = 16
    hidden: int = 256
    layers: int = 2
    seq_len: int = 100


class FusedLSTMDirection(nn.Module):
    """One direction of one LSTM layer with masked updates."""

    def __init__(self, in_dim: int, hidden: int, reverse: bool) -> None:
        super().__init__()
        self.hidden = hidden
        self.reverse = reverse
        self.w_ih = nn.Parameter(torch.empty(4 * hidden, in_dim))
        self.w_hh = nn.Parameter(torch.empty(4 * hidden, hidden))
        self.b = nn.Parameter(torch.zeros(4 * hidden))
        nn.init.xavier_uniform_(self.w_ih)
        nn.init.orthogonal_(self.w_hh[:hidden])
        nn.init.orthogonal_(self.w_hh[hidden : 2 * hidden])
        nn.init.orthogonal_(self.w_hh[2 * hidden : 3 * hidden])
        nn.init.orthogonal_(self.w_hh[3 * hidden :])
        with torch.no_grad():  # forget-gate bias 1.0
            self.b[self.hidden : 2 * self.hidden] = 1.0

    def forward(self, x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """x: [T, B, E] time-major; mask: [T, B]. Returns [T, B, H] time-major."""
        t, b, _ = x.shape
        # one big GEMM for all timesteps' input projection (time-major slices
        # stay contiguous for the per-step fused kernel)
        xg = torch.matmul(x.reshape(t * b, -1), self.w_ih.t()).reshape(t, b, 4 * self.hidden)
        h0 = x.new_zeros(b, self.hidden)
        c0 = x.new_zeros(b, self.hidden)
        return lstm_sequence(xg, h0, c0, self.w_hh, self.b, mask, reverse=self.reverse)


class BiLSTMDetector(nn.Module):
    def __init__(self, cfg: LSTMConfig | None = None) -> None:
        super().__init__()
        self.cfg = cfg or LSTMConfig()
        c = self.cfg
        dirs = []
        in_dim = c.in_dim
        for _ in range(c.layers):
            dirs.append(
                nn.ModuleList(
                    [
                        FusedLSTMDirection(in_dim, c.hidden, reverse=False),
                        FusedLSTMDirection(in_dim, c.hidden, reverse=True),
                    ]
                )
            )
            in_dim = 2 * c.hidden
        self.dirs = nn.ModuleList(dirs)
        self.head = nn.Linear(2 * c.hidden, 1)

    def forward(
        self,
        feats: torch.Tensor,
        lengths: torch.Tensor,
        plan: Optional[SeqPlan] = None,
    ) -> torch.Tensor:
        """feats: [B, T, E]; lengths: [B] -> per-sequence logit [B].

        `plan` (optional): the `SeqPlan` of `lengths`, e.g. the one
        `WindowBatch.to_torch` builds on the host; without it the packed
        path builds one from `lengths` with one device-to-host copy."""
        packed = (
            os.environ.get("NERRF_LSTM_PACKED", "1") == "1"
            and torch.is_grad_enabled()
            and any(p.requires_grad for p in self.parameters())
        )
        if packed:
            return self._forward_packed(feats, lengths, plan)
        return self._forward_dense(feats, lengths)

    def _forward_packed(self, feats, lengths, plan) -> torch.Tensor:
        """Training path: only the sum(lengths) live (timestep, sequence)
        rows exist; sequences are sorted by length and every layer runs on
        packed time-major tensors (ops/lstm_seq.py, `SeqPlan`)."""
        b, t, e = feats.shape
        hid = self.cfg.hidden
        if plan is None:
            plan = build_seq_plan(lengths, t, feats.device)
        assert plan.n_seq == b and plan.t_max == t, "plan does not match feats"
        n = plan.n_rows
        if n == 0:  # every sequence is empty: zero final states
            return self.head(feats.new_zeros(b, 2 * hid)).squeeze(-1)
        h = feats.reshape(b * t, e).index_select(0, plan.pack_idx)  # [N, E]
        for layer in self.dirs:
            f, r = layer[0], layer[1]
            w_cat = torch.cat([f.w_ih, r.w_ih], dim=0)  # [2*4H, K]
            xg2p = torch.matmul(h, w_cat.t())  # [N, 2*4H], one GEMM
            h = lstm_bilayer2_packed(xg2p, plan, f.w_hh, f.b, r.w_hh, r.b)
        # forward state of sorted row r at t = len-1, backward state at t = 0,
        # gathered in the original sequence order.  The indices are unique
        # (but for length-0 sequences, zeroed below), so the backward is an
        # index_add_ and not the sort-based indexing backward.
        fin = h.reshape(2 * n, hid).index_select(0, plan.fin_idx).view(b, 2 * hid)
        if plan.has_empty:
            fin = fin * plan.live.to(fin.dtype)
        return self.head(fin).squeeze(-1)

    def _forward_dense(self, feats: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """Dense masked path over all B x T positions: inference (the
        rec-fused step kernel) and NERRF_LSTM_PACKED=0."""
        b, t, _ = feats.shape
        ar = torch.arange(t, device=feats.device)
        mask = (ar.unsqueeze(1) < lengths.unsqueeze(0)).to(feats.dtype)  # [T, B]
        h = feats.transpose(0, 1).contiguous()  # time-major [T, B, E]
        for layer in self.dirs:
            f, r = layer[0], layer[1]
            # both directions in ONE projection GEMM ([M,K] x [K, 2*4H]:
            # the A panel is read once instead of twice) and one [T,B,2H]
            # output buffer; the layer backward then sees a single
            # contiguous grad tensor, so dgrad and wgrad are single GEMMs
            flat = h.reshape(t * b, -1)
            w_cat = torch.cat([f.w_ih, r.w_ih], dim=0)  # [2*4H, K]
            xg2 = torch.matmul(flat, w_cat.t()).reshape(t, b, 8 * f.hidden)
            h0 = h.new_zeros(b, f.hidden)
            c0 = h.new_zeros(b, f.hidden)
            h = lstm_bilayer2(xg2, h0, c0, f.w_hh, f.b, r.w_hh, r.b, mask)
        # forward state at t=len-1, backward state at t=0
        idx = (lengths.clamp(min=1) - 1).view(1, b, 1).expand(1, b, self.cfg.hidden)
        h_fwd = h[:, :, : self.cfg.hidden].gather(0, idx).squeeze(0)  # [B, H]
        h_bwd = h[0, :, self.cfg.hidden :]
        return self.head(torch.cat([h_fwd, h_bwd], dim=-1)).squeeze(-1)

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters())
