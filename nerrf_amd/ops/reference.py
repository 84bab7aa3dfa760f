"""Pure-PyTorch reference implementations of the fused ops.

These are the numerics ground truth: every HIP kernel is validated against
these in fp32 (tests/test_ops_gpu.py) and they are the CPU execution path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def gather_mean_ref(
    h: torch.Tensor,  # [N, D]
    idx: torch.Tensor,  # [N, K] int64
    w: torch.Tensor,  # [N, K] float
) -> torch.Tensor:
    """Weighted mean of gathered neighbor rows."""
    n, k = idx.shape
    gathered = h[idx.reshape(-1)].reshape(n, k, h.shape[1])  # [N, K, D]
    wf = w.to(h.dtype).unsqueeze(-1)
    denom = w.sum(dim=1, keepdim=True).to(h.dtype).clamp_min(1e-6)
    return (gathered * wf).sum(dim=1) / denom


def edge_head_ref(
    h: torch.Tensor,  # [N, D]
    edge_index: torch.Tensor,  # [2, E] int64
    edge_weight: torch.Tensor,  # [E]
    edge_ts: torch.Tensor,  # [E]
    head,  # nn.Sequential(Linear(2D+2, H), GELU, Linear(H, 1))
) -> torch.Tensor:
    """Edge logits [E] in h's dtype: the edge branch of GraphSAGET.forward."""
    hs, hd = h[edge_index[0]], h[edge_index[1]]
    feat = torch.cat(
        [
            hs * hd,
            (hs - hd).abs(),
            edge_weight.unsqueeze(-1).to(h.dtype),
            edge_ts.unsqueeze(-1).to(h.dtype),
        ],
        dim=-1,
    )
    return head(feat).squeeze(-1)


def edge_attribution_ref(
    logit: torch.Tensor,  # [E]
    edge_index: torch.Tensor,  # [2, E] int64
    n_files: int,
    n_nodes: int,
    direction: str = "write",
    thr_logit: float = 0.0,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per file node, the best edge of one direction: (culprit [F] int64,
    best_logit [F] fp32, n_hot [F] int32).

    Nodes [0, n_files) are files, [n_files, n_nodes) processes.  A "write"
    edge runs process -> file, a "read" edge file -> process.  culprit is the
    process node index of the highest-logit edge (ties: lowest index), -1 and
    -inf where a file has no such edge; n_hot counts the file's edges with
    logit >= thr_logit (compared in fp32).  Edges with an endpoint outside
    [0, n_nodes), between two files or two processes, of the other direction
    or with a NaN logit are skipped; -0.0 counts as +0.0.
    """
    if direction not in ("write", "read"):
        raise ValueError(f"direction must be 'write' or 'read', got {direction!r}")
    n_files, n_nodes = int(n_files), int(n_nodes)
    dev = logit.device
    v = logit.detach().float().reshape(-1) + 0.0  # -0.0 -> +0.0
    src, dst = edge_index[0].reshape(-1), edge_index[1].reshape(-1)
    ok = (src >= 0) & (src < n_nodes) & (dst >= 0) & (dst < n_nodes)
    s_file, d_file = src < n_files, dst < n_files
    if direction == "write":
        ok = ok & ~s_file & d_file
        f, p = dst, src
    else:
        ok = ok & s_file & ~d_file
        f, p = src, dst
    ok = ok & ~torch.isnan(v)
    f, p, v = f[ok], p[ok], v[ok]
    best = torch.full((n_files,), float("-inf"), device=dev, dtype=torch.float32)
    best = best.scatter_reduce(0, f, v, "amax", include_self=True)
    # lowest process index among the edges that equal their file's maximum
    win = v == best[f]
    none = torch.iinfo(torch.int64).max
    culprit = torch.full((n_files,), none, device=dev, dtype=torch.int64)
    culprit = culprit.scatter_reduce(0, f[win], p[win], "amin", include_self=True)
    culprit = torch.where(culprit == none, torch.full_like(culprit, -1), culprit)
    hot = v >= torch.tensor(thr_logit, dtype=torch.float32, device=dev)
    n_hot = torch.zeros(n_files, device=dev, dtype=torch.int32)
    n_hot.index_add_(0, f[hot], torch.ones_like(f[hot], dtype=torch.int32))
    return culprit, best, n_hot


def lstm_pointwise_fwd_ref(
    gates_pre: torch.Tensor,  # [B, 4H] pre-activation (x_t W_ih + h W_hh + b)
    c: torch.Tensor,  # [B, H]
    h_prev: torch.Tensor,  # [B, H] (returned unchanged where mask == 0)
    mask: Optional[torch.Tensor],  # [B] or None
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (h_new, c_new, gates_act[B,4H] saved for backward)."""
    hdim = c.shape[1]
    i = torch.sigmoid(gates_pre[:, :hdim])
    f = torch.sigmoid(gates_pre[:, hdim : 2 * hdim])
    g = torch.tanh(gates_pre[:, 2 * hdim : 3 * hdim])
    o = torch.sigmoid(gates_pre[:, 3 * hdim :])
    c_new = f * c + i * g
    h_new = o * torch.tanh(c_new)
    if mask is not None:
        m = mask.to(c.dtype).unsqueeze(-1)
        c_new = m * c_new + (1 - m) * c
        h_new = m * h_new + (1 - m) * h_prev
    gates_act = torch.cat([i, f, g, o], dim=1)
    return h_new, c_new, gates_act


def lstm_pointwise_bwd_ref(
    grad_h: torch.Tensor,  # [B, H]
    grad_c: torch.Tensor,  # [B, H]
    gates_act: torch.Tensor,  # [B, 4H]
    c: torch.Tensor,  # [B, H] previous cell
    mask: Optional[torch.Tensor],
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (grad_gates_pre [B,4H], grad_c_prev [B,H], grad_h_prev_passthrough [B,H]).

    The unmasked c_new is recomputed from (f, i, g, c); where mask == 0 the
    upstream grads are routed straight through to (h_prev, c_prev).
    """
    hdim = c.shape[1]
    i = gates_act[:, :hdim]
    f = gates_act[:, hdim : 2 * hdim]
    g = gates_act[:, 2 * hdim : 3 * hdim]
    o = gates_act[:, 3 * hdim :]
    if mask is not None:
        m = mask.to(c.dtype).unsqueeze(-1)
    else:
        m = torch.ones_like(c[:, :1])
    tanh_c_new = torch.tanh(f * c + i * g)
    # grads on the *active* branch
    gh = grad_h * m
    gc = grad_c * m
    do = gh * tanh_c_new
    dc = gc + gh * o * (1 - tanh_c_new * tanh_c_new)
    di = dc * g
    df = dc * c
    dg = dc * i
    dc_prev = dc * f + grad_c * (1 - m)
    d_ip = di * i * (1 - i)
    d_fp = df * f * (1 - f)
    d_gp = dg * (1 - g * g)
    d_op = do * o * (1 - o)
    grad_gates = torch.cat([d_ip, d_fp, d_gp, d_op], dim=1)
    grad_h_pass = grad_h * (1 - m)  # flows straight to h_prev where masked
    return grad_gates, dc_prev, grad_h_pass


def gather_mean_bwd_ref(
    grad_out: torch.Tensor,  # [N, D]
    idx: torch.Tensor,  # [N, K]
    w: torch.Tensor,  # [N, K]
    num_nodes: int,
) -> torch.Tensor:
    """grad wrt h: scatter-add of normalised weights x grad_out rows."""
    n, k = idx.shape
    denom = w.sum(dim=1, keepdim=True).clamp_min(1e-6)
    wn = (w / denom).to(grad_out.dtype)  # [N, K]
    grad_h = torch.zeros(num_nodes, grad_out.shape[1], device=grad_out.device, dtype=grad_out.dtype)
    contrib = wn.unsqueeze(-1) * grad_out.unsqueeze(1)  # [N, K, D]
    grad_h.index_add_(0, idx.reshape(-1), contrib.reshape(n * k, -1))
    return grad_h
