"""Time-major fused LSTM sequence ops.

One autograd Function per (layer, direction) — or per bidirectional layer —
covering all T timesteps.  Each direction picks ONE step path up front
(`_dir_forward` / `_dir_backward`) and runs one timestep loop:

  forward
    reference : pure PyTorch (CPU tensors).
    rec-fused : one launch per step, GEMM + pointwise (lstm_rec_fused.hip).
                Default at inference; bf16, H=256, contiguous W_hh only.
    split     : per step 1 GEMM (h @ W_hh^T: rec_gemm.hip where its stride
                conditions hold, else hipBLASLt) and 1 fused HIP kernel (add
                xg + bias, 4-gate pointwise, masked state update) writing
                straight into time-major output buffers.  Default in training.
  backward
    reference : pure PyTorch (CPU tensors).
    rec-fused : gate grads + grad_h GEMM in one launch per step.
    split     : per step 1 fused gate-gradient kernel (which also folds the
                bias gradient into an f32 slab) + 1 in-place addmm.  Default.
  then, on every path, the weight gradients as two large batched GEMMs over
  all timesteps (grad_gates [T*B,4H]^T @ h_in [T*B,H]) and the bias gradient.

Flags (docs/flags.md), read once per forward / backward call:
  NERRF_REC_FUSED   infer (default) | 1 | 0 — where the rec-fused path runs
  NERRF_REC_GEMM    1 (default) | 0 — rec_gemm.hip vs hipBLASLt in the split fwd
  NERRF_FUSED_BIAS  1 (default) | 0 — in-kernel bias-grad slab in the split bwd
  NERRF_STREAM_DIRS 0 (default) | 1 — `lstm_bilayer2` inference on two streams

The bidirectional layer ops (`lstm_bilayer`, `lstm_bilayer2`) run both
directions into ONE [T, B, 2H] buffer using the kernels' row-stride
arguments: no `torch.cat` on the forward path (2.3 ms/window of strided
CatArrayBatchedCopy at serving shapes) and a contiguous incoming gradient on
the backward path (no narrow+contiguous copies of the per-direction grads).

This removes the per-step elementwise adds / stacks / reduces that dominated
the naive schedule (profiles/: 84% of busy time before the restructure).
Everything is time-major [T, B, ...]; the model transposes once per sequence.

`lstm_bilayer2_packed` is the training layer op.  It runs the split path
over a length-sorted packed layout (`SeqPlan`): every LSTM tensor holds only
the N = sum(lengths) live (timestep, sequence) rows, and both directions loop
over max(lengths) steps instead of T.  The dense masked ops above compute,
store and read back a row for every padded position (62.6 % of the rows of
the benchmark batch) and stay for inference and for A/B runs
(NERRF_LSTM_PACKED=0, read by the model).  The packed path has no mask: the
pointwise kernels take row counts instead (`prev_rows`, `in_rows`), so a
step may cover more rows than its predecessor produced without a zero-fill.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import reference as _ref
from .native import get_native


def _mfma_eligible(dt: torch.dtype, hdim: int, w_hh: torch.Tensor) -> bool:
    """Shape contract of the MFMA step kernels (lstm_rec_fused.hip,
    rec_gemm.hip)."""
    return dt == torch.bfloat16 and hdim == 256 and w_hh.is_contiguous()


def _rec_fused(infer: bool) -> bool:
    """Whether NERRF_REC_FUSED asks for the fused recurrent step:
    "infer" (default) = forward passes that save nothing for a backward,
    "1" = everywhere, anything else = nowhere."""
    mode = os.environ.get("NERRF_REC_FUSED", "infer")
    return mode == "1" or (mode == "infer" and infer)


def _dir_forward(ext, xg, h0, c0, w_hh, bias, mask, reverse, infer, h_all):
    """Run one direction's recurrence, writing hidden states into `h_all`
    ([T, B, H], rows uniformly strided — may be a column slab of a wider
    dual-direction buffer).  Returns (c_all, gates_all)."""
    t_len, batch, gdim = xg.shape
    hdim = gdim // 4
    dev, dt = xg.device, xg.dtype
    c_all = torch.empty(t_len, batch, hdim, device=dev, dtype=dt)
    gates_all = torch.empty(
        0 if infer else t_len, batch, gdim, device=dev, dtype=dt
    )

    # each step(ti, h, c) consumes the previous state and returns the new one
    if ext is None:
        def step(ti, h, c):
            gates_pre = torch.addmm(bias, h, w_hh.t()) + xg[ti]
            h_new, c_new, g_act = _ref.lstm_pointwise_fwd_ref(
                gates_pre, c, h, mask[ti] if mask is not None else None
            )
            h_all[ti] = h_new
            c_all[ti] = c_new
            if not infer:
                gates_all[ti] = g_act
            return h_new, c_new
    else:
        mfma = _mfma_eligible(dt, hdim, w_hh)
        g_none = torch.empty(0, device=dev, dtype=dt)
        empty_mask = torch.empty(0, device=dev)
        if mfma and _rec_fused(infer):
            # Fused recurrent step (lstm_rec_fused.hip): keeps the [B, 4H]
            # pre-activation slab out of HBM (one launch per timestep).
            # Measured: TRAINING at parity fwd / -13% bwd vs split (LDS
            # transpose stage caps occupancy — profiles/PROFILES.md ladder),
            # but INFERENCE 16% faster per serving window (no gate store:
            # 394 -> ~100 MB/timestep).  Default: fused on the infer path,
            # split for training; NERRF_REC_FUSED=1/0 forces either.
            bias_c = bias.contiguous()

            def step(ti, h, c):
                h_t, c_t = h_all[ti], c_all[ti]
                ext.lstm_rec_fwd(
                    h, w_hh, xg[ti], bias_c, c,
                    mask[ti] if mask is not None else empty_mask,
                    h_t, c_t, g_none if infer else gates_all[ti],
                )
                return h_t, c_t
        else:
            w_hh_t = w_hh.t().contiguous()
            hg = torch.empty(batch, gdim, device=dev, dtype=dt)
            # dedicated NT MFMA kernel for the [B,256]x[1024,256]^T step
            # (rec_gemm.hip): hipBLASLt's tuned tiles run this shape at
            # ~2.2 TB/s effective (profiles/train_kstats_r02.txt) —
            # K=256 is too short to hide latency and the C epilogue
            # dominates.  NERRF_REC_GEMM=0 falls back to hipBLASLt.
            use_rg = mfma and os.environ.get("NERRF_REC_GEMM", "1") == "1"

            def step(ti, h, c):
                # per step: h goes from h0 to a slab view after the first
                if use_rg and h.stride(1) == 1 and h.stride(0) % 8 == 0:
                    ext.rec_gemm_fwd(h, w_hh, hg)
                else:
                    torch.mm(h, w_hh_t, out=hg)
                h_t, c_t = h_all[ti], c_all[ti]
                ext.lstm_pointwise_fwd(
                    hg, xg[ti], bias, c, h,
                    mask[ti] if mask is not None else empty_mask,
                    h_t, c_t, g_none if infer else gates_all[ti],
                )
                return h_t, c_t

    h = h0.contiguous()
    c = c0.contiguous()
    for ti in (range(t_len - 1, -1, -1) if reverse else range(t_len)):
        h, c = step(ti, h, c)
    return c_all, gates_all


# Rows P of the f32 bias-gradient slab [P, 4H] that the backward pointwise
# kernel accumulates into; the kernel then runs on min(P, blocks needed)
# blocks.  2048 = 256 CUs x 8 blocks, the fastest of 512..8192 at B=64k
# (tools/bias_slab_ab.py; profiles/PROFILES.md, "Bias-gradient slab").
_BIAS_SLAB_ROWS = 2048


def _bias_slab_rows(batch: int, hdim: int, dt: torch.dtype) -> int:
    vec = 8 if dt == torch.bfloat16 else 4  # elements per thread (16 B)
    blocks = -(-batch * max(hdim // vec, 1) // 256)  # 256-thread blocks
    return max(1, min(_BIAS_SLAB_ROWS, blocks))


def _weight_grads(grad_gates_all, h_flat, h0, reverse, bias_slab):
    """(grad_whh, grad_bias) over all timesteps.  The h input of step ti is
    the hidden history shifted by one step, whose bulk is a contiguous-rank
    slice of h_flat — two GEMMs (bulk + the h0 boundary row) instead of
    materialising a shifted copy of the whole history.  `bias_slab` is the
    f32 slab every step accumulated into, or None to reduce grad_gates."""
    t_len, batch, gdim = grad_gates_all.shape
    dt = grad_gates_all.dtype
    gg2 = grad_gates_all.reshape(t_len * batch, gdim)
    if t_len > 1:
        if reverse:
            bulk_gg = grad_gates_all[:-1].reshape((t_len - 1) * batch, gdim)
            bulk_h = h_flat[batch:]
            edge_gg = grad_gates_all[t_len - 1]
        else:
            bulk_gg = grad_gates_all[1:].reshape((t_len - 1) * batch, gdim)
            bulk_h = h_flat[: (t_len - 1) * batch]
            edge_gg = grad_gates_all[0]
        grad_whh = torch.mm(bulk_gg.t(), bulk_h)
        grad_whh = torch.addmm(grad_whh, edge_gg.t(), h0.to(dt))
    else:
        grad_whh = torch.mm(gg2.t(), h0.to(dt))
    grad_bias = (
        bias_slab.sum(dim=0).to(dt) if bias_slab is not None
        else gg2.sum(dim=0)
    )
    return grad_whh, grad_bias


def _dir_backward(ext, grad_out, gates_all, h_flat, c_all, h0, c0, w_hh,
                  mask, reverse, gg_out=None):
    """One direction's backward.

    grad_out: [T, B, H] (rows may be strided — a slab of the dual buffer).
    h_flat:   [T*B, H] flat view of this direction's hidden history with
              uniform row stride (slab of the dual buffer or contiguous).
    gg_out:   optional [T, B, 4H] target for grad_gates — may be a slab of
              a wider [T, B, 2*4H] buffer (rows contiguous), so the caller's
              input-projection backward sees ONE contiguous gradient tensor
              and runs as a single GEMM.
    Returns (grad_xg, grad_h0, grad_c0, grad_whh, grad_bias).
    """
    t_len, batch, hdim = grad_out.shape
    gdim = 4 * hdim
    dev, dt = c_all.device, c_all.dtype

    grad_gates_all = (
        gg_out if gg_out is not None
        else torch.empty(t_len, batch, gdim, device=dev, dtype=dt)
    )
    # running state and its ping-pong partners: a native step writes the
    # new grad_h / grad_c into the spare pair, which the loop then swaps in
    grad_h = torch.zeros(batch, hdim, device=dev, dtype=dt)
    grad_c = torch.zeros(batch, hdim, device=dev, dtype=dt)
    spare_h = torch.empty(batch, hdim, device=dev, dtype=dt)
    spare_c = torch.empty(batch, hdim, device=dev, dtype=dt)
    slab, slab_used = None, False  # f32 bias-grad slab of the split path

    # each step(ti, c_in, grad_h, grad_c, spare_h, spare_c) returns the
    # (grad_h, grad_c) flowing into the next (earlier-in-forward) step
    if ext is None:
        def step(ti, c_in, grad_h, grad_c, spare_h, spare_c):
            gg, grad_c_prev, grad_h_pass = _ref.lstm_pointwise_bwd_ref(
                grad_h + grad_out[ti], grad_c, gates_all[ti], c_in,
                mask[ti] if mask is not None else None,
            )
            grad_gates_all[ti] = gg
            return torch.mm(grad_gates_all[ti], w_hh) + grad_h_pass, grad_c_prev
    else:
        empty_mask = torch.empty(0, device=dev)
        if _mfma_eligible(dt, hdim, w_hh) and _rec_fused(infer=False):
            # fused gate grads + in-launch grad_h GEMM (lstm_rec_fused.hip):
            # grad_gates goes to HBM once, the addmm disappears.  A backward
            # only follows a training forward, hence infer=False.
            w_hh_t = w_hh.t().contiguous()

            def step(ti, c_in, grad_h, grad_c, spare_h, spare_c):
                ext.lstm_rec_bwd(
                    grad_h.contiguous(), grad_out[ti], grad_c.contiguous(),
                    gates_all[ti], c_in.contiguous(), w_hh_t,
                    mask[ti] if mask is not None else empty_mask,
                    grad_gates_all[ti], spare_c, spare_h,
                )
                return spare_h, spare_c
        else:
            # in-kernel bias-grad accumulation: every step's pointwise
            # kernel adds its sum over rows of grad_gates into an f32 slab
            # [P, 4H] (block p owns row p; register sums, plain stores, no
            # atomics), so the four whole-history gg2.sum(0) re-reads per
            # step disappear.  NERRF_FUSED_BIAS=0 keeps the separate
            # reduction for A/B runs.
            slab_on = os.environ.get("NERRF_FUSED_BIAS", "1") == "1"
            slab = (
                torch.zeros(_bias_slab_rows(batch, hdim, dt), gdim,
                            device=dev, dtype=torch.float32)
                if slab_on else empty_mask
            )
            slab_used = slab_on

            def step(ti, c_in, grad_h, grad_c, spare_h, spare_c):
                nonlocal slab_used
                gg_t = grad_gates_all[ti]
                # grad_out[ti] is folded inside the kernel (no separate
                # add), and so is this step's bias-grad partial (sum over
                # batch) — the big gg2.sum(0) re-read disappears when every
                # step fused
                used = ext.lstm_pointwise_bwd(
                    grad_h.contiguous(), grad_out[ti], grad_c.contiguous(),
                    gates_all[ti], c_in.contiguous(),
                    mask[ti] if mask is not None else empty_mask,
                    gg_t, spare_c, spare_h, slab,
                )
                slab_used = slab_used and bool(used)
                # in place: an out-of-place addmm first copies its 2-D
                # `self` into a fresh output (33 MB each way per step);
                # the kernel's pass-through buffer becomes the next grad_h
                # and the old grad_h the next pass-through target
                spare_h.addmm_(gg_t, w_hh)
                return spare_h, spare_c

    # iterate in the opposite order of forward; the c input of step ti is
    # the previous forward step's output (or c0 at the start)
    steps = range(t_len) if reverse else range(t_len - 1, -1, -1)
    first, prev = (t_len - 1, 1) if reverse else (0, -1)
    for ti in steps:
        c_in = c0 if ti == first else c_all[ti + prev]
        new_h, new_c = step(ti, c_in, grad_h, grad_c, spare_h, spare_c)
        spare_h, spare_c, grad_h, grad_c = grad_h, grad_c, new_h, new_c

    grad_whh, grad_bias = _weight_grads(
        grad_gates_all, h_flat, h0, reverse, slab if slab_used else None
    )
    return grad_gates_all, grad_h, grad_c, grad_whh, grad_bias


def _infer_mode(*tensors) -> bool:
    return not torch.is_grad_enabled() or not any(t.requires_grad for t in tensors)


def _norm_mask(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """[T, B] mask as the contiguous f32 constant the kernels read."""
    return mask.detach().contiguous().to(torch.float32) if mask is not None else None


class _LSTMSeqFn(torch.autograd.Function):
    """Single direction: h_all is its own contiguous [T, B, H] tensor."""

    @staticmethod
    def forward(ctx, xg, h0, c0, w_hh, bias, mask, reverse: bool, infer: bool = False):
        t_len, batch, gdim = xg.shape
        hdim = gdim // 4
        h_all = torch.empty(t_len, batch, hdim, device=xg.device, dtype=xg.dtype)
        ext = get_native(xg)
        c_all, gates_all = _dir_forward(
            ext, xg, h0, c0, w_hh, bias, mask, reverse, infer, h_all
        )
        ctx.save_for_backward(
            gates_all, h_all, c_all, h0, c0, w_hh,
            mask if mask is not None else torch.empty(0, device=xg.device),
        )
        ctx.reverse = reverse
        return h_all

    @staticmethod
    def backward(ctx, grad_out):
        gates_all, h_all, c_all, h0, c0, w_hh, mask_t = ctx.saved_tensors
        mask = mask_t if mask_t.numel() else None
        t_len, batch, hdim = h_all.shape
        ext = get_native(h_all)
        grad_xg, grad_h0, grad_c0, grad_whh, grad_bias = _dir_backward(
            ext, grad_out.contiguous(), gates_all,
            h_all.reshape(t_len * batch, hdim), c_all, h0, c0, w_hh,
            mask, ctx.reverse,
        )
        return grad_xg, grad_h0, grad_c0, grad_whh, grad_bias, None, None, None


def _bi_forward(xg_f, xg_b, h0, c0, w_f, b_f, w_b, b_b, mask, infer,
                overlap=False):
    """Both directions of one layer into a single [T, B, 2H] buffer (fwd
    cols 0:H, bwd H:2H).  Returns (h2, tensors to save for `_bi_backward`)."""
    t_len, batch, gdim = xg_f.shape
    hdim = gdim // 4
    h2 = torch.empty(t_len, batch, 2 * hdim, device=xg_f.device, dtype=xg_f.dtype)
    ext = get_native(xg_f)
    if overlap:
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(main)  # xg/h0/c0 ready
    c_f, g_f = _dir_forward(
        ext, xg_f, h0, c0, w_f, b_f, mask, False, infer, h2[:, :, :hdim]
    )
    with torch.cuda.stream(side) if overlap else contextlib.nullcontext():
        c_b, g_b = _dir_forward(
            ext, xg_b, h0, c0, w_b, b_b, mask, True, infer, h2[:, :, hdim:]
        )
    if overlap:
        main.wait_stream(side)
        # cross-stream allocator safety: h2 (allocated on main) was
        # written on the side stream; c_b (allocated on side) is
        # consumed/freed on main — record each tensor's FOREIGN stream
        h2.record_stream(side)
        c_b.record_stream(main)
    return h2, (
        g_f, g_b, h2, c_f, c_b, h0, c0, w_f, w_b,
        mask if mask is not None else torch.empty(0, device=xg_f.device),
    )


def _bi_backward(saved, grad2, gg_f=None, gg_b=None):
    """Backward of `_bi_forward`.  gg_f / gg_b: optional [T, B, 4H] targets
    for the two directions' gate grads (see `_dir_backward`).  Returns
    (grad_xg_f, grad_xg_b, grad_h0, grad_c0, grad_w_f, grad_b_f, grad_w_b,
    grad_b_b)."""
    g_f, g_b, h2, c_f, c_b, h0, c0, w_f, w_b, mask_t = saved
    mask = mask_t if mask_t.numel() else None
    t_len, batch, hdim2 = h2.shape
    hdim = hdim2 // 2
    ext = get_native(h2)
    grad2 = grad2.contiguous()  # one [T, B, 2H] layout fix at most
    h2_flat = h2.reshape(t_len * batch, hdim2)
    gxf, gh0f, gc0f, gwf, gbf = _dir_backward(
        ext, grad2[:, :, :hdim], g_f, h2_flat[:, :hdim], c_f, h0, c0,
        w_f, mask, False, gg_out=gg_f,
    )
    gxb, gh0b, gc0b, gwb, gbb = _dir_backward(
        ext, grad2[:, :, hdim:], g_b, h2_flat[:, hdim:], c_b, h0, c0,
        w_b, mask, True, gg_out=gg_b,
    )
    return gxf, gxb, gh0f + gh0b, gc0f + gc0b, gwf, gbf, gwb, gbb


class _LSTMBiLayerFn(torch.autograd.Function):
    """One bidirectional layer from two [T, B, 4H] input projections."""

    @staticmethod
    def forward(ctx, xg_f, xg_b, h0, c0, w_f, b_f, w_b, b_b, mask, infer: bool = False):
        h2, saved = _bi_forward(xg_f, xg_b, h0, c0, w_f, b_f, w_b, b_b, mask, infer)
        ctx.save_for_backward(*saved)
        return h2

    @staticmethod
    def backward(ctx, grad2):
        return (*_bi_backward(ctx.saved_tensors, grad2), None, None)


class _LSTMBiLayer2Fn(torch.autograd.Function):
    """One bidirectional layer whose input projection is a SINGLE
    [T, B, 2*4H] tensor (forward slab 0:4H, backward slab 4H:8H) — the
    layout one concatenated-weights GEMM produces.  The backward writes
    both directions' gate grads into one [T, B, 2*4H] buffer, so the
    projection's dgrad/wgrad run as single GEMMs too (A panels read once)."""

    @staticmethod
    def forward(ctx, xg2, h0, c0, w_f, b_f, w_b, b_b, mask, infer: bool = False):
        gdim = xg2.shape[2] // 2
        # the two directions are independent recurrence chains; at inference
        # (no autograd stream bookkeeping) they can overlap on a side HIP
        # stream — each chain is 100 serial small-grid kernels, so the
        # other direction's work fills the idle CUs.  Opt-in
        # (NERRF_STREAM_DIRS=1) pending an in-context A/B.
        overlap = (
            infer
            and xg2.is_cuda
            and os.environ.get("NERRF_STREAM_DIRS", "0") == "1"
        )
        h2, saved = _bi_forward(
            xg2[:, :, :gdim], xg2[:, :, gdim:], h0, c0, w_f, b_f, w_b, b_b,
            mask, infer, overlap,
        )
        ctx.save_for_backward(*saved)
        return h2

    @staticmethod
    def backward(ctx, grad2):
        h2 = ctx.saved_tensors[2]
        t_len, batch, hdim2 = h2.shape
        gdim = 2 * hdim2  # 4H
        grad_xg2 = torch.empty(t_len, batch, 2 * gdim, device=h2.device,
                               dtype=h2.dtype)
        grads = _bi_backward(
            ctx.saved_tensors, grad2, grad_xg2[:, :, :gdim], grad_xg2[:, :, gdim:]
        )
        return (grad_xg2, *grads[2:], None, None)


def lstm_sequence(
    xg: torch.Tensor,  # [T, B, 4H]
    h0: torch.Tensor,
    c0: torch.Tensor,
    w_hh: torch.Tensor,
    bias: torch.Tensor,
    mask: Optional[torch.Tensor] = None,  # [T, B]
    reverse: bool = False,
) -> torch.Tensor:
    infer = _infer_mode(xg, h0, c0, w_hh, bias)
    return _LSTMSeqFn.apply(
        xg.contiguous(), h0, c0, w_hh, bias, _norm_mask(mask), reverse, infer
    )


def lstm_bilayer(
    xg_f: torch.Tensor,  # [T, B, 4H] forward-direction input projection
    xg_b: torch.Tensor,  # [T, B, 4H] backward-direction input projection
    h0: torch.Tensor,
    c0: torch.Tensor,
    w_f: torch.Tensor,
    b_f: torch.Tensor,
    w_b: torch.Tensor,
    b_b: torch.Tensor,
    mask: Optional[torch.Tensor] = None,  # [T, B]
) -> torch.Tensor:
    """Both directions of one layer -> [T, B, 2H] (fwd cols 0:H, bwd H:2H)."""
    infer = _infer_mode(xg_f, xg_b, h0, c0, w_f, b_f, w_b, b_b)
    return _LSTMBiLayerFn.apply(
        xg_f.contiguous(), xg_b.contiguous(), h0, c0, w_f, b_f, w_b, b_b,
        _norm_mask(mask), infer,
    )


def lstm_bilayer2(
    xg2: torch.Tensor,  # [T, B, 2*4H]: fwd projection 0:4H, bwd 4H:8H
    h0: torch.Tensor,
    c0: torch.Tensor,
    w_f: torch.Tensor,
    b_f: torch.Tensor,
    w_b: torch.Tensor,
    b_b: torch.Tensor,
    mask: Optional[torch.Tensor] = None,  # [T, B]
) -> torch.Tensor:
    """Both directions of one layer from a single concatenated projection
    -> [T, B, 2H].  Rows of xg2 must be contiguous (the tensor itself may
    be a reshaped GEMM output)."""
    infer = _infer_mode(xg2, h0, c0, w_f, b_f, w_b, b_b)
    assert xg2.stride(2) == 1, "xg2 rows must be contiguous"
    return _LSTMBiLayer2Fn.apply(
        xg2, h0, c0, w_f, b_f, w_b, b_b, _norm_mask(mask), infer
    )


# ---------------------------------------------------------------------------
# packed (length-sorted) bidirectional layer
# ---------------------------------------------------------------------------

# Below this many rows the recurrent step GEMM goes to hipBLASLt even where
# rec_gemm.hip's shape contract holds.  rec_gemm loses to hipBLASLt below
# ~32k rows (0.73x at M=16k, 0.93x at 24k, 1.04x at 32k, 1.18x at 64k:
# tools/rec_gemm_ab.py; profiles/PROFILES.md, "Packed BiLSTM"), but the two
# round differently and the dense path runs rec_gemm on every step: with the
# threshold at 1 the packed forward is bitwise the dense forward
# (tests/test_lstm_packed_gpu.py).  That is worth the ~2 ms/step (113.4 ->
# 115.7) which a threshold at the crossover saves on the benchmark.
_REC_GEMM_MIN_ROWS = 1


@dataclass
class SeqPlan:
    """Length-sorted packing of a padded [B, T] batch of sequences.

    Sequences are sorted by (clamped) length, descending and stable; sorted
    row r is sequence perm[r].  At timestep t the live sequences are the
    sorted rows [0, batch_sizes[t]) and batch_sizes is non-increasing, so a
    packed time-major tensor has N = sum(lengths) rows: slab t sits at rows
    [offsets[t], offsets[t] + batch_sizes[t]).  Timesteps at or past
    max(lengths) do not exist.  perm, inv_perm, batch_sizes and offsets live
    on the host; the index tensors on the device the op runs on, so a step
    that is handed a plan does no device-to-host copy.
    """

    n_seq: int                 # B
    t_max: int                 # padded length T the lengths were clamped to
    perm: np.ndarray           # [B] sorted row -> sequence
    inv_perm: np.ndarray       # [B] sequence -> sorted row
    batch_sizes: List[int]     # [T_live] n_t
    offsets: List[int]         # [T_live + 1] off_t, offsets[-1] == N
    has_empty: bool            # some sequence has length 0
    pack_idx: torch.Tensor     # [N] rows of feats.reshape(B*T, E)
    hin_idx: torch.Tensor      # [2N] rows of the [(N+1)*2, H] view of the
    #                            layer output (+1: a trailing zero row) that
    #                            form the steps' h inputs, both directions
    fin_idx: torch.Tensor      # [2B] rows of the [2N, H] view holding each
    #                            sequence's final fwd / bwd state
    live: torch.Tensor         # [B, 1] f32, 0 where length == 0

    def to(self, device) -> "SeqPlan":
        """The same plan with its index tensors on `device` (host fields
        shared) — building a plan costs ~0.15 s of numpy at B = 64k, so a
        batch builds it once on the CPU and stages it per use."""
        device = torch.device(device)
        if self.pack_idx.device == device:
            return self
        moved = {
            k: getattr(self, k).to(device, non_blocking=True)
            for k in ("pack_idx", "hin_idx", "fin_idx", "live")
        }
        return dataclasses.replace(self, **moved)

    @property
    def n_rows(self) -> int:
        return self.offsets[-1]

    @property
    def t_live(self) -> int:
        return len(self.batch_sizes)

    def steps(self, reverse: bool) -> List[Tuple[int, int, int, int]]:
        """(off, n, prev_off, k) per step in execution order: the step
        covers rows [off, off + n); its previous state is the first k rows
        of the slab at prev_off (k == 0: zero initial state)."""
        n, off = self.batch_sizes, self.offsets
        tl = len(n)
        if reverse:
            return [
                (off[t], n[t], off[t + 1], n[t + 1] if t + 1 < tl else 0)
                for t in range(tl - 1, -1, -1)
            ]
        return [
            (off[t], n[t], off[t - 1] if t else 0, n[t] if t else 0)
            for t in range(tl)
        ]


def build_seq_plan(lengths, t_max: int, device="cpu") -> SeqPlan:
    """Plan from `lengths` ([B]; numpy array or tensor — a device tensor
    costs one device-to-host copy here).  Lengths are clamped to
    [0, t_max]."""
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    ln = np.clip(np.asarray(lengths).astype(np.int64).reshape(-1), 0, int(t_max))
    b = int(ln.shape[0])
    perm = np.argsort(-ln, kind="stable")
    inv_perm = np.empty(b, dtype=np.int64)
    inv_perm[perm] = np.arange(b, dtype=np.int64)
    t_live = int(ln.max()) if b else 0
    # n_t = number of sequences longer than t
    n_t = b - np.cumsum(np.bincount(ln, minlength=t_live + 1))[:t_live]
    off = np.zeros(t_live + 1, dtype=np.int64)
    np.cumsum(n_t, out=off[1:])
    n_rows = int(off[-1])

    t_of = np.repeat(np.arange(t_live, dtype=np.int64), n_t)  # [N]
    r_of = np.arange(n_rows, dtype=np.int64) - off[t_of]
    pack_idx = perm[r_of] * int(t_max) + t_of
    # h input of packed row (t, r).  Forward direction: row r of slab t-1
    # (slab 0 starts from zero).  Reverse: row r of slab t+1 where that slab
    # has such a row, else zero.  Zero = row N of the padded layer output.
    src_f = np.where(t_of > 0, off[np.maximum(t_of - 1, 0)] + r_of, n_rows)
    n_next = np.append(n_t, 0)[t_of + 1] if t_live else n_t
    src_b = np.where(r_of < n_next, off[np.minimum(t_of + 1, t_live)] + r_of, n_rows)
    hin_idx = np.stack([2 * src_f, 2 * src_b + 1], axis=1).reshape(-1)
    # final states per sequence, in the original order
    r_seq = inv_perm
    live = ln > 0
    fin_f = np.where(live, off[np.maximum(ln - 1, 0)] + r_seq, 0)
    fin_b = np.where(live, r_seq, 0)
    fin_idx = np.stack([2 * fin_f, 2 * fin_b + 1], axis=1).reshape(-1)

    def dev(a, dt=torch.int64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device, non_blocking=True)

    return SeqPlan(
        n_seq=b, t_max=int(t_max), perm=perm, inv_perm=inv_perm,
        batch_sizes=[int(x) for x in n_t], offsets=[int(x) for x in off],
        has_empty=bool((~live).any()),
        pack_idx=dev(pack_idx), hin_idx=dev(hin_idx), fin_idx=dev(fin_idx),
        live=dev(live.reshape(b, 1), torch.float32),
    )


def _packed_dir_forward(ext, xg, w_hh, bias, plan, reverse, infer, h_out,
                        c_all, gates_all, hg):
    """One direction over the packed layout.  xg [N, 4H], h_out [N, H] (rows
    uniformly strided: slabs of the dual-direction buffers); c_all [N, H],
    gates_all [N, 4H] contiguous; hg: [n_0, 4H] scratch, sliced per step —
    rows past a step's k hold stale data of a longer step and are never
    read (prev_rows)."""
    dt, hdim = xg.dtype, w_hh.shape[1]
    if ext is None:
        for off, n, poff, k in plan.steps(reverse):
            pre = xg[off:off + n] + bias
            c_in = pre.new_zeros(n, hdim)
            if k:
                pre[:k] += h_out[poff:poff + k] @ w_hh.t()
                c_in[:k] = c_all[poff:poff + k]
            h_new, c_new, g_act = _ref.lstm_pointwise_fwd_ref(pre, c_in, None, None)
            h_out[off:off + n] = h_new
            c_all[off:off + n] = c_new
            if not infer:
                gates_all[off:off + n] = g_act
        return
    mfma = _mfma_eligible(dt, hdim, w_hh)
    use_rg = (
        mfma and os.environ.get("NERRF_REC_GEMM", "1") == "1"
        and h_out.stride(0) % 8 == 0
    )
    w_hh_t = w_hh.t().contiguous()
    g_none = torch.empty(0, device=xg.device, dtype=dt)
    empty_mask = torch.empty(0, device=xg.device)
    for off, n, poff, k in plan.steps(reverse):
        h_prev = h_out[poff:poff + k]
        if k:  # no zero-row GEMMs
            if use_rg and k >= _REC_GEMM_MIN_ROWS:
                ext.rec_gemm_fwd(h_prev, w_hh, hg[:k])
            else:
                torch.mm(h_prev, w_hh_t, out=hg[:k])
        ext.lstm_pointwise_fwd(
            hg[:k], xg[off:off + n], bias, c_all[poff:poff + k], h_prev,
            empty_mask, h_out[off:off + n], c_all[off:off + n],
            g_none if infer else gates_all[off:off + n], k,
        )


def _packed_dir_backward(ext, grad_out, gates_all, c_all, w_hh, plan, reverse,
                         gg_out):
    """Backward of `_packed_dir_forward`: fills gg_out [N, 4H] (a slab of
    the dual gate-grad buffer) and returns the bias gradient source: the f32
    slab the kernel accumulated into, or None (reduce gg_out instead)."""
    dt, dev = c_all.dtype, c_all.device
    hdim = w_hh.shape[1]
    steps = plan.steps(reverse)
    n0 = plan.batch_sizes[0]
    # the step after s in execution order consumed the first k rows of s's
    # output, so that is how many rows of recurrent gradient s receives
    in_rows = [st[3] for st in steps[1:]] + [0]
    if ext is None:
        grad_h = grad_c = None
        for (off, n, poff, k), rin in zip(reversed(steps), reversed(in_rows)):
            gh_in = grad_out[off:off + n].clone()
            gc_in = gh_in.new_zeros(n, hdim)
            c_in = gh_in.new_zeros(n, hdim)
            if rin:
                gh_in[:rin] += grad_h[:rin]
                gc_in[:rin] = grad_c[:rin]
            if k:
                c_in[:k] = c_all[poff:poff + k]
            gg, gc_prev, _ = _ref.lstm_pointwise_bwd_ref(
                gh_in, gc_in, gates_all[off:off + n], c_in, None
            )
            gg_out[off:off + n] = gg
            grad_h, grad_c = gg[:k] @ w_hh, gc_prev[:k]
        return None
    slab_on = os.environ.get("NERRF_FUSED_BIAS", "1") == "1"
    empty = torch.empty(0, device=dev)
    slab = (
        torch.zeros(_bias_slab_rows(n0, hdim, dt), 4 * hdim, device=dev,
                    dtype=torch.float32)
        if slab_on else empty
    )
    slab_used = slab_on
    # without a mask the pass-through gradient is identically zero: the
    # kernel skips its store and the recurrent dgrad is a plain mm into the
    # one grad_h buffer (the kernel that read it ran before, same stream)
    grad_h = torch.empty(n0, hdim, device=dev, dtype=dt)
    grad_c = torch.empty(n0, hdim, device=dev, dtype=dt)
    spare_c = torch.empty(n0, hdim, device=dev, dtype=dt)
    no_pass = torch.empty(0, device=dev, dtype=dt)
    for (off, n, poff, k), rin in zip(reversed(steps), reversed(in_rows)):
        gg_t = gg_out[off:off + n]
        used = ext.lstm_pointwise_bwd(
            grad_h[:rin], grad_out[off:off + n], grad_c[:rin],
            gates_all[off:off + n], c_all[poff:poff + k], empty, gg_t,
            spare_c[:n], no_pass, slab, rin, k,
        )
        slab_used = slab_used and bool(used)
        if k:  # dgrad only on the rows the next step consumes
            torch.mm(gg_t[:k], w_hh, out=grad_h[:k])
        grad_c, spare_c = spare_c, grad_c
    return slab if slab_used else None


class _LSTMBiLayer2PackedFn(torch.autograd.Function):
    """`_LSTMBiLayer2Fn` over the packed layout: xg2p [N, 2*4H] -> h2p
    [N, 2H], zero initial state, no mask — padding rows do not exist."""

    @staticmethod
    def forward(ctx, xg2p, w_f, b_f, w_b, b_b, plan: SeqPlan, infer: bool = False):
        n_rows, gdim2 = xg2p.shape
        gdim = gdim2 // 2
        hdim = gdim // 4
        dev, dt = xg2p.device, xg2p.dtype
        ext = get_native(xg2p)
        # one extra, zero row: the h input of a step's rows that have no
        # previous state (see SeqPlan.hin_idx)
        h2p_buf = torch.empty(n_rows + 1, 2 * hdim, device=dev, dtype=dt)
        h2p_buf[n_rows].zero_()
        h2p = h2p_buf[:n_rows]
        c_f = torch.empty(n_rows, hdim, device=dev, dtype=dt)
        c_b = torch.empty(n_rows, hdim, device=dev, dtype=dt)
        g_rows = 0 if infer else n_rows
        g_f = torch.empty(g_rows, gdim, device=dev, dtype=dt)
        g_b = torch.empty(g_rows, gdim, device=dev, dtype=dt)
        hg = (
            torch.empty(plan.batch_sizes[0], gdim, device=dev, dtype=dt)
            if ext is not None and n_rows else None
        )
        _packed_dir_forward(ext, xg2p[:, :gdim], w_f, b_f, plan, False, infer,
                            h2p[:, :hdim], c_f, g_f, hg)
        _packed_dir_forward(ext, xg2p[:, gdim:], w_b, b_b, plan, True, infer,
                            h2p[:, hdim:], c_b, g_b, hg)
        ctx.save_for_backward(g_f, g_b, h2p_buf, c_f, c_b, w_f, w_b)
        ctx.plan = plan
        return h2p

    @staticmethod
    def backward(ctx, grad2):
        g_f, g_b, h2p_buf, c_f, c_b, w_f, w_b = ctx.saved_tensors
        plan = ctx.plan
        n_rows = h2p_buf.shape[0] - 1
        hdim = h2p_buf.shape[1] // 2
        gdim = 4 * hdim
        dev, dt = h2p_buf.device, h2p_buf.dtype
        ext = get_native(h2p_buf)
        grad2 = grad2.contiguous()
        # ONE [N, 2*4H] gate-grad buffer: the projection's dgrad / wgrad
        # stay single GEMMs
        gg2 = torch.empty(n_rows, 2 * gdim, device=dev, dtype=dt)
        if n_rows == 0:
            zw = torch.zeros_like(w_f)
            zb = torch.zeros(gdim, device=dev, dtype=dt)
            return gg2, zw, zb, zw.clone(), zb.clone(), None, None
        slab_f = _packed_dir_backward(ext, grad2[:, :hdim], g_f, c_f, w_f,
                                      plan, False, gg2[:, :gdim])
        slab_b = _packed_dir_backward(ext, grad2[:, hdim:], g_b, c_b, w_b,
                                      plan, True, gg2[:, gdim:])
        # recurrent weight grads: one GEMM per direction over all live rows
        n0 = plan.batch_sizes[0]
        if plan.batch_sizes[-1] == n0:
            # all sequences equally long: every slab has n0 rows, so the
            # steps' h inputs are the history shifted by one slab — views
            # (the edge slab's h input is zero and drops out)
            if n_rows > n0:
                gw_f = torch.mm(gg2[n0:, :gdim].t(), h2p_buf[:n_rows - n0, :hdim])
                gw_b = torch.mm(gg2[:n_rows - n0, gdim:].t(), h2p_buf[n0:n_rows, hdim:])
            else:
                gw_f, gw_b = torch.zeros_like(w_f), torch.zeros_like(w_b)
        else:
            # slabs differ in size, so the shifted history is not a view:
            # both directions' h inputs as ONE [N, 2H] gather
            h_in = (
                h2p_buf.view(2 * (n_rows + 1), hdim)
                .index_select(0, plan.hin_idx).view(n_rows, 2 * hdim)
            )
            gw_f = torch.mm(gg2[:, :gdim].t(), h_in[:, :hdim])
            gw_b = torch.mm(gg2[:, gdim:].t(), h_in[:, hdim:])
        gb_f = (slab_f.sum(dim=0).to(dt) if slab_f is not None
                else gg2[:, :gdim].sum(dim=0))
        gb_b = (slab_b.sum(dim=0).to(dt) if slab_b is not None
                else gg2[:, gdim:].sum(dim=0))
        return gg2, gw_f, gb_f, gw_b, gb_b, None, None


def lstm_bilayer2_packed(
    xg2p: torch.Tensor,  # [N, 2*4H] packed: fwd projection 0:4H, bwd 4H:8H
    plan: SeqPlan,
    w_f: torch.Tensor,
    b_f: torch.Tensor,
    w_b: torch.Tensor,
    b_b: torch.Tensor,
) -> torch.Tensor:
    """Both directions of one layer over length-sorted packed rows ->
    [N, 2H] (fwd cols 0:H, bwd H:2H).  Every LSTM tensor holds only the
    N = sum(lengths) live (timestep, sequence) rows, both directions loop
    over max(lengths) steps, and the state starts from zero."""
    assert xg2p.dim() == 2 and xg2p.stride(1) == 1, "xg2p rows must be contiguous"
    assert xg2p.shape[0] == plan.n_rows, "xg2p does not match the plan"
    infer = _infer_mode(xg2p, w_f, b_f, w_b, b_b)
    return _LSTMBiLayer2PackedFn.apply(xg2p, w_f, b_f, w_b, b_b, plan, infer)
