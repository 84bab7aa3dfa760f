"""GPU numerics tests: HIP kernels vs pure-PyTorch fp32 references."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nerrf_amd.ops import gather_mean, lstm_cell  # noqa: E402
from nerrf_amd.ops import reference as ref  # noqa: E402


@pytest.fixture(autouse=True)
def _require_native(gpu_device):
    from nerrf_amd.ops.native import load_extension

    load_extension(required=True)


def test_gather_mean_fwd_fp32(gpu_device):
    torch.manual_seed(0)
    n, k, d = 517, 16, 128
    h = torch.randn(n, d, device=gpu_device)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    out = gather_mean(h, idx, w)
    out_ref = ref.gather_mean_ref(h.cpu(), idx.cpu(), w.cpu())
    assert torch.allclose(out.cpu(), out_ref, atol=1e-5, rtol=1e-5)


def test_gather_mean_fwd_bf16_vs_fp32ref(gpu_device):
    torch.manual_seed(1)
    n, k, d = 1024, 16, 128
    h32 = torch.randn(n, d, device=gpu_device)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    out = gather_mean(h32.to(torch.bfloat16), idx, w)
    out_ref = ref.gather_mean_ref(h32.cpu(), idx.cpu(), w.cpu())
    # bf16 inputs: ~3 decimal digits
    assert torch.allclose(out.float().cpu(), out_ref, atol=3e-2, rtol=3e-2)


def test_gather_mean_fwd_odd_dim(gpu_device):
    """Non-128-multiple feature dim exercises the generic kernel path."""
    torch.manual_seed(2)
    n, k, d = 203, 7, 96
    h = torch.randn(n, d, device=gpu_device)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device)
    out = gather_mean(h, idx, w)
    out_ref = ref.gather_mean_ref(h.cpu(), idx.cpu(), w.cpu())
    assert torch.allclose(out.cpu(), out_ref, atol=1e-5, rtol=1e-5)


def test_gather_mean_bwd_fp32(gpu_device):
    torch.manual_seed(3)
    n, k, d = 301, 16, 128
    h = torch.randn(n, d, device=gpu_device, requires_grad=True)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    out = gather_mean(h, idx, w)
    g = torch.randn_like(out)
    out.backward(g)
    grad_ref = ref.gather_mean_bwd_ref(g.cpu(), idx.cpu(), w.cpu(), n)
    assert torch.allclose(h.grad.cpu(), grad_ref, atol=1e-4, rtol=1e-4)


def test_lstm_pointwise_fwd_fp32(gpu_device):
    torch.manual_seed(4)
    b, hd = 333, 256
    xg = torch.randn(b, 4 * hd, device=gpu_device)
    h0 = torch.randn(b, hd, device=gpu_device)
    c0 = torch.randn(b, hd, device=gpu_device)
    w_hh = torch.randn(4 * hd, hd, device=gpu_device) * 0.1
    bias = torch.randn(4 * hd, device=gpu_device)
    mask = (torch.rand(b, device=gpu_device) > 0.3).float()
    h1, c1 = lstm_cell(xg, h0, c0, w_hh, bias, mask)
    gates_pre = torch.addmm(bias.cpu(), h0.cpu(), w_hh.cpu().t()) + xg.cpu()
    h_ref, c_ref, _ = ref.lstm_pointwise_fwd_ref(gates_pre, c0.cpu(), h0.cpu(), mask.cpu())
    assert torch.allclose(h1.cpu(), h_ref, atol=1e-4, rtol=1e-4)
    assert torch.allclose(c1.cpu(), c_ref, atol=1e-4, rtol=1e-4)


def test_lstm_cell_bwd_fp32(gpu_device):
    torch.manual_seed(5)
    b, hd = 65, 256
    xg = torch.randn(b, 4 * hd, device=gpu_device, requires_grad=True)
    h0 = torch.randn(b, hd, device=gpu_device, requires_grad=True)
    c0 = torch.randn(b, hd, device=gpu_device, requires_grad=True)
    w_hh = (torch.randn(4 * hd, hd, device=gpu_device) * 0.1).requires_grad_(True)
    bias = torch.randn(4 * hd, device=gpu_device, requires_grad=True)
    mask = (torch.rand(b, device=gpu_device) > 0.3).float()
    h1, c1 = lstm_cell(xg, h0, c0, w_hh, bias, mask)
    loss = (h1 * 1.3).sum() + (c1 * 0.7).sum()
    loss.backward()
    grads_gpu = [t.grad.cpu().clone() for t in (xg, h0, c0, w_hh, bias)]

    xg2 = xg.detach().cpu().requires_grad_(True)
    h02 = h0.detach().cpu().requires_grad_(True)
    c02 = c0.detach().cpu().requires_grad_(True)
    w2 = w_hh.detach().cpu().requires_grad_(True)
    b2 = bias.detach().cpu().requires_grad_(True)
    gates_pre = torch.addmm(b2, h02, w2.t()) + xg2
    h_ref, c_ref, _ = ref.lstm_pointwise_fwd_ref(gates_pre, c02, h02, mask.cpu())
    ((h_ref * 1.3).sum() + (c_ref * 0.7).sum()).backward()
    grads_cpu = [t.grad for t in (xg2, h02, c02, w2, b2)]
    for g_gpu, g_cpu, name in zip(grads_gpu, grads_cpu, ["xg", "h0", "c0", "w_hh", "b"]):
        assert torch.allclose(g_gpu, g_cpu, atol=1e-3, rtol=1e-3), f"grad {name}"


def test_lstm_cell_bf16(gpu_device):
    torch.manual_seed(6)
    b, hd = 128, 256
    xg = torch.randn(b, 4 * hd, device=gpu_device)
    h0 = torch.randn(b, hd, device=gpu_device)
    c0 = torch.randn(b, hd, device=gpu_device)
    w_hh = torch.randn(4 * hd, hd, device=gpu_device) * 0.1
    bias = torch.randn(4 * hd, device=gpu_device)
    h1, c1 = lstm_cell(
        xg.to(torch.bfloat16), h0.to(torch.bfloat16), c0.to(torch.bfloat16),
        w_hh.to(torch.bfloat16), bias.to(torch.bfloat16),
    )
    gates_pre = torch.addmm(bias.cpu(), h0.cpu(), w_hh.cpu().t()) + xg.cpu()
    h_ref, c_ref, _ = ref.lstm_pointwise_fwd_ref(gates_pre, c0.cpu(), h0.cpu(), None)
    assert torch.allclose(h1.float().cpu(), h_ref, atol=5e-2, rtol=5e-2)
    assert torch.allclose(c1.float().cpu(), c_ref, atol=5e-2, rtol=5e-2)


def test_joint_model_train_step_gpu(gpu_device):
    """End-to-end: one bf16 training step of the joint model on GPU."""
    from nerrf_amd.data.dataset import synth_window_batches
    from nerrf_amd.models.graphsage import SageConfig
    from nerrf_amd.models.joint import JointConfig, NerrfJointModel
    from nerrf_amd.models.lstm import LSTMConfig

    batches = synth_window_batches(n_scenarios=1, duration_s=40.0, benign_rate_hz=200.0, base_seed=7)
    batch = batches[0].to_torch(device=gpu_device, dtype=torch.bfloat16)
    model = NerrfJointModel(
        JointConfig(sage=SageConfig(layers=6, hidden=128), lstm=LSTMConfig(hidden=256))
    ).to(device=gpu_device, dtype=torch.bfloat16)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    node_logit, edge_logit, seq_logit = model(batch)
    losses = model.loss(node_logit, edge_logit, seq_logit, batch)
    losses["total"].backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(losses["total"].float()).item()


def test_lstm_sequence_gpu_fp32(gpu_device):
    """Full sequence op on GPU vs CPU reference loop."""
    from nerrf_amd.ops import lstm_sequence
    from nerrf_amd.ops.reference import lstm_pointwise_fwd_ref

    torch.manual_seed(7)
    t, b, hd = 13, 97, 64
    xg = torch.randn(t, b, 4 * hd, device=gpu_device)
    h0 = torch.randn(b, hd, device=gpu_device)
    c0 = torch.randn(b, hd, device=gpu_device)
    w_hh = torch.randn(4 * hd, hd, device=gpu_device) * 0.2
    bias = torch.randn(4 * hd, device=gpu_device)
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()

    for rev in (False, True):
        out = lstm_sequence(xg, h0, c0, w_hh, bias, mask, reverse=rev)
        h, c = h0.cpu(), c0.cpu()
        outs = [None] * t
        steps = range(t - 1, -1, -1) if rev else range(t)
        for ti in steps:
            gp = torch.addmm(bias.cpu(), h, w_hh.cpu().t()) + xg[ti].cpu()
            h, c, _ = lstm_pointwise_fwd_ref(gp, c, h, mask[ti].cpu())
            outs[ti] = h
        ref = torch.stack(outs)
        assert torch.allclose(out.cpu(), ref, atol=1e-4, rtol=1e-4), f"rev={rev}"


def test_lstm_sequence_gpu_backward(gpu_device):
    from nerrf_amd.ops import lstm_sequence
    from nerrf_amd.ops.reference import lstm_pointwise_fwd_ref

    torch.manual_seed(8)
    t, b, hd = 7, 33, 32
    xg_g = torch.randn(t, b, 4 * hd, device=gpu_device, requires_grad=True)
    h0 = torch.zeros(b, hd, device=gpu_device)
    c0 = torch.zeros(b, hd, device=gpu_device)
    w_hh = (torch.randn(4 * hd, hd, device=gpu_device) * 0.2).requires_grad_(True)
    bias = torch.randn(4 * hd, device=gpu_device, requires_grad=True)
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()

    out = lstm_sequence(xg_g, h0, c0, w_hh, bias, mask, reverse=False)
    g = torch.randn_like(out)
    out.backward(g)
    grads_gpu = [p.grad.cpu().clone() for p in (xg_g, w_hh, bias)]

    xg_c = xg_g.detach().cpu().requires_grad_(True)
    w_c = w_hh.detach().cpu().requires_grad_(True)
    b_c = bias.detach().cpu().requires_grad_(True)
    h, c = h0.cpu(), c0.cpu()
    outs = []
    for ti in range(t):
        gp = torch.addmm(b_c, h, w_c.t()) + xg_c[ti]
        h, c, _ = lstm_pointwise_fwd_ref(gp, c, h, mask[ti].cpu())
        outs.append(h)
    torch.stack(outs).backward(g.cpu())
    grads_cpu = [p.grad for p in (xg_c, w_c, b_c)]
    for gg, gc, name in zip(grads_gpu, grads_cpu, ["xg", "w_hh", "bias"]):
        assert torch.allclose(gg, gc, atol=1e-3, rtol=1e-3), f"grad {name}"


def test_mcts_eval_plans_matches_cpu(gpu_device):
    """Device eval_plan vs CPU simulate_plan on enumerated plans."""
    from nerrf_amd.planner.mcts import UCB_C
    from nerrf_amd.planner.rewards import PlannerParams, build_state, simulate_plan
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    rng = np.random.default_rng(0)
    scores = rng.random(40)
    mb = rng.random(40) * 5
    st = build_state(scores, mb, proc_score=0.8, remaining_clean_mb=30.0)
    params = PlannerParams()
    pd = {
        "n_groups": st.n_groups, "max_depth": params.max_depth, "sims_per_tree": 1,
        "downtime_weight": params.downtime_weight, "revert_time_s": params.revert_time_s,
        "kill_time_s": params.kill_time_s, "fp_weight": params.fp_weight,
        "attack_rate_mbps": params.attack_rate_mbps, "horizon_s": params.horizon_s,
        "restore_time_s": params.restore_time_s,
        "restore_loss_mb": params.restore_loss_mb,
        "ucb_c": UCB_C, "seed": 0,
    }
    n_actions = st.n_groups + 3  # STOP, KILL, RESTORE, reverts
    plans = rng.integers(0, n_actions, size=(200, 6)).astype(np.int32)
    gs = torch.from_numpy(st.group_score.astype(np.float32)).to(gpu_device)
    gm = torch.from_numpy(st.group_mb.astype(np.float32)).to(gpu_device)
    gf = torch.from_numpy(st.group_files.astype(np.float32)).to(gpu_device)
    out = ext.mcts_eval_plans(gs, gm, gf, st.proc_score, st.remaining_clean_mb, pd,
                              torch.from_numpy(plans).to(gpu_device))
    cpu = np.array([simulate_plan(st, list(p), params) for p in plans])
    assert np.allclose(out.cpu().numpy(), cpu, rtol=1e-4, atol=1e-3)


def test_mcts_search_gpu_agrees_with_cpu(gpu_device):
    from nerrf_amd.planner.mcts import run_mcts, run_mcts_gpu
    from nerrf_amd.planner.rewards import A_KILL, build_state

    scores = np.concatenate([np.full(20, 0.95), np.full(20, 0.03)])
    mb = np.full(40, 2.0)
    st = build_state(scores, mb, proc_score=0.97, remaining_clean_mb=50.0)
    cpu = run_mcts(st, n_sims=1024, seed=1)
    gpu = run_mcts_gpu(st, n_sims=1024, seed=1, device=str(gpu_device))
    assert gpu.simulations == 1024
    # same dominant action and comparable plan quality
    assert gpu.ranked_actions[0][0] == cpu.ranked_actions[0][0] == A_KILL
    assert abs(gpu.root_value - cpu.root_value) < 1.0


def test_lstm_step_fused_raw_gemm_matches_mm(gpu_device):
    """RAW mode: fused-kernel gates_pre == h @ W_hh^T + xg + bias (bf16 MFMA
    vs hipBLASLt).  Asymmetric operands so operand/output transposes are
    caught (guide rule G9)."""
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(11)
    b, hd = 333, 256  # non-multiple of 32 exercises row guards
    h = (torch.randn(b, hd, device=gpu_device) * 0.3).to(torch.bfloat16)
    w = (torch.randn(4 * hd, hd, device=gpu_device) * 0.1).to(torch.bfloat16)
    w += torch.arange(4 * hd, device=gpu_device).unsqueeze(1).to(torch.bfloat16) * 1e-4  # asymmetry
    xg = (torch.randn(b, 4 * hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    bias = torch.randn(4 * hd, device=gpu_device).to(torch.bfloat16)
    c = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    h_out = torch.empty_like(c)
    c_out = torch.empty_like(c)
    gates = torch.empty_like(xg)
    w_tiled = w.reshape(4 * hd, hd // 32, 32).permute(1, 0, 2).contiguous()
    ext.lstm_step_fused(h, w_tiled, xg, bias, c, torch.empty(0, device=gpu_device),
                        h_out, c_out, gates, True)
    ref = (h.float() @ w.float().t() + xg.float() + bias.float())
    assert torch.allclose(gates.float(), ref, atol=8e-2, rtol=4e-2)


def test_lstm_step_fused_full_matches_reference(gpu_device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(12)
    b, hd = 256, 256
    h = (torch.randn(b, hd, device=gpu_device) * 0.3).to(torch.bfloat16)
    w = (torch.randn(4 * hd, hd, device=gpu_device) * 0.1).to(torch.bfloat16)
    xg = (torch.randn(b, 4 * hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    bias = torch.randn(4 * hd, device=gpu_device).to(torch.bfloat16)
    c = (torch.randn(b, hd, device=gpu_device) * 0.5).to(torch.bfloat16)
    mask = (torch.rand(b, device=gpu_device) > 0.3).float()
    h_out = torch.empty_like(c)
    c_out = torch.empty_like(c)
    gates = torch.empty_like(xg)
    w_tiled = w.reshape(4 * hd, hd // 32, 32).permute(1, 0, 2).contiguous()
    ext.lstm_step_fused(h, w_tiled, xg, bias, c, mask, h_out, c_out, gates, False)

    gp = h.float().cpu() @ w.float().cpu().t() + xg.float().cpu() + bias.float().cpu()
    h_ref, c_ref, g_ref = ref.lstm_pointwise_fwd_ref(gp, c.float().cpu(), h.float().cpu(), mask.cpu())
    assert torch.allclose(h_out.float().cpu(), h_ref, atol=5e-2, rtol=5e-2)
    assert torch.allclose(c_out.float().cpu(), c_ref, atol=5e-2, rtol=5e-2)
    assert torch.allclose(gates.float().cpu(), g_ref, atol=5e-2, rtol=5e-2)


def test_lstm_sequence_bf16_default_path(gpu_device):
    """bf16 lstm_sequence on the default path (no flag set; no input requires
    grad, so H=256 takes the default inference step) vs fp32 CPU loop."""
    from nerrf_amd.ops import lstm_sequence
    from nerrf_amd.ops.reference import lstm_pointwise_fwd_ref

    torch.manual_seed(13)
    t, b, hd = 6, 64, 256
    xg32 = torch.randn(t, b, 4 * hd, device=gpu_device) * 0.3
    w32 = torch.randn(4 * hd, hd, device=gpu_device) * 0.1
    bias32 = torch.randn(4 * hd, device=gpu_device) * 0.3
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()
    h0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    c0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    out = lstm_sequence(xg32.to(torch.bfloat16), h0, c0, w32.to(torch.bfloat16),
                        bias32.to(torch.bfloat16), mask, reverse=False)
    h = torch.zeros(b, hd)
    c = torch.zeros(b, hd)
    outs = []
    for ti in range(t):
        gp = h @ w32.cpu().t() + xg32[ti].cpu() + bias32.cpu()
        h, c, _ = lstm_pointwise_fwd_ref(gp, c, h, mask[ti].cpu())
        outs.append(h)
    ref_out = torch.stack(outs)
    assert torch.allclose(out.float().cpu(), ref_out, atol=1e-1, rtol=1e-1)


def test_gather_mean_bwd_csr_matches_ref(gpu_device):
    from nerrf_amd.graph.sampling import reverse_index
    from nerrf_amd.ops import gather_mean

    torch.manual_seed(14)
    n, k, d = 411, 16, 128
    h = torch.randn(n, d, device=gpu_device, requires_grad=True)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    rd, rs, rw = reverse_index(idx.cpu().numpy(), w.cpu().numpy())
    rev = (
        torch.from_numpy(rd).to(gpu_device),
        torch.from_numpy(rs).to(gpu_device),
        torch.from_numpy(rw).to(gpu_device),
    )
    out = gather_mean(h, idx, w, rev)
    g = torch.randn_like(out)
    out.backward(g)
    grad_ref = ref.gather_mean_bwd_ref(g.cpu(), idx.cpu(), w.cpu(), n)
    assert torch.allclose(h.grad.cpu(), grad_ref, atol=1e-4, rtol=1e-4)


def test_gather_rows_matches_indexing(gpu_device):
    from nerrf_amd.ops import gather_rows

    torch.manual_seed(15)
    n, d, e = 200, 128, 5000
    h = torch.randn(n, d, device=gpu_device, requires_grad=True)
    idx = torch.randint(0, n, (e,), device=gpu_device)
    out = gather_rows(h, idx)
    g = torch.randn_like(out)
    out.backward(g)
    grad_fast = h.grad.clone()

    h2 = h.detach().clone().requires_grad_(True)
    out2 = h2[idx]
    assert torch.allclose(out.detach(), out2.detach())
    out2.backward(g)
    assert torch.allclose(grad_fast, h2.grad, atol=1e-3, rtol=1e-3)


def test_gpu_window_graph_matches_cpu(gpu_device):
    """GPU delta-compaction features == CPU build_graph features."""
    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.graph.constructor import build_graph
    from nerrf_amd.graph.gpu_store import gpu_window_graph

    arr, _ = generate(SynthConfig(seed=21, duration_s=45, benign_rate_hz=400, n_victim_files=12))
    g_cpu = build_graph(arr)
    g_gpu = gpu_window_graph(arr, gpu_device)
    assert g_gpu is not None
    x_gpu = g_gpu["x"].cpu().numpy()
    assert x_gpu.shape == g_cpu.x.shape
    # ms-quantised timestamps: loose tolerance on the 4 time columns
    for col in range(32):
        atol = 5e-3 if col in (15, 16, 17, 18, 19) else 1e-4
        assert np.allclose(x_gpu[:, col], g_cpu.x[:, col], atol=atol, rtol=1e-3), f"col {col}"
    assert np.array_equal(g_gpu["edge_index"].cpu().numpy(), g_cpu.edge_index)
    assert np.allclose(g_gpu["edge_weight"].cpu().numpy(), g_cpu.edge_weight, atol=1e-6)
    assert np.array_equal(g_gpu["node_kind"].cpu().numpy(), g_cpu.node_kind)


def test_gpu_proc_identity_channel(gpu_device, monkeypatch):
    """x[:, 27] (trusted-process channel, flags bit 4) CPU/GPU parity with
    the gate enabled, and all-zero with it off (default)."""
    import numpy as np

    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.graph.constructor import build_graph
    from nerrf_amd.graph.gpu_store import gpu_window_graph

    arr, _ = generate(SynthConfig(seed=22, duration_s=30, benign_rate_hz=300, n_victim_files=8))
    g_off = gpu_window_graph(arr, gpu_device)
    assert float(g_off["x"][:, 27].abs().sum()) == 0.0

    monkeypatch.setenv("NERRF_PROC_IDENTITY", "1")
    g_cpu = build_graph(arr)
    g_gpu = gpu_window_graph(arr, gpu_device)
    x27 = g_gpu["x"][:, 27].cpu().numpy()
    assert np.array_equal(x27, g_cpu.x[:, 27])
    assert x27.sum() > 0  # benign daemon comms present in the synth mix


def test_streaming_engine_gpu_scores(gpu_device):
    """Engine scoring on GPU (delta compaction + model + planner kernels)."""
    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.models.graphsage import SageConfig
    from nerrf_amd.models.joint import JointConfig, NerrfJointModel
    from nerrf_amd.models.lstm import LSTMConfig
    from nerrf_amd.serve.engine import StreamingEngine

    model = NerrfJointModel(
        JointConfig(sage=SageConfig(layers=4, hidden=128), lstm=LSTMConfig(hidden=256))
    )
    engine = StreamingEngine(model=model, device=str(gpu_device), dtype=torch.bfloat16)
    engine.store.window_s = 1e9
    arr, _ = generate(SynthConfig(seed=31, duration_s=40, benign_rate_hz=100, n_victim_files=8))
    engine.ingest_events(arr)
    det = engine.score_window()
    assert det.alarm
    assert det.window_events == len(arr)
    plan = engine.plan(det, n_sims=512, use_gpu=True)
    assert plan.simulations == 512


def test_gather_mean_max_fanout_k64(gpu_device):
    """K=64 is the wave-resident bound — exercise it exactly."""
    torch.manual_seed(40)
    n, k, d = 130, 64, 128
    h = torch.randn(n, d, device=gpu_device)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.01
    out = gather_mean(h, idx, w)
    out_ref = ref.gather_mean_ref(h.cpu(), idx.cpu(), w.cpu())
    assert torch.allclose(out.cpu(), out_ref, atol=1e-4, rtol=1e-4)


def test_gather_mean_fanout_over_64_rejected(gpu_device):
    h = torch.randn(8, 32, device=gpu_device)
    idx = torch.randint(0, 8, (8, 65), device=gpu_device)
    w = torch.rand(8, 65, device=gpu_device)
    with pytest.raises(RuntimeError):
        gather_mean(h, idx, w)


def test_mcts_search_16_groups(gpu_device):
    """Upper bound of the planner's group space (MAX_GROUPS=16)."""
    from nerrf_amd.planner.mcts import run_mcts_gpu
    from nerrf_amd.planner.rewards import PlannerParams, build_state

    rng = np.random.default_rng(3)
    st = build_state(rng.random(80), rng.random(80) * 3, 0.9, 40.0, n_groups=16)
    res = run_mcts_gpu(st, PlannerParams(n_groups=16), n_sims=512, device=str(gpu_device))
    assert res.simulations == 512
    assert len(res.ranked_actions) == 19  # STOP, KILL, RESTORE + 16 groups


def test_lstm_sequence_t1_edge(gpu_device):
    """Single-timestep sequences (boundary of the bwd two-GEMM split)."""
    from nerrf_amd.ops import lstm_sequence

    torch.manual_seed(41)
    t, b, hd = 1, 17, 32
    xg = torch.randn(t, b, 4 * hd, device=gpu_device, requires_grad=True)
    h0 = torch.randn(b, hd, device=gpu_device)
    c0 = torch.randn(b, hd, device=gpu_device)
    w_hh = (torch.randn(4 * hd, hd, device=gpu_device) * 0.2).requires_grad_(True)
    bias = torch.randn(4 * hd, device=gpu_device, requires_grad=True)
    out = lstm_sequence(xg, h0, c0, w_hh, bias, torch.ones(t, b, device=gpu_device))
    out.sum().backward()
    assert torch.isfinite(xg.grad).all()
    assert torch.isfinite(w_hh.grad).all()


def test_sage_layer_fused_matches_torch(gpu_device):
    """One fused SAGE layer == the eval-mode PyTorch layer (bf16 tolerance)."""
    from nerrf_amd.models.graphsage import SageLayer
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(50)
    n, k, d = 333, 16, 128  # non-multiple of 64 exercises the tail guards
    layer = SageLayer(d).to(gpu_device, torch.bfloat16).eval()
    h = (torch.randn(n, d, device=gpu_device) * 0.5).to(torch.bfloat16)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    out = ext.sage_layer_fwd(
        h, idx, w.to(torch.float32),
        layer.w_self.weight, layer.w_nbr.weight, layer.w_nbr.bias,
        layer.norm.weight, layer.norm.bias,
    )
    with torch.no_grad():
        ref_out = layer(h, idx, w)
    assert torch.allclose(out.float(), ref_out.float(), atol=6e-2, rtol=6e-2)


def test_sage_encode_fused_full_stack(gpu_device):
    """28 fused layers vs the module stack end-to-end."""
    from nerrf_amd.models.graphsage import GraphSAGET, SageConfig
    from nerrf_amd.ops import sage_encode_fused

    torch.manual_seed(51)
    gnn = GraphSAGET(SageConfig(dropout=0.0)).to(gpu_device, torch.bfloat16).eval()
    n, k = 500, 16
    x = (torch.randn(n, 32, device=gpu_device) * 0.5).to(torch.bfloat16)
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05
    with torch.no_grad():
        h_ref = gnn.encode(x, idx, w)
        h_fused = sage_encode_fused(gnn, x, idx, w)
    # bf16 over 28 layers: compare with generous tolerance + correlation
    ref = h_ref.float()
    fus = h_fused.float()
    denom = ref.abs().clamp_min(1.0)
    rel = ((fus - ref).abs() / denom)
    assert float(rel.mean()) < 0.05
    corr = torch.corrcoef(torch.stack([ref.flatten(), fus.flatten()]))[0, 1]
    assert float(corr) > 0.999


@pytest.mark.gpu
def test_build_sequences_torch_gpu_matches_numpy(gpu_device):
    """On-device sequence assembly (serving path) matches the numpy build."""
    import numpy as np

    from nerrf_amd.data.sequences import build_sequences, build_sequences_torch
    from nerrf_amd.data.synth import SynthConfig, generate

    arr, _ = generate(SynthConfig(duration_s=8.0, benign_rate_hz=3000.0,
                                  n_benign_files=300, seed=21))
    ref = build_sequences(arr, None)
    feats, lengths, fids = build_sequences_torch(arr, device=gpu_device)
    assert np.array_equal(lengths.numpy(), ref.lengths)
    assert np.array_equal(fids.numpy(), ref.file_path_id)
    torch.testing.assert_close(
        feats.cpu(), torch.from_numpy(ref.feats), rtol=1e-5, atol=1e-5
    )


@pytest.mark.gpu
def test_lstm_sequence_infer_matches_train_forward(gpu_device):
    """The inference fast path (gates store skipped) produces the same h."""
    from nerrf_amd.ops.lstm_seq import lstm_sequence

    torch.manual_seed(3)
    t_len, b, h = 7, 64, 256
    xg = torch.randn(t_len, b, 4 * h, device=gpu_device, dtype=torch.bfloat16)
    h0 = torch.zeros(b, h, device=gpu_device, dtype=torch.bfloat16)
    c0 = torch.zeros_like(h0)
    w = torch.randn(4 * h, h, device=gpu_device, dtype=torch.bfloat16) * 0.05
    bias = torch.randn(4 * h, device=gpu_device, dtype=torch.bfloat16) * 0.05
    wg = w.clone().requires_grad_(True)
    out_train = lstm_sequence(xg, h0, c0, wg, bias)
    with torch.no_grad():
        out_infer = lstm_sequence(xg, h0, c0, w, bias)
    torch.testing.assert_close(out_infer, out_train.detach(), rtol=0, atol=0)


@pytest.mark.gpu
def test_lstm_bilayer_gpu_matches_two_directions(gpu_device):
    """The strided dual-buffer layer matches two single-direction calls on
    the native kernels (bf16, H=256 exercises the vec + strided paths)."""
    from nerrf_amd.ops.lstm_seq import lstm_bilayer, lstm_sequence

    torch.manual_seed(19)
    t, b, h = 6, 129, 256
    dt = torch.bfloat16
    mk = (torch.rand(t, b, device=gpu_device) > 0.3).float()
    xf = (torch.randn(t, b, 4 * h, device=gpu_device, dtype=dt) * 0.3).requires_grad_(True)
    xb = (torch.randn(t, b, 4 * h, device=gpu_device, dtype=dt) * 0.3).requires_grad_(True)
    wf = (torch.randn(4 * h, h, device=gpu_device, dtype=dt) * 0.1).requires_grad_(True)
    wb = (torch.randn(4 * h, h, device=gpu_device, dtype=dt) * 0.1).requires_grad_(True)
    bf = (torch.randn(4 * h, device=gpu_device, dtype=dt) * 0.1).requires_grad_(True)
    bb = (torch.randn(4 * h, device=gpu_device, dtype=dt) * 0.1).requires_grad_(True)
    h0 = torch.zeros(b, h, device=gpu_device, dtype=dt)
    c0 = torch.zeros_like(h0)

    out = lstm_bilayer(xf, xb, h0, c0, wf, bf, wb, bb, mk)
    g = torch.randn_like(out)
    out.backward(g)
    got = [p.grad.clone() for p in (xf, xb, wf, wb, bf, bb)]
    for p in (xf, xb, wf, wb, bf, bb):
        p.grad = None

    ref = torch.cat(
        [
            lstm_sequence(xf, h0, c0, wf, bf, mk, reverse=False),
            lstm_sequence(xb, h0, c0, wb, bb, mk, reverse=True),
        ],
        dim=-1,
    )
    torch.testing.assert_close(out, ref, rtol=0, atol=0)
    ref.backward(g)
    for have, p, name in zip(got, (xf, xb, wf, wb, bf, bb),
                             ["xg_f", "xg_b", "w_f", "w_b", "b_f", "b_b"]):
        torch.testing.assert_close(have, p.grad, rtol=0, atol=0, msg=name)


def _lstm_cpu_ref_seq(xg, h0, c0, w_hh, bias, mask, rev):
    from nerrf_amd.ops.reference import lstm_pointwise_fwd_ref

    t = xg.shape[0]
    h, c = h0.cpu().float(), c0.cpu().float()
    outs = [None] * t
    steps = range(t - 1, -1, -1) if rev else range(t)
    for ti in steps:
        gp = torch.addmm(bias.cpu().float(), h, w_hh.cpu().float().t()) + xg[ti].cpu().float()
        h, c, _ = lstm_pointwise_fwd_ref(gp, c, h, mask[ti].cpu().float())
        outs[ti] = h
    return torch.stack(outs)


def test_lstm_rec_fused_fwd_matches_split_and_ref(gpu_device, monkeypatch):
    """The fused recurrent step (lstm_rec_fused.hip) vs the split
    GEMM+pointwise path and the fp32 CPU reference, H=256 bf16."""
    from nerrf_amd.ops import lstm_sequence

    torch.manual_seed(21)
    t, b, hd = 5, 200, 256  # b NOT divisible by 64: tail-block guard
    xg = (torch.randn(t, b, 4 * hd, device=gpu_device) * 0.5).to(torch.bfloat16)
    h0 = (torch.randn(b, hd, device=gpu_device) * 0.5).to(torch.bfloat16)
    c0 = (torch.randn(b, hd, device=gpu_device) * 0.5).to(torch.bfloat16)
    w_hh = ((torch.randn(4 * hd, hd, device=gpu_device)) * 0.05).to(torch.bfloat16)
    bias = torch.randn(4 * hd, device=gpu_device).to(torch.bfloat16)
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()

    for rev in (False, True):
        monkeypatch.setenv("NERRF_REC_FUSED", "1")
        out_fused = lstm_sequence(xg, h0, c0, w_hh, bias, mask, reverse=rev)
        monkeypatch.setenv("NERRF_REC_FUSED", "0")
        out_split = lstm_sequence(xg, h0, c0, w_hh, bias, mask, reverse=rev)
        ref = _lstm_cpu_ref_seq(xg, h0, c0, w_hh, bias, mask, rev)
        # fused vs split: both bf16 paths, tiny accumulation-order diff
        assert torch.allclose(out_fused.float().cpu(), out_split.float().cpu(),
                              atol=3e-2, rtol=3e-2), f"fused vs split rev={rev}"
        assert torch.allclose(out_fused.float().cpu(), ref, atol=6e-2,
                              rtol=6e-2), f"fused vs fp32 ref rev={rev}"


def test_lstm_rec_fused_backward_matches_split(gpu_device, monkeypatch):
    from nerrf_amd.ops import lstm_sequence

    torch.manual_seed(22)
    t, b, hd = 4, 130, 256
    xg32 = torch.randn(t, b, 4 * hd, device=gpu_device) * 0.5
    w32 = torch.randn(4 * hd, hd, device=gpu_device) * 0.05
    b32 = torch.randn(4 * hd, device=gpu_device) * 0.5
    mask = (torch.rand(t, b, device=gpu_device) > 0.15).float()
    h0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    c0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    g_out = torch.randn(t, b, hd, device=gpu_device).to(torch.bfloat16)

    grads = {}
    for tag in ("1", "0"):
        monkeypatch.setenv("NERRF_REC_FUSED", tag)
        xg = xg32.to(torch.bfloat16).requires_grad_(True)
        w = w32.to(torch.bfloat16).requires_grad_(True)
        bb = b32.to(torch.bfloat16).requires_grad_(True)
        out = lstm_sequence(xg, h0, c0, w, bb, mask, reverse=False)
        out.backward(g_out)
        grads[tag] = [p.grad.float().cpu() for p in (xg, w, bb)]
    for gf, gs, name in zip(grads["1"], grads["0"], ["xg", "w_hh", "bias"]):
        scale = gs.abs().max().clamp(min=1.0)
        assert torch.allclose(gf / scale, gs / scale, atol=4e-2), (
            f"grad {name}: max diff {(gf - gs).abs().max()}"
        )


def test_lstm_bilayer_rec_fused_strided_slabs(gpu_device, monkeypatch):
    """Bidirectional layer (strided [T,B,2H] slabs) through the fused
    recurrent kernels, fwd + bwd vs the split path."""
    from nerrf_amd.ops.lstm_seq import lstm_bilayer

    torch.manual_seed(23)
    t, b, hd = 6, 96, 256
    xf32 = torch.randn(t, b, 4 * hd, device=gpu_device) * 0.5
    xb32 = torch.randn(t, b, 4 * hd, device=gpu_device) * 0.5
    wf32 = torch.randn(4 * hd, hd, device=gpu_device) * 0.05
    wb32 = torch.randn(4 * hd, hd, device=gpu_device) * 0.05
    bf32 = torch.randn(4 * hd, device=gpu_device) * 0.5
    bb32 = torch.randn(4 * hd, device=gpu_device) * 0.5
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()
    h0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    c0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    g_out = torch.randn(t, b, 2 * hd, device=gpu_device).to(torch.bfloat16)

    res = {}
    for tag in ("1", "0"):
        monkeypatch.setenv("NERRF_REC_FUSED", tag)
        args = [x.to(torch.bfloat16).requires_grad_(True)
                for x in (xf32, xb32, wf32, bf32, wb32, bb32)]
        xf, xb, wf, bf, wb, bb = args
        out = lstm_bilayer(xf, xb, h0, c0, wf, bf, wb, bb, mask)
        out.backward(g_out)
        res[tag] = ([out.detach().float().cpu()] +
                    [p.grad.float().cpu() for p in args])
    names = ["out", "gxf", "gxb", "gwf", "gbf", "gwb", "gbb"]
    for a, s, name in zip(res["1"], res["0"], names):
        scale = s.abs().max().clamp(min=1.0)
        assert torch.allclose(a / scale, s / scale, atol=4e-2), (
            f"{name}: max diff {(a - s).abs().max()}"
        )


def test_rec_gemm_fwd_matches_matmul(gpu_device):
    """rec_gemm.hip NT step GEMM vs fp32 matmul, contiguous + strided rows
    + tail guard (M not a multiple of 128)."""
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(41)
    for m in (1000, 4096):
        a = (torch.randn(m, 256, device=gpu_device) * 0.3).to(torch.bfloat16)
        w = (torch.randn(1024, 256, device=gpu_device) * 0.05).to(torch.bfloat16)
        c = torch.empty(m, 1024, device=gpu_device, dtype=torch.bfloat16)
        ext.rec_gemm_fwd(a, w, c)
        ref = a.float() @ w.float().t()
        assert torch.allclose(c.float(), ref, atol=3e-2, rtol=3e-2), f"M={m}"
        # column-slab A (the recurrence reads h out of the [T,B,2H] buffer)
        slab = (torch.randn(m, 512, device=gpu_device) * 0.3).to(torch.bfloat16)
        a_s = slab[:, 256:]
        ext.rec_gemm_fwd(a_s, w, c)
        refs = a_s.float() @ w.float().t()
        assert torch.allclose(c.float(), refs, atol=3e-2, rtol=3e-2), f"M={m} strided"


def test_stream_dirs_inference_matches_sequential(gpu_device, monkeypatch):
    """Opt-in dual-stream inference (NERRF_STREAM_DIRS=1): both directions
    overlapped on a side HIP stream must produce bit-identical output to
    the sequential path."""
    from nerrf_amd.models.lstm import BiLSTMDetector, LSTMConfig

    torch.manual_seed(44)
    model = BiLSTMDetector(LSTMConfig(in_dim=32, hidden=256, layers=2)).to(
        gpu_device, torch.bfloat16
    ).eval()
    x = (torch.randn(128, 20, 32, device=gpu_device) * 0.3).to(torch.bfloat16)
    lengths = torch.full((128,), 20, device=gpu_device, dtype=torch.int64)
    with torch.no_grad():
        y_seq = model(x, lengths)
        monkeypatch.setenv("NERRF_STREAM_DIRS", "1")
        y_ovl = model(x, lengths)
        torch.cuda.synchronize()
    assert torch.equal(y_seq, y_ovl)


def test_rec_gemm_dgrad_matches_addmm(gpu_device):
    """Opt-in dgrad kernel (rec_gemm.hip): c = a @ wt^T + d vs fp32 addmm,
    with and without the addend, strided gate-slab rows, tail guard."""
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(43)
    for m in (1000, 4096):
        gg = (torch.randn(m, 1024, device=gpu_device) * 0.1).to(torch.bfloat16)
        w = (torch.randn(1024, 256, device=gpu_device) * 0.1).to(torch.bfloat16)
        wt = w.t().contiguous()
        d = (torch.randn(m, 256, device=gpu_device) * 0.1).to(torch.bfloat16)
        out = torch.empty(m, 256, device=gpu_device, dtype=torch.bfloat16)
        ext.rec_gemm_dgrad(gg, wt, d, out)
        ref = torch.addmm(d.float(), gg.float(), w.float())
        assert torch.allclose(out.float(), ref, atol=3e-2, rtol=3e-2), f"M={m}"
        # no addend + strided A (gate slab of the bilayer [T,B,2*4H] buffer)
        slab = (torch.randn(m, 2048, device=gpu_device) * 0.1).to(torch.bfloat16)
        gg_s = slab[:, 1024:]
        empty = torch.empty(0, device=gpu_device, dtype=torch.bfloat16)
        ext.rec_gemm_dgrad(gg_s, wt, empty, out)
        refs = gg_s.float() @ w.float()
        assert torch.allclose(out.float(), refs, atol=3e-2, rtol=3e-2), f"M={m} strided"


def test_rec_gemm_in_recurrence_matches_reference(gpu_device):
    """lstm_bilayer2 with NERRF_REC_GEMM=1 == reference recurrence (the
    step GEMM swap must not move training numerics)."""
    import os

    from nerrf_amd.models.lstm import BiLSTMDetector, LSTMConfig

    torch.manual_seed(42)
    t_len, batch = 12, 96
    model = BiLSTMDetector(LSTMConfig(in_dim=32, hidden=256, layers=2)).to(
        gpu_device, torch.bfloat16
    )
    x = (torch.randn(batch, t_len, 32, device=gpu_device) * 0.3).to(torch.bfloat16)
    lengths = torch.full((batch,), t_len, device=gpu_device, dtype=torch.int64)
    old = os.environ.get("NERRF_REC_GEMM")
    try:
        os.environ["NERRF_REC_GEMM"] = "1"
        y1 = model(x, lengths)
        os.environ["NERRF_REC_GEMM"] = "0"
        y0 = model(x, lengths)
    finally:
        if old is None:
            os.environ.pop("NERRF_REC_GEMM", None)
        else:
            os.environ["NERRF_REC_GEMM"] = old
    assert torch.allclose(y1.float(), y0.float(), atol=3e-2, rtol=3e-2)


def test_proj_fwd_dual_matches_matmul(gpu_device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(31)
    m = 1000  # not a multiple of 128: tail guard
    x = (torch.randn(m, 512, device=gpu_device) * 0.3).to(torch.bfloat16)
    w1 = (torch.randn(1024, 512, device=gpu_device) * 0.05).to(torch.bfloat16)
    w2 = (torch.randn(1024, 512, device=gpu_device) * 0.05).to(torch.bfloat16)
    c1 = torch.empty(m, 1024, device=gpu_device, dtype=torch.bfloat16)
    c2 = torch.empty_like(c1)
    ext.proj_fwd_dual(x, w1, w2, c1, c2)
    r1 = (x.float() @ w1.float().t())
    r2 = (x.float() @ w2.float().t())
    assert torch.allclose(c1.float(), r1, atol=3e-2, rtol=3e-2)
    assert torch.allclose(c2.float(), r2, atol=3e-2, rtol=3e-2)


def test_proj_dgrad_dual_matches_matmul(gpu_device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(32)
    m = 700
    a1 = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)
    a2 = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)
    w1 = (torch.randn(1024, 512, device=gpu_device) * 0.05).to(torch.bfloat16)
    w2 = (torch.randn(1024, 512, device=gpu_device) * 0.05).to(torch.bfloat16)
    c = torch.empty(m, 512, device=gpu_device, dtype=torch.bfloat16)
    ext.proj_dgrad_dual(a1, a2, w1.t().contiguous(), w2.t().contiguous(), c)
    ref = a1.float() @ w1.float() + a2.float() @ w2.float()
    assert torch.allclose(c.float(), ref, atol=8e-2, rtol=4e-2)


def test_dual_projection_autograd_matches_matmul(gpu_device):
    from nerrf_amd.ops.proj import dual_projection

    torch.manual_seed(33)
    m = 513
    x32 = torch.randn(m, 512, device=gpu_device) * 0.3
    wf32 = torch.randn(1024, 512, device=gpu_device) * 0.05
    wb32 = torch.randn(1024, 512, device=gpu_device) * 0.05
    gf = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)
    gb = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)

    res = {}
    for use in ("1", "0"):
        import os
        os.environ["NERRF_STREAM_PROJ"] = use
        x = x32.to(torch.bfloat16).requires_grad_(True)
        wf = wf32.to(torch.bfloat16).requires_grad_(True)
        wb = wb32.to(torch.bfloat16).requires_grad_(True)
        c1, c2 = dual_projection(x, wf, wb)
        (c1 * gf.float().to(c1.dtype)).sum().backward(retain_graph=False)
        res[use] = [c1.detach().float().cpu(), c2.detach().float().cpu(),
                    x.grad.float().cpu(), wf.grad.float().cpu()]
    os.environ["NERRF_STREAM_PROJ"] = "1"
    for a, b, name in zip(res["1"], res["0"], ["c1", "c2", "gx", "gwf"]):
        scale = b.abs().max().clamp(min=1.0)
        assert torch.allclose(a / scale, b / scale, atol=3e-2), name


def test_proj_wgrad_matches_matmul(gpu_device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(34)
    m = 5000  # exercises several m-chunks and the 32-row tail
    g1 = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)
    g2 = (torch.randn(m, 1024, device=gpu_device) * 0.3).to(torch.bfloat16)
    x = (torch.randn(m, 512, device=gpu_device) * 0.3).to(torch.bfloat16)
    dw1, dw2 = ext.proj_wgrad(g1, g2, x, 16)
    r1 = g1.float().t() @ x.float()
    r2 = g2.float().t() @ x.float()
    # f32 accumulate over bf16 products; tolerance scales with K=m
    assert torch.allclose(dw1, r1, atol=0.5, rtol=2e-2)
    assert torch.allclose(dw2, r2, atol=0.5, rtol=2e-2)


def test_lstm_bilayer2_matches_bilayer(gpu_device):
    """Single-projection-tensor bilayer (cat-GEMM layout, slab grads) vs
    the two-tensor bilayer, fwd + bwd."""
    from nerrf_amd.ops.lstm_seq import lstm_bilayer, lstm_bilayer2

    torch.manual_seed(41)
    t, b, hd = 5, 150, 256
    gd = 4 * hd
    xf32 = torch.randn(t, b, gd, device=gpu_device) * 0.4
    xb32 = torch.randn(t, b, gd, device=gpu_device) * 0.4
    wf32 = torch.randn(gd, hd, device=gpu_device) * 0.05
    wb32 = torch.randn(gd, hd, device=gpu_device) * 0.05
    bf32 = torch.randn(gd, device=gpu_device) * 0.5
    bb32 = torch.randn(gd, device=gpu_device) * 0.5
    mask = (torch.rand(t, b, device=gpu_device) > 0.2).float()
    h0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    c0 = torch.zeros(b, hd, device=gpu_device, dtype=torch.bfloat16)
    g_out = torch.randn(t, b, 2 * hd, device=gpu_device).to(torch.bfloat16)

    # two-tensor path
    xf = xf32.to(torch.bfloat16).requires_grad_(True)
    xb = xb32.to(torch.bfloat16).requires_grad_(True)
    wf = wf32.to(torch.bfloat16).requires_grad_(True)
    wb = wb32.to(torch.bfloat16).requires_grad_(True)
    bf = bf32.to(torch.bfloat16).requires_grad_(True)
    bb = bb32.to(torch.bfloat16).requires_grad_(True)
    out_a = lstm_bilayer(xf, xb, h0, c0, wf, bf, wb, bb, mask)
    out_a.backward(g_out)

    # single-tensor path
    xg2 = torch.cat([xf32, xb32], dim=-1).to(torch.bfloat16).requires_grad_(True)
    wf2 = wf32.to(torch.bfloat16).requires_grad_(True)
    wb2 = wb32.to(torch.bfloat16).requires_grad_(True)
    bf2 = bf32.to(torch.bfloat16).requires_grad_(True)
    bb2 = bb32.to(torch.bfloat16).requires_grad_(True)
    out_b = lstm_bilayer2(xg2, h0, c0, wf2, bf2, wb2, bb2, mask)
    out_b.backward(g_out)

    assert torch.allclose(out_a.float(), out_b.float(), atol=1e-5)
    gx2 = torch.cat([xf.grad, xb.grad], dim=-1).float()
    assert torch.allclose(gx2, xg2.grad.float(), atol=1e-5)
    for a, c, name in ((wf.grad, wf2.grad, "wf"), (wb.grad, wb2.grad, "wb"),
                       (bf.grad, bf2.grad, "bf"), (bb.grad, bb2.grad, "bb")):
        assert torch.allclose(a.float(), c.float(), atol=1e-5), name


def test_lstm_bilayer2_inference_matches_cpu_reference(gpu_device):
    """The serving hot path: lstm_bilayer2 under no_grad with default flags
    (fused recurrent step, null gates pointer, xg slabs of row stride 2*4H,
    h slabs of row stride 2H) vs the fp32 CPU loop per direction.  B is a
    multiple of neither 64 nor 128; lengths include 1 and T; h0/c0 non-zero.
    Tolerance: that of test_lstm_rec_fused_fwd_matches_split_and_ref, the
    same kernel against the same reference at the same T."""
    from nerrf_amd.ops.lstm_seq import lstm_bilayer2

    torch.manual_seed(47)
    t, b, hd = 5, 130, 256
    gd = 4 * hd
    dt = torch.bfloat16
    xg2 = (torch.randn(t, b, 2 * gd, device=gpu_device) * 0.5).to(dt)
    h0 = (torch.randn(b, hd, device=gpu_device) * 0.5).to(dt)
    c0 = (torch.randn(b, hd, device=gpu_device) * 0.5).to(dt)
    w_f = (torch.randn(gd, hd, device=gpu_device) * 0.05).to(dt)
    w_b = (torch.randn(gd, hd, device=gpu_device) * 0.05).to(dt)
    b_f = torch.randn(gd, device=gpu_device).to(dt)
    b_b = torch.randn(gd, device=gpu_device).to(dt)
    lengths = torch.randint(1, t + 1, (b,), device=gpu_device)
    lengths[0], lengths[1] = 1, t
    mask = (torch.arange(t, device=gpu_device).unsqueeze(1)
            < lengths.unsqueeze(0)).float()  # [T, B]

    with torch.no_grad():
        out = lstm_bilayer2(xg2, h0, c0, w_f, b_f, w_b, b_b, mask)
    ref_out = torch.cat(
        [
            _lstm_cpu_ref_seq(xg2[:, :, :gd], h0, c0, w_f, b_f, mask, False),
            _lstm_cpu_ref_seq(xg2[:, :, gd:], h0, c0, w_b, b_b, mask, True),
        ],
        dim=-1,
    )
    assert out.shape == (t, b, 2 * hd)
    assert torch.allclose(out.float().cpu(), ref_out, atol=6e-2, rtol=6e-2), (
        f"max diff {(out.float().cpu() - ref_out).abs().max()}"
    )


def test_engine_device_delta_ring_matches_host_path(gpu_device):
    """Scoring with the HBM-resident delta ring (per-delta device columns,
    device-side window cat) must match the host-upload path exactly, and
    the cache must stay bounded across eviction."""
    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.models.graphsage import SageConfig
    from nerrf_amd.models.joint import JointConfig, NerrfJointModel
    from nerrf_amd.models.lstm import LSTMConfig
    from nerrf_amd.serve.engine import StreamingEngine

    torch.manual_seed(5)
    model = NerrfJointModel(JointConfig(sage=SageConfig(layers=3, hidden=64),
                                        lstm=LSTMConfig(hidden=256)))
    arr, _ = generate(SynthConfig(seed=4, duration_s=40, benign_rate_hz=200,
                                  n_victim_files=8))

    def run(use_ring):
        eng = StreamingEngine(model=model, device=gpu_device,
                              dtype=torch.bfloat16, window_s=1e9)
        if not use_ring:
            eng.store.device_columns = lambda *a, **k: None
        eng.ingest_events(arr)
        det = eng.score_window()
        return det, eng

    det_ring, eng_ring = run(True)
    det_host, _ = run(False)
    assert det_ring.alarm == det_host.alarm
    assert det_ring.window_events == det_host.window_events
    for p, s in det_host.file_scores.items():
        assert abs(det_ring.file_scores[p] - s) < 1e-3, p
    # cache reuse + boundedness: more ticks than deltas
    eng2 = StreamingEngine(model=model, device=gpu_device,
                           dtype=torch.bfloat16, window_s=8.0)
    t0 = float(arr.ts.min())
    for k in range(6):
        lo = arr.ts < t0 + 6 * (k + 1)
        hi = arr.ts >= t0 + 6 * k
        seg = arr.time_window(t0 + 6 * k, t0 + 6 * (k + 1) - 1e-9)
        if len(seg):
            eng2.ingest_events(seg)
        eng2.score_window()
    assert len(eng2.store._dev_cache) <= len(eng2.store._deltas) + 1


def test_sage_ln_act_matches_eager(gpu_device):
    """Fused training-layer tail vs eager torch, fwd + grads (dropout 0)."""
    from nerrf_amd.ops.sage_tail import _SageTailFn

    torch.manual_seed(51)
    n = 1000
    h32 = torch.randn(n, 128, device=gpu_device) * 0.5
    zs32 = torch.randn(n, 128, device=gpu_device) * 0.5
    zn32 = torch.randn(n, 128, device=gpu_device) * 0.5
    g32 = torch.rand(128, device=gpu_device) + 0.5
    b32 = torch.randn(128, device=gpu_device) * 0.1
    dy = (torch.randn(n, 128, device=gpu_device) * 0.3).to(torch.bfloat16)

    h = h32.to(torch.bfloat16).requires_grad_(True)
    zs = zs32.to(torch.bfloat16).requires_grad_(True)
    zn = zn32.to(torch.bfloat16).requires_grad_(True)
    g = g32.to(torch.bfloat16).requires_grad_(True)
    b = b32.to(torch.bfloat16).requires_grad_(True)
    y = _SageTailFn.apply(h, zs, zn, g, b, 0.0, 7)
    y.backward(dy)

    import torch.nn.functional as F
    h2 = h32.to(torch.bfloat16).requires_grad_(True)
    zs2 = zs32.to(torch.bfloat16).requires_grad_(True)
    zn2 = zn32.to(torch.bfloat16).requires_grad_(True)
    g2 = g32.to(torch.bfloat16).requires_grad_(True)
    b2 = b32.to(torch.bfloat16).requires_grad_(True)
    y2 = h2 + F.layer_norm(F.gelu(zs2 + zn2), (128,), g2, b2, 1e-5)
    y2.backward(dy)

    assert torch.allclose(y.float(), y2.float(), atol=3e-2, rtol=3e-2)
    for a, c, name in ((h.grad, h2.grad, "dh"), (zs.grad, zs2.grad, "dzs"),
                       (zn.grad, zn2.grad, "dzn"), (g.grad, g2.grad, "dgamma"),
                       (b.grad, b2.grad, "dbeta")):
        scale = c.float().abs().max().clamp(min=1.0)
        assert torch.allclose(a.float() / scale, c.float() / scale,
                              atol=4e-2), f"{name}: {(a.float()-c.float()).abs().max()}"


def test_sage_ln_act_dropout_mask_consistency(gpu_device):
    """Dropout path: the debug mask reproduces the forward, the keep rate is
    ~1-p, and backward replays the same mask (zero grad where dropped)."""
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(52)
    n, p, seed = 2000, 0.3, 99
    h = torch.zeros(n, 128, device=gpu_device, dtype=torch.bfloat16)
    zs = (torch.randn(n, 128, device=gpu_device) * 0.5).to(torch.bfloat16)
    zn = (torch.randn(n, 128, device=gpu_device) * 0.5).to(torch.bfloat16)
    g = torch.ones(128, device=gpu_device, dtype=torch.bfloat16)
    b = torch.zeros(128, device=gpu_device, dtype=torch.bfloat16)
    y, s_save, stats, mask = ext.sage_ln_act_fwd(h, zs, zn, g, b, p, seed, True)
    keep = mask.float().mean().item()
    assert abs(keep - (1 - p)) < 0.02
    # reference with the extracted mask
    import torch.nn.functional as F
    x = F.gelu((zs + zn).float()) * mask.float() / (1 - p)
    ref = F.layer_norm(x, (128,))
    assert torch.allclose(y.float(), ref, atol=3e-2, rtol=3e-2)
    # backward replays the same mask: dz == 0 exactly where dropped
    dy = torch.ones(n, 128, device=gpu_device, dtype=torch.bfloat16)
    dz, _, _ = ext.sage_ln_act_bwd(dy, s_save, stats, g, p, seed)
    dropped = mask == 0
    assert (dz.float()[dropped] == 0).all()


def test_sage_layer_training_fused_matches_eager_path(gpu_device):
    """Full SageLayer on GPU bf16 (fused tail) vs the eager composition."""
    from nerrf_amd.models.graphsage import SageLayer

    torch.manual_seed(53)
    layer = SageLayer(128, dropout=0.0).to(gpu_device, torch.bfloat16)
    n, k = 700, 16
    h32 = torch.randn(n, 128, device=gpu_device) * 0.5
    idx = torch.randint(0, n, (n, k), device=gpu_device)
    w = torch.rand(n, k, device=gpu_device) + 0.05

    h = h32.to(torch.bfloat16).requires_grad_(True)
    out = layer(h, idx, w)
    out.sum().backward()
    gf = h.grad.float().clone()

    import torch.nn.functional as F
    from nerrf_amd.ops import gather_mean
    h2 = h32.to(torch.bfloat16).requires_grad_(True)
    agg = gather_mean(h2, idx, w)
    z = F.gelu(layer.w_self(h2) + layer.w_nbr(agg))
    out2 = h2 + layer.norm(z)
    out2.sum().backward()
    assert torch.allclose(out.float(), out2.float(), atol=3e-2, rtol=3e-2)
    scale = h2.grad.float().abs().max().clamp(min=1.0)
    assert torch.allclose(gf / scale, h2.grad.float() / scale, atol=4e-2)


def test_lstm_bwd_fused_bias_accum_matches_sum(gpu_device):
    """The in-kernel bias-grad accumulation equals gg.sum(0)."""
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    torch.manual_seed(61)
    b, hd = 3000, 256
    g = 4 * hd
    gh = (torch.randn(b, hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    gout = (torch.randn(b, hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    gc = (torch.randn(b, hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    gacts = torch.sigmoid(torch.randn(b, g, device=gpu_device)).to(torch.bfloat16)
    c = (torch.randn(b, hd, device=gpu_device) * 0.2).to(torch.bfloat16)
    mask = (torch.rand(b, device=gpu_device) > 0.2).float()
    gg = torch.empty(b, g, device=gpu_device, dtype=torch.bfloat16)
    gcp = torch.empty(b, hd, device=gpu_device, dtype=torch.bfloat16)
    ghp = torch.empty_like(gcp)
    accum = torch.zeros(64, g, device=gpu_device, dtype=torch.float32)
    used = ext.lstm_pointwise_bwd(gh, gout, gc, gacts, c, mask, gg, gcp, ghp, accum)
    assert used
    ref = gg.float().sum(0)
    assert torch.allclose(accum.sum(0), ref, atol=0.5, rtol=1e-2)
    # accumulates ACROSS calls (the sequence loop reuses one accumulator)
    ext.lstm_pointwise_bwd(gh, gout, gc, gacts, c, mask, gg, gcp, ghp, accum)
    assert torch.allclose(accum.sum(0), 2 * ref, atol=1.0, rtol=1e-2)


def test_sample_fanout_torch_structural(gpu_device):
    """Device-side fanout sampler: every drawn neighbor is a valid CSR
    in-neighbor with its edge weight; isolated nodes self-fill."""
    import numpy as np

    from nerrf_amd.graph.sampling import sample_fanout_torch, to_csr

    rng = np.random.default_rng(9)
    n, e = 500, 3000
    ei = np.stack([rng.integers(0, n - 5, e), rng.integers(0, n - 5, e)]).astype(np.int64)
    ew = rng.random(e).astype(np.float32) + 0.01
    t_ei = torch.from_numpy(ei).to(gpu_device)
    t_ew = torch.from_numpy(ew).to(gpu_device)
    idx, w = sample_fanout_torch(t_ei, t_ew, n, 16, seed=3)
    assert idx.shape == (n, 16) and w.shape == (n, 16)
    csr = to_csr(ei, n, ew)
    idx_np = idx.cpu().numpy()
    w_np = w.float().cpu().numpy()
    deg = np.diff(csr.indptr)
    for node in list(range(0, n, 37)) + [n - 1]:
        nbrs = set(csr.indices[csr.indptr[node]:csr.indptr[node + 1]].tolist())
        wmap = {}
        for j, nb in enumerate(csr.indices[csr.indptr[node]:csr.indptr[node + 1]]):
            wmap.setdefault(int(nb), set()).add(round(float(csr.weights[csr.indptr[node] + j]), 5))
        if deg[node] == 0:
            assert (idx_np[node] == node).all() and (w_np[node] == 1.0).all()
        else:
            for nb, wv in zip(idx_np[node], w_np[node]):
                assert int(nb) in nbrs
                assert round(float(wv), 5) in wmap[int(nb)]
