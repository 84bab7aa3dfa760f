"""Fused edge-head kernel (ops/hip/edge_head.hip) and per-edge scores in the
GPU serving engine.

Kernel parity is measured against an fp64 reference that takes the bf16
operands upcast and keeps the 258 features unrounded.  The kernel rounds less
often than the eager bf16 head (features once, nothing after the MFMA), so
the yardstick is the eager bf16 head's own error against that reference:
mean error no larger, maximum within 2x (a maximum over a few hundred samples
is noisy).  An fp32 CPU emulation of the kernel's rounding gives mean 0.0007 /
max 0.0032 at E = 333 against 0.0015 / 0.0054 for the eager head; measured on
an MI355X: kernel 0.00073 / 0.0026, eager head 0.0018 / 0.0089
(profiles/PROFILES.md, "Fused edge head").
"""
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

N_NODES = 97
E_BIG = 333
E_SMALL = (1, 64, 65)  # one row, an exact tile, a tile plus one row
CKPT = Path(__file__).resolve().parents[1] / "checkpoints" / "pretrained"


def _fp64_reference(h, ei, ew, ets, head):
    hd = h.double()
    hs, ht = hd[ei[0]], hd[ei[1]]
    feat = torch.cat([hs * ht, (hs - ht).abs(), ew.double()[:, None], ets.double()[:, None]], -1)
    z = feat @ head[0].weight.double().t() + head[0].bias.double()
    z = 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    return (z @ head[2].weight.double().t() + head[2].bias.double()).squeeze(-1)


@pytest.fixture(scope="module")
def parity(gpu_device):
    """Inputs, kernel logits, eager bf16 logits and fp64 reference per E."""
    from nerrf_amd.models.graphsage import GraphSAGET, SageConfig
    from nerrf_amd.ops import edge_head_logits
    from nerrf_amd.ops.reference import edge_head_ref

    torch.manual_seed(0)
    head = GraphSAGET(SageConfig(layers=1)).edge_head.to(gpu_device, torch.bfloat16).eval()
    g = torch.Generator().manual_seed(1)
    h = (torch.randn(N_NODES, 128, generator=g) * 1.5).to(gpu_device, torch.bfloat16)
    cases = {}
    with torch.no_grad():
        for e in (E_BIG,) + E_SMALL:
            ei = torch.randint(0, N_NODES, (2, e), generator=g)
            if e >= 3:
                ei[1, 0] = ei[0, 0]  # self-loop: the difference half is 0
                ei[:, 2] = ei[:, 1]  # duplicated edge
            ei = ei.to(gpu_device)
            ew = torch.rand(e, generator=g) * 3
            ets = torch.rand(e, generator=g)
            if e >= 3:
                ew[2], ets[2] = ew[1], ets[1]
            ew, ets = ew.to(gpu_device), ets.to(gpu_device)
            out = edge_head_logits(h, ei, ew, ets, head)
            eager = edge_head_ref(h, ei, ew, ets, head)
            ref = _fp64_reference(h, ei, ew, ets, head)
            torch.cuda.synchronize()
            cases[e] = dict(ei=ei, ew=ew, ets=ets, out=out, eager=eager, ref=ref)
    return dict(h=h, head=head, cases=cases)


def _errors(case):
    k = (case["out"].double() - case["ref"]).abs()
    e = (case["eager"].double() - case["ref"]).abs()
    return k, e


def test_kernel_is_taken_and_returns_fp32(parity):
    for e, case in parity["cases"].items():
        assert case["out"].dtype == torch.float32, e  # the reference path returns bf16
        assert case["out"].shape == (e,)
        assert case["eager"].dtype == torch.bfloat16
        assert torch.isfinite(case["out"]).all()


def test_kernel_parity_several_tiles(parity):
    case = parity["cases"][E_BIG]
    k, e = _errors(case)
    print(f"E={E_BIG}: kernel mean {k.mean():.6f} max {k.max():.6f} | "
          f"eager bf16 mean {e.mean():.6f} max {e.max():.6f} | "
          f"logit range [{case['ref'].min():.3f}, {case['ref'].max():.3f}]")
    assert k.mean() <= e.mean()
    assert k.max() <= 2.0 * e.max()
    # self-loop and duplicated edge
    assert case["out"][1] == case["out"][2]


@pytest.mark.parametrize("e", E_SMALL)
def test_kernel_parity_small(parity, e):
    _, e_big = _errors(parity["cases"][E_BIG])
    bound = 2.0 * e_big.max()
    k, _ = _errors(parity["cases"][e])
    print(f"E={e}: kernel max {k.max():.6f} (bound {bound:.6f})")
    assert (k <= bound).all()


def test_empty_edge_list(parity, gpu_device):
    from nerrf_amd.ops import edge_head_logits

    h, head = parity["h"], parity["head"]
    ei = torch.zeros(2, 0, dtype=torch.int64, device=gpu_device)
    none = torch.zeros(0, device=gpu_device)
    with torch.no_grad():
        out = edge_head_logits(h, ei, none, none, head)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (0,)


def test_binding_rejects_contract_violations(parity):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    h, head = parity["h"], parity["head"]
    case = parity["cases"][64]
    w1 = head[0].weight.detach()
    args = [h, case["ei"][0].contiguous(), case["ei"][1].contiguous(), case["ew"], case["ets"],
            w1[:, :256].contiguous(), w1[:, 256:].float().contiguous(),
            head[0].bias.detach(), head[2].weight.detach().reshape(-1), head[2].bias.detach()]
    assert torch.equal(ext.edge_head_fwd(*args), case["out"])
    for pos, bad in ((0, h.float()), (0, h[:, :64].contiguous()),
                     (1, args[1].int()), (3, case["ew"].bfloat16()),
                     (5, w1[:, :256]), (4, case["ets"][:-1].contiguous())):
        broken = list(args)
        broken[pos] = bad
        with pytest.raises(RuntimeError):
            ext.edge_head_fwd(*broken)


# ----------------------------------------------------------------- engine


def _engine_detection(device, dtype, top_edges):
    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.serve.engine import StreamingEngine, load_model_from_checkpoint

    arr, _ = generate(SynthConfig(seed=77, duration_s=40, benign_rate_hz=60, n_victim_files=10))
    eng = StreamingEngine(model=load_model_from_checkpoint(str(CKPT)), device=device,
                          dtype=dtype, top_edges=top_edges)
    eng.store.window_s = 1e9
    eng.ingest_events(arr)
    return eng.score_window()


@pytest.fixture(scope="module")
def gpu_det32(gpu_device):
    return _engine_detection(str(gpu_device), torch.bfloat16, 32)


def test_engine_gpu_names_the_same_edges_as_cpu(gpu_det32):
    cpu = _engine_detection("cpu", torch.float32, 32)

    def hot(det):
        return {(h.proc, h.path, h.direction) for h in det.top_edges if h.score > 0.5}

    best_cold = max((h.score for h in gpu_det32.top_edges if h.score <= 0.5), default=None)
    print(f"gpu bf16: {len(hot(gpu_det32))} edges > 0.5, edge_max {gpu_det32.edge_max:.4f}, "
          f"best edge <= 0.5: {best_cold} | cpu fp32: {len(hot(cpu))} edges > 0.5")
    assert len(hot(cpu)) >= 10
    assert hot(gpu_det32) == hot(cpu)
    scores = [h.score for h in gpu_det32.top_edges]
    assert scores == sorted(scores, reverse=True)
    assert gpu_det32.edge_max == scores[0]


def test_engine_gpu_edge_scoring_leaves_other_heads_alone(gpu_det32, gpu_device):
    det0 = _engine_detection(str(gpu_device), torch.bfloat16, 0)
    assert det0.top_edges == [] and det0.edge_max == 0.0
    assert det0.node_max == gpu_det32.node_max
    assert det0.seq_max == gpu_det32.seq_max
