"""Per-edge anomaly scores on the CPU path: NerrfJointModel.score,
ops.reference.edge_head_ref, Detection.top_edges / edge_max, the registry
record and merge_detections."""
from pathlib import Path

import pytest
import torch

from nerrf_amd.data.synth import SynthConfig, generate
from nerrf_amd.models.graphsage import GraphSAGET, SageConfig
from nerrf_amd.models.joint import JointConfig, NerrfJointModel
from nerrf_amd.models.lstm import LSTMConfig

CKPT = Path(__file__).resolve().parents[1] / "checkpoints" / "pretrained"
TOP_K = 32


def _small_batch(model, n=30, k=4, e=40, b=5, t=12):
    g = torch.Generator().manual_seed(0)
    return {
        "x": torch.randn(n, model.cfg.sage.in_dim, generator=g),
        "nbr_idx": torch.randint(0, n, (n, k), generator=g),
        "nbr_w": torch.rand(n, k, generator=g),
        "edge_index": torch.randint(0, n, (2, e), generator=g),
        "edge_weight": torch.rand(e, generator=g),
        "edge_ts": torch.rand(e, generator=g),
        "seq_feats": torch.randn(b, t, model.cfg.lstm.in_dim, generator=g),
        "seq_lengths": torch.randint(1, t, (b,), generator=g),
    }


def test_score_equals_forward_cpu_fp32():
    torch.manual_seed(0)
    model = NerrfJointModel(
        JointConfig(sage=SageConfig(layers=3, hidden=32), lstm=LSTMConfig(hidden=24))
    ).eval()
    batch = _small_batch(model)
    with torch.no_grad():
        n_f, e_f, s_f = model(batch)
    n_s, e_s, s_s = model.score(batch)
    assert torch.equal(n_s, n_f)
    assert torch.equal(e_s, e_f)
    assert torch.equal(s_s, s_f)
    assert not e_s.requires_grad
    # defaults (weight ones, ts zeros) match forward's too
    bare = {k: v for k, v in batch.items() if k not in ("edge_weight", "edge_ts")}
    with torch.no_grad():
        _, e_f2, _ = model(bare)
    assert torch.equal(model.score(bare)[1], e_f2)
    # edges=False skips the head, nothing else
    n_0, e_0, s_0 = model.score(batch, edges=False)
    assert e_0 is None and torch.equal(n_0, n_f) and torch.equal(s_0, s_f)


def test_edge_head_ref_equals_module_branch():
    from nerrf_amd.ops import edge_head_logits
    from nerrf_amd.ops.reference import edge_head_ref

    torch.manual_seed(1)
    gnn = GraphSAGET(SageConfig(layers=2)).eval()
    n, k, e = 23, 4, 57
    x = torch.randn(n, gnn.cfg.in_dim)
    idx = torch.randint(0, n, (n, k))
    w = torch.rand(n, k)
    ei = torch.randint(0, n, (2, e))
    ew, ets = torch.rand(e) * 3, torch.rand(e)
    with torch.no_grad():
        _, el = gnn(x, idx, w, ei, ew, ets)
        h = gnn.encode(x, idx, w)
        assert torch.equal(edge_head_ref(h, ei, ew, ets, gnn.edge_head), el)
        # CPU dispatch of the public op and of the model method is the reference
        assert torch.equal(edge_head_logits(h, ei, ew, ets, gnn.edge_head), el)
        assert torch.equal(gnn.score_edges(h, ei, ew, ets), el)


@pytest.fixture(scope="module")
def seed77():
    arr, _ = generate(SynthConfig(seed=77, duration_s=40, benign_rate_hz=60, n_victim_files=10))
    return arr


def _detect(arr, top_edges):
    from nerrf_amd.serve.engine import StreamingEngine, load_model_from_checkpoint

    assert (CKPT / "checkpoint.json").exists(), "vendored checkpoint missing"
    eng = StreamingEngine(model=load_model_from_checkpoint(str(CKPT)), device="cpu",
                          top_edges=top_edges)
    eng.store.window_s = 1e9
    eng.ingest_events(arr)
    return eng, eng.score_window()


@pytest.fixture(scope="module")
def det32(seed77):
    return _detect(seed77, TOP_K)


def test_detection_top_edges_pretrained(det32, seed77):
    from nerrf_amd.graph.constructor import build_edges_and_flags, build_graph_parts
    from nerrf_amd.serve.engine import EdgeHit

    _eng, det = det32
    n_edges = build_edges_and_flags(build_graph_parts(seed77))["edge_index"].shape[1]
    hits = det.top_edges
    assert len(hits) == min(TOP_K, n_edges)
    assert all(isinstance(h, EdgeHit) for h in hits)
    scores = [h.score for h in hits]
    assert scores == sorted(scores, reverse=True)
    assert all(h.direction in ("read", "write") for h in hits)
    assert all(h.proc in det.proc_scores and h.path in det.file_scores for h in hits)
    hot = [h for h in hits if h.score > 0.5]
    print("hits > 0.5:", len(hot), "edge_max:", det.edge_max,
          "best benign:", max((h.score for h in hits if h.score <= 0.5), default=None))
    assert all(h.path.startswith("/app/uploads/") for h in hot)
    assert len(hot) >= 10
    # ... and names the attacking process: the one the node head ranks first
    assert {h.proc for h in hot} == {max(det.proc_scores, key=det.proc_scores.get)}
    assert det.edge_max > 0.9
    assert det.edge_max == hits[0].score


def test_top_edges_zero_changes_nothing_else(det32, seed77):
    _eng, det = det32
    _eng0, det0 = _detect(seed77, 0)
    assert det0.top_edges == [] and det0.edge_max == 0.0
    assert det0.file_scores == det.file_scores
    assert det0.proc_scores == det.proc_scores
    assert det0.node_max == det.node_max
    assert det0.seq_max == det.seq_max
    assert det0.alarm == det.alarm


def test_registry_roundtrip_and_world1_merge(det32, tmp_path):
    from nerrf_amd.serve.registry import DetectionRegistry

    eng, det = det32
    assert det.top_edges
    reg = DetectionRegistry(str(tmp_path / "st"))
    rec = reg.load(reg.record(det))
    assert rec["top_edges"] == [h.as_dict() for h in det.top_edges]
    assert rec["edge_max"] == det.edge_max
    first = rec["top_edges"][0]
    assert set(first) == {"proc", "path", "direction", "score", "weight"}
    # `nerrf status` lists the first few hits of each detection
    listed = reg.list()[0]["top_edges"]
    assert 0 < len(listed) <= len(rec["top_edges"]) and listed[0] == first

    merged = eng.merge_detections(det)
    assert merged.top_edges == det.top_edges
    assert merged.edge_max == det.edge_max


def _worker_merge_edges(rank, world, port, results):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nerrf_amd.serve.engine import StreamingEngine

        torch.manual_seed(rank)
        model = NerrfJointModel(
            JointConfig(sage=SageConfig(layers=2, hidden=24), lstm=LSTMConfig(hidden=16))
        )
        eng = StreamingEngine(model=model, device="cpu", top_edges=8)
        eng.store.window_s = 1e9
        arr, _ = generate(SynthConfig(seed=40 + rank, duration_s=25, benign_rate_hz=40))
        eng.ingest_events(arr)
        det = eng.score_window()
        merged = eng.merge_detections(det)
        results[rank] = {
            "local": [h.as_dict() for h in det.top_edges],
            "merged": [h.as_dict() for h in merged.top_edges],
            "edge_max": merged.edge_max,
        }
    finally:
        dist.destroy_process_group()


def test_merge_detections_keeps_global_top_k():
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    results = mp.Manager().dict()
    mp.spawn(_worker_merge_edges, args=(2, port, results), nprocs=2, join=True)
    union = sorted(results[0]["local"] + results[1]["local"], key=lambda h: -h["score"])
    assert len(results[0]["local"]) == len(results[1]["local"]) == 8
    for rank in (0, 1):
        assert results[rank]["merged"] == union[:8]
        assert results[rank]["edge_max"] == union[0]["score"]
