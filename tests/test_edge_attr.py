"""Per-file attribution on the CPU path: ops.reference.edge_attribution_ref on
hand-made edge lists, Detection.file_culprit / culprits / contested from the
engine, the registry record, merge_detections and per-culprit planning."""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch

from nerrf_amd.data.synth import SynthConfig, generate

CKPT = Path(__file__).resolve().parents[1] / "checkpoints" / "pretrained"
INF = float("inf")
NAN = float("nan")

# Hand-made graphs: file nodes 0..4, process nodes 5, 6, 7.
N_FILES, N_NODES = 5, 8
NONE = (-1, -INF, 0)  # a file with no edge of the wanted direction


def _case(edges, direction, expected, thr=0.0):
    """edges: (src, dst, logit); expected: {file: (culprit, best_logit, n_hot)},
    every other file NONE."""
    return dict(edges=edges, direction=direction, thr=thr,
                expected=[expected.get(f, NONE) for f in range(N_FILES)])


HAND_CASES = {
    # (a) two writers of file 0 with different logits
    "a_two_writers": _case([(5, 0, 1.0), (6, 0, 2.0)], "write", {0: (6, 2.0, 2)}),
    # (b) equal logits: the lower process node index wins
    "b_tie_lowest_index": _case(
        [(6, 1, 0.5), (5, 1, 0.5), (7, 1, 0.5)], "write", {1: (5, 0.5, 3)}),
    # (c) +0.0 from process 6 against -0.0 from process 5: equal, so 5 wins;
    # the winner's value is +0.0 and both edges are hot at thr_logit = 0
    "c_signed_zero": _case([(6, 2, 0.0), (5, 2, -0.0)], "write", {2: (5, 0.0, 2)}),
    # (d) file 3 has only a read edge
    "d_read_edge_under_write": _case([(3, 5, 1.5)], "write", {}),
    "d_read_edge_under_read": _case([(3, 5, 1.5)], "read", {3: (5, 1.5, 1)}),
    # (e) NaN is skipped; -inf wins a file that has nothing else, not hot;
    # +inf wins; a file with only a NaN edge has no edge
    "e_non_finite": _case(
        [(5, 0, NAN), (6, 0, -1.0), (5, 1, -INF), (6, 2, 3.0), (5, 2, INF), (7, 2, NAN),
         (7, 3, NAN)],
        "write", {0: (6, -1.0, 0), 1: (5, -INF, 0), 2: (5, INF, 2)}),
    # (f) file->file, proc->proc, an index equal to n_nodes, index -1: skipped
    "f_bad_edges": _case(
        [(0, 1, 5.0), (5, 6, 5.0), (8, 0, 5.0), (5, 8, 5.0), (-1, 0, 5.0), (5, -1, 5.0),
         (7, 4, 1.0)],
        "write", {4: (7, 1.0, 1)}),
    # (g) all logits negative: winners still right, nothing hot
    "g_all_negative": _case(
        [(5, 0, -2.0), (6, 0, -1.0), (7, 1, -3.0)], "write",
        {0: (6, -1.0, 0), 1: (7, -3.0, 0)}),
    # a threshold other than 0: hot means logit >= thr_logit
    "thr_one": _case(
        [(5, 0, 1.0), (6, 0, 0.5), (7, 0, 2.0)], "write", {0: (7, 2.0, 2)}, thr=1.0),
}


def case_tensors(case, device="cpu"):
    e = case["edges"]
    logit = torch.tensor([x[2] for x in e], dtype=torch.float32, device=device)
    ei = torch.tensor([[x[0] for x in e], [x[1] for x in e]], dtype=torch.int64,
                      device=device).reshape(2, len(e))
    return logit, ei


def expected_tensors(case, device="cpu"):
    exp = case["expected"]
    return (torch.tensor([x[0] for x in exp], dtype=torch.int64, device=device),
            torch.tensor([x[1] for x in exp], dtype=torch.float32, device=device),
            torch.tensor([x[2] for x in exp], dtype=torch.int32, device=device))


def assert_triple_equal(got, want):
    for g, w, name in zip(got, want, ("culprit", "best_logit", "n_hot")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), (name, g, w)


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_reference_hand_made(name):
    from nerrf_amd.ops import edge_attribution
    from nerrf_amd.ops.reference import edge_attribution_ref

    case = HAND_CASES[name]
    logit, ei = case_tensors(case)
    got = edge_attribution_ref(logit, ei, N_FILES, N_NODES, case["direction"], case["thr"])
    assert_triple_equal(got, expected_tensors(case))
    assert not torch.signbit(got[1][got[1] == 0]).any()  # -0.0 never comes back
    # the CPU dispatch of the public op is the reference
    assert_triple_equal(
        edge_attribution(logit, ei, N_FILES, N_NODES, case["direction"], case["thr"]), got)


def test_reference_empty_inputs():
    from nerrf_amd.ops.reference import edge_attribution_ref

    none = torch.zeros(0)
    no_edges = torch.zeros(2, 0, dtype=torch.int64)
    c, b, h = edge_attribution_ref(none, no_edges, N_FILES, N_NODES)
    assert_triple_equal((c, b, h), expected_tensors(_case([], "write", {})))
    # no file nodes: three empty outputs, with or without edges
    for logit, ei in ((none, no_edges),
                      (torch.ones(2), torch.tensor([[0, 1], [1, 2]]))):
        c, b, h = edge_attribution_ref(logit, ei, 0, 3)
        assert c.shape == b.shape == h.shape == (0,)
        assert (c.dtype, b.dtype, h.dtype) == (torch.int64, torch.float32, torch.int32)


def test_direction_is_checked():
    from nerrf_amd.ops import edge_attribution
    from nerrf_amd.ops.reference import edge_attribution_ref

    logit, ei = case_tensors(HAND_CASES["a_two_writers"])
    for fn in (edge_attribution, edge_attribution_ref):
        with pytest.raises(ValueError):
            fn(logit, ei, N_FILES, N_NODES, "both")


# ----------------------------------------------------------------- engine

VICTIMS = {f"/app/uploads/doc_{i:04d}.dat" for i in range(10)} | {
    "/app/uploads/README_LOCKBIT.txt"}
ATTACKER = 6666


@pytest.fixture(scope="module")
def seed77():
    arr, _ = generate(SynthConfig(seed=77, duration_s=40, benign_rate_hz=60, n_victim_files=10))
    return arr


def _detect(arr, **kw):
    from nerrf_amd.planner.rewards import PlannerParams
    from nerrf_amd.serve.engine import StreamingEngine, load_model_from_checkpoint

    assert (CKPT / "checkpoint.json").exists(), "vendored checkpoint missing"
    eng = StreamingEngine(model=load_model_from_checkpoint(str(CKPT)), device="cpu", **kw)
    eng.store.window_s = 1e9
    # a plan space the CPU oracle enumerates in well under a second
    eng.planner_params = PlannerParams(n_groups=3, max_depth=4)
    eng.ingest_events(arr)
    return eng, eng.score_window()


@pytest.fixture(scope="module")
def det_attr(seed77):
    return _detect(seed77)


def test_engine_attributes_every_victim_file(det_attr):
    from nerrf_amd.serve.engine import Culprit

    _eng, det = det_attr
    print("file_culprit:", sorted(det.file_culprit.items()))
    assert set(det.file_culprit) == VICTIMS
    assert {p for p, _s in det.file_culprit.values()} == {ATTACKER}
    assert all(s > 0.9 for _p, s in det.file_culprit.values())
    assert ATTACKER in det.proc_scores and VICTIMS <= set(det.file_scores)
    assert len(det.culprits) == 1
    c = det.culprits[0]
    assert isinstance(c, Culprit)
    assert c.proc == ATTACKER and c.n_files == 11 and set(c.files) == VICTIMS
    assert c.score == max(s for _p, s in det.file_culprit.values())
    assert c.mb == pytest.approx(sum(det.file_mb.get(p, 0.0) for p in VICTIMS))
    assert c.files == sorted(c.files, key=lambda p: (-det.file_culprit[p][1], p))
    assert c.as_dict() == {"proc": ATTACKER, "score": c.score, "n_files": 11,
                           "mb": c.mb, "files": c.files}
    assert det.contested == []


def test_attribution_is_not_bounded_by_top_k(det_attr, seed77):
    _eng, det = det_attr
    _eng4, det4 = _detect(seed77, top_edges=4)
    assert len(det4.top_edges) == 4
    assert det4.file_culprit == det.file_culprit
    assert det4.culprits == det.culprits


@pytest.mark.parametrize("kw", [dict(attribute=False), dict(top_edges=0)])
def test_attribution_off_changes_nothing_else(det_attr, seed77, kw):
    _eng, det = det_attr
    _eng0, det0 = _detect(seed77, **kw)
    assert det0.file_culprit == {} and det0.culprits == [] and det0.contested == []
    assert det0.file_scores == det.file_scores
    assert det0.proc_scores == det.proc_scores
    assert det0.node_max == det.node_max
    assert det0.seq_max == det.seq_max
    assert det0.alarm == det.alarm
    if kw.get("top_edges", 32) > 0:
        assert det0.top_edges == det.top_edges
        assert det0.edge_max == det.edge_max
    else:
        assert det0.top_edges == []


def test_attribute_threshold_is_checked():
    from nerrf_amd.serve.engine import StreamingEngine

    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            StreamingEngine(device="cpu", attribute_threshold=bad)


def test_build_culprits_order():
    from nerrf_amd.serve.engine import build_culprits

    fc = {"/a": (1, 0.6), "/b": (2, 0.9), "/c": (2, 0.9), "/d": (3, 0.95), "/e": (4, 0.95)}
    got = build_culprits(fc, {"/b": 1.5, "/c": 0.25, "/d": 2.0})
    # most files first, then best score, then process key
    assert [c.proc for c in got] == [2, 3, 4, 1]
    assert got[0].files == ["/b", "/c"] and got[0].mb == 1.75 and got[0].n_files == 2
    assert got[2].mb == 0.0  # a file absent from file_mb counts 0


# ------------------------------------------------ registry, merge and plan


def test_registry_roundtrip_and_world1_merge(det_attr, tmp_path):
    from nerrf_amd.serve.registry import DetectionRegistry

    eng, det = det_attr
    reg = DetectionRegistry(str(tmp_path / "st"))
    rec = reg.load(reg.record(det))
    assert rec["culprits"] == [c.as_dict() for c in det.culprits]
    assert rec["contested"] == det.contested
    # `nerrf status` lists each culprit without its files
    assert reg.list()[0]["culprits"] == [
        {"proc": ATTACKER, "n_files": 11, "score": det.culprits[0].score}]

    # the file list of a record is capped like file_scores
    big = copy.copy(det)
    big.culprits = [copy.copy(det.culprits[0])]
    big.culprits[0].files = [f"/x/{i}" for i in range(500)]
    big.culprits[0].n_files = 500
    rec = reg.load(reg.record(big))
    assert len(rec["culprits"][0]["files"]) == 200 and rec["culprits"][0]["n_files"] == 500

    merged = eng.merge_detections(det)
    assert merged is det


def _worker_merge_culprits(rank, world, port, results):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nerrf_amd.serve.engine import Detection, StreamingEngine, build_culprits

        eng = StreamingEngine(device="cpu")
        # the ranks disagree on /shared: rank 1 holds the stronger attribution
        if rank == 0:
            fc = {"/shared": (100, 0.7), "/only0": (100, 0.8)}
            mb = {"/shared": 1.0, "/only0": 2.0}
            contested = ["/only0"]
        else:
            fc = {"/shared": (200, 0.9), "/only1": (200, 0.6)}
            mb = {"/shared": 0.5, "/only1": 4.0}
            contested = ["/shared"]
        det = Detection(alarm=rank == 1, t_detect=float(rank),
                        file_scores={p: s for p, (_k, s) in fc.items()}, file_mb=mb,
                        proc_scores={100: 0.5, 200: 0.5}, file_culprit=fc,
                        culprits=build_culprits(fc, mb), contested=contested)
        merged = eng.merge_detections(det)
        results[rank] = {
            "file_culprit": dict(merged.file_culprit),
            "culprits": [c.as_dict() for c in merged.culprits],
            "contested": list(merged.contested),
        }
    finally:
        dist.destroy_process_group()


def test_merge_detections_keeps_stronger_attribution():
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    results = mp.Manager().dict()
    mp.spawn(_worker_merge_culprits, args=(2, port, results), nprocs=2, join=True)
    for rank in (0, 1):
        r = results[rank]
        assert r["file_culprit"] == {"/shared": (200, 0.9), "/only0": (100, 0.8),
                                     "/only1": (200, 0.6)}
        assert r["contested"] == ["/only0", "/shared"]
        # rebuilt from the merged map; mb from the merged (summed) file_mb
        assert r["culprits"] == [
            {"proc": 200, "score": 0.9, "n_files": 2, "mb": 5.5,
             "files": ["/shared", "/only1"]},
            {"proc": 100, "score": 0.8, "n_files": 1, "mb": 2.0, "files": ["/only0"]},
        ]


def _same_plan(a, b):
    assert a.plan == b.plan
    assert a.ranked_actions == b.ranked_actions
    assert a.root_value == b.root_value
    assert a.simulations == b.simulations


def test_plan_per_culprit_equals_plan_on_cut_detection(det_attr):
    eng, det = det_attr
    cut = copy.copy(det)
    cut.file_scores = {p: s for p, s in det.file_scores.items() if p in VICTIMS}
    cut.proc_scores = {ATTACKER: det.proc_scores[ATTACKER]}
    assert len(cut.file_scores) == 11 < len(det.file_scores)
    got = eng.plan(det, culprit=ATTACKER, planner="exact", model_refine=False)
    _same_plan(got, eng.plan(cut, planner="exact", model_refine=False))


def test_plan_without_culprit_is_unchanged(det_attr):
    """plan(det) is what it was before attribution existed: the plan of the
    state built from every file and the best process score."""
    from nerrf_amd.planner.oracle import exhaustive_best_cpu
    from nerrf_amd.planner.rewards import build_state

    eng, det = det_attr
    paths = list(det.file_scores.keys())
    scores = np.array([det.file_scores[p] for p in paths], dtype=np.float64)
    mb = np.array([max(det.file_mb.get(p, 0.01), 0.01) for p in paths], dtype=np.float64)
    proc = max(det.proc_scores.values(), default=0.0)
    if det.encrypted_paths:
        proc = max(proc, 0.9)
    state = build_state(scores, mb, proc_score=proc,
                        remaining_clean_mb=float(sum(det.file_mb.values())),
                        n_groups=eng.planner_params.n_groups)
    ref = exhaustive_best_cpu(state, eng.planner_params)
    got = eng.plan(det, planner="exact", model_refine=False)
    assert got.plan == ref.plan
    assert got.root_value == ref.reward
    assert got.simulations == ref.n_plans
    # ... and does not look at the attribution fields
    bare = copy.copy(det)
    bare.file_culprit, bare.culprits, bare.contested = {}, [], []
    _same_plan(got, eng.plan(bare, planner="exact", model_refine=False))


def test_plan_for_a_benign_process_raises(det_attr):
    eng, det = det_attr
    benign = next(k for k in det.proc_scores if k != ATTACKER)
    with pytest.raises(ValueError):
        eng.plan(det, culprit=benign, planner="exact", model_refine=False)
