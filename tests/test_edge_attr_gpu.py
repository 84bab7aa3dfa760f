"""Edge-attribution kernels (ops/hip/edge_attr.hip) against the torch
reference, the binding's contract checks, and per-file attribution in the GPU
serving engine.  Attribution is a selection: every comparison is exact."""
from pathlib import Path

import pytest
import torch

from test_edge_attr import (ATTACKER, HAND_CASES, N_FILES, N_NODES, VICTIMS,
                            assert_triple_equal, case_tensors, expected_tensors)

pytestmark = pytest.mark.gpu

CKPT = Path(__file__).resolve().parents[1] / "checkpoints" / "pretrained"


def _kernel(logit, ei, n_files, n_nodes, direction="write", thr=0.0):
    from nerrf_amd.ops import edge_attribution

    out = edge_attribution(logit, ei, n_files, n_nodes, direction, thr)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in out)
    return out


def _reference_on_cpu(logit, ei, n_files, n_nodes, direction="write", thr=0.0):
    from nerrf_amd.ops.reference import edge_attribution_ref

    return edge_attribution_ref(logit.cpu(), ei.cpu(), n_files, n_nodes, direction, thr)


def _assert_matches_reference(logit, ei, n_files, n_nodes, direction="write", thr=0.0):
    got = _kernel(logit, ei, n_files, n_nodes, direction, thr)
    want = _reference_on_cpu(logit, ei, n_files, n_nodes, direction, thr)
    assert_triple_equal([t.cpu() for t in got], want)
    return got


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_kernel_hand_made(gpu_device, name):
    case = HAND_CASES[name]
    logit, ei = case_tensors(case, gpu_device)
    got = _assert_matches_reference(logit, ei, N_FILES, N_NODES, case["direction"], case["thr"])
    assert_triple_equal([t.cpu() for t in got], expected_tensors(case))
    best = got[1].cpu()
    assert not torch.signbit(best[best == 0]).any()


def test_kernel_empty_inputs(gpu_device):
    none = torch.zeros(0, device=gpu_device)
    no_edges = torch.zeros(2, 0, dtype=torch.int64, device=gpu_device)
    _assert_matches_reference(none, no_edges, N_FILES, N_NODES)
    _assert_matches_reference(none, no_edges, 0, 3)
    some = torch.tensor([[0, 1], [1, 2]], device=gpu_device)
    _assert_matches_reference(torch.ones(2, device=gpu_device), some, 0, 3)


def _random_edges(e, n_files, n_procs, seed):
    """Random file<->process edges of both directions, logits on a coarse
    grid so that ties are everywhere."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randint(0, n_files, (e,), generator=g)
    p = torch.randint(n_files, n_files + n_procs, (e,), generator=g)
    write = torch.rand(e, generator=g) < 0.7
    ei = torch.stack([torch.where(write, p, f), torch.where(write, f, p)])
    logit = torch.randint(-8, 9, (e,), generator=g).float() / 4
    return logit, ei


@pytest.mark.parametrize("e", [1, 256, 257])
@pytest.mark.parametrize("direction", ["write", "read"])
def test_kernel_block_edges(gpu_device, e, direction):
    logit, ei = _random_edges(e, 7, 5, seed=e)
    _assert_matches_reference(logit.to(gpu_device), ei.to(gpu_device), 7, 12, direction)


def test_kernel_hub_file(gpu_device):
    """2048 distinct writers of one file: every atomic lands on one address."""
    n_files, n_procs = 3, 2048
    g = torch.Generator().manual_seed(3)
    src = n_files + torch.randperm(n_procs, generator=g)
    dst = torch.full((n_procs,), 1, dtype=torch.int64)
    logit = torch.randint(-8, 9, (n_procs,), generator=g).float() / 4
    got = _assert_matches_reference(logit.to(gpu_device), torch.stack([src, dst]).to(gpu_device),
                                    n_files, n_files + n_procs)
    assert int(got[2][1]) == int((logit >= 0).sum())
    assert got[0][[0, 2]].tolist() == [-1, -1]


@pytest.fixture(scope="module")
def large(gpu_device):
    """E = 300 001 over 1000 files and 500 processes: more edges than the
    capped grid has threads, so the stride loop runs.  Endpoints are drawn
    over all 1500 nodes, so file-file, process-process and read edges are
    mixed in with the 2/9 that are write edges."""
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, 1500, (2, 300_001), generator=g)
    logit = torch.randint(-8, 9, (300_001,), generator=g).float() / 4
    want = _reference_on_cpu(logit, ei, 1000, 1500)
    return logit.to(gpu_device), ei.to(gpu_device), want


def test_kernel_large_strided(large):
    logit, ei, want = large
    assert logit.numel() > 1024 * 256
    got = _kernel(logit, ei, 1000, 1500)
    assert_triple_equal([t.cpu() for t in got], want)
    assert (want[0] >= 0).all() and int(want[2].max()) >= 2


def test_kernel_large_is_deterministic(large):
    logit, ei, _want = large
    first = _kernel(logit, ei, 1000, 1500)
    again = _kernel(logit, ei, 1000, 1500)
    assert_triple_equal(again, first)


def test_binding_rejects_contract_violations(gpu_device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    logit, ei = _random_edges(64, 7, 5, seed=0)
    logit, ei = logit.to(gpu_device), ei.to(gpu_device)
    args = [logit, ei[0].contiguous(), ei[1].contiguous(), 7, 12, True, 0.0]
    got = ext.edge_attr(*args)
    torch.cuda.synchronize()
    assert_triple_equal([t.cpu() for t in got], _reference_on_cpu(logit, ei, 7, 12))
    wide = torch.stack([ei[0], ei[1]], dim=1)  # [E, 2]: columns are strided
    for pos, bad in ((0, logit.double()),            # fp64 logits
                     (1, args[1].int()),             # int32 indices
                     (2, args[2][:-1].contiguous()),  # length mismatch
                     (1, wide[:, 0]),                # non-contiguous view
                     (3, 13),                        # n_files > n_nodes
                     (0, logit.cpu())):              # CPU tensor
        broken = list(args)
        broken[pos] = bad
        with pytest.raises(RuntimeError):
            ext.edge_attr(*broken)


# ----------------------------------------------------------------- engine


def _engine_detection(device, dtype):
    from nerrf_amd.data.synth import SynthConfig, generate
    from nerrf_amd.serve.engine import StreamingEngine, load_model_from_checkpoint

    arr, _ = generate(SynthConfig(seed=77, duration_s=40, benign_rate_hz=60, n_victim_files=10))
    eng = StreamingEngine(model=load_model_from_checkpoint(str(CKPT)), device=device,
                          dtype=dtype)
    eng.store.window_s = 1e9
    eng.ingest_events(arr)
    return eng.score_window()


def test_engine_gpu_attributes_the_same_files_as_cpu(gpu_device):
    gpu = _engine_detection(str(gpu_device), torch.bfloat16)
    cpu = _engine_detection("cpu", torch.float32)

    def who(det):
        return {path: proc for path, (proc, _s) in det.file_culprit.items()}

    print("gpu bf16:", sorted((p, k, round(s, 4)) for p, (k, s) in gpu.file_culprit.items()))
    assert who(cpu) == {p: ATTACKER for p in VICTIMS}
    assert who(gpu) == who(cpu)
    assert gpu.contested == cpu.contested
    assert set(gpu.culprits[0].files) == set(cpu.culprits[0].files)
    assert gpu.culprits[0].proc == cpu.culprits[0].proc == ATTACKER
