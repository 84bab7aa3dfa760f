"""Joint multi-culprit planning on the CPU: the P-process reward, its planner
and oracle, and StreamingEngine.plan_joint."""
import numpy as np
import pytest
import torch

from nerrf_amd.planner.mcts import run_mcts_multi
from nerrf_amd.planner.oracle import exhaustive_best_cpu, plan_regret, reward_tol
from nerrf_amd.planner.rewards import (MultiPlannerState, PlannerParams, PlannerState,
                                       simulate_plan, simulate_plan_multi)
from nerrf_amd.serve.engine import Detection, StreamingEngine, build_culprits


def multi_state(n_procs, n_groups, seed):
    rng = np.random.default_rng(seed)
    return MultiPlannerState(
        group_score=rng.uniform(0.05, 1.0, n_groups), group_mb=rng.uniform(0.5, 30.0, n_groups),
        group_files=rng.integers(1, 12, n_groups).astype(np.float64),
        proc_score=rng.uniform(0.3, 1.0, n_procs), remaining_clean_mb=60.0,
        group_owner=rng.integers(0, n_procs, n_groups))


# The fixed P = 2, G = 3, D = 5 state of the oracle and select-phase tests.
FIXED_PARAMS = PlannerParams(n_groups=3, max_depth=5)
FIXED_STATE = MultiPlannerState(
    group_score=np.array([0.9, 0.7, 0.3]), group_mb=np.array([20.0, 10.0, 5.0]),
    group_files=np.array([4.0, 3.0, 2.0]), proc_score=np.array([0.95, 0.6]),
    remaining_clean_mb=100.0, group_owner=np.array([0, 0, 1]))


def two_culprit_detection():
    """Processes 11 (five files) and 22 (three), and one unattributed file."""
    fc = {f"/d/a{i}": (11, 0.9) for i in range(5)}
    fc.update({f"/d/b{i}": (22, 0.8) for i in range(3)})
    scores = {p: 0.9 - 0.01 * i for i, p in enumerate(fc)}
    scores["/d/x"] = 0.7
    mb = {p: 2.0 for p in scores}
    return Detection(alarm=True, t_detect=0.0, file_scores=scores, file_mb=mb,
                     proc_scores={11: 0.95, 22: 0.6}, file_culprit=fc,
                     culprits=build_culprits(fc, mb))


class CpuEngine:
    """What plan_joint reads of an engine."""
    planner_params = PlannerParams()
    device = torch.device("cpu")


@pytest.mark.parametrize("n_groups", [1, 8])
def test_one_process_equals_simulate_plan(n_groups):
    ms = multi_state(1, n_groups, seed=n_groups)
    st = PlannerState(ms.group_score, ms.group_mb, ms.group_files,
                      float(ms.proc_score[0]), ms.remaining_clean_mb)
    params = PlannerParams(n_groups=n_groups)
    rng = np.random.default_rng(7)
    for _ in range(300):  # STOP, duplicates and out-of-range ids included
        acts = [int(a) for a in rng.integers(-2, n_groups + 6, rng.integers(0, 12))]
        assert simulate_plan_multi(ms, acts, params) == simulate_plan(st, acts, params)


def test_reward_semantics():
    p = PlannerParams(n_groups=2)
    st = MultiPlannerState(np.array([0.9, 0.8]), np.array([10.0, 5.0]), np.array([4.0, 2.0]),
                           np.array([0.7, 0.4]), remaining_clean_mb=1e9)
    r = lambda acts: simulate_plan_multi(st, acts, p)
    kill0, kill1, restore, rev0, rev1 = 1, 2, 3, 4, 5
    assert r([kill0, kill0]) == r([kill0])  # second KILL of one process: no-op
    dt = p.revert_time_s * 4.0
    # both processes dead at the end, so all ongoing damage stems from the revert
    both = r([kill0, kill1, rev0]) - r([rev0, kill0, kill1])
    assert both == pytest.approx(p.attack_rate_mbps * dt * (0.7 + 0.4), rel=1e-9)
    only1 = r([kill0, kill1, rev0]) - r([kill0, rev0, kill1])
    assert only1 == pytest.approx(p.attack_rate_mbps * dt * 0.4, rel=1e-9)
    # one RESTORE recovers every group: reverts after it change nothing
    assert r([kill0, kill1, restore, rev0, rev1]) == r([kill0, kill1, restore])
    assert r([kill0, kill1, restore]) == pytest.approx(
        -(p.restore_loss_mb + p.downtime_weight * (2 * p.kill_time_s + p.restore_time_s)))


def test_planner_reaches_oracle_on_fixed_state():
    orc = exhaustive_best_cpu(FIXED_STATE, FIXED_PARAMS)
    assert orc.n_plans == 1237
    assert orc.plan[:2] == [1, 2]  # both processes killed, the higher-scored first
    res = run_mcts_multi(FIXED_STATE, FIXED_PARAMS, n_sims=1024)
    regret = plan_regret(FIXED_STATE, res.plan, FIXED_PARAMS, oracle=orc)
    print(f"oracle {orc.plan} {orc.reward:.6f}  mcts {res.plan} regret {regret:.3e}")
    assert regret <= reward_tol(orc.reward)


def test_plan_joint_on_two_culprits():
    det = two_culprit_detection()
    res = StreamingEngine.plan_joint(CpuEngine(), det, use_gpu=False)
    assert res.proc_keys == [11, 22]
    assert {1, 2} <= set(res.plan)  # both kill actions
    assert {"kill_process:11", "kill_process:22"} <= set(res.describe())
    assert res.unplanned == ["/d/x"]
    assert len(res.group_owner) == len(res.group_paths) <= 16
    for owner, paths in zip(res.group_owner, res.group_paths):
        assert paths and all(det.file_culprit[p][0] == res.proc_keys[owner] for p in paths)
    assert sorted(p for ps in res.group_paths for p in ps) == sorted(det.file_culprit)
    with pytest.raises(ValueError):
        StreamingEngine.plan_joint(CpuEngine(), det, culprits=[33], use_gpu=False)
