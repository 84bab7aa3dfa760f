"""The joint plan oracle's CPU-side surface: plan_joint(planner="exact") and the
plan-quality report over joint states."""
import numpy as np
import pytest

from nerrf_amd.planner.oracle import exhaustive_best_cpu, plans_under
from nerrf_amd.planner.quality import measure_plan_quality
from nerrf_amd.planner.rewards import MultiPlannerState, PlannerParams, build_state
from nerrf_amd.serve.engine import StreamingEngine
from test_plan_joint import CpuEngine, two_culprit_detection


class SmallCpuEngine(CpuEngine):
    planner_params = PlannerParams(n_groups=4, max_depth=4)  # P=2, G=4: 1100 plans


def test_plan_joint_exact_is_the_cpu_oracle():
    det = two_culprit_detection()
    res = StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="exact", use_gpu=False)
    # the state plan_joint builds: two score buckets per culprit
    parts = [build_state(np.array([det.file_scores[p] for p in paths]), np.full(len(paths), 2.0),
                         0.0, 0.0, n_groups=2)
             for paths in ([f"/d/a{i}" for i in range(5)], [f"/d/b{i}" for i in range(3)])]
    state = MultiPlannerState(
        group_score=np.concatenate([s.group_score for s in parts]),
        group_mb=np.concatenate([s.group_mb for s in parts]),
        group_files=np.concatenate([s.group_files for s in parts]),
        proc_score=np.array([0.95, 0.6]), remaining_clean_mb=float(sum(det.file_mb.values())))
    ref = exhaustive_best_cpu(state, SmallCpuEngine.planner_params)
    assert ref.n_plans == 1100
    assert (res.plan, res.root_value, res.simulations) == (ref.plan, ref.reward, 1100)
    assert res.ranked_actions == sorted(
        [(a, q, plans_under(a, 7, 4)) for a, (q, _plan) in ref.first_action_best.items()],
        key=lambda t: (-t[1], t[0]))
    assert res.proc_keys == [11, 22] and res.unplanned == ["/d/x"]


@pytest.mark.parametrize("kwargs", [{"planner": "greedy"}, {"planner": "exact", "max_plans": 10}])
def test_plan_joint_refuses(kwargs):
    with pytest.raises(ValueError):
        StreamingEngine.plan_joint(SmallCpuEngine(), two_culprit_detection(), use_gpu=False, **kwargs)


def test_plan_quality_over_joint_states():
    params = PlannerParams(n_groups=4, max_depth=4)
    rep = measure_plan_quality(n_states=3, seed=2, sims=(64,), n_procs=2, device="cpu", params=params)
    assert (rep["n_procs"], rep["n_groups"], rep["plans_per_state"]) == (2, 4, 1100)
    stats = rep["budgets"]["64"]
    assert np.isfinite([stats["mean_regret"], stats["max_regret"]]).all()
    assert stats["min_regret"] >= 0.0  # the CPU oracle is exact in fp64: no plan beats it


def test_plan_quality_of_one_process_is_unchanged():
    """The report of this seed before `n_procs` existed."""
    rep = measure_plan_quality(3, seed=2, sims=(64,), device="cpu",
                               params=PlannerParams(n_groups=4, max_depth=4), n_procs=1)
    del rep["oracle_s_per_state"]
    assert rep == {
        "states": 3, "seed": 2, "device": "cpu", "n_groups": 4, "max_depth": 4,
        "plans_per_state": 517,
        "budgets": {"64": {"mean_regret": pytest.approx(13.703463616968387, rel=1e-12),
                           "median_regret": 0.0,
                           "max_regret": pytest.approx(41.11039085090516, rel=1e-12),
                           "min_regret": 0.0, "optimal_share": pytest.approx(2 / 3)}}}
