"""The subset planner's CPU side: the fp64 closed form over action sets
(oracle.subset_best_cpu) against the exhaustive CPU oracle, and
plan_joint(planner="sets")."""
import dataclasses

import numpy as np
import pytest

from nerrf_amd.planner.oracle import (count_sets, exhaustive_best_cpu, plan_regret, reward_tol,
                                      subset_best_cpu)
from nerrf_amd.planner.rewards import MultiPlannerState, PlannerParams
from nerrf_amd.serve.engine import StreamingEngine
from test_plan_joint import FIXED_PARAMS, FIXED_STATE, CpuEngine, multi_state, two_culprit_detection


def shape_state(n_procs, n_groups, depth):
    if (n_procs, n_groups) == (2, 3):
        return FIXED_STATE, FIXED_PARAMS
    return (multi_state(n_procs, n_groups, seed=10 * n_procs + n_groups),
            PlannerParams(n_groups=n_groups, max_depth=depth))


@pytest.mark.parametrize("clean_mb", [0.5, 60.0, 1e9])  # cap binding, in between, never binding
@pytest.mark.parametrize("n_procs,n_groups,depth", [(1, 1, 10), (2, 3, 5), (3, 4, 6), (8, 2, 4)])
def test_closed_form_matches_exhaustive_oracle(n_procs, n_groups, depth, clean_mb):
    st, params = shape_state(n_procs, n_groups, depth)
    st = dataclasses.replace(st, remaining_clean_mb=clean_mb)
    ref = exhaustive_best_cpu(st, params)
    got = subset_best_cpu(st, params)
    n = st.n_actions - 1
    assert got.n_plans == count_sets(n, depth)
    assert set(got.first_action_best) == set(range(0, n + 1))
    for a, (r_ref, _plan) in ref.first_action_best.items():
        r, plan = got.first_action_best[a]
        assert abs(r - r_ref) <= reward_tol(r_ref), (a, plan, r, r_ref)
        assert plan[:1] == ([a] if a else [])
    assert plan_regret(st, got.plan, params, oracle=ref) <= reward_tol(ref.reward)


def test_exact_tie_and_clean_state():
    params = PlannerParams(n_groups=2, max_depth=5)
    tie = MultiPlannerState(np.array([0.9, 0.9]), np.array([2.0, 2.0]), np.array([3.0, 3.0]),
                            np.array([0.9, 0.9]), remaining_clean_mb=30.0)
    clean = MultiPlannerState(np.zeros(2), np.full(2, 2.0), np.full(2, 3.0), np.zeros(2),
                              remaining_clean_mb=30.0)
    assert subset_best_cpu(tie, params).plan == exhaustive_best_cpu(tie, params).plan
    assert subset_best_cpu(clean, params).plan == exhaustive_best_cpu(clean, params).plan == []


def test_plan_joint_sets_equals_exact():
    class SmallCpuEngine(CpuEngine):
        planner_params = PlannerParams(n_groups=4, max_depth=4)  # P=2, G=4: n=7, 99 sets

    det = two_culprit_detection()
    sets = StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="sets", use_gpu=False)
    exact = StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="exact", use_gpu=False)
    assert (sets.plan, sets.root_value) == (exact.plan, exact.root_value)
    assert sets.simulations == count_sets(7, 4) == 99
    assert [a for a, _q, _n in sets.ranked_actions] == [a for a, _q, _n in exact.ranked_actions]
    assert {a: k for a, _q, k in sets.ranked_actions} == {0: 1, **{a: count_sets(6, 3) for a in range(1, 8)}}
    with pytest.raises(ValueError, match="'mcts', 'exact' or 'sets'"):
        StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="greedy", use_gpu=False)
