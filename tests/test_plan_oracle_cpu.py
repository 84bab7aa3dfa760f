"""Exhaustive plan oracle: plan-space helpers, CPU reference, regret metric,
exact planner mode and CLI wiring (no GPU needed)."""
import itertools

import numpy as np
import pytest

from nerrf_amd.planner.mcts import run_mcts
from nerrf_amd.planner.oracle import (OracleResult, canonical_plan, count_plans,
                                      exhaustive_best, exhaustive_best_cpu,
                                      plan_regret, reward_tol)
from nerrf_amd.planner.rewards import (A_KILL, A_RESTORE, A_REVERT_BASE, A_STOP,
                                       PlannerParams, PlannerState, build_state,
                                       simulate_plan)


def _random_state(n_groups, seed, n_files=40):
    rng = np.random.default_rng(seed)
    scores = rng.uniform(0.0, 1.0, n_files)
    mb = rng.uniform(0.05, 4.0, n_files)
    return build_state(scores, mb, proc_score=float(rng.uniform(0.3, 1.0)),
                       remaining_clean_mb=float(mb.sum() * 0.8), n_groups=n_groups)


def _probe_state():
    """G=5 state on which run_mcts(seed=1, n_sims=1024) builds its plan around
    RESTORE and misses the kill-plus-reverts optimum (regret about 16)."""
    rng = np.random.default_rng(2)
    scores = rng.uniform(0.0, 1.0, 40)
    mb = rng.uniform(0.1, 8.0, 40)
    return build_state(scores, mb, proc_score=float(rng.uniform(0.5, 1.0)),
                       remaining_clean_mb=float(mb.sum()), n_groups=5)


def _tie_state():
    return PlannerState(
        group_score=np.array([0.9, 0.9, 0.9]), group_mb=np.array([2.0, 2.0, 2.0]),
        group_files=np.array([3.0, 3.0, 3.0]), proc_score=0.9, remaining_clean_mb=30.0)


def _clean_state(n_groups=3):
    return PlannerState(
        group_score=np.zeros(n_groups), group_mb=np.full(n_groups, 2.0),
        group_files=np.full(n_groups, 3.0), proc_score=0.0, remaining_clean_mb=30.0)


def _brute_force(state, params):
    """Independent sweep: itertools.permutations, sorted by the tie-break."""
    n = 2 + state.n_groups
    best = {}
    for k in range(0, min(n, params.max_depth) + 1):
        for perm in itertools.permutations(range(1, n + 1), k):
            r = simulate_plan(state, list(perm) + [A_STOP], params)
            first = perm[0] if perm else A_STOP
            key = (-r, len(perm), perm)
            if first not in best or key < best[first]:
                best[first] = key
    overall = min(best.values())
    return best, overall


@pytest.mark.parametrize("n,d,expect", [
    (3, 1, 4), (5, 5, 326), (6, 3, 157), (7, 10, 13700), (8, 6, 28961),
    (10, 10, 9864101), (18, 16, 4598708691828421),
])
def test_count_plans(n, d, expect):
    assert count_plans(n, d) == expect


def test_count_plans_matches_enumeration():
    for n, d in [(3, 1), (5, 5), (6, 3)]:
        total = sum(1 for k in range(0, min(n, d) + 1)
                    for _ in itertools.permutations(range(n), k))
        assert count_plans(n, d) == total


def test_canonical_plan_basics():
    assert canonical_plan([1, 1, 3, 0, 4]) == [1, 3]
    assert canonical_plan([0, 1]) == []
    assert canonical_plan([2, 3, 2, 3, 4]) == [2, 3, 4]


@pytest.mark.parametrize("n_groups", [1, 3, 5])
def test_canonicalisation_preserves_reward_exactly(n_groups):
    state = _random_state(n_groups, seed=10 + n_groups)
    params = PlannerParams(n_groups=n_groups)
    rng = np.random.default_rng(n_groups)
    for _ in range(300):
        x = [int(a) for a in rng.integers(0, 3 + n_groups, size=int(rng.integers(0, 14)))]
        assert simulate_plan(state, x, params) == simulate_plan(state, canonical_plan(x), params)


@pytest.mark.parametrize("n_groups,depth", [(3, 5), (4, 3)])
def test_reference_matches_permutation_sweep(n_groups, depth):
    state = _random_state(n_groups, seed=100 + n_groups)
    params = PlannerParams(n_groups=n_groups, max_depth=depth)
    res = exhaustive_best_cpu(state, params)
    best, overall = _brute_force(state, params)
    assert isinstance(res, OracleResult)
    assert res.n_plans == count_plans(2 + n_groups, depth)
    assert res.plan == list(overall[2])
    assert res.reward == -overall[0]
    assert res.reward == simulate_plan(state, res.plan + [A_STOP], params)
    assert set(res.first_action_best) == set(best)
    for a, (neg_r, _len, perm) in best.items():
        r, plan = res.first_action_best[a]
        assert r == -neg_r
        assert plan == list(perm)


def test_clean_state_empty_plan_wins():
    params = PlannerParams(n_groups=3, max_depth=5)
    res = exhaustive_best_cpu(_clean_state(), params)
    assert res.plan == []
    assert res.reward == 0.0
    assert res.first_action_best[A_STOP] == (0.0, [])


def test_exact_tie_returns_first_ordering():
    state = _tie_state()
    params = PlannerParams(n_groups=3, max_depth=5)
    tied = [simulate_plan(state, [A_KILL] + list(p) + [A_STOP], params)
            for p in itertools.permutations([3, 4, 5])]
    assert len(set(tied)) == 1
    assert tied[0] == pytest.approx(-0.125, abs=1e-9)
    res = exhaustive_best_cpu(state, params)
    assert res.plan == [1, 3, 4, 5]
    assert res.reward == tied[0]


def test_restore_alone_preferred_over_restore_then_revert():
    state = _random_state(3, seed=7)
    params = PlannerParams(n_groups=3, max_depth=5)
    res = exhaustive_best_cpu(state, params)
    r, plan = res.first_action_best[A_RESTORE]
    # a revert after a restore is a no-op: the tie goes to the shorter plan
    assert simulate_plan(state, [A_RESTORE, A_REVERT_BASE, A_STOP], params) == \
        simulate_plan(state, [A_RESTORE, A_STOP], params)
    assert A_REVERT_BASE not in plan[1:] and all(a < A_REVERT_BASE for a in plan)
    assert plan in ([A_RESTORE], [A_RESTORE, A_KILL])


def test_plan_regret_of_oracle_plan_is_zero():
    state = _random_state(4, seed=3)
    params = PlannerParams(n_groups=4, max_depth=4)
    res = exhaustive_best_cpu(state, params)
    assert plan_regret(state, res.plan, params, oracle=res) == 0.0
    assert plan_regret(state, res.plan, params) == 0.0


def test_plan_regret_of_mcts_is_nonnegative():
    state = _probe_state()
    params = PlannerParams(n_groups=5, max_depth=10)
    res = exhaustive_best_cpu(state, params)
    assert res.n_plans == 13700
    mcts = run_mcts(state, params, n_sims=1024, seed=1)
    regret = plan_regret(state, mcts.plan, params, oracle=res)
    print(f"oracle {res.plan} {res.reward:.4f}  mcts {mcts.plan}  regret {regret:.4f}")
    assert regret >= -reward_tol(res.reward)
    assert regret >= 0.0  # both sides are fp64 on the CPU: no near-tie slack


def _small_engine_and_detection(n_groups=3, max_depth=4):
    from nerrf_amd.serve.engine import Detection, StreamingEngine

    eng = StreamingEngine(device="cpu")
    eng.planner_params = PlannerParams(n_groups=n_groups, max_depth=max_depth)
    rng = np.random.default_rng(0)
    file_scores = {f"/data/f{i}.bin": float(s) for i, s in enumerate(rng.uniform(0, 1, 12))}
    file_mb = {p: float(m) for p, m in zip(file_scores, rng.uniform(0.1, 3.0, 12))}
    det = Detection(
        alarm=True, t_detect=0.0, file_scores=file_scores, file_mb=file_mb,
        proc_scores={4242: 0.95})
    return eng, det


def _state_of(eng, det):
    paths = list(det.file_scores.keys())
    scores = np.array([det.file_scores[p] for p in paths], dtype=np.float64)
    mb = np.array([max(det.file_mb.get(p, 0.01), 0.01) for p in paths], dtype=np.float64)
    proc = max(det.proc_scores.values(), default=0.0)
    return build_state(scores, mb, proc_score=proc,
                       remaining_clean_mb=float(sum(det.file_mb.values())),
                       n_groups=eng.planner_params.n_groups)


def test_engine_exact_planner_returns_reference_plan():
    eng, det = _small_engine_and_detection()
    ref = exhaustive_best_cpu(_state_of(eng, det), eng.planner_params)
    res = eng.plan(det, planner="exact")
    assert res.plan == ref.plan
    assert res.root_value == ref.reward
    assert res.simulations == ref.n_plans == count_plans(5, 4)
    qs = [q for _a, q, _n in res.ranked_actions]
    assert qs == sorted(qs, reverse=True)
    assert {a for a, _q, _n in res.ranked_actions} == set(range(0, 6))
    for a, q, n_under in res.ranked_actions:
        assert q == ref.first_action_best[a][0]
        assert n_under == (1 if a == A_STOP else count_plans(4, 3))
    assert sum(n for _a, _q, n in res.ranked_actions) == ref.n_plans
    assert res.ranked_actions[0][1] == ref.reward


def test_engine_mcts_planner_is_the_default():
    eng, det = _small_engine_and_detection()
    a = eng.plan(det, n_sims=128)
    b = eng.plan(det, n_sims=128, planner="mcts")
    assert (a.plan, a.ranked_actions, a.root_value, a.simulations) == \
        (b.plan, b.ranked_actions, b.root_value, b.simulations)
    with pytest.raises(ValueError):
        eng.plan(det, planner="greedy")


def test_max_plans_overflow_raises():
    state = _random_state(5, seed=5)
    params = PlannerParams(n_groups=5, max_depth=10)
    with pytest.raises(ValueError, match="13700"):
        exhaustive_best_cpu(state, params, max_plans=13699)
    with pytest.raises(ValueError, match="G=5"):
        exhaustive_best(state, params, device="cpu", max_plans=100)
    # the default configuration is beyond the CPU reference's default cap
    with pytest.raises(ValueError, match="9864101"):
        exhaustive_best(_random_state(8, seed=1), PlannerParams(), device="cpu")
    eng, det = _small_engine_and_detection()
    with pytest.raises(ValueError, match="D=4"):
        eng.plan(det, planner="exact", max_plans=10)


def test_non_finite_inputs_rejected():
    state = _random_state(3, seed=1)
    state.group_mb[1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        exhaustive_best(state, PlannerParams(n_groups=3, max_depth=3), device="cpu")


def test_cli_parser_accepts_planner_and_plan_quality():
    from nerrf_amd.cli import build_parser

    ap = build_parser()
    assert ap.parse_args(["undo", "--dir", "d"]).planner == "mcts"
    assert ap.parse_args(["undo", "--dir", "d", "--planner", "exact"]).planner == "exact"
    assert ap.parse_args(["scenario", "--dir", "d", "--planner", "exact"]).planner == "exact"
    assert ap.parse_args(["scenario", "--dir", "d"]).planner == "mcts"
    with pytest.raises(SystemExit):
        ap.parse_args(["undo", "--dir", "d", "--planner", "greedy"])
    args = ap.parse_args(["plan-quality", "--states", "4", "--seed", "9",
                          "--sims", "128,512", "--device", "cpu"])
    assert (args.cmd, args.states, args.seed, args.sims, args.device) == \
        ("plan-quality", 4, 9, "128,512", "cpu")


def test_plan_quality_report_on_cpu():
    from nerrf_amd.planner.quality import generate_states, measure_plan_quality

    params = PlannerParams(n_groups=3, max_depth=4)
    a = generate_states(3, seed=2, n_groups=3)
    b = generate_states(3, seed=2, n_groups=3)
    for x, y in zip(a, b):  # seeded: the same states every time
        assert np.array_equal(x.group_score, y.group_score) and x.proc_score == y.proc_score
    rep = measure_plan_quality(3, seed=2, sims=(64,), device="cpu", params=params)
    assert rep["plans_per_state"] == count_plans(5, 4)
    stats = rep["budgets"]["64"]
    assert stats["min_regret"] >= 0.0
    assert stats["max_regret"] >= stats["median_regret"] >= stats["min_regret"]
    assert 0.0 <= stats["optimal_share"] <= 1.0
    assert rep["oracle_s_per_state"] > 0.0
