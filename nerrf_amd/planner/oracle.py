"""Exhaustive plan oracle: the exact optimum of the rollback-planning MDP.

Plan space.  `simulate_plan` stops at the first STOP and treats a repeated
action as a no-op, so every action list has bit-identical reward to its
canonical form (`canonical_plan`).  The space to search is therefore the
ordered arrangements of distinct non-STOP actions: with n = 2 + G non-STOP
actions and D = max_depth there are

    count_plans(n, D) = sum_{k=0..min(n,D)} n! / (n-k)!

plans (G=8, D=10: 9 864 101).  `exhaustive_best_cpu` enumerates them with
`simulate_plan` in fp64 (the ground truth); `exhaustive_best` on a GPU device
runs the batched HIP search (ops/hip/plan_oracle.hip) and re-scores the
per-first-action winners in fp64.

Tie-break (shared by both paths): among plans of equal reward the shorter plan
wins, then the lexicographically smaller action tuple.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .rewards import A_STOP, PlannerParams, PlannerState, simulate_plan

# Default cap of the CPU reference.  simulate_plan costs about 10 us per plan
# in CPython on one core (13 700 plans: ~0.12 s), so 1e6 plans return in
# roughly 10 s.
CPU_MAX_PLANS = 1_000_000
# Default cap of the GPU search (see profiles/PROFILES.md for the measurement).
GPU_MAX_PLANS = 2**31 - 1

# "reward agrees with the fp64 truth": the project's tolerance for fp32
# device rewards (tests/test_ops_gpu.py::test_mcts_eval_plans_matches_cpu)
REWARD_RTOL = 1e-4
REWARD_ATOL = 1e-3

MAX_GROUPS_DEV = 16
MAX_DEPTH_DEV = 16


def count_plans(n_actions_nonstop: int, max_depth: int) -> int:
    """Number of canonical plans: arrangements of up to `max_depth` distinct
    actions out of `n_actions_nonstop`, the empty plan included (exact int)."""
    n = int(n_actions_nonstop)
    total, term = 0, 1
    for k in range(0, min(n, int(max_depth)) + 1):
        total += term
        term *= n - k
    return total


def canonical_plan(actions: Sequence[int]) -> List[int]:
    """Truncate at the first STOP and drop repeated actions."""
    out: List[int] = []
    seen = set()
    for a in actions:
        a = int(a)
        if a == A_STOP:
            break
        if a not in seen:
            seen.add(a)
            out.append(a)
    return out


@dataclass
class OracleResult:
    plan: List[int]
    reward: float  # fp64 simulate_plan value of `plan`
    # exact root action values: first action a (A_STOP = the empty plan) ->
    # (best reward, best plan) among the plans that start with a
    first_action_best: Dict[int, Tuple[float, List[int]]]
    n_plans: int
    # GPU path only: first action -> fp32 reward of its winner as the device
    # reported it (eval_plan's value, equal to mcts_eval_plans on that plan)
    device_rewards: Dict[int, float] = field(default_factory=dict)


def _better(r: float, plan: Sequence[int], best_r: float, best_plan: Optional[Sequence[int]]) -> bool:
    """The tie-break: reward, then shorter, then lexicographically smaller."""
    if best_plan is None or r > best_r:
        return True
    if r < best_r:
        return False
    if len(plan) != len(best_plan):
        return len(plan) < len(best_plan)
    return tuple(plan) < tuple(best_plan)


def _pick(first_action_best: Dict[int, Tuple[float, List[int]]]) -> Tuple[float, List[int]]:
    best_r, best_plan = 0.0, None
    for a in sorted(first_action_best):
        r, plan = first_action_best[a]
        if _better(r, plan, best_r, best_plan):
            best_r, best_plan = r, plan
    return best_r, list(best_plan)


def _check_state(state: PlannerState, params: PlannerParams) -> None:
    arrs = (state.group_score, state.group_mb, state.group_files)
    if state.n_groups < 1 or any(len(a) != state.n_groups for a in arrs):
        raise ValueError("planner state needs >= 1 group and equal-length group arrays")
    vals = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrs]
                          + [np.array([state.proc_score, state.remaining_clean_mb], dtype=np.float64)])
    if not np.all(np.isfinite(vals)):
        raise ValueError("planner state holds non-finite values")
    pvals = [params.downtime_weight, params.revert_time_s, params.kill_time_s,
             params.fp_weight, params.attack_rate_mbps, params.horizon_s,
             params.restore_time_s, params.restore_loss_mb]
    if not np.all(np.isfinite(np.array(pvals, dtype=np.float64))):
        raise ValueError("planner params hold non-finite values")


def _too_many(state: PlannerState, params: PlannerParams, n_plans: int, cap: int) -> ValueError:
    return ValueError(
        f"exhaustive planner: G={state.n_groups} groups at max_depth D={params.max_depth} "
        f"give {n_plans} plans, above max_plans={cap}; lower max_depth or n_groups, "
        f"or use planner='mcts'"
    )


def exhaustive_best_cpu(
    state: PlannerState,
    params: Optional[PlannerParams] = None,
    max_plans: int = CPU_MAX_PLANS,
) -> OracleResult:
    """CPU ground truth: depth-first enumeration of every canonical plan,
    each scored by `simulate_plan` in fp64.

    Raises ValueError when the plan count exceeds `max_plans`.  The default,
    CPU_MAX_PLANS = 1e6, keeps a capped call to roughly 10 s on one core
    (about 10 us per plan)."""
    params = params or PlannerParams()
    _check_state(state, params)
    n = 2 + state.n_groups
    n_plans = count_plans(n, params.max_depth)
    if n_plans > max_plans:
        raise _too_many(state, params, n_plans, max_plans)
    depth_lim = min(n, max(int(params.max_depth), 0))
    fab: Dict[int, Tuple[float, List[int]]] = {
        A_STOP: (float(simulate_plan(state, [A_STOP], params)), [])
    }
    actions = list(range(1, n + 1))
    plan: List[int] = []
    used = [False] * (n + 1)

    def rec() -> None:
        # plans arrive in lexicographic preorder, so a tie between equal
        # lengths keeps the earlier plan
        r = float(simulate_plan(state, plan, params))
        cur = fab.get(plan[0])
        if cur is None or r > cur[0] or (r == cur[0] and len(plan) < len(cur[1])):
            fab[plan[0]] = (r, list(plan))
        if len(plan) >= depth_lim:
            return
        for a in actions:
            if not used[a]:
                used[a] = True
                plan.append(a)
                rec()
                plan.pop()
                used[a] = False

    if depth_lim >= 1:
        for a in actions:
            used[a] = True
            plan.append(a)
            rec()
            plan.pop()
            used[a] = False
    reward, best = _pick(fab)
    return OracleResult(plan=best, reward=reward, first_action_best=fab, n_plans=n_plans)


def _params_dict(n_groups: int, params: PlannerParams) -> dict:
    return {
        "n_groups": n_groups,
        "max_depth": params.max_depth,
        "sims_per_tree": 0,
        "downtime_weight": params.downtime_weight,
        "revert_time_s": params.revert_time_s,
        "kill_time_s": params.kill_time_s,
        "fp_weight": params.fp_weight,
        "attack_rate_mbps": params.attack_rate_mbps,
        "horizon_s": params.horizon_s,
        "restore_time_s": params.restore_time_s,
        "restore_loss_mb": params.restore_loss_mb,
        "ucb_c": 0.0,
        "seed": 0,
    }


def _exhaustive_best_gpu(
    states: List[PlannerState], params: PlannerParams, device: str, prefix_len: int = 0
) -> List[OracleResult]:
    import torch

    from ..ops.native import load_extension

    ext = load_extension(required=True)  # a missing kernel on GPU is an error
    g = states[0].n_groups
    if g > MAX_GROUPS_DEV or params.max_depth > MAX_DEPTH_DEV:
        raise ValueError(f"GPU plan oracle supports G <= {MAX_GROUPS_DEV} and "
                         f"max_depth <= {MAX_DEPTH_DEV} (got G={g}, D={params.max_depth})")
    if any(s.n_groups != g for s in states):
        raise ValueError("all states of one batch must have the same number of groups")
    dev = torch.device(device)

    def stack(get) -> "torch.Tensor":
        return torch.from_numpy(np.stack([np.asarray(get(s), dtype=np.float32) for s in states])).to(dev)

    gs = stack(lambda s: s.group_score)
    gm = stack(lambda s: s.group_mb)
    gf = stack(lambda s: s.group_files)
    pr = torch.tensor([float(s.proc_score) for s in states], dtype=torch.float32, device=dev)
    cl = torch.tensor([float(s.remaining_clean_mb) for s in states], dtype=torch.float32, device=dev)
    w_reward, w_len, w_plan, _meta = ext.plan_oracle_search(
        gs, gm, gf, pr, cl, _params_dict(g, params), int(prefix_len))
    w_reward = w_reward.numpy()
    w_len = w_len.numpy()
    w_plan = w_plan.numpy()
    n = 2 + g
    n_plans = count_plans(n, params.max_depth)
    out = []
    for si, st in enumerate(states):
        fab: Dict[int, Tuple[float, List[int]]] = {}
        dev_r: Dict[int, float] = {}
        for a in range(0, n + 1):
            plan = [int(x) for x in w_plan[si, a, : int(w_len[si, a])]]
            # the final choice is made in fp64 among the <= n+1 winners
            fab[a] = (float(simulate_plan(st, plan + [A_STOP], params)), plan)
            dev_r[a] = float(w_reward[si, a])
        reward, best = _pick(fab)
        out.append(OracleResult(plan=best, reward=reward, first_action_best=fab,
                                n_plans=n_plans, device_rewards=dev_r))
    return out


def exhaustive_best(
    state_or_states: Union[PlannerState, Sequence[PlannerState]],
    params: Optional[PlannerParams] = None,
    device: str = "cpu",
    max_plans: int = GPU_MAX_PLANS,
    prefix_len: int = 0,
) -> Union[OracleResult, List[OracleResult]]:
    """Exact optimum of one state (-> OracleResult) or a batch (-> list).

    On a GPU device the batched HIP search finds, per state, the best plan
    under each first action in fp32; those at most n+1 winners are re-scored
    with `simulate_plan` in fp64 and the final plan is picked among them in
    fp64 with the module's tie-break.  On "cpu" the reference runs (its own
    cap, CPU_MAX_PLANS, applies as well).  Raises ValueError when the plan
    count exceeds `max_plans` and on non-finite inputs.  `prefix_len`
    overrides the GPU work decomposition (0 = automatic)."""
    params = params or PlannerParams()
    single = isinstance(state_or_states, PlannerState)
    states = [state_or_states] if single else list(state_or_states)
    if not states:
        return []
    for st in states:
        _check_state(st, params)
        n_plans = count_plans(2 + st.n_groups, params.max_depth)
        if n_plans > max_plans:
            raise _too_many(st, params, n_plans, max_plans)
    dev = str(device)
    if dev == "cpu" or params.max_depth < 1:
        res = [exhaustive_best_cpu(st, params, max_plans=min(max_plans, CPU_MAX_PLANS)) for st in states]
    else:
        res = _exhaustive_best_gpu(states, params, dev, prefix_len=prefix_len)
    return res[0] if single else res


def plan_regret(
    state: PlannerState,
    plan: Sequence[int],
    params: Optional[PlannerParams] = None,
    oracle: Optional[OracleResult] = None,
    device: str = "cpu",
) -> float:
    """Oracle reward minus the fp64 reward of `plan`, reported raw.

    The oracle is exact, so regret is >= 0 up to one caveat: a GPU oracle
    chooses each first action's winner in fp32, and may keep a plan that is
    worse in fp64 than an fp32 near-tie it discarded.  A value in [-tol, 0)
    (tol = REWARD_ATOL + REWARD_RTOL * |reward|) can only come from such a
    near-tie; anything below -tol is a bug."""
    params = params or PlannerParams()
    if oracle is None:
        oracle = exhaustive_best(state, params, device=device)
    return float(oracle.reward - simulate_plan(state, list(plan) + [A_STOP], params))


def reward_tol(reward: float) -> float:
    return REWARD_ATOL + REWARD_RTOL * abs(float(reward))


def plans_under(first_action: int, n_actions_nonstop: int, max_depth: int) -> int:
    """How many canonical plans start with `first_action`."""
    if first_action == A_STOP:
        return 1
    if max_depth < 1:
        return 0
    return count_plans(n_actions_nonstop - 1, max_depth - 1)


__all__ = [
    "CPU_MAX_PLANS", "GPU_MAX_PLANS",
    "OracleResult", "REWARD_ATOL", "REWARD_RTOL", "canonical_plan", "count_plans",
    "exhaustive_best", "exhaustive_best_cpu", "plan_regret", "plans_under", "reward_tol",
]
