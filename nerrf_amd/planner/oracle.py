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

A `MultiPlannerState` (P processes, rewards.simulate_plan_multi) has
n = P + 1 + G non-STOP actions and the same canonical form (P=2, G=8, D=10:
68 588 312 plans).  Both paths take it: the CPU reference scores it with
`simulate_plan_multi`, and a GPU device runs ops/hip/plan_oracle_multi.hip.
One GPU batch holds one kind of state and one (P, G).

Tie-break (shared by all paths): among plans of equal reward the shorter plan
wins, then the lexicographically smaller action tuple.

Search over sets (`subset_best`, `subset_best_cpu`, ops/hip/plan_subsets.hip).
The optimum does not need ordered enumeration.  In `simulate_plan_multi` every
term but `ongoing` depends only on the SET of executed actions: the kills, the
downtime, the false-positive MB, the recovered groups and the staleness are
the same in any order.  `ongoing` is a sum of `rate * dt * live` over the
time-consuming actions (RESTORE and the reverts); a KILL adds nothing to it and
only lowers `live`, and the loss is non-decreasing in `ongoing`.  So, with
non-negative times, rates and scores, moving a KILL in front of a
time-consuming action never lowers the reward, and a revert that follows a
RESTORE is a no-op that a revert in front of it is not.  The best ordering of
a set S of distinct actions is therefore ascending action id: kills first,
then RESTORE, then reverts (no-ops, which the shorter set without them beats on
length).  It is also the lexicographically smallest ordering, so it wins every
tie.  With a forced first action a, the same holds for the rest: a, then S - {a}
ascending.  The exact optimum, and the exact best plan under each first
action, is a maximum over at most

    count_sets(n, D) = sum_{k=0..min(n,D)} C(n, k)

sets (n = 25, D = 10: 7 119 516; under 2^25 at any depth) instead of
`count_plans(n, D)` arrangements, which serves every joint state the engine can
build (P <= 8, G <= 16).  Two orderings of one set can differ in the last ulp
of the fp64 sum `ongoing`; such a difference is far below `reward_tol`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .rewards import (A_STOP, MultiPlannerState, PlannerParams, PlannerState,
                      plan_reward)

# Default cap of the CPU reference.  simulate_plan costs about 10 us per plan
# in CPython on one core (13 700 plans: ~0.12 s), so 1e6 plans return in
# roughly 10 s.
CPU_MAX_PLANS = 1_000_000
# Default cap of the GPU search (see profiles/PROFILES.md for the measurement).
GPU_MAX_PLANS = 2**31 - 1
# Default cap of StreamingEngine.plan_joint(planner="exact") on a GPU.  The
# largest D=10 joint state under it, P=4, G=8 (1 359 245 486 plans), measured
# 8.7 ms per call on one MI355X (profiles/PROFILES.md, "Joint plan oracle"),
# so the cap is not lowered; it is also the joint kernel's hard bound
# (bindings.cpp refuses more).
GPU_MAX_PLANS_JOINT = 2**31 - 1

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


def count_sets(n_actions_nonstop: int, max_depth: int) -> int:
    """Number of sets of up to `max_depth` distinct actions out of
    `n_actions_nonstop`, the empty set included (exact int)."""
    n = int(n_actions_nonstop)
    return sum(math.comb(n, k) for k in range(0, min(n, int(max_depth)) + 1))


def sets_under(first_action: int, n_actions_nonstop: int, max_depth: int) -> int:
    """How many of those sets can start with `first_action` (hold it)."""
    if first_action == A_STOP:
        return 1
    if max_depth < 1:
        return 0
    return count_sets(n_actions_nonstop - 1, max_depth - 1)


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
                          + [np.atleast_1d(np.asarray(state.proc_score, dtype=np.float64)),
                             np.array([state.remaining_clean_mb], dtype=np.float64)])
    if not np.all(np.isfinite(vals)):
        raise ValueError("planner state holds non-finite values")
    pvals = [params.downtime_weight, params.revert_time_s, params.kill_time_s,
             params.fp_weight, params.attack_rate_mbps, params.horizon_s,
             params.restore_time_s, params.restore_loss_mb]
    if not np.all(np.isfinite(np.array(pvals, dtype=np.float64))):
        raise ValueError("planner params hold non-finite values")


def _too_many(state: PlannerState, params: PlannerParams, n_plans: int, cap: int) -> ValueError:
    procs = f"P={state.n_procs} processes and " if isinstance(state, MultiPlannerState) else ""
    return ValueError(
        f"exhaustive planner: {procs}G={state.n_groups} groups at max_depth D={params.max_depth} "
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
    n = state.n_actions - 1
    n_plans = count_plans(n, params.max_depth)
    if n_plans > max_plans:
        raise _too_many(state, params, n_plans, max_plans)
    depth_lim = min(n, max(int(params.max_depth), 0))
    fab: Dict[int, Tuple[float, List[int]]] = {
        A_STOP: (float(plan_reward(state, [A_STOP], params)), [])
    }
    actions = list(range(1, n + 1))
    plan: List[int] = []
    used = [False] * (n + 1)

    def rec() -> None:
        # plans arrive in lexicographic preorder, so a tie between equal
        # lengths keeps the earlier plan
        r = float(plan_reward(state, plan, params))
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


def _results_of_winners(states, params: PlannerParams, w_reward, w_len, w_plan,
                        n_plans: int) -> List[OracleResult]:
    """OracleResults from a search binding's per-first-action winners (CPU
    tensors [S, n+1], [S, n+1], [S, n+1, 16])."""
    w_reward = w_reward.numpy()
    w_len = w_len.numpy()
    w_plan = w_plan.numpy()
    n = states[0].n_actions - 1
    out = []
    for si, st in enumerate(states):
        fab: Dict[int, Tuple[float, List[int]]] = {}
        dev_r: Dict[int, float] = {}
        for a in range(0, n + 1):
            plan = [int(x) for x in w_plan[si, a, : int(w_len[si, a])]]
            # the final choice is made in fp64 among the <= n+1 winners
            fab[a] = (float(plan_reward(st, plan + [A_STOP], params)), plan)
            dev_r[a] = float(w_reward[si, a])
        reward, best = _pick(fab)
        out.append(OracleResult(plan=best, reward=reward, first_action_best=fab,
                                n_plans=n_plans, device_rewards=dev_r))
    return out


def _exhaustive_best_gpu(
    states: List[PlannerState], params: PlannerParams, device: str, prefix_len: int = 0
) -> List[OracleResult]:
    import torch

    from ..ops.native import load_extension

    ext = load_extension(required=True)  # a missing kernel on GPU is an error
    g = states[0].n_groups
    joint = isinstance(states[0], MultiPlannerState)
    if any(isinstance(s, MultiPlannerState) != joint for s in states):
        raise ValueError("one batch holds PlannerStates or MultiPlannerStates, not both")
    if g > MAX_GROUPS_DEV or params.max_depth > MAX_DEPTH_DEV:
        raise ValueError(f"GPU plan oracle supports G <= {MAX_GROUPS_DEV} and "
                         f"max_depth <= {MAX_DEPTH_DEV} (got G={g}, D={params.max_depth})")
    if any(s.n_groups != g for s in states):
        raise ValueError("all states of one batch must have the same number of groups")
    if joint and any(s.n_procs != states[0].n_procs for s in states):
        raise ValueError("all states of one batch must have the same number of processes")
    dev = torch.device(device)

    def stack(get) -> "torch.Tensor":
        return torch.from_numpy(np.stack([np.asarray(get(s), dtype=np.float32) for s in states])).to(dev)

    gs = stack(lambda s: s.group_score)
    gm = stack(lambda s: s.group_mb)
    gf = stack(lambda s: s.group_files)
    pr = stack(lambda s: s.proc_score)  # [S], or [S, P] of a joint batch
    cl = torch.tensor([float(s.remaining_clean_mb) for s in states], dtype=torch.float32, device=dev)
    search = ext.plan_oracle_multi_search if joint else ext.plan_oracle_search
    w_reward, w_len, w_plan, _meta = search(
        gs, gm, gf, pr, cl, _params_dict(g, params), int(prefix_len))
    n = states[0].n_actions - 1
    return _results_of_winners(states, params, w_reward, w_len, w_plan,
                               count_plans(n, params.max_depth))


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
    with the state's reward (`plan_reward`) in fp64 and the final plan is
    picked among them in fp64 with the module's tie-break.  On "cpu" the
    reference runs (its own cap, CPU_MAX_PLANS, applies as well).  A GPU batch
    holds PlannerStates or MultiPlannerStates, not both, and one (P, G).
    Raises ValueError on a batch that does not, when the plan count exceeds
    `max_plans`, and on non-finite inputs.  `prefix_len` overrides the GPU
    work decomposition (0 = automatic)."""
    params = params or PlannerParams()
    single = isinstance(state_or_states, (PlannerState, MultiPlannerState))
    states = [state_or_states] if single else list(state_or_states)
    if not states:
        return []
    for st in states:
        _check_state(st, params)
        n_plans = count_plans(st.n_actions - 1, params.max_depth)
        if n_plans > max_plans:
            raise _too_many(st, params, n_plans, max_plans)
    dev = str(device)
    if dev == "cpu" or params.max_depth < 1:
        res = [exhaustive_best_cpu(st, params, max_plans=min(max_plans, CPU_MAX_PLANS)) for st in states]
    else:
        res = _exhaustive_best_gpu(states, params, dev, prefix_len=prefix_len)
    return res[0] if single else res


def _as_joint(state) -> MultiPlannerState:
    """A PlannerState is the P = 1 joint state (same action ids, same reward)."""
    if isinstance(state, MultiPlannerState):
        return state
    return MultiPlannerState(state.group_score, state.group_mb, state.group_files,
                             np.array([state.proc_score], dtype=np.float64),
                             state.remaining_clean_mb)


def _ascending_plan(first_action: int, members: Sequence[int]) -> List[int]:
    return [int(first_action)] + [int(b) for b in sorted(members) if b != first_action]


# subset_best_cpu re-scores with plan_reward every set whose closed-form reward
# is within this relative distance of its first action's best: the closed form
# and simulate_plan_multi round differently, and only the latter breaks ties.
_NEAR_TIE_RTOL = 1e-9


def subset_best_cpu(state: PlannerState, params: Optional[PlannerParams] = None) -> OracleResult:
    """The exact optimum as a maximum over action sets (module docstring), in
    vectorised numpy fp64: no plan is simulated but the near-ties of each first
    action's winner, which `plan_reward` re-scores and `_better` decides.
    `n_plans` is the number of sets, `count_sets(n, D)`.  Needs no cap: a state
    has at most 2^25 sets."""
    params = params or PlannerParams()
    _check_state(state, params)
    joint = _as_joint(state)
    n_procs, g = joint.n_procs, joint.n_groups
    n = n_procs + 1 + g
    depth_lim = min(n, max(int(params.max_depth), 0))
    a_restore, a_revert = n_procs + 1, n_procs + 2
    ps = np.asarray(joint.proc_score, dtype=np.float64)
    score = np.asarray(joint.group_score, dtype=np.float64)
    mb = np.asarray(joint.group_mb, dtype=np.float64)
    dt_g = params.revert_time_s * np.maximum(np.asarray(joint.group_files, dtype=np.float64), 1.0)
    fp_g = (1.0 - score) * mb * 0.05
    un_g = score * mb
    rate, rem = params.attack_rate_mbps, float(joint.remaining_clean_mb)
    live0 = float(ps.sum())

    # per revert mask R: popcount and the sums over its groups, by doubling
    r_pop = np.zeros(1, dtype=np.int64)
    r_dt, r_fp, r_rec = np.zeros(1), np.zeros(1), np.zeros(1)
    for gi in range(g):
        r_pop = np.concatenate([r_pop, r_pop + 1])
        r_dt = np.concatenate([r_dt, r_dt + dt_g[gi]])
        r_fp = np.concatenate([r_fp, r_fp + fp_g[gi]])
        r_rec = np.concatenate([r_rec, r_rec + un_g[gi]])
    order = np.argsort(r_pop, kind="stable")  # by size, so a budget is a prefix
    r_mask, r_pop = order, r_pop[order]
    r_dt, r_fp, r_un = r_dt[order], r_fp[order], float(un_g.sum()) - r_rec[order]
    r_has = [((r_mask >> gi) & 1).astype(bool) for gi in range(g)]

    # first action -> [(closed-form reward, kill mask, restore, revert mask)]
    cands: Dict[int, List[Tuple[float, int, int, int]]] = {a: [] for a in range(1, n + 1)}

    def offer(a: int, rewards: np.ndarray, kmask: int, restore: int, rmasks: np.ndarray) -> None:
        if len(rewards):
            top = float(rewards.max())
            for i in np.nonzero(rewards >= top - _NEAR_TIE_RTOL * (1.0 + abs(top)))[0]:
                cands[a].append((float(rewards[i]), kmask, restore, int(rmasks[i])))

    for kmask in range(1 << n_procs):
        kills = [q for q in range(n_procs) if (kmask >> q) & 1]
        budget = depth_lim - len(kills)
        if budget < 0:
            continue
        live_k = float(sum(ps[q] for q in range(n_procs) if not (kmask >> q) & 1))
        alive = len(kills) < n_procs
        hz_og = rate * params.horizon_s * live_k if alive else 0.0
        fixed_dn = params.kill_time_s * len(kills) + (params.horizon_s * live_k if alive else 0.0)
        dlive = live0 - live_k

        def reward(og, dt, fp, un, stale):
            return -(un + np.minimum(og, rem) + stale
                     + params.downtime_weight * (fixed_dn + dt) + params.fp_weight * fp)

        # sets without RESTORE: kills first, then the reverts of R
        m = int(np.searchsorted(r_pop, budget, side="right"))
        og = rate * r_dt[:m] * live_k + hz_og
        base = reward(og, r_dt[:m], r_fp[:m], r_un[:m], 0.0)
        for q in kills:
            offer(1 + q, base, kmask, 0, r_mask[:m])
        for gi in range(g):
            sel = r_has[gi][:m]
            offer(a_revert + gi, reward(og[sel] + rate * dt_g[gi] * dlive, r_dt[:m][sel],
                                        r_fp[:m][sel], r_un[:m][sel], 0.0),
                  kmask, 0, r_mask[:m][sel])
        # sets with RESTORE: a revert next to it is a no-op unless it goes first
        if budget >= 1:
            og_r = rate * params.restore_time_s * live_k + hz_og
            zero = np.zeros(1, dtype=np.int64)
            base_r = np.atleast_1d(reward(og_r, params.restore_time_s, 0.0, 0.0, params.restore_loss_mb))
            for q in kills:
                offer(1 + q, base_r, kmask, 1, zero)
            offer(a_restore, np.atleast_1d(reward(og_r + rate * params.restore_time_s * dlive,
                                                  params.restore_time_s, 0.0, 0.0,
                                                  params.restore_loss_mb)), kmask, 1, zero)
        if budget >= 2:
            for gi in range(g):
                offer(a_revert + gi,
                      np.atleast_1d(reward(og_r + rate * dt_g[gi] * live0,
                                           params.restore_time_s + dt_g[gi], fp_g[gi], 0.0,
                                           params.restore_loss_mb)),
                      kmask, 1, np.array([1 << gi]))

    fab: Dict[int, Tuple[float, List[int]]] = {
        A_STOP: (float(plan_reward(state, [A_STOP], params)), [])
    }
    for a in range(1, n + 1) if depth_lim >= 1 else ():
        top = max(c[0] for c in cands[a])
        best_r, best_plan = 0.0, None
        for r, kmask, restore, rmask in cands[a]:
            if r < top - _NEAR_TIE_RTOL * (1.0 + abs(top)):
                continue  # a near-tie of another kill mask only
            members = ([1 + q for q in range(n_procs) if (kmask >> q) & 1]
                       + ([a_restore] if restore else [])
                       + [a_revert + gi for gi in range(g) if (rmask >> gi) & 1])
            plan = _ascending_plan(a, members)
            exact = float(plan_reward(state, plan + [A_STOP], params))
            if _better(exact, plan, best_r, best_plan):
                best_r, best_plan = exact, plan
        fab[a] = (best_r, best_plan)
    reward_best, best = _pick(fab)
    return OracleResult(plan=best, reward=reward_best, first_action_best=fab,
                        n_plans=count_sets(n, params.max_depth))


def _subset_best_gpu(states: List[PlannerState], params: PlannerParams, device: str) -> List[OracleResult]:
    import torch

    from ..ops.native import load_extension

    ext = load_extension(required=True)  # a missing kernel on GPU is an error
    joints = [_as_joint(s) for s in states]
    g, n_procs = joints[0].n_groups, joints[0].n_procs
    if any(s.n_groups != g or s.n_procs != n_procs for s in joints):
        raise ValueError("all states of one batch must have the same number of groups and processes")
    dev = torch.device(device)

    def stack(get) -> "torch.Tensor":
        return torch.from_numpy(np.stack([np.asarray(get(s), dtype=np.float32) for s in joints])).to(dev)

    cl = torch.tensor([float(s.remaining_clean_mb) for s in joints], dtype=torch.float32, device=dev)
    w_reward, w_len, w_plan, _meta = ext.plan_subsets_search(
        stack(lambda s: s.group_score), stack(lambda s: s.group_mb), stack(lambda s: s.group_files),
        stack(lambda s: s.proc_score), cl, _params_dict(g, params))
    return _results_of_winners(states, params, w_reward, w_len, w_plan,
                               count_sets(n_procs + 1 + g, params.max_depth))


def subset_best(
    state_or_states: Union[PlannerState, Sequence[PlannerState]],
    params: Optional[PlannerParams] = None,
    device: str = "cpu",
) -> Union[OracleResult, List[OracleResult]]:
    """Exact optimum of one state (-> OracleResult) or a batch (-> list) by
    search over action sets: no plan-count cap, any P <= 8 and G <= 16.

    On a GPU device one launch of ops/hip/plan_subsets.hip finds, per state,
    the best set under each first action in fp32; those n+1 winners are
    re-scored with `plan_reward` in fp64 and the plan is picked among them with
    the module's tie-break, as `exhaustive_best` does.  On "cpu" it is
    `subset_best_cpu`.  `n_plans` is the number of sets considered.  A
    PlannerState is searched as the P = 1 joint state; a GPU batch holds one
    (P, G).  Raises ValueError on a batch that does not, on non-finite
    inputs, and on a GPU device for max_depth > 16."""
    params = params or PlannerParams()
    single = isinstance(state_or_states, (PlannerState, MultiPlannerState))
    states = [state_or_states] if single else list(state_or_states)
    if not states:
        return []
    for st in states:
        _check_state(st, params)
    dev = str(device)
    if dev == "cpu" or params.max_depth < 1:
        res = [subset_best_cpu(st, params) for st in states]
    else:
        res = _subset_best_gpu(states, params, dev)
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
    return float(oracle.reward - plan_reward(state, list(plan) + [A_STOP], params))


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
    "CPU_MAX_PLANS", "GPU_MAX_PLANS", "GPU_MAX_PLANS_JOINT",
    "OracleResult", "REWARD_ATOL", "REWARD_RTOL", "canonical_plan", "count_plans", "count_sets",
    "exhaustive_best", "exhaustive_best_cpu", "plan_regret", "plans_under", "reward_tol",
    "sets_under", "subset_best", "subset_best_cpu",
]
