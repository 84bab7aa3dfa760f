"""Rollback-plan reward model.

Spec (reference README.md:115, architecture.mdx:64-72, threat-model.mdx:206-222):
  reward = restoration gain - side effects  ==  -(data_loss + 0.1 * downtime)

Concrete MDP used by both the CPU planner and the CDNA4 batched kernel:

State after executing a partial plan:
  * each candidate file group g has expected encrypted-but-unrecovered bytes;
  * the attack process is alive or killed; while alive, encryption continues
    at `attack_rate_mbps` against remaining un-encrypted target data;
  * every action costs wall time (downtime) and wrong actions on clean files
    add false-positive side effects (counted as data made unavailable).

All quantities are expectations under the detector's anomaly scores, so the
planner maximises  -(E[data_loss_MB] + 0.1 * downtime_s + fp_penalty_MB).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

# action ids (shared with the HIP kernel — keep in sync with mcts.hip)
A_STOP = 0
A_KILL = 1
A_RESTORE = 2  # restore everything from backup (reference threat-model.mdx:206-222)
A_REVERT_BASE = 3  # A_REVERT_BASE + g : revert file group g


@dataclass
class PlannerParams:
    n_groups: int = 8
    downtime_weight: float = 0.1
    revert_time_s: float = 0.05  # per-file rename-back (reference measured ~1 ms/file; batched overhead)
    kill_time_s: float = 0.5
    fp_weight: float = 1.0  # MB-equivalent penalty per wrongly-reverted MB
    attack_rate_mbps: float = 2.0  # reference simulator rate limit
    horizon_s: float = 60.0
    max_depth: int = 10
    # restore-from-backup (reference threat-model.mdx:206-222: "cost 100 —
    # data loss risk, confidence 1.0"): recovers every group at a large
    # fixed downtime plus the data written since the last backup
    restore_time_s: float = 30.0
    restore_loss_mb: float = 16.0


@dataclass
class PlannerState:
    """Detector output aggregated into file groups (score-bucketed)."""

    group_score: np.ndarray  # [G] mean anomaly score of group
    group_mb: np.ndarray  # [G] total MB in group
    group_files: np.ndarray  # [G] file count
    proc_score: float  # attack-process anomaly score
    remaining_clean_mb: float  # target data not yet encrypted

    @property
    def n_groups(self) -> int:
        return int(len(self.group_score))

    @property
    def n_actions(self) -> int:
        return 3 + self.n_groups  # STOP, KILL, RESTORE, revert g


def build_state(
    file_scores: np.ndarray,
    file_mb: np.ndarray,
    proc_score: float,
    remaining_clean_mb: float,
    n_groups: int = 8,
) -> PlannerState:
    """Bucket files by anomaly score into n_groups candidate groups."""
    order = np.argsort(-file_scores, kind="stable")
    gs = np.zeros(n_groups, dtype=np.float64)
    gm = np.zeros(n_groups, dtype=np.float64)
    gf = np.zeros(n_groups, dtype=np.float64)
    if len(order):
        split = np.array_split(order, n_groups)
        for g, ids in enumerate(split):
            if len(ids):
                gs[g] = float(file_scores[ids].mean())
                gm[g] = float(file_mb[ids].sum())
                gf[g] = float(len(ids))
    return PlannerState(
        group_score=gs,
        group_mb=gm,
        group_files=gf,
        proc_score=float(proc_score),
        remaining_clean_mb=float(remaining_clean_mb),
    )


def simulate_plan(
    state: PlannerState,
    actions: List[int],
    params: PlannerParams,
) -> float:
    """Expected reward of executing `actions` in order.

    Mirrors the device function `eval_plan` in ops/hip/mcts.hip — any change
    here must be mirrored there (tests assert bit-level agreement in fp32).
    """
    g = state.n_groups
    unrec = state.group_score * state.group_mb  # expected encrypted MB per group
    reverted = np.zeros(g, dtype=np.float64)
    fp_mb = 0.0
    downtime = 0.0
    alive = True
    restored = False
    staleness = 0.0
    ongoing = 0.0  # extra MB encrypted while we act
    for a in actions:
        if a == A_STOP:
            break
        if a == A_KILL:
            if alive:
                downtime += params.kill_time_s
                alive = False
            continue
        if a == A_RESTORE:
            if restored:
                continue
            dt = params.restore_time_s
            if alive:
                ongoing += params.attack_rate_mbps * dt * state.proc_score
            downtime += dt
            reverted[:] = 1.0
            staleness = params.restore_loss_mb
            restored = True
            continue
        gi = a - A_REVERT_BASE
        if gi < 0 or gi >= g or reverted[gi] > 0:
            continue  # invalid / duplicate: no-op
        dt = params.revert_time_s * max(state.group_files[gi], 1.0)
        if alive:
            ongoing += params.attack_rate_mbps * dt * state.proc_score
        downtime += dt
        reverted[gi] = 1.0
        fp_mb += (1.0 - state.group_score[gi]) * state.group_mb[gi] * 0.05
    if alive:  # attack keeps running until the horizon
        ongoing += params.attack_rate_mbps * params.horizon_s * state.proc_score
        # the service-degradation charge scales with our belief the process
        # is actually malicious: a clean state pays ~nothing for inaction
        downtime += params.horizon_s * state.proc_score
    loss = (
        float(((1.0 - reverted) * unrec).sum())
        + min(ongoing, state.remaining_clean_mb)
        + staleness
    )
    return -(loss + params.downtime_weight * downtime + params.fp_weight * fp_mb)


# ---- joint plan over P processes (ops/hip/mcts_multi.hip) ----
#
# action ids: 0 STOP | 1 + p KILL process p | P + 1 RESTORE | P + 2 + g REVERT g
# (P = 1 is the numbering above)
MAX_PROCS = 8
MAX_GROUPS = 16


@dataclass
class MultiPlannerState:
    """PlannerState with P attack processes instead of one."""

    group_score: np.ndarray  # [G]
    group_mb: np.ndarray  # [G]
    group_files: np.ndarray  # [G]
    proc_score: np.ndarray  # [P] anomaly score per process
    remaining_clean_mb: float
    # [G] process index each group's files are attributed to: bookkeeping for
    # the engine and describe_multi, never read by the reward
    group_owner: Optional[np.ndarray] = None

    def __post_init__(self) -> None:
        self.proc_score = np.atleast_1d(np.asarray(self.proc_score, dtype=np.float64))
        if not 1 <= len(self.proc_score) <= MAX_PROCS:
            raise ValueError(f"a joint plan covers 1..{MAX_PROCS} processes (got {len(self.proc_score)})")
        if len(self.group_score) > MAX_GROUPS:
            raise ValueError(f"a joint plan covers at most {MAX_GROUPS} groups (got {len(self.group_score)})")

    @property
    def n_groups(self) -> int:
        return int(len(self.group_score))

    @property
    def n_procs(self) -> int:
        return int(len(self.proc_score))

    @property
    def n_actions(self) -> int:
        return self.n_procs + 2 + self.n_groups


def simulate_plan_multi(
    state: MultiPlannerState,
    actions: List[int],
    params: PlannerParams,
) -> float:
    """`simulate_plan` with P processes: each KILL stops one of them, and what
    the attack adds while we act scales with `live`, the summed score of the
    processes still alive.

    Mirrors `eval_plan_multi` in ops/hip/mcts_multi.hip.  `live` is summed in
    ascending p from zero after every KILL (never decremented), so host and
    device add in one order.  For P = 1 the value equals `simulate_plan`'s.

    The search over action sets (oracle.subset_best, ops/hip/plan_subsets.hip)
    relies on this function's structure: everything but `ongoing` depends only
    on the set of executed actions, a KILL adds nothing to `ongoing`, and the
    loss never decreases in it.  A change that breaks any of these breaks it.
    """
    g = state.n_groups
    n_procs = state.n_procs
    a_restore = n_procs + 1
    unrec = state.group_score * state.group_mb
    reverted = np.zeros(g, dtype=np.float64)
    fp_mb = 0.0
    downtime = 0.0
    alive = [True] * n_procs
    live = 0.0
    for p in range(n_procs):
        live += float(state.proc_score[p])
    restored = False
    staleness = 0.0
    ongoing = 0.0
    for a in actions:
        if a == A_STOP:
            break
        if 1 <= a <= n_procs:
            if alive[a - 1]:
                downtime += params.kill_time_s
                alive[a - 1] = False
                live = 0.0
                for p in range(n_procs):
                    if alive[p]:
                        live += float(state.proc_score[p])
            continue
        if a == a_restore:
            if restored:
                continue
            dt = params.restore_time_s
            ongoing += params.attack_rate_mbps * dt * live
            downtime += dt
            reverted[:] = 1.0
            staleness = params.restore_loss_mb
            restored = True
            continue
        gi = a - (n_procs + 2)
        if gi < 0 or gi >= g or reverted[gi] > 0:
            continue  # invalid / duplicate: no-op
        dt = params.revert_time_s * max(state.group_files[gi], 1.0)
        ongoing += params.attack_rate_mbps * dt * live
        downtime += dt
        reverted[gi] = 1.0
        fp_mb += (1.0 - state.group_score[gi]) * state.group_mb[gi] * 0.05
    if any(alive):
        ongoing += params.attack_rate_mbps * params.horizon_s * live
        downtime += params.horizon_s * live
    loss = (
        float(((1.0 - reverted) * unrec).sum())
        + min(ongoing, state.remaining_clean_mb)
        + staleness
    )
    return -(loss + params.downtime_weight * downtime + params.fp_weight * fp_mb)


def plan_reward(state, actions: List[int], params: PlannerParams) -> float:
    """The state's own reward: `simulate_plan_multi` for a MultiPlannerState,
    `simulate_plan` otherwise."""
    if isinstance(state, MultiPlannerState):
        return simulate_plan_multi(state, actions, params)
    return simulate_plan(state, actions, params)
