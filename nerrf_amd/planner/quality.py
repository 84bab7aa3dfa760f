"""Plan-quality measurement: MCTS regret against the exhaustive oracle.

State generator (`generate_states`).  State i of a run is drawn from
`np.random.default_rng([seed, i])` and cycles through three kinds, so any
N >= 3 covers all of them:

  attack  (i % 3 == 0)  40 files; a random 30-70 % of them score
                        U(0.75, 1.0), the rest U(0, 0.15); proc_score
                        U(0.8, 1.0) — a live encryptor with a clear victim set
  mixed   (i % 3 == 1)  40 files with scores U(0, 1); proc_score U(0.2, 0.9)
                        — an ambiguous detection
  clean   (i % 3 == 2)  40 files with scores U(0, 0.05); proc_score U(0, 0.05)
                        — nothing to undo; the empty plan should be near-optimal

File sizes are U(0.1, 8) MB; remaining_clean_mb is U(0.2, 1.5) times the
total size.  Files are bucketed into groups by `rewards.build_state`, exactly
as `StreamingEngine.plan` does.

Joint states (`n_procs` P > 1, `generate_joint_state`).  The same draws in the
same order give the files, their scores and sizes; the kind's proc_score
distribution is then drawn P times, once per process.  The 40 files are
attributed to the processes by shares: every process gets
`per_proc = min(n_groups, 16) // P` files, and the remaining files are split
by a multinomial over Dirichlet(1, ..., 1) shares; which files a process gets
is a random permutation.  Each process's files are bucketed by score into
`per_proc` groups with `rewards.build_state`, as `StreamingEngine.plan_joint`
does, so every state of a run has G = P * per_proc groups (no bucket is
empty) and one oracle batch serves the run.  The planner measured is
`run_mcts_multi` (`run_mcts_multi_gpu` on a GPU device).
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from .mcts import run_mcts, run_mcts_gpu, run_mcts_multi, run_mcts_multi_gpu
from .oracle import exhaustive_best, plan_regret, reward_tol, subset_best
from .rewards import (MAX_GROUPS, MAX_PROCS, MultiPlannerState, PlannerParams, PlannerState,
                      build_state)

KINDS = ("attack", "mixed", "clean")
N_FILES = 40


def _draw(rng, index: int, n_procs: int):
    """The module docstring's draws: (scores, mb, proc [n_procs], clean_mb)."""
    kind = KINDS[index % 3]
    mb = rng.uniform(0.1, 8.0, N_FILES)
    if kind == "attack":
        hit = rng.random(N_FILES) < rng.uniform(0.3, 0.7)
        scores = np.where(hit, rng.uniform(0.75, 1.0, N_FILES), rng.uniform(0.0, 0.15, N_FILES))
        proc = rng.uniform(0.8, 1.0, n_procs)
    elif kind == "mixed":
        scores = rng.uniform(0.0, 1.0, N_FILES)
        proc = rng.uniform(0.2, 0.9, n_procs)
    else:
        scores = rng.uniform(0.0, 0.05, N_FILES)
        proc = rng.uniform(0.0, 0.05, n_procs)
    clean_mb = float(mb.sum() * rng.uniform(0.2, 1.5))
    return scores, mb, proc, clean_mb


def generate_state(seed: int, index: int, n_groups: int = 8) -> PlannerState:
    rng = np.random.default_rng([int(seed), int(index)])
    scores, mb, proc, clean_mb = _draw(rng, index, 1)
    return build_state(scores, mb, proc_score=float(proc[0]), remaining_clean_mb=clean_mb,
                       n_groups=n_groups)


def generate_joint_state(seed: int, index: int, n_procs: int, n_groups: int = 8) -> MultiPlannerState:
    if not 1 <= n_procs <= min(n_groups, MAX_PROCS):
        raise ValueError(f"n_procs must lie in 1..min(n_groups, {MAX_PROCS}) (got {n_procs})")
    rng = np.random.default_rng([int(seed), int(index)])
    scores, mb, proc, clean_mb = _draw(rng, index, n_procs)
    per_proc = min(n_groups, MAX_GROUPS) // n_procs
    counts = per_proc + rng.multinomial(N_FILES - n_procs * per_proc, rng.dirichlet(np.ones(n_procs)))
    file_owner = rng.permutation(np.repeat(np.arange(n_procs), counts))
    parts = [build_state(scores[file_owner == p], mb[file_owner == p], proc_score=0.0,
                         remaining_clean_mb=clean_mb, n_groups=per_proc) for p in range(n_procs)]
    return MultiPlannerState(
        group_score=np.concatenate([s.group_score for s in parts]),
        group_mb=np.concatenate([s.group_mb for s in parts]),
        group_files=np.concatenate([s.group_files for s in parts]),
        proc_score=proc, remaining_clean_mb=clean_mb,
        group_owner=np.repeat(np.arange(n_procs), per_proc))


def generate_states(n_states: int, seed: int, n_groups: int = 8, n_procs: int = 1) -> List:
    if n_procs == 1:
        return [generate_state(seed, i, n_groups) for i in range(int(n_states))]
    return [generate_joint_state(seed, i, n_procs, n_groups) for i in range(int(n_states))]


def measure_plan_quality(
    n_states: int,
    seed: int,
    sims: Sequence[int] = (128, 512, 1024),
    device: str = "cpu",
    params: Optional[PlannerParams] = None,
    mcts_seed: int = 1,
    n_procs: int = 1,
    oracle: str = "exact",
) -> Dict:
    """Regret of the MCTS planner at each simulation budget, against the
    exhaustive oracle, over `n_states` generated states.  On a GPU device both
    the oracle and MCTS run their HIP kernels.  `n_procs` > 1 measures the
    joint planner on joint states; the report then carries "n_procs", and its
    "n_groups" is the states' G.  `oracle` "exact" enumerates every plan
    (exhaustive_best, with its plan-count cap); "sets" searches action sets
    (subset_best: any P <= 8), and "plans_per_state" then counts sets."""
    if oracle not in ("exact", "sets"):
        raise ValueError(f"unknown oracle {oracle!r}: expected 'exact' or 'sets'")
    params = params or PlannerParams()
    best = exhaustive_best if oracle == "exact" else subset_best
    states = generate_states(n_states, seed, params.n_groups, n_procs)
    on_gpu = str(device) != "cpu"
    if n_procs == 1:
        mcts = run_mcts_gpu if on_gpu else run_mcts
    else:
        mcts = run_mcts_multi_gpu if on_gpu else run_mcts_multi
    dev_kw = {"device": str(device)} if on_gpu else {}
    if on_gpu:
        import torch

        best(states[:1], params, device=device)  # warm-up: module load
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    oracles = best(states, params, device=device)
    oracle_s = time.perf_counter() - t0
    report: Dict = {
        "states": len(states),
        "seed": int(seed),
        "device": str(device),
        "n_groups": params.n_groups,
        "max_depth": params.max_depth,
        "plans_per_state": oracles[0].n_plans if oracles else 0,
        "oracle_s_per_state": oracle_s / max(len(states), 1),
        "budgets": {},
    }
    if oracle != "exact":
        report["oracle"] = oracle
    if n_procs > 1:
        report["n_procs"] = int(n_procs)
        report["n_groups"] = states[0].n_groups if states else 0
    for n_sims in sims:
        regrets, optimal = [], 0
        for st, orc in zip(states, oracles):
            res = mcts(st, params, n_sims=int(n_sims), seed=mcts_seed, **dev_kw)
            reg = plan_regret(st, res.plan, params, oracle=orc)
            regrets.append(reg)
            optimal += int(reg <= reward_tol(orc.reward))
        arr = np.array(regrets, dtype=np.float64)
        report["budgets"][str(int(n_sims))] = {
            "mean_regret": float(arr.mean()),
            "median_regret": float(np.median(arr)),
            "max_regret": float(arr.max()),
            "min_regret": float(arr.min()),
            "optimal_share": optimal / max(len(states), 1),
        }
    return report
