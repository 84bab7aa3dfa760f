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
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from .mcts import run_mcts, run_mcts_gpu
from .oracle import exhaustive_best, plan_regret, reward_tol
from .rewards import PlannerParams, PlannerState, build_state

KINDS = ("attack", "mixed", "clean")
N_FILES = 40


def generate_state(seed: int, index: int, n_groups: int = 8) -> PlannerState:
    rng = np.random.default_rng([int(seed), int(index)])
    kind = KINDS[index % 3]
    mb = rng.uniform(0.1, 8.0, N_FILES)
    if kind == "attack":
        hit = rng.random(N_FILES) < rng.uniform(0.3, 0.7)
        scores = np.where(hit, rng.uniform(0.75, 1.0, N_FILES), rng.uniform(0.0, 0.15, N_FILES))
        proc = rng.uniform(0.8, 1.0)
    elif kind == "mixed":
        scores = rng.uniform(0.0, 1.0, N_FILES)
        proc = rng.uniform(0.2, 0.9)
    else:
        scores = rng.uniform(0.0, 0.05, N_FILES)
        proc = rng.uniform(0.0, 0.05)
    clean_mb = float(mb.sum() * rng.uniform(0.2, 1.5))
    return build_state(scores, mb, proc_score=float(proc), remaining_clean_mb=clean_mb,
                       n_groups=n_groups)


def generate_states(n_states: int, seed: int, n_groups: int = 8) -> List[PlannerState]:
    return [generate_state(seed, i, n_groups) for i in range(int(n_states))]


def measure_plan_quality(
    n_states: int,
    seed: int,
    sims: Sequence[int] = (128, 512, 1024),
    device: str = "cpu",
    params: Optional[PlannerParams] = None,
    mcts_seed: int = 1,
) -> Dict:
    """Regret of the MCTS planner at each simulation budget, against the
    exhaustive oracle, over `n_states` generated states.  On a GPU device both
    the oracle and MCTS run their HIP kernels."""
    params = params or PlannerParams()
    states = generate_states(n_states, seed, params.n_groups)
    on_gpu = str(device) != "cpu"
    if on_gpu:
        import torch

        exhaustive_best(states[:1], params, device=device)  # warm-up: module load
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    oracles = exhaustive_best(states, params, device=device)
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
    for n_sims in sims:
        regrets, optimal = [], 0
        for st, orc in zip(states, oracles):
            if on_gpu:
                res = run_mcts_gpu(st, params, n_sims=int(n_sims), seed=mcts_seed, device=str(device))
            else:
                res = run_mcts(st, params, n_sims=int(n_sims), seed=mcts_seed)
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
