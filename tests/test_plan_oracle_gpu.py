"""GPU plan oracle (ops/hip/plan_oracle.hip) against the CPU reference, at the
smallest shapes where the kernel can go wrong."""
import numpy as np
import pytest
import torch

from nerrf_amd.planner.oracle import (REWARD_ATOL, REWARD_RTOL, _params_dict,
                                      count_plans, exhaustive_best,
                                      exhaustive_best_cpu, plan_regret, reward_tol)
from nerrf_amd.planner.rewards import (A_KILL, A_RESTORE, A_STOP, PlannerParams,
                                       PlannerState, build_state, simulate_plan)

pytestmark = pytest.mark.gpu


def _state(n_groups, seed):
    rng = np.random.default_rng(seed)
    scores = rng.uniform(0.0, 1.0, 40)
    mb = rng.uniform(0.1, 8.0, 40)
    return build_state(scores, mb, proc_score=float(rng.uniform(0.3, 1.0)),
                       remaining_clean_mb=float(mb.sum() * 0.8), n_groups=n_groups)


def _close(a, b):
    return abs(a - b) <= REWARD_ATOL + REWARD_RTOL * abs(b)


_CPU_REF = {}


def _cpu_ref(n_groups, depth, seed):
    key = (n_groups, depth, seed)
    if key not in _CPU_REF:  # computed once, shared between tests
        st = _state(n_groups, seed)
        _CPU_REF[key] = (st, exhaustive_best_cpu(st, PlannerParams(n_groups=n_groups, max_depth=depth)))
    return _CPU_REF[key]


def _check_against_cpu(st, params, gpu, ref, device):
    from nerrf_amd.ops.native import load_extension

    ext = load_extension(required=True)
    n = 2 + st.n_groups
    assert gpu.n_plans == ref.n_plans == count_plans(n, params.max_depth)
    print(f"G={st.n_groups} D={params.max_depth}: gpu {gpu.plan} {gpu.reward:.6f}  "
          f"cpu {ref.plan} {ref.reward:.6f}")
    assert gpu.reward == simulate_plan(st, gpu.plan + [A_STOP], params)
    assert _close(gpu.reward, ref.reward)
    assert set(gpu.first_action_best) == set(ref.first_action_best) == set(range(0, n + 1))
    gs = torch.from_numpy(st.group_score.astype(np.float32)).to(device)
    gm = torch.from_numpy(st.group_mb.astype(np.float32)).to(device)
    gf = torch.from_numpy(st.group_files.astype(np.float32)).to(device)
    plans = np.zeros((n + 1, 16), dtype=np.int32)
    for a in range(0, n + 1):
        r_gpu, plan = gpu.first_action_best[a]
        r_cpu, _ = ref.first_action_best[a]
        assert (plan[0] if plan else A_STOP) == a
        assert len(set(plan)) == len(plan) <= min(n, params.max_depth)
        assert _close(r_gpu, r_cpu), (a, plan, r_gpu, r_cpu)
        plans[a, : len(plan)] = plan
    dev_eval = ext.mcts_eval_plans(
        gs, gm, gf, float(np.float32(st.proc_score)), float(np.float32(st.remaining_clean_mb)),
        _params_dict(st.n_groups, params), torch.from_numpy(plans).to(device)).cpu().numpy()
    for a in range(0, n + 1):  # exact: both are eval_plan on the same plan
        assert np.float32(gpu.device_rewards[a]) == dev_eval[a], (a, gpu.device_rewards[a], dev_eval[a])


@pytest.mark.parametrize("n_groups,depth", [
    (1, 1),    # 4 plans: fewer than one wave
    (3, 5),    # D == n: full permutations
    (4, 3),    # D < n
    (5, 10),   # D > n, clipped; 13 700 plans, work items not a multiple of the block
    (16, 3),   # 5 221 plans: MAX_GROUPS edge of the bitmask
])
def test_gpu_oracle_matches_cpu_reference(gpu_device, n_groups, depth):
    st, ref = _cpu_ref(n_groups, depth, seed=20 + n_groups)
    params = PlannerParams(n_groups=n_groups, max_depth=depth)
    gpu = exhaustive_best(st, params, device=str(gpu_device))
    _check_against_cpu(st, params, gpu, ref, gpu_device)


@pytest.mark.parametrize("prefix_len", [1, 2, 3, 7])
def test_gpu_oracle_is_independent_of_the_work_split(gpu_device, prefix_len):
    st, ref = _cpu_ref(5, 10, seed=25)
    params = PlannerParams(n_groups=5, max_depth=10)
    gpu = exhaustive_best(st, params, device=str(gpu_device), prefix_len=prefix_len)
    _check_against_cpu(st, params, gpu, ref, gpu_device)


def test_gpu_oracle_batch_of_three_states(gpu_device):
    params = PlannerParams(n_groups=3, max_depth=5)
    refs = [_cpu_ref(3, 5, seed=s) for s in (23, 41, 42)]
    states = [st for st, _ in refs]
    out = exhaustive_best(states, params, device=str(gpu_device))
    assert len(out) == 3
    for (st, ref), gpu in zip(refs, out):
        _check_against_cpu(st, params, gpu, ref, gpu_device)
    # really different states, each answered from its own row of the batch
    assert len({o.first_action_best[A_KILL][0] for o in out}) == 3


def test_gpu_oracle_exact_tie_and_clean_state(gpu_device):
    params = PlannerParams(n_groups=3, max_depth=5)
    tie = PlannerState(
        group_score=np.array([0.9, 0.9, 0.9]), group_mb=np.array([2.0, 2.0, 2.0]),
        group_files=np.array([3.0, 3.0, 3.0]), proc_score=0.9, remaining_clean_mb=30.0)
    clean = PlannerState(
        group_score=np.zeros(3), group_mb=np.full(3, 2.0), group_files=np.full(3, 3.0),
        proc_score=0.0, remaining_clean_mb=30.0)
    gpu_tie, gpu_clean = exhaustive_best([tie, clean], params, device=str(gpu_device))
    cpu_tie = exhaustive_best_cpu(tie, params)
    cpu_clean = exhaustive_best_cpu(clean, params)
    assert gpu_tie.plan == cpu_tie.plan == [1, 3, 4, 5]
    assert gpu_clean.plan == cpu_clean.plan == []
    assert gpu_clean.reward == 0.0
    # ties inside a first action are exact by symmetry too
    for a, (_r, plan) in cpu_tie.first_action_best.items():
        assert gpu_tie.first_action_best[a][1] == plan, a


def test_gpu_oracle_default_configuration(gpu_device):
    from nerrf_amd.planner.mcts import run_mcts_gpu

    params = PlannerParams()  # G=8, D=10
    st = _state(8, seed=2)
    orc = exhaustive_best(st, params, device=str(gpu_device))
    assert orc.n_plans == 9864101
    assert orc.reward == simulate_plan(st, orc.plan + [A_STOP], params)
    tol = reward_tol(orc.reward)
    # the automatic split (L=6) leaves the search 4 levels; L=1 walks 9 levels
    # per lane.  Same fp32 arithmetic, same tie-break: identical winners.
    deep = exhaustive_best(st, params, device=str(gpu_device), prefix_len=1)
    assert deep.plan == orc.plan
    assert deep.first_action_best == orc.first_action_best
    assert deep.device_rewards == orc.device_rewards
    mcts = run_mcts_gpu(st, params, n_sims=1024, seed=1, device=str(gpu_device))
    regret = plan_regret(st, mcts.plan, params, oracle=orc)
    print(f"oracle {orc.plan} {orc.reward:.4f}  mcts {mcts.plan}  regret {regret:.4f}")
    assert regret >= -tol
    # the hand-built candidates StreamingEngine._refine_plan scores
    top_reverts = [a for a, _v, _n in mcts.ranked_actions if a >= 3][:3]
    cands = [list(mcts.plan), [A_KILL] + top_reverts, [A_KILL, A_RESTORE],
             [A_KILL] + list(mcts.plan)]
    for c in cands:
        assert orc.reward >= simulate_plan(st, c + [A_STOP], params) - tol, c


def test_engine_exact_planner_on_gpu(gpu_device):
    from nerrf_amd.serve.engine import Detection, StreamingEngine

    eng = StreamingEngine(device=str(gpu_device))
    eng.planner_params = PlannerParams(n_groups=4, max_depth=5)
    rng = np.random.default_rng(0)
    file_scores = {f"/data/f{i}.bin": float(s) for i, s in enumerate(rng.uniform(0, 1, 12))}
    file_mb = {p: float(m) for p, m in zip(file_scores, rng.uniform(0.1, 3.0, 12))}
    det = Detection(alarm=True, t_detect=0.0, file_scores=file_scores, file_mb=file_mb,
                    proc_scores={4242: 0.95})
    res = eng.plan(det, planner="exact")
    paths = list(file_scores)
    state = build_state(np.array([file_scores[p] for p in paths]),
                        np.array([max(file_mb[p], 0.01) for p in paths]),
                        proc_score=0.95, remaining_clean_mb=float(sum(file_mb.values())),
                        n_groups=4)
    ref = exhaustive_best_cpu(state, eng.planner_params)
    assert res.simulations == ref.n_plans == count_plans(6, 5)
    assert res.root_value == simulate_plan(state, res.plan + [A_STOP], eng.planner_params)
    assert _close(res.root_value, ref.reward)
    qs = [q for _a, q, _n in res.ranked_actions]
    assert qs == sorted(qs, reverse=True) and len(qs) == 7
    for a, q, _n in res.ranked_actions:
        assert _close(q, ref.first_action_best[a][0])
