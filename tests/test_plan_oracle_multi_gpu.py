"""The joint plan oracle's kernel (ops/hip/plan_oracle_multi.hip) against the
fp64 CPU reference, at the smallest shapes where it can go wrong."""
import functools

import numpy as np
import pytest
import torch

from nerrf_amd.planner.mcts import multi_params_dict, multi_state_tensors
from nerrf_amd.planner.oracle import (_params_dict, exhaustive_best, exhaustive_best_cpu,
                                      plan_regret, reward_tol)
from nerrf_amd.planner.rewards import MultiPlannerState, PlannerParams, PlannerState
from nerrf_amd.serve.engine import StreamingEngine
from test_plan_joint import (FIXED_PARAMS, FIXED_STATE, CpuEngine, multi_state,
                             two_culprit_detection)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from nerrf_amd.ops.native import load_extension

    return load_extension(required=True)


@functools.lru_cache(maxsize=None)
def _cpu_ref(n_procs, n_groups, depth):  # computed once, shared between tests
    if (n_procs, n_groups) == (2, 3):
        st, params = FIXED_STATE, FIXED_PARAMS
    else:
        st = multi_state(n_procs, n_groups, seed=10 * n_procs + n_groups)
        params = PlannerParams(n_groups=n_groups, max_depth=depth)
    return st, params, exhaustive_best_cpu(st, params)


def _check_against_cpu(st, params, gpu, ref, device, ext):
    n = st.n_actions - 1
    assert gpu.n_plans == ref.n_plans
    print(f"P={st.n_procs} G={st.n_groups} D={params.max_depth}: gpu {gpu.plan} {gpu.reward:.6f}  "
          f"cpu {ref.plan} {ref.reward:.6f}")
    assert set(gpu.first_action_best) == set(range(0, n + 1))
    plans = np.zeros((n + 1, 16), dtype=np.int32)
    for a in range(0, n + 1):
        r_gpu, plan = gpu.first_action_best[a]
        r_cpu, _ = ref.first_action_best[a]
        assert abs(r_gpu - r_cpu) <= reward_tol(r_cpu), (a, plan, r_gpu, r_cpu)
        plans[a, : len(plan)] = plan
    dev_eval = ext.mcts_multi_eval_plans(*multi_state_tensors(st, device), multi_params_dict(st, params),
                                         torch.from_numpy(plans).to(device)).cpu().numpy()
    for a in range(0, n + 1):  # exact: both are eval_plan_multi on the same plan
        assert np.float32(gpu.device_rewards[a]) == dev_eval[a], (a, gpu.device_rewards[a], dev_eval[a])
    assert plan_regret(st, gpu.plan, params, oracle=ref) <= reward_tol(ref.reward)


@pytest.mark.parametrize("n_procs,n_groups,depth", [
    (1, 1, 10),   # 16 plans: n = 3 < depth, fewer items than one wave
    (2, 3, 5),    # 1 237 plans: the state the CPU tests pin
    (3, 4, 6),    # 28 961 plans: more than one block of work items
    (8, 2, 4),    # 9 032 plans: all eight processes in the live sum
    (8, 16, 3),   # 14 426 plans: action ids up to 25, revert bits above bit 16
])
def test_joint_oracle_matches_cpu_reference(gpu_device, ext, n_procs, n_groups, depth):
    st, params, ref = _cpu_ref(n_procs, n_groups, depth)
    gpu = exhaustive_best(st, params, device=str(gpu_device))
    _check_against_cpu(st, params, gpu, ref, gpu_device, ext)
    if n_procs == 1:  # the single-process oracle searches the same MDP
        one = exhaustive_best(PlannerState(st.group_score, st.group_mb, st.group_files,
                                           float(st.proc_score[0]), st.remaining_clean_mb),
                              params, device=str(gpu_device))
        assert one.n_plans == gpu.n_plans == 16
        for a, (r, _plan) in one.first_action_best.items():
            assert abs(gpu.first_action_best[a][0] - r) <= reward_tol(r)


def test_joint_oracle_is_independent_of_the_work_split(gpu_device, ext):
    st, params, ref = _cpu_ref(3, 4, 6)
    runs = [exhaustive_best(st, params, device=str(gpu_device), prefix_len=pl) for pl in (0, 1, 3)]
    for gpu in runs:
        _check_against_cpu(st, params, gpu, ref, gpu_device, ext)
        # same fp32 arithmetic, same tie-break: identical winners
        assert gpu.first_action_best == runs[0].first_action_best
        assert gpu.device_rewards == runs[0].device_rewards


def test_joint_oracle_exact_tie_and_clean_state(gpu_device):
    params = PlannerParams(n_groups=2, max_depth=5)
    tie = MultiPlannerState(np.array([0.9, 0.9]), np.array([2.0, 2.0]), np.array([3.0, 3.0]),
                            np.array([0.9, 0.9]), remaining_clean_mb=30.0)
    clean = MultiPlannerState(np.zeros(2), np.full(2, 2.0), np.full(2, 3.0), np.zeros(2),
                              remaining_clean_mb=30.0)
    gpu_tie, gpu_clean = exhaustive_best([tie, clean], params, device=str(gpu_device))
    cpu_tie = exhaustive_best_cpu(tie, params)
    assert gpu_tie.plan == cpu_tie.plan and len(cpu_tie.plan) >= 2
    assert gpu_tie.device_rewards[1] == gpu_tie.device_rewards[2]  # KILL 0 / KILL 1
    assert gpu_tie.device_rewards[4] == gpu_tie.device_rewards[5]  # REVERT 0 / REVERT 1
    assert plan_regret(tie, cpu_tie.plan, params, device=str(gpu_device)) == 0.0
    assert gpu_clean.plan == exhaustive_best_cpu(clean, params).plan == []
    assert gpu_clean.reward == 0.0


@pytest.mark.parametrize("n_procs,n_groups,depth", [
    (9, 3, 10), (2, 17, 10), (2, 3, 17),
    (8, 16, 16),  # 4.4e19 plans: over the binding's own bound, 2^31 - 1
])
def test_binding_refuses_what_the_kernel_cannot_take(gpu_device, ext, n_procs, n_groups, depth):
    f32 = lambda *shape: torch.full(shape, 0.5, dtype=torch.float32, device=gpu_device)
    pd = _params_dict(n_groups, PlannerParams(n_groups=n_groups, max_depth=depth))
    with pytest.raises(ValueError):
        ext.plan_oracle_multi_search(f32(1, n_groups), f32(1, n_groups), f32(1, n_groups),
                                     f32(1, n_procs), f32(1), pd, 0)


def test_oracle_refuses_too_many_plans_and_mixed_batches(gpu_device):
    with pytest.raises(ValueError, match="P=2"):
        exhaustive_best(FIXED_STATE, FIXED_PARAMS, device=str(gpu_device), max_plans=10)
    single = PlannerState(FIXED_STATE.group_score, FIXED_STATE.group_mb, FIXED_STATE.group_files,
                          0.9, FIXED_STATE.remaining_clean_mb)
    with pytest.raises(ValueError):
        exhaustive_best([FIXED_STATE, single], FIXED_PARAMS, device=str(gpu_device))
    with pytest.raises(ValueError):
        exhaustive_best([FIXED_STATE, multi_state(3, 3, seed=1)], FIXED_PARAMS, device=str(gpu_device))


def test_plan_joint_exact_gpu_equals_cpu(gpu_device):
    class SmallCpuEngine(CpuEngine):
        planner_params = PlannerParams(n_groups=4, max_depth=4)  # P=2, G=4: 1100 plans

    class SmallGpuEngine(SmallCpuEngine):
        device = gpu_device

    det = two_culprit_detection()
    gpu = StreamingEngine.plan_joint(SmallGpuEngine(), det, planner="exact")
    cpu = StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="exact", use_gpu=False)
    assert (gpu.plan, gpu.root_value, gpu.simulations) == (cpu.plan, cpu.root_value, 1100)
    assert sorted(a for a, _q, _n in gpu.ranked_actions) == list(range(0, 8))
    assert (gpu.proc_keys, gpu.group_owner, gpu.group_paths, gpu.unplanned) == (
        cpu.proc_keys, cpu.group_owner, cpu.group_paths, cpu.unplanned)
