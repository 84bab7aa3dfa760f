"""The subset plan search kernel (ops/hip/plan_subsets.hip) against the fp64 CPU
references, at the smallest shapes where it can go wrong."""
import functools

import numpy as np
import pytest
import torch

from nerrf_amd.planner.mcts import multi_params_dict, multi_state_tensors
from nerrf_amd.planner.oracle import (_params_dict, count_sets, exhaustive_best_cpu, plan_regret,
                                      reward_tol, subset_best, subset_best_cpu)
from nerrf_amd.planner.rewards import PlannerParams
from nerrf_amd.serve.engine import StreamingEngine
from test_plan_joint import CpuEngine, multi_state, two_culprit_detection
from test_plan_subsets import shape_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from nerrf_amd.ops.native import load_extension

    return load_extension(required=True)


@functools.lru_cache(maxsize=None)
def _ref(n_procs, n_groups, depth, restore_loss_mb=None):  # computed once, shared between tests
    st, params = shape_state(n_procs, n_groups, depth)
    if restore_loss_mb is not None:
        params = PlannerParams(n_groups=n_groups, max_depth=depth, restore_loss_mb=restore_loss_mb)
        return st, params, subset_best_cpu(st, params)
    return st, params, exhaustive_best_cpu(st, params)


def _check(st, params, gpu, ref, device, ext):
    n = st.n_actions - 1
    assert gpu.n_plans == count_sets(n, params.max_depth)
    print(f"P={st.n_procs} G={st.n_groups} D={params.max_depth}: gpu {gpu.plan} {gpu.reward:.6f}  "
          f"ref {ref.plan} {ref.reward:.6f}")
    assert set(gpu.first_action_best) == set(range(0, n + 1))
    plans = np.zeros((n + 1, 16), dtype=np.int32)
    for a in range(0, n + 1):
        r_gpu, plan = gpu.first_action_best[a]
        r_ref, _ = ref.first_action_best[a]
        assert abs(r_gpu - r_ref) <= reward_tol(r_ref), (a, plan, r_gpu, r_ref)
        assert plan[:1] == ([a] if a else []) and len(plan) <= min(n, params.max_depth)
        plans[a, : len(plan)] = plan
    dev_eval = ext.mcts_multi_eval_plans(*multi_state_tensors(st, device), multi_params_dict(st, params),
                                         torch.from_numpy(plans).to(device)).cpu().numpy()
    for a in range(0, n + 1):  # exact: both are eval_plan_multi on the same plan
        assert np.float32(gpu.device_rewards[a]) == dev_eval[a], (a, gpu.device_rewards[a], dev_eval[a])
    assert plan_regret(st, gpu.plan, params, oracle=ref) <= reward_tol(ref.reward)


@pytest.mark.parametrize("n_procs,n_groups,depth", [
    (1, 1, 10),   # n = 3 < depth; two masks per unit, a padded block
    (2, 3, 5),    # the state the CPU tests pin
    (3, 4, 6),    # more than one block of units
    (8, 2, 4),    # all eight processes in the live sum; units beyond the depth budget
    (8, 16, 3),   # action ids up to 25, both halves of the revert tables, chunked units
])
def test_kernel_matches_exhaustive_cpu_oracle(gpu_device, ext, n_procs, n_groups, depth):
    st, params, ref = _ref(n_procs, n_groups, depth)
    _check(st, params, subset_best(st, params, device=str(gpu_device)), ref, gpu_device, ext)


@pytest.mark.parametrize("n_procs,n_groups,depth,restore_loss_mb", [
    (4, 12, 10, 16.0),   # 109 294 sets; RESTORE wins at the default staleness
    (4, 12, 10, 500.0),  # the same sets with RESTORE priced out: reverts decide
    (8, 16, 6, 500.0),   # 245 506 sets of 2^25 masks
])
def test_kernel_matches_closed_form_beyond_enumeration(gpu_device, ext, n_procs, n_groups, depth,
                                                       restore_loss_mb):
    st, params, ref = _ref(n_procs, n_groups, depth, restore_loss_mb)
    _check(st, params, subset_best(st, params, device=str(gpu_device)), ref, gpu_device, ext)


def test_batch_equals_single_calls(gpu_device):
    params = PlannerParams(n_groups=4, max_depth=6)
    states = [multi_state(3, 4, seed=s) for s in (34, 5, 6)]
    batch = subset_best(states, params, device=str(gpu_device))
    for st, got in zip(states, batch):
        one = subset_best(st, params, device=str(gpu_device))
        assert (got.plan, got.reward, got.first_action_best, got.device_rewards) == (
            one.plan, one.reward, one.first_action_best, one.device_rewards)


@pytest.mark.parametrize("n_procs,n_groups,depth", [(9, 3, 10), (2, 17, 10), (2, 3, 0)])
def test_binding_refuses_what_the_kernel_cannot_take(gpu_device, ext, n_procs, n_groups, depth):
    f32 = lambda *shape: torch.full(shape, 0.5, dtype=torch.float32, device=gpu_device)
    pd = _params_dict(n_groups, PlannerParams(n_groups=n_groups, max_depth=depth))
    with pytest.raises(ValueError):
        ext.plan_subsets_search(f32(1, n_groups), f32(1, n_groups), f32(1, n_groups),
                                f32(1, n_procs), f32(1), pd)


def test_plan_joint_sets_gpu_equals_cpu(gpu_device):
    class SmallCpuEngine(CpuEngine):
        planner_params = PlannerParams(n_groups=4, max_depth=4)

    class SmallGpuEngine(SmallCpuEngine):
        device = gpu_device

    det = two_culprit_detection()
    gpu = StreamingEngine.plan_joint(SmallGpuEngine(), det, planner="sets")
    cpu = StreamingEngine.plan_joint(SmallCpuEngine(), det, planner="sets", use_gpu=False)
    assert (gpu.plan, gpu.root_value, gpu.simulations) == (cpu.plan, cpu.root_value, 99)
    assert sorted(a for a, _q, _n in gpu.ranked_actions) == list(range(0, 8))
    assert (gpu.proc_keys, gpu.group_owner, gpu.group_paths, gpu.unplanned) == (
        cpu.proc_keys, cpu.group_owner, cpu.group_paths, cpu.unplanned)
