"""The joint planner's kernel (ops/hip/mcts_multi.hip) against the fp64 CPU
reference, at the smallest shapes where it can go wrong."""
import numpy as np
import pytest
import torch

from nerrf_amd.planner.mcts import (UCB_C, multi_params_dict, multi_state_tensors,
                                    run_mcts_multi, run_mcts_multi_gpu)
from nerrf_amd.planner.oracle import (REWARD_ATOL, REWARD_RTOL, exhaustive_best_cpu,
                                      plan_regret, reward_tol)
from nerrf_amd.planner.rewards import A_STOP, PlannerParams, simulate_plan_multi
from nerrf_amd.serve.engine import StreamingEngine
from test_plan_joint import (FIXED_PARAMS, FIXED_STATE, CpuEngine, multi_state,
                             two_culprit_detection)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from nerrf_amd.ops.native import load_extension

    return load_extension(required=True)


@pytest.mark.parametrize("n_procs,n_groups", [(1, 1), (2, 3), (8, 16)])
def test_reward_matches_fp64(gpu_device, ext, n_procs, n_groups):
    st = multi_state(n_procs, n_groups, seed=3)
    params = PlannerParams(n_groups=n_groups)
    plans = np.random.default_rng(5).integers(0, st.n_actions + 2, (512, 10)).astype(np.int32)
    ref = np.array([simulate_plan_multi(st, [int(a) for a in pl], params) for pl in plans])
    pd = multi_params_dict(st, params)
    dplans = torch.from_numpy(plans).to(gpu_device)
    gs, gm, gf, ps, clean = multi_state_tensors(st, gpu_device)
    got = ext.mcts_multi_eval_plans(gs, gm, gf, ps, clean, pd, dplans).cpu().numpy()
    print(f"P={n_procs} G={n_groups}: max |err| {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=REWARD_RTOL, atol=REWARD_ATOL)
    if n_procs == 1:  # the single-process kernel computes the same MDP
        old = ext.mcts_eval_plans(gs, gm, gf, float(ps[0]), clean, pd, dplans).cpu().numpy()
        np.testing.assert_allclose(got, old, rtol=REWARD_RTOL, atol=REWARD_ATOL)


@pytest.mark.parametrize("n_procs,n_groups", [(2, 3), (8, 16)])
def test_expansion_rollout_backup_without_ucb(gpu_device, ext, n_procs, n_groups):
    """sims_per_tree == n_actions: every simulation expands one root child."""
    st = multi_state(n_procs, n_groups, seed=11)
    params = PlannerParams(n_groups=n_groups)
    n_trees, spt = 8, st.n_actions
    _, tv, tw = run_mcts_multi(st, params, n_sims=n_trees * spt, sims_per_tree=spt, seed=4,
                               return_tree_stats=True)
    rv, rw = ext.mcts_multi_search(*multi_state_tensors(st, gpu_device),
                                   multi_params_dict(st, params, spt, seed=4), n_trees)
    assert torch.equal(rv.cpu(), torch.ones(n_trees, spt, dtype=torch.int32))
    assert np.array_equal(tv, np.ones((n_trees, spt)))
    np.testing.assert_allclose(rw.cpu().numpy(), tw, rtol=REWARD_RTOL, atol=REWARD_ATOL)


@pytest.mark.parametrize("case", ["fixed_2x3", "random_8x16"])
def test_select_phase_matches_cpu_planner(gpu_device, ext, case):
    if case == "fixed_2x3":
        st, params = FIXED_STATE, FIXED_PARAMS
    else:
        st, params = multi_state(8, 16, seed=21), PlannerParams(n_groups=16)
    cpu = run_mcts_multi(st, params, n_sims=1024, sims_per_tree=32)
    rv, _ = ext.mcts_multi_search(*multi_state_tensors(st, gpu_device),
                                  multi_params_dict(st, params, 32), 32)
    assert torch.equal(rv.sum(1).cpu(), torch.full((32,), 32, dtype=torch.int64))
    gpu = run_mcts_multi_gpu(st, params, n_sims=1024, sims_per_tree=32, device=str(gpu_device))
    print(f"{case}: cpu {cpu.plan} {cpu.root_value:.6f}  gpu {gpu.plan} {gpu.root_value:.6f}")
    assert gpu.ranked_actions[0][0] == cpu.ranked_actions[0][0]
    r_cpu = simulate_plan_multi(st, cpu.plan + [A_STOP], params)
    r_gpu = simulate_plan_multi(st, gpu.plan + [A_STOP], params)
    if case == "fixed_2x3":
        orc = exhaustive_best_cpu(st, params)
        assert plan_regret(st, gpu.plan, params, oracle=orc) <= (
            plan_regret(st, cpu.plan, params, oracle=orc) + reward_tol(orc.reward))
    else:  # no oracle at this size
        assert r_gpu >= r_cpu - reward_tol(r_cpu)


@pytest.mark.parametrize("n_procs,n_groups,spt,depth", [
    (9, 3, 32, 10), (2, 17, 32, 10),
    (8, 16, 512, 16),  # one tree of 8194 nodes x 26 actions: 508 KB of LDS
])
def test_binding_refuses_what_the_kernel_cannot_take(gpu_device, ext, n_procs, n_groups, spt, depth):
    f32 = lambda n, dev: torch.full((n,), 0.5, dtype=torch.float32, device=dev)
    pd = {"n_groups": n_groups, "max_depth": depth, "sims_per_tree": spt, "downtime_weight": 0.1,
          "revert_time_s": 0.05, "kill_time_s": 0.5, "fp_weight": 1.0, "attack_rate_mbps": 2.0,
          "horizon_s": 60.0, "restore_time_s": 30.0, "restore_loss_mb": 16.0, "ucb_c": UCB_C,
          "seed": 0}
    with pytest.raises(ValueError):
        ext.mcts_multi_search(f32(n_groups, gpu_device), f32(n_groups, gpu_device),
                              f32(n_groups, gpu_device), f32(n_procs, "cpu"), 10.0, pd, 4)


def test_plan_joint_gpu_equals_cpu(gpu_device):
    class GpuEngine(CpuEngine):
        device = gpu_device

    det = two_culprit_detection()
    gpu = StreamingEngine.plan_joint(GpuEngine(), det)
    cpu = StreamingEngine.plan_joint(CpuEngine(), det, use_gpu=False)
    assert gpu.plan == cpu.plan
    assert (gpu.proc_keys, gpu.group_owner, gpu.group_paths, gpu.unplanned) == (
        cpu.proc_keys, cpu.group_owner, cpu.group_paths, cpu.unplanned)
