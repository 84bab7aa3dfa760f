// Shared host/device planner parameter block (bindings.cpp + mcts.hip).
#pragma once

namespace nerrf {

struct PlannerParamsDev {
  int n_groups;
  int n_actions;
  int max_depth;
  int sims_per_tree;
  float downtime_weight;
  float revert_time_s;
  float kill_time_s;
  float fp_weight;
  float attack_rate_mbps;
  float horizon_s;
  float restore_time_s;
  float restore_loss_mb;
  float ucb_c;
  unsigned seed;
};

// Joint planner over P processes (bindings.cpp + mcts_multi.hip).  Actions:
// 0 STOP | 1 + p KILL p | P + 1 RESTORE | P + 2 + g REVERT g.
#define NERRF_MULTI_MAX_PROCS 8

// One CU's LDS: the most a single tree's arena may take.
#define NERRF_MULTI_MAX_TREE_BYTES (160 * 1024)

// LDS bytes of one tree's arena (layout in mcts_multi.hip), a multiple of 4:
// value f32 + visits i32 per node, then parent, action and n_actions children
// as i16.
inline long mcts_multi_tree_bytes(long cap, long n_actions) {
  return (8 * cap + 2 * cap * (2 + n_actions) + 3) & ~3L;
}

struct MultiPlannerParamsDev {
  PlannerParamsDev base;  // n_actions = n_procs + 2 + n_groups
  int n_procs;
  float proc_score[NERRF_MULTI_MAX_PROCS];
};

}  // namespace nerrf
