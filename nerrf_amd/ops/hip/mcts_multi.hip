// Joint multi-culprit rollback planner: root-parallel MCTS over the
// P-process MDP — CDNA4 (gfx950).
//
// The MDP is rewards.simulate_plan_multi: P attack processes, each stopped by
// its own KILL, and the damage that accrues while the plan acts scales with
// `live`, the summed score of the processes still alive.  Actions:
//   0 STOP | 1 + p KILL p | P + 1 RESTORE | P + 2 + g REVERT g
// (n_actions = P + 2 + G <= 26).  Search, RNG and seeding are those of
// mcts.hip and planner/mcts.py::run_mcts_multi, which is the numerics
// reference of the tests.
//
// Unlike mcts.hip, the kernel is built around the wave:
//
//   arena in LDS      one wave64 owns one tree, and the tree's whole arena
//       sits in dynamic LDS:  value f32[cap] | visits i32[cap] |
//       parent i16[cap] | action i16[cap] | children i16[cap * n_actions]
//       (cap = sims_per_tree * max_depth + 2 < 32768, so node ids fit 16
//       bits; 20.6 KB at 32 sims, depth 10, 26 actions).  A block carries as
//       many trees (waves) as fit an 80 KB budget, which leaves room for two
//       blocks per CU.  Waves never share data, so the kernel has no block
//       barrier.  Only the [n_trees, n_actions] root statistics reach HBM.
//   lane per action   in the select phase lane a holds child a of the current
//       node.  "First untried" and "first unvisited" are the lowest set bit
//       of a ballot; the UCB1 winner is a DPP/shuffle max-reduce followed by a
//       ballot over `u == max`, whose lowest bit is the lowest action index
//       among ties — the CPU's first strict maximum.
//   plan in lanes     action i of the simulated plan lives in lane i's
//       register and is read back with v_readlane, as are the per-group
//       statistics (group g in lane g): no private arrays, no scratch.
//   wave-uniform walk node, depth, n_nodes, the RNG and the alive mask are
//       the same on every lane; arena writes come from lane 0, the arena
//       init and the root export are lane-parallel.
//
// Packed f32 VALU ops stay out of this file's device code; see
// lstm_rec_packed.hip for why the push precedes the includes and why ids are
// read through the builtins.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "common.h"
#include "mcts_params.h"

namespace nerrf {

namespace {

constexpr int MM_BLOCK_LDS_BUDGET = 80 * 1024;  // two blocks per 160 KB CU
constexpr int MM_MAX_WAVES = 16;                // 1024 threads
constexpr int MM_MAX_GRID = 2048;               // 8 blocks per CU; blocks stride

__device__ __forceinline__ unsigned mm_xorshift32(unsigned s) {
  s ^= s << 13;
  s ^= s >> 17;
  s ^= s << 5;
  return s;
}

// v_readlane: `l` is wave-uniform at every call site.
__device__ __forceinline__ int lane_get(int v, int l) {
  return __builtin_amdgcn_readlane(v, l);
}
__device__ __forceinline__ float lane_getf(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Lane-0 arena writes are read back by other lanes of the same wave.  LDS
// operations of one wave execute in order; this keeps the compiler from
// moving accesses across the hand-over.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v),
                                            CTRL, 0xF, 0xF, false);
  return fmaxf(v, __int_as_float(o));
}

// Max over lanes 0..31 (n_actions <= 26), valid on those lanes; all 64 lanes
// must be active.  Within a row of 16: quad_perm [1,0,3,2] and [2,3,0,1],
// then row_half_mirror and row_mirror (after the quad steps every quad holds
// its own max, so a mirror pairs each quad with the one it still lacks).
// Across the two rows: one shuffle.
__device__ __forceinline__ float wave_max32(float v) {
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  v = dpp_max<0x141>(v);
  v = dpp_max<0x140>(v);
  return fmaxf(v, __shfl_xor(v, 16, NERRF_WAVE));
}

// Summed score of the processes still alive: ascending p from zero, the
// order of rewards.simulate_plan_multi.  Bits >= n_procs are never set.
__device__ __forceinline__ float live_score(const MultiPlannerParamsDev& mp,
                                            unsigned alive) {
  float live = 0.0f;
#pragma unroll
  for (int q = 0; q < NERRF_MULTI_MAX_PROCS; ++q)
    if ((alive >> q) & 1u) live += mp.proc_score[q];
  return live;
}

// Mirrors rewards.simulate_plan_multi (fp32), one thread per plan.  The
// reverted set is a bit mask: a reverted group contributes exactly 0 to the
// loss, as (1 - 1) * score * mb does.
__device__ __forceinline__ float eval_plan_multi(
    const float* __restrict__ gscore, const float* __restrict__ gmb,
    const float* __restrict__ gfiles, float remaining_clean_mb,
    const int* __restrict__ actions, int n_act,
    const MultiPlannerParamsDev& mp) {
  const PlannerParamsDev& p = mp.base;
  const int a_restore = mp.n_procs + 1;
  const int a_revert = mp.n_procs + 2;
  unsigned reverted = 0u;
  unsigned alive = (1u << mp.n_procs) - 1u;
  float live = live_score(mp, alive);
  float fp_mb = 0.0f, downtime = 0.0f, ongoing = 0.0f, staleness = 0.0f;
  bool restored = false;
  for (int i = 0; i < n_act; ++i) {
    const int a = actions[i];
    if (a == 0) break;
    if (a >= 1 && a < a_restore) {
      const unsigned bit = 1u << (a - 1);
      if (alive & bit) {
        downtime += p.kill_time_s;
        alive &= ~bit;
        live = live_score(mp, alive);
      }
      continue;
    }
    if (a == a_restore) {
      if (restored) continue;
      const float dt = p.restore_time_s;
      ongoing += p.attack_rate_mbps * dt * live;
      downtime += dt;
      reverted = (1u << p.n_groups) - 1u;
      staleness = p.restore_loss_mb;
      restored = true;
      continue;
    }
    const int gi = a - a_revert;
    if (gi < 0 || gi >= p.n_groups || ((reverted >> gi) & 1u)) continue;
    const float dt = p.revert_time_s * fmaxf(gfiles[gi], 1.0f);
    ongoing += p.attack_rate_mbps * dt * live;
    downtime += dt;
    reverted |= 1u << gi;
    fp_mb += (1.0f - gscore[gi]) * gmb[gi] * 0.05f;
  }
  if (alive) {
    ongoing += p.attack_rate_mbps * p.horizon_s * live;
    downtime += p.horizon_s * live;
  }
  float loss = 0.0f;
  for (int g = 0; g < p.n_groups; ++g)
    loss += ((reverted >> g) & 1u) ? 0.0f : gscore[g] * gmb[g];
  loss += fminf(ongoing, remaining_clean_mb);
  loss += staleness;
  return -(loss + p.downtime_weight * downtime + p.fp_weight * fp_mb);
}

// The same reward wave-wide, as eval_plan_wave of mcts.hip: group g's score,
// MB, files and reverted flag are lane g's registers, plan action i is lane
// i's `my_act`; control flow is wave-uniform and the final loss is a
// sequential chain over g, so the fp32 sum order equals the scalar one.
__device__ __forceinline__ float eval_plan_multi_wave(
    float my_score, float my_mb, float my_files, float remaining_clean_mb,
    int my_act, int n_act, const MultiPlannerParamsDev& mp, int lane) {
  const PlannerParamsDev& p = mp.base;
  const int a_restore = mp.n_procs + 1;
  const int a_revert = mp.n_procs + 2;
  float my_rev = 0.0f;
  unsigned alive = (1u << mp.n_procs) - 1u;
  float live = live_score(mp, alive);
  float fp_mb = 0.0f, downtime = 0.0f, ongoing = 0.0f, staleness = 0.0f;
  bool restored = false;
  for (int i = 0; i < n_act; ++i) {
    const int a = lane_get(my_act, i);
    if (a == 0) break;
    if (a >= 1 && a < a_restore) {
      const unsigned bit = 1u << (a - 1);
      if (alive & bit) {
        downtime += p.kill_time_s;
        alive &= ~bit;
        live = live_score(mp, alive);
      }
      continue;
    }
    if (a == a_restore) {
      if (restored) continue;
      const float dt = p.restore_time_s;
      ongoing += p.attack_rate_mbps * dt * live;
      downtime += dt;
      my_rev = 1.0f;
      staleness = p.restore_loss_mb;
      restored = true;
      continue;
    }
    const int gi = a - a_revert;
    if (gi < 0 || gi >= p.n_groups) continue;
    if (lane_getf(my_rev, gi) > 0.0f) continue;
    const float dt = p.revert_time_s * fmaxf(lane_getf(my_files, gi), 1.0f);
    ongoing += p.attack_rate_mbps * dt * live;
    downtime += dt;
    if (lane == gi) my_rev = 1.0f;
    fp_mb += (1.0f - lane_getf(my_score, gi)) * lane_getf(my_mb, gi) * 0.05f;
  }
  if (alive) {
    ongoing += p.attack_rate_mbps * p.horizon_s * live;
    downtime += p.horizon_s * live;
  }
  const float my_term = (my_rev > 0.0f) ? 0.0f : my_score * my_mb;
  float loss = 0.0f;
  for (int g = 0; g < p.n_groups; ++g) loss += lane_getf(my_term, g);
  loss += fminf(ongoing, remaining_clean_mb);
  loss += staleness;
  return -(loss + p.downtime_weight * downtime + p.fp_weight * fp_mb);
}

__launch_bounds__(MM_MAX_WAVES * NERRF_WAVE)
__global__ void mcts_multi_kernel(
    const float* __restrict__ gscore,  // [G]
    const float* __restrict__ gmb,     // [G]
    const float* __restrict__ gfiles,  // [G]
    float remaining_clean_mb, MultiPlannerParamsDev mp, int n_trees, int cap,
    int tree_bytes,                    // LDS bytes of one tree, multiple of 4
    int trees_per_block,               // == waves per block
    int* __restrict__ root_visits,     // [n_trees, n_actions]
    float* __restrict__ root_value) {  // [n_trees, n_actions]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const PlannerParamsDev& p = mp.base;
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int lane = tid % NERRF_WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / NERRF_WAVE);
  const int n_actions = p.n_actions;
  const bool act_lane = lane < n_actions;

  char* base = smem + wave * tree_bytes;
  float* value = reinterpret_cast<float*>(base);
  int* visits = reinterpret_cast<int*>(base + 4 * cap);
  short* parent = reinterpret_cast<short*>(base + 8 * cap);
  short* action = parent + cap;
  short* children = action + cap;

  const float my_score = (lane < p.n_groups) ? gscore[lane] : 0.0f;
  const float my_mb = (lane < p.n_groups) ? gmb[lane] : 0.0f;
  const float my_files = (lane < p.n_groups) ? gfiles[lane] : 0.0f;

  // the launcher's grid is min(n_tree_groups, MM_MAX_GRID)
  const int n_tree_groups = (n_trees + trees_per_block - 1) / trees_per_block;
  for (int tg = (int)__builtin_amdgcn_workgroup_id_x(); tg < n_tree_groups;
       tg += MM_MAX_GRID) {
    const int tree = tg * trees_per_block + wave;
    if (tree >= n_trees) continue;  // wave-uniform; waves share nothing

    // ---- arena init, lane-parallel: value and visits are zero words, the
    // whole 16-bit region (parent, action, children) is -1 ----
    {
      unsigned* w = reinterpret_cast<unsigned*>(base);
      const int zero_words = 2 * cap, words = tree_bytes / 4;
      for (int i = lane; i < words; i += NERRF_WAVE)
        w[i] = (i < zero_words) ? 0u : 0xFFFFFFFFu;
    }
    wave_sync();
    int n_nodes = 1;
    unsigned rng = p.seed * 2654435761u + (unsigned)tree * 40503u + 1u;

    for (int si = 0; si < p.sims_per_tree; ++si) {
      // ---- selection + expansion ----
      int node = 0, depth = 0;
      int last = -1;   // last action of the plan so far (-1: empty plan)
      int my_act = 0;  // lane i: action i of the plan
      while (depth < p.max_depth) {
        short* kids = children + node * n_actions;
        // lanes past n_actions pose as a tried, visited child
        const int ch = act_lane ? (int)kids[lane] : 0;
        const unsigned long long untried = __ballot(ch < 0);
        int pick;
        if (untried) {
          if (n_nodes >= cap) break;  // arena full: treat as leaf
          pick = __builtin_ctzll(untried);
          const int nw = n_nodes++;
          if (lane == 0) {
            parent[nw] = (short)node;
            action[nw] = (short)pick;
            kids[pick] = (short)nw;
          }
          wave_sync();
          node = nw;
        } else {
          const int nv = act_lane ? visits[ch] : 1;
          const unsigned long long unvisited = __ballot(nv == 0);
          if (unvisited) {
            pick = __builtin_ctzll(unvisited);
          } else {
            // UCB1, one child per lane
            const float logn = __logf(fmaxf((float)visits[node], 1.0f));
            const float fnv = (float)nv;
            const float u = act_lane
                ? value[ch] / fnv + p.ucb_c * __fsqrt_rn(logn / fnv)
                : -INFINITY;
            const float umax = wave_max32(u);
            const unsigned long long top =
                __ballot(u == lane_getf(umax, 0));
            pick = top ? __builtin_ctzll(top) : 0;
          }
          node = lane_get(ch, pick);
        }
        if (lane == depth) my_act = pick;
        ++depth;
        last = pick;
        if (untried || pick == 0) break;
      }
      // ---- rollout ----
      int n_act = depth;
      rng = mm_xorshift32(rng ^ ((unsigned)si * 747796405u + 2891336453u));
      unsigned r = rng;
      while (n_act < p.max_depth && last != 0) {
        r = mm_xorshift32(r);
        last = (int)(r % (unsigned)n_actions);
        if (lane == n_act) my_act = last;
        ++n_act;
      }
      const float reward =
          eval_plan_multi_wave(my_score, my_mb, my_files, remaining_clean_mb,
                               my_act, n_act, mp, lane);
      // ---- backup along parent[] ----
      if (lane == 0) {
        for (int nd = node; nd >= 0; nd = parent[nd]) {
          visits[nd] += 1;
          value[nd] += reward;
        }
      }
      wave_sync();
    }

    // ---- export root child statistics, one action per lane ----
    if (act_lane) {
      const int ch = children[lane];  // node 0
      root_visits[(long)tree * n_actions + lane] = (ch >= 0) ? visits[ch] : 0;
      root_value[(long)tree * n_actions + lane] = (ch >= 0) ? value[ch] : 0.0f;
    }
    wave_sync();  // the next tree's init overwrites what was just read
  }
}

// Batch plan evaluator: the parity harness of the reward against the CPU.
__global__ void mcts_multi_eval_plans_kernel(
    const float* __restrict__ gscore, const float* __restrict__ gmb,
    const float* __restrict__ gfiles, float remaining_clean_mb,
    MultiPlannerParamsDev mp,
    const int* __restrict__ plans,  // [n_plans, plan_len]
    int n_plans, int plan_len, float* __restrict__ out) {
  const int i = (int)__builtin_amdgcn_workgroup_id_x() * 256 +
                (int)__builtin_amdgcn_workitem_id_x();
  if (i >= n_plans) return;
  out[i] = eval_plan_multi(gscore, gmb, gfiles, remaining_clean_mb,
                           plans + (long)i * plan_len, plan_len, mp);
}

}  // namespace

// Blocks carry as many trees as fit the LDS budget (one, when a single tree
// is larger than the budget; the caller has checked that it fits the CU).
hipError_t launch_mcts_multi(const float* gscore, const float* gmb,
                             const float* gfiles, float remaining_clean_mb,
                             const MultiPlannerParamsDev& mp, int n_trees,
                             int cap, int tree_bytes, int* root_visits,
                             float* root_value, hipStream_t s) {
  int tpb = MM_BLOCK_LDS_BUDGET / tree_bytes;
  tpb = tpb < 1 ? 1 : (tpb > MM_MAX_WAVES ? MM_MAX_WAVES : tpb);
  if (tpb > n_trees) tpb = n_trees;
  const int n_tree_groups = (n_trees + tpb - 1) / tpb;
  const int grid = n_tree_groups < MM_MAX_GRID ? n_tree_groups : MM_MAX_GRID;
  mcts_multi_kernel<<<grid, tpb * NERRF_WAVE, (size_t)tpb * tree_bytes, s>>>(
      gscore, gmb, gfiles, remaining_clean_mb, mp, n_trees, cap, tree_bytes,
      tpb, root_visits, root_value);
  return hipGetLastError();
}

hipError_t launch_mcts_multi_eval_plans(
    const float* gscore, const float* gmb, const float* gfiles,
    float remaining_clean_mb, const MultiPlannerParamsDev& mp,
    const int* plans, int n_plans, int plan_len, float* out, hipStream_t s) {
  const int grid = (n_plans + 255) / 256;
  mcts_multi_eval_plans_kernel<<<grid, 256, 0, s>>>(
      gscore, gmb, gfiles, remaining_clean_mb, mp, plans, n_plans, plan_len,
      out);
  return hipGetLastError();
}

}  // namespace nerrf

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
