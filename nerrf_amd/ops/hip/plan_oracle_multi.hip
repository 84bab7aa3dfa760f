// Exhaustive oracle of the joint (P-process) rollback-planning MDP — CDNA4
// (gfx950).
//
// Enumerates EVERY canonical plan (ordered arrangements of distinct non-STOP
// actions, length <= max_depth) of a batch of MultiPlannerStates and returns,
// per work item, the best plan under the project's fixed tie-break: higher
// reward, then shorter plan, then lexicographically smaller action tuple.
// The MDP is rewards.simulate_plan_multi / eval_plan_multi (mcts_multi.hip):
//   0 STOP | 1 + p KILL p | P + 1 RESTORE | P + 2 + g REVERT g
// with P <= 8 and G <= 16, so n = P + 1 + G <= 25 non-STOP actions: ids fit
// 5 bits (6 per word) and the `used` set fits one 32-bit mask.
//
// The search skeleton is plan_oracle.hip's.  Work item = (state, length-L
// prefix), prefixes numbered in lexicographic order (mixed radix n, n-1, ...).
// A lane walks its prefix, scoring the prefix nodes (they share the item's
// first action), then runs a depth-first search over the suffixes as a
// compile-time-depth template recursion: every level's saved state is a named
// register set, nothing is runtime-indexed, nothing goes to scratch.  Children
// are visited by RANK among the unused actions, so all lanes of a wave walk
// isomorphic trees with equal trip counts; what differs per lane is which
// kind of action a rank is.
//
// What the joint MDP adds to a node is `live`, the summed score of the
// processes still alive, which scales all damage that accrues while the plan
// acts.  It changes only on a KILL, where it is re-summed from zero in
// ascending p over the alive bits of `used` (the order of live_score and of
// simulate_plan_multi; a dead process adds +0.0f, an exact identity), and is
// otherwise carried down the recursion: one VGPR per level instead of eight
// selects and adds per node.  The re-sum sits behind a branch, so a wave whose
// lanes expand no KILL at a rank skips it.
//
// Per-state data: the per-group tables (revert time, rate * revert time,
// false-positive MB, unrecovered MB) and the eight process scores are
// filled into LDS once per (block, state); the process scores and the
// unrecovered MB are then held in registers through the search.  The revert
// bit field of `used` starts at bit P + 2: a wave-uniform shift.
//
// The reward keeps eval_plan_multi's operation order (`rate * dt * live`, the
// loss summed over g = 0..15 in order, no-ops added as +0.0f).  FP contraction
// is off so that symmetric plans tie bit-for-bit whatever level they are
// scored at; the rewards REPORTED to callers come from eval_plan_multi itself
// (bindings.cpp re-evaluates the winners).
//
// Packed f32 VALU ops stay out of this file's device code, as in
// mcts_multi.hip.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include <math.h>

#include "common.h"
#include "mcts_params.h"

#pragma clang fp contract(off)

namespace nerrf {

namespace {

constexpr int POM_MAX_GROUPS = 16;
constexpr int POM_MAX_PROCS = NERRF_MULTI_MAX_PROCS;
constexpr int POM_MAX_DEPTH = 16;
constexpr int POM_BLOCK = 256;
constexpr int POM_MAX_GRID = 2048;
constexpr int POM_FIELDS_PER_WORD = 6;  // 5-bit action ids, 6 per u32

// Wave-uniform data of the state a block is working on.
struct PomCtx {
  float unrec[POM_MAX_GROUPS];  // score*mb, 0 beyond G
  float ps[POM_MAX_PROCS];      // process scores, 0 beyond P
  float kill_t, restore_t;
  float rdt_restore;  // rate * restore time
  float rdt_horizon;  // rate * horizon
  float horizon;
  float remaining, restore_loss, dw, fpw;
  int a_restore;         // P + 1
  int a_revert;          // P + 2
  unsigned proc_mask;    // bits 1..P
  unsigned action_mask;  // bits 1..n
  const float* dt;       // LDS [16]: revert time of group g
  const float* rdt;      // LDS [16]: rate * revert time of group g
  const float* fp;       // LDS [16]: false-positive MB of reverting group g
};

// Plan state after a partial plan.  `used` holds one bit per action id:
// process p is alive while bit 1 + p is clear, restored == used[RESTORE], and
// the reverted groups are the used revert actions (all groups once restored).
struct PomNode {
  float fp_mb, downtime, ongoing, live;
  unsigned used;
};

struct PomBest {
  float reward;
  int len;
  unsigned s0, s1, s2;  // packed suffix of the winner
};

struct PomPath {
  unsigned s0, s1, s2;  // packed suffix being walked (stale beyond the depth)
};

// Ascending p from zero over the alive bits; bits of p >= P belong to other
// actions, and their scores are +0.0f whichever way the select goes.
__device__ __forceinline__ float pom_live(const PomCtx& c, unsigned used) {
  float live = 0.0f;
#pragma unroll
  for (int q = 0; q < POM_MAX_PROCS; ++q)
    live += ((used >> (q + 1)) & 1u) ? 0.0f : c.ps[q];
  return live;
}

__device__ __forceinline__ PomNode pom_step(const PomCtx& c, PomNode s, int a) {
  const bool restored = ((s.used >> c.a_restore) & 1u) != 0u;
  const bool is_kill = a < c.a_restore;
  const bool is_restore = a == c.a_restore;
  const bool is_revert = a > c.a_restore;
  const int gi = (a - c.a_revert) & (POM_MAX_GROUPS - 1);
  const float gdt = c.dt[gi], grdt = c.rdt[gi], gfp = c.fp[gi];
  // a revert after RESTORE is a no-op (eval_plan_multi: reverted bit set)
  const bool noop = is_revert && restored;
  const float dt =
      is_kill ? c.kill_t : (is_restore ? c.restore_t : (noop ? 0.0f : gdt));
  const float rdt = is_restore ? c.rdt_restore : grdt;
  const float og = (is_kill || noop) ? 0.0f : rdt * s.live;
  const float fp = (is_revert && !restored) ? gfp : 0.0f;
  s.ongoing += og;
  s.downtime += dt;
  s.fp_mb += fp;
  s.used |= 1u << a;
  if (is_kill) s.live = pom_live(c, s.used);
  return s;
}

__device__ __forceinline__ float pom_score(const PomCtx& c, const PomNode& s) {
  const bool any_alive = (~s.used & c.proc_mask) != 0u;
  const bool restored = ((s.used >> c.a_restore) & 1u) != 0u;
  const float ongoing = s.ongoing + (any_alive ? c.rdt_horizon * s.live : 0.0f);
  const float downtime = s.downtime + (any_alive ? c.horizon * s.live : 0.0f);
  const unsigned rev = restored ? 0xFFFFu : (s.used >> c.a_revert);
  float loss = 0.0f;
#pragma unroll
  for (int g = 0; g < POM_MAX_GROUPS; ++g)  // sequential order == eval_plan_multi
    loss += ((rev >> g) & 1u) ? 0.0f : c.unrec[g];
  loss += fminf(ongoing, c.remaining);
  loss += restored ? c.restore_loss : 0.0f;
  return -(loss + c.dw * downtime + c.fpw * s.fp_mb);
}

// Plans of one length reach a lane in lexicographic order, so an equal
// reward replaces the incumbent only when the newcomer is shorter.
__device__ __forceinline__ void pom_offer(PomBest& b, float r, int len,
                                          unsigned s0, unsigned s1,
                                          unsigned s2) {
  if (r > b.reward || (r == b.reward && len < b.len)) {
    b.reward = r;
    b.len = len;
    b.s0 = s0;
    b.s1 = s1;
    b.s2 = s2;
  }
}

__device__ __forceinline__ unsigned pom_set_field(unsigned w, int field, int a) {
  const int sh = 5 * field;
  return (w & ~(31u << sh)) | ((unsigned)a << sh);
}

// Expands the children of `node`, a plan of length L + J.  `levels` is
// depth_lim - L and `free_l` is n - L (both wave-uniform); depth_lim <= n, so
// a level that may expand always has a child.
template <int J>
__device__ __forceinline__ void pom_dfs(const PomCtx& c, const PomNode& node,
                                        int L, int levels, int free_l,
                                        PomPath& path, PomBest& best) {
  if constexpr (J < POM_MAX_DEPTH - 1) {  // L >= 1, so L + J + 1 <= MAX_DEPTH
    // Opaque copies (empty asm), as in plan_oracle.hip: they keep each
    // level's loop invariants from being hoisted out of all 15 nested loops
    // at once, which costs several SGPRs per level and spills.
    int lv = levels;
    asm volatile("" : "+s"(lv));
    if (J >= lv) return;
    unsigned avail = ~node.used & c.action_mask;
    int fl = free_l;
    asm volatile("" : "+s"(fl));
    for (int r = fl - J; r > 0; --r) {  // fl - J == popcount(avail)
      const int a = (__ffs(avail) - 1) & 31;
      avail &= avail - 1u;
      PomNode parent = node;
      asm volatile("" : "+v"(parent.used));
      int len = L;
      asm volatile("" : "+s"(len));
      len += J;
      const PomNode child = pom_step(c, parent, a);
      if constexpr (J / POM_FIELDS_PER_WORD == 0)
        path.s0 = pom_set_field(path.s0, J % POM_FIELDS_PER_WORD, a);
      else if constexpr (J / POM_FIELDS_PER_WORD == 1)
        path.s1 = pom_set_field(path.s1, J % POM_FIELDS_PER_WORD, a);
      else
        path.s2 = pom_set_field(path.s2, J % POM_FIELDS_PER_WORD, a);
      pom_offer(best, pom_score(c, child), len + 1, path.s0, path.s1, path.s2);
      pom_dfs<J + 1>(c, child, L, levels, free_l, path, best);
    }
  }
}

// out_plan holds six words per item: the packed prefix (3) and the packed
// winning suffix (3), 5 bits per action, 6 actions per word.  The winner is
// prefix[:min(L, len)] + suffix[:len - L].
__global__ __launch_bounds__(POM_BLOCK) void plan_oracle_multi_kernel(
    const float* __restrict__ gscore,  // [S, G]
    const float* __restrict__ gmb,     // [S, G]
    const float* __restrict__ gfiles,  // [S, G]
    const float* __restrict__ proc,    // [S, P]
    const float* __restrict__ clean,   // [S]
    PlannerParamsDev p, int P, int L, int n_prefix, int n_chunks, long n_units,
    float* __restrict__ out_reward,    // [S, n_prefix]
    int* __restrict__ out_len,         // [S, n_prefix]
    unsigned* __restrict__ out_plan) { // [S, n_prefix, 6]
  __shared__ float lds_dt[POM_MAX_GROUPS];
  __shared__ float lds_rdt[POM_MAX_GROUPS];
  __shared__ float lds_fp[POM_MAX_GROUPS];
  __shared__ float lds_unrec[POM_MAX_GROUPS];
  __shared__ float lds_ps[POM_MAX_PROCS];

  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int G = p.n_groups;
  const int n = P + 1 + G;  // non-STOP actions: KILL p, RESTORE, revert g
  const int depth_lim = p.max_depth < n ? p.max_depth : n;

  for (long u = (long)__builtin_amdgcn_workgroup_id_x(); u < n_units;
       u += POM_MAX_GRID) {  // the launcher's grid is min(n_units, MAX_GRID)
    const int s = (int)(u / n_chunks);
    const int chunk = (int)(u - (long)s * n_chunks);

    __syncthreads();  // readers of the previous unit's tables are done
    if (tid < POM_MAX_GROUPS) {
      const int g = tid;
      float dt = 0.0f, rdt = 0.0f, fp = 0.0f, unrec = 0.0f;
      if (g < G) {
        const float sc = gscore[(long)s * G + g];
        const float mb = gmb[(long)s * G + g];
        const float files = gfiles[(long)s * G + g];
        dt = p.revert_time_s * fmaxf(files, 1.0f);
        rdt = p.attack_rate_mbps * dt;
        fp = (1.0f - sc) * mb * 0.05f;
        unrec = sc * mb;
      }
      lds_dt[g] = dt;
      lds_rdt[g] = rdt;
      lds_fp[g] = fp;
      lds_unrec[g] = unrec;
    } else if (tid < POM_MAX_GROUPS + POM_MAX_PROCS) {
      const int q = tid - POM_MAX_GROUPS;
      lds_ps[q] = (q < P) ? proc[(long)s * P + q] : 0.0f;
    }
    __syncthreads();

    PomCtx c;
#pragma unroll
    for (int g = 0; g < POM_MAX_GROUPS; ++g)
      c.unrec[g] = lds_unrec[g];
#pragma unroll
    for (int q = 0; q < POM_MAX_PROCS; ++q)
      c.ps[q] = lds_ps[q];
    c.kill_t = p.kill_time_s;
    c.restore_t = p.restore_time_s;
    c.rdt_restore = p.attack_rate_mbps * p.restore_time_s;
    c.rdt_horizon = p.attack_rate_mbps * p.horizon_s;
    c.horizon = p.horizon_s;
    c.remaining = clean[s];
    c.restore_loss = p.restore_loss_mb;
    c.dw = p.downtime_weight;
    c.fpw = p.fp_weight;
    c.a_restore = P + 1;
    c.a_revert = P + 2;
    c.proc_mask = ((1u << (P + 1)) - 1u) & ~1u;
    c.action_mask = ((1u << (n + 1)) - 1u) & ~1u;
    c.dt = lds_dt;
    c.rdt = lds_rdt;
    c.fp = lds_fp;

    const int pi = chunk * POM_BLOCK + tid;
    if (pi < n_prefix) {
      PomNode node = {0.0f, 0.0f, 0.0f, 0.0f, 0u};
      node.live = pom_live(c, 0u);
      PomBest best = {-INFINITY, 1 << 30, 0u, 0u, 0u};
      unsigned p0 = 0u, p1 = 0u, p2 = 0u;

      // ---- prefix: decode the item's rank digits front to back ----
      unsigned rem = (unsigned)pi;
      unsigned stride = (unsigned)n_prefix;
      for (int k = 0; k < L; ++k) {
        stride /= (unsigned)(n - k);
        const unsigned r = rem / stride;
        rem -= r * stride;
        unsigned avail = ~node.used & c.action_mask;
        for (int t = 0; t < n; ++t)
          if (t < (int)r) avail &= avail - 1u;  // drop the r lowest
        const int a = (__ffs(avail) - 1) & 31;
        node = pom_step(c, node, a);
        const int w = k / POM_FIELDS_PER_WORD;
        const int f = k - w * POM_FIELDS_PER_WORD;
        p0 = (w == 0) ? pom_set_field(p0, f, a) : p0;
        p1 = (w == 1) ? pom_set_field(p1, f, a) : p1;
        p2 = (w == 2) ? pom_set_field(p2, f, a) : p2;
        // prefix nodes share the item's first action, so they compete here
        pom_offer(best, pom_score(c, node), k + 1, 0u, 0u, 0u);
      }

      // ---- suffixes ----
      PomPath path = {0u, 0u, 0u};
      pom_dfs<0>(c, node, L, depth_lim - L, n - L, path, best);

      const long o = (long)s * n_prefix + pi;
      out_reward[o] = best.reward;
      out_len[o] = best.len;
      out_plan[o * 6 + 0] = p0;
      out_plan[o * 6 + 1] = p1;
      out_plan[o * 6 + 2] = p2;
      out_plan[o * 6 + 3] = best.s0;
      out_plan[o * 6 + 4] = best.s1;
      out_plan[o * 6 + 5] = best.s2;
    }
  }
}

}  // namespace

// Caller guarantees: 1 <= P <= 8, 1 <= G <= 16, n = P + 1 + G,
// 1 <= L <= min(max_depth, n) <= 16, n_prefix == n!/(n-L)! < 2^31,
// outputs sized [S, n_prefix(, 6)].
hipError_t launch_plan_oracle_multi(const float* gscore, const float* gmb,
                                    const float* gfiles, const float* proc,
                                    const float* clean,
                                    const PlannerParamsDev& p, int P, int S,
                                    int L, int n_prefix, float* out_reward,
                                    int* out_len, unsigned* out_plan,
                                    hipStream_t s) {
  const int n_chunks = (n_prefix + POM_BLOCK - 1) / POM_BLOCK;
  const long n_units = (long)S * n_chunks;
  const int grid = (int)(n_units < POM_MAX_GRID ? n_units : POM_MAX_GRID);
  plan_oracle_multi_kernel<<<grid, POM_BLOCK, 0, s>>>(
      gscore, gmb, gfiles, proc, clean, p, P, L, n_prefix, n_chunks, n_units,
      out_reward, out_len, out_plan);
  return hipGetLastError();
}

}  // namespace nerrf

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
