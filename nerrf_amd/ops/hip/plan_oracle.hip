// Exhaustive rollback-plan oracle — CDNA4 (gfx950).
//
// Enumerates EVERY canonical plan (ordered arrangements of distinct non-STOP
// actions, length <= max_depth) of a batch of planner states and returns, per
// work item, the best plan under the project's fixed tie-break: higher reward,
// then shorter plan, then lexicographically smaller action tuple.
//
// Work item = (state, length-L prefix).  Prefixes are numbered in
// lexicographic order (mixed radix n, n-1, ...), so a smaller item index is a
// lexicographically smaller prefix.  A lane first walks its prefix (scoring
// the prefix nodes of length >= 1, which all share the item's first action),
// then runs a depth-first search over the suffixes.  The search is a
// compile-time-depth template recursion: every level's saved state is a
// named register set, nothing is runtime-indexed, nothing goes to scratch.
// Children are visited by RANK among the unused actions, so all lanes of a
// wave (same L, same n, same depth limit) walk isomorphic trees with equal
// trip counts; only the KILL/RESTORE/revert selects differ per lane.
//
// The reward arithmetic keeps eval_plan's (mcts.hip) operation order: the
// three accumulators take the same addends in plan order, and the final loss
// sums the groups g = 0..G-1 in order.  No-op contributions are added as
// +0.0f, which is an exact identity.  FP contraction is off in this file so
// that symmetric plans tie bit-for-bit whatever level they are scored at;
// the rewards REPORTED to callers come from eval_plan itself (bindings.cpp
// re-evaluates the winners through launch_eval_plans).
#include <math.h>

#include "common.h"
#include "mcts_params.h"

#pragma clang fp contract(off)

namespace nerrf {

namespace {

constexpr int PO_MAX_GROUPS = 16;
constexpr int PO_MAX_DEPTH = 16;
constexpr int PO_BLOCK = 256;
constexpr int PO_MAX_GRID = 2048;
constexpr int PO_A_KILL = 1;
constexpr int PO_A_RESTORE = 2;
constexpr int PO_A_REVERT_BASE = 3;
constexpr int PO_FIELDS_PER_WORD = 6;  // 5-bit action ids, 6 per u32

// Wave-uniform data of the state a block is working on.
struct PoCtx {
  float unrec[PO_MAX_GROUPS];  // score*mb, 0 beyond G
  float kill_t, restore_t;
  float og_restore;  // MB encrypted while a restore runs (process alive)
  float og_horizon;  // MB encrypted up to the horizon (process alive)
  float dt_horizon;  // degradation charge when the process stays alive
  float remaining, restore_loss, dw, fpw;
  unsigned action_mask;  // bits 1..n
  const float* dt;       // LDS [16]: revert time of group g
  const float* og;       // LDS [16]: MB encrypted while reverting group g
  const float* fp;       // LDS [16]: false-positive MB of reverting group g
};

// Plan state after a partial plan.  `used` holds one bit per action id:
// alive == !used[KILL], restored == used[RESTORE], reverted groups are the
// used revert actions (or all groups once restored).
struct PoNode {
  float fp_mb, downtime, ongoing;
  unsigned used;
};

struct PoBest {
  float reward;
  int len;
  unsigned s0, s1, s2;  // packed suffix of the winner
};

struct PoPath {
  unsigned s0, s1, s2;  // packed suffix being walked (stale beyond the depth)
};

__device__ __forceinline__ PoNode po_step(const PoCtx& c, PoNode s, int a) {
  const bool alive = (s.used & (1u << PO_A_KILL)) == 0u;
  const bool restored = (s.used & (1u << PO_A_RESTORE)) != 0u;
  const bool is_kill = a == PO_A_KILL;
  const bool is_restore = a == PO_A_RESTORE;
  const bool is_revert = !is_kill && !is_restore;
  const int gi = (a - PO_A_REVERT_BASE) & (PO_MAX_GROUPS - 1);
  const float rdt = c.dt[gi], rog = c.og[gi], rfp = c.fp[gi];
  // a revert after RESTORE is a no-op (eval_plan: reverted[gi] > 0)
  const float dt = is_kill ? c.kill_t
                           : (is_restore ? c.restore_t : (restored ? 0.0f : rdt));
  const float og =
      (is_kill || !alive) ? 0.0f
                          : (is_restore ? c.og_restore : (restored ? 0.0f : rog));
  const float fp = (is_revert && !restored) ? rfp : 0.0f;
  s.ongoing += og;
  s.downtime += dt;
  s.fp_mb += fp;
  s.used |= 1u << a;
  return s;
}

__device__ __forceinline__ float po_score(const PoCtx& c, const PoNode& s) {
  const bool alive = (s.used & (1u << PO_A_KILL)) == 0u;
  const bool restored = (s.used & (1u << PO_A_RESTORE)) != 0u;
  const float ongoing = s.ongoing + (alive ? c.og_horizon : 0.0f);
  const float downtime = s.downtime + (alive ? c.dt_horizon : 0.0f);
  const unsigned rev = restored ? 0xFFFFu : (s.used >> PO_A_REVERT_BASE);
  float loss = 0.0f;
#pragma unroll
  for (int g = 0; g < PO_MAX_GROUPS; ++g)  // sequential order == eval_plan
    loss += ((rev >> g) & 1u) ? 0.0f : c.unrec[g];
  loss += fminf(ongoing, c.remaining);
  loss += restored ? c.restore_loss : 0.0f;
  return -(loss + c.dw * downtime + c.fpw * s.fp_mb);
}

// Plans of one length reach a lane in lexicographic order, so an equal
// reward replaces the incumbent only when the newcomer is shorter.
__device__ __forceinline__ void po_offer(PoBest& b, float r, int len,
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

__device__ __forceinline__ unsigned po_set_field(unsigned w, int field, int a) {
  const int sh = 5 * field;
  return (w & ~(31u << sh)) | ((unsigned)a << sh);
}

// Expands the children of `node`, a plan of length L + J.  `levels` is
// depth_lim - L and `free_l` is n - L (both wave-uniform); depth_lim <= n, so
// a level that may expand always has a child.
template <int J>
__device__ __forceinline__ void po_dfs(const PoCtx& c, const PoNode& node,
                                       int L, int levels, int free_l,
                                       PoPath& path, PoBest& best) {
  if constexpr (J < PO_MAX_DEPTH - 1) {  // L >= 1, so L + J + 1 <= MAX_DEPTH
    // Opaque copies (empty asm): without them every level's loop invariants
    // (the alive/restored lane masks derived from `used`, J >= levels,
    // free_l - J, L + J + 1) are hoisted out of all 15 nested loops at once,
    // which costs several SGPRs per level and spills.  Recomputing them is a
    // couple of scalar instructions per node.
    int lv = levels;
    asm volatile("" : "+s"(lv));
    if (J >= lv) return;
    unsigned avail = ~node.used & c.action_mask;
    int fl = free_l;
    asm volatile("" : "+s"(fl));
    for (int r = fl - J; r > 0; --r) {  // fl - J == popcount(avail)
      const int a = (__ffs(avail) - 1) & 31;
      avail &= avail - 1u;
      PoNode parent = node;
      asm volatile("" : "+v"(parent.used));
      int len = L;
      asm volatile("" : "+s"(len));
      len += J;
      const PoNode child = po_step(c, parent, a);
      if constexpr (J / PO_FIELDS_PER_WORD == 0)
        path.s0 = po_set_field(path.s0, J % PO_FIELDS_PER_WORD, a);
      else if constexpr (J / PO_FIELDS_PER_WORD == 1)
        path.s1 = po_set_field(path.s1, J % PO_FIELDS_PER_WORD, a);
      else
        path.s2 = po_set_field(path.s2, J % PO_FIELDS_PER_WORD, a);
      po_offer(best, po_score(c, child), len + 1, path.s0, path.s1, path.s2);
      po_dfs<J + 1>(c, child, L, levels, free_l, path, best);
    }
  }
}

// out_plan holds six words per item: the packed prefix (3) and the packed
// winning suffix (3), 5 bits per action, 6 actions per word.  The winner is
// prefix[:min(L, len)] + suffix[:len - L].
__global__ __launch_bounds__(PO_BLOCK) void plan_oracle_kernel(
    const float* __restrict__ gscore,  // [S, G]
    const float* __restrict__ gmb,     // [S, G]
    const float* __restrict__ gfiles,  // [S, G]
    const float* __restrict__ proc,    // [S]
    const float* __restrict__ clean,   // [S]
    PlannerParamsDev p, int L, int n_prefix, int n_chunks, long n_units,
    float* __restrict__ out_reward,    // [S, n_prefix]
    int* __restrict__ out_len,         // [S, n_prefix]
    unsigned* __restrict__ out_plan) { // [S, n_prefix, 6]
  __shared__ float lds_dt[PO_MAX_GROUPS];
  __shared__ float lds_og[PO_MAX_GROUPS];
  __shared__ float lds_fp[PO_MAX_GROUPS];
  __shared__ float lds_unrec[PO_MAX_GROUPS];

  const int G = p.n_groups;
  const int n = G + 2;  // non-STOP actions: KILL, RESTORE, revert g
  const int depth_lim = p.max_depth < n ? p.max_depth : n;

  for (long u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int s = (int)(u / n_chunks);
    const int chunk = (int)(u - (long)s * n_chunks);
    const float proc_s = proc[s];

    __syncthreads();  // readers of the previous unit's tables are done
    if (threadIdx.x < PO_MAX_GROUPS) {
      const int g = threadIdx.x;
      float dt = 0.0f, og = 0.0f, fp = 0.0f, unrec = 0.0f;
      if (g < G) {
        const float sc = gscore[(long)s * G + g];
        const float mb = gmb[(long)s * G + g];
        const float files = gfiles[(long)s * G + g];
        dt = p.revert_time_s * fmaxf(files, 1.0f);
        og = p.attack_rate_mbps * dt * proc_s;
        fp = (1.0f - sc) * mb * 0.05f;
        unrec = sc * mb;
      }
      lds_dt[g] = dt;
      lds_og[g] = og;
      lds_fp[g] = fp;
      lds_unrec[g] = unrec;
    }
    __syncthreads();

    PoCtx c;
#pragma unroll
    for (int g = 0; g < PO_MAX_GROUPS; ++g)
      c.unrec[g] = lds_unrec[g];
    c.kill_t = p.kill_time_s;
    c.restore_t = p.restore_time_s;
    c.og_restore = p.attack_rate_mbps * p.restore_time_s * proc_s;
    c.og_horizon = p.attack_rate_mbps * p.horizon_s * proc_s;
    c.dt_horizon = p.horizon_s * proc_s;
    c.remaining = clean[s];
    c.restore_loss = p.restore_loss_mb;
    c.dw = p.downtime_weight;
    c.fpw = p.fp_weight;
    c.action_mask = ((1u << (n + 1)) - 1u) & ~1u;
    c.dt = lds_dt;
    c.og = lds_og;
    c.fp = lds_fp;

    const int pi = chunk * PO_BLOCK + (int)threadIdx.x;
    if (pi < n_prefix) {
      PoNode node = {0.0f, 0.0f, 0.0f, 0u};
      PoBest best = {-INFINITY, 1 << 30, 0u, 0u, 0u};
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
        node = po_step(c, node, a);
        const int w = k / PO_FIELDS_PER_WORD;
        const int f = k - w * PO_FIELDS_PER_WORD;
        p0 = (w == 0) ? po_set_field(p0, f, a) : p0;
        p1 = (w == 1) ? po_set_field(p1, f, a) : p1;
        p2 = (w == 2) ? po_set_field(p2, f, a) : p2;
        // prefix nodes share the item's first action, so they compete here
        po_offer(best, po_score(c, node), k + 1, 0u, 0u, 0u);
      }

      // ---- suffixes ----
      PoPath path = {0u, 0u, 0u};
      po_dfs<0>(c, node, L, depth_lim - L, n - L, path, best);

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

// Caller guarantees: 1 <= G <= 16, 1 <= L <= min(max_depth, G + 2) <= 16,
// n_prefix == (G+2)!/(G+2-L)! < 2^31, outputs sized [S, n_prefix(, 6)].
void launch_plan_oracle(const float* gscore, const float* gmb,
                        const float* gfiles, const float* proc,
                        const float* clean, const PlannerParamsDev& p, int S,
                        int L, int n_prefix, float* out_reward, int* out_len,
                        unsigned* out_plan, hipStream_t s) {
  const int n_chunks = (n_prefix + PO_BLOCK - 1) / PO_BLOCK;
  const long n_units = (long)S * n_chunks;
  const int grid = (int)(n_units < PO_MAX_GRID ? n_units : PO_MAX_GRID);
  plan_oracle_kernel<<<grid, PO_BLOCK, 0, s>>>(gscore, gmb, gfiles, proc, clean,
                                               p, L, n_prefix, n_chunks,
                                               n_units, out_reward, out_len,
                                               out_plan);
}

}  // namespace nerrf
