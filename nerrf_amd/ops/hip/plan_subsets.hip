// Subset-lattice search of the joint (P-process) rollback-planning MDP —
// CDNA4 (gfx950).
//
// The exact optimum of rewards.simulate_plan_multi / eval_plan_multi
// (mcts_multi.hip) as a maximum over SETS of actions, not arrangements.  Every
// term of the reward but `ongoing` depends only on the set of executed
// actions; `ongoing` sums rate * dt * live over the time-consuming actions, a
// KILL adds nothing to it and only lowers `live`, and the loss does not
// decrease in it.  So the best ordering of a set is ascending action id
// (kills, then RESTORE, then reverts; a revert behind a RESTORE is a no-op),
// and with a forced first action a it is a followed by the rest ascending
// (planner/oracle.py has the argument in full).  With n = P + 1 + G <= 25
// actions a state has at most 2^25 sets, whatever the depth.
//
//   0 STOP | 1 + p KILL p | P + 1 RESTORE | P + 2 + g REVERT g
//
// Work split.  A unit is (state, kill mask K, chunk of the 2^G revert masks);
// one WAVE owns a unit and its 64 lanes stride over the chunk's revert masks
// R.  K, popc(K) and live(K) are wave-uniform.  A set larger than
// min(n, max_depth) is skipped.  The sets with RESTORE are few: a revert next
// to RESTORE is a no-op unless it is the first action, and the set with the
// no-op ties with the one without it and loses on length, so per K only
// {K, RESTORE} and the G sets {K, RESTORE, g} with g in front are scored, by
// lanes 0..G of the unit's chunk 0 (lane g's key joins slot g at the
// reduction).
//
// Per-set cost.  The sums over R of the revert time, the false-positive MB
// and the MB left unrecovered are looked up meet-in-the-middle: LDS tables of
// the partial sums over the low 8 and the high 8 group bits (2 x 256 entries
// per quantity), filled once per (block, state).  A set then costs two LDS
// reads per quantity and a few VALU ops for its kills-first reward.  Moving a
// non-kill member a to the front adds rate * dt_a * (live(0) - live(K)) to
// `ongoing` before the min with the damage cap; moving a kill to the front
// changes the plan, not the reward.  No loop over the plan.
//
// Reduction.  A winner is (reward, set mask); its plan is implied.  Between
// equal-length sets the lexicographically smaller ascending plan owns the
// lowest bit of the xor of the masks, so a winner packs into one orderable
// 64-bit key: reward bits (order-preserving) | 31 - length | bit-reversed
// mask.  A lane keeps 18 keys in named registers (one per revert-first
// action, the kills-first best that serves every KILL of K, RESTORE-first);
// nothing is runtime-indexed, nothing goes to scratch.  A butterfly of
// shuffles reduces each over the wave, which writes one row per unit; a
// second, small kernel reduces the rows of a state to its n + 1 winners.
// Key 0 means "no set".
//
// `live` is summed from zero in ascending p (live_score's order).  FP
// contraction is off, so sets that are symmetric in their inputs tie
// bit-for-bit.  The rewards REPORTED to callers come from eval_plan_multi
// itself (bindings.cpp re-evaluates the winners).
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

typedef unsigned long long ps_key_t;

constexpr int PS_MAX_GROUPS = 16;
constexpr int PS_MAX_PROCS = NERRF_MULTI_MAX_PROCS;
constexpr int PS_WAVES = 4;  // units per block
constexpr int PS_BLOCK = PS_WAVES * NERRF_WAVE;
constexpr int PS_HALF = 256;  // entries of one half table: 2^8 group bits
constexpr int PS_MAX_GRID = 4096;
static_assert(PS_BLOCK == PS_HALF, "thread t fills entry t of both half tables");
constexpr int PS_SLOT_BASE = PS_MAX_GROUPS;         // kills-first best
constexpr int PS_SLOT_RESTORE = PS_MAX_GROUPS + 1;  // RESTORE-first best
constexpr int PS_SLOTS = PS_MAX_GROUPS + 2;

// (reward, set mask) as one key; the larger key is the better winner.  The
// mask has bits 1..n (n <= 25): reversed and shifted it fills bits 24..0,
// lowest action id on top.
__device__ __forceinline__ ps_key_t ps_key(float reward, unsigned mask) {
  const unsigned b = __float_as_uint(reward);
  const unsigned hi = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  const unsigned lo = ((31u - (unsigned)__popc(mask)) << 25) | (__brev(mask) >> 6);
  return ((ps_key_t)hi << 32) | lo;
}

__device__ __forceinline__ void ps_offer(ps_key_t& w, ps_key_t k) {
  w = k > w ? k : w;
}

__device__ __forceinline__ ps_key_t ps_wave_max(ps_key_t v) {
#pragma unroll
  for (int off = NERRF_WAVE / 2; off > 0; off >>= 1) {
    const ps_key_t o = __shfl_xor(v, off, NERRF_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// eval_plan_multi's closing expression; 0 - x so that a zero loss is +0.
__device__ __forceinline__ float ps_reward(float loss, float wdown, float wfp) {
  return 0.0f - ((loss + wdown) + wfp);
}

__global__ __launch_bounds__(PS_BLOCK) void plan_subsets_kernel(
    const float* __restrict__ gscore,  // [S, G]
    const float* __restrict__ gmb,     // [S, G]
    const float* __restrict__ gfiles,  // [S, G]
    const float* __restrict__ proc,    // [S, P]
    const float* __restrict__ clean,   // [S]
    PlannerParamsDev p, int P, int chunk_log, int blocks_per_state,
    long n_blocks,
    ps_key_t* __restrict__ rows) {  // [S, 2^P << chunk_log, PS_SLOTS]
  // [0, 256): sums over the low 8 group bits; [256, 512): over the high 8
  __shared__ float t_dt[2 * PS_HALF];  // revert time of the groups in R
  __shared__ float t_fp[2 * PS_HALF];  // false-positive MB of the groups in R
  __shared__ float t_un[2 * PS_HALF];  // unrecovered MB of the groups NOT in R
  // per group, 0 beyond G: revert time, false-positive MB, unrecovered MB,
  // rate * revert time
  __shared__ float g_dt[PS_MAX_GROUPS], g_fp[PS_MAX_GROUPS];
  __shared__ float g_un[PS_MAX_GROUPS], g_rdt[PS_MAX_GROUPS];

  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int lane = tid & (NERRF_WAVE - 1);
  // uniform by construction; readfirstlane tells the compiler so, and the
  // unit's K, live sums and budget stay in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(tid / NERRF_WAVE);
  const int G = p.n_groups;
  const int n = P + 1 + G;
  const int depth_lim = p.max_depth < n ? p.max_depth : n;
  const int n_units = (1 << P) << chunk_log;  // per state
  const int chunk_bits = G - chunk_log;       // revert masks per chunk, log2
  const float rate = p.attack_rate_mbps;
  const float rdt_restore = rate * p.restore_time_s;

  for (long b = (long)__builtin_amdgcn_workgroup_id_x(); b < n_blocks;
       b += (long)gridDim.x) {
    const int s = (int)(b / blocks_per_state);
    const int unit = (int)(b - (long)s * blocks_per_state) * PS_WAVES + wave;

    __syncthreads();  // readers of the previous state's tables are done
    if (tid < PS_MAX_GROUPS) {
      float dt = 0.0f, fp = 0.0f, un = 0.0f;
      if (tid < G) {
        const float sc = gscore[(long)s * G + tid];
        const float mb = gmb[(long)s * G + tid];
        dt = p.revert_time_s * fmaxf(gfiles[(long)s * G + tid], 1.0f);
        fp = (1.0f - sc) * mb * 0.05f;
        un = sc * mb;
      }
      g_dt[tid] = dt;
      g_fp[tid] = fp;
      g_un[tid] = un;
      g_rdt[tid] = rate * dt;
    }
    __syncthreads();
    {
      // entry `tid` of both halves; ascending g from zero within a half
      float dl = 0.0f, dh = 0.0f, fl = 0.0f, fh = 0.0f, ul = 0.0f, uh = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = ((tid >> j) & 1) != 0;
        dl += in ? g_dt[j] : 0.0f;
        dh += in ? g_dt[j + 8] : 0.0f;
        fl += in ? g_fp[j] : 0.0f;
        fh += in ? g_fp[j + 8] : 0.0f;
        ul += in ? 0.0f : g_un[j];
        uh += in ? 0.0f : g_un[j + 8];
      }
      t_dt[tid] = dl;
      t_dt[PS_HALF + tid] = dh;
      t_fp[tid] = fl;
      t_fp[PS_HALF + tid] = fh;
      t_un[tid] = ul;
      t_un[PS_HALF + tid] = uh;
    }
    __syncthreads();
    if (unit >= n_units) continue;  // a padding wave of the state's last block

    const unsigned K = (unsigned)unit >> chunk_log;
    const unsigned chunk = (unsigned)unit & ((1u << chunk_log) - 1u);
    const int k = __popc(K);
    float live0 = 0.0f, live_k = 0.0f;
#pragma unroll
    for (int q = 0; q < PS_MAX_PROCS; ++q) {
      const float ps = q < P ? proc[(long)s * P + q] : 0.0f;
      live0 += ps;
      live_k += ((K >> q) & 1u) ? 0.0f : ps;
    }
    const bool any_alive = K != (1u << P) - 1u;
    const float hz_og = any_alive ? rate * p.horizon_s * live_k : 0.0f;
    const float hz_dn = any_alive ? p.horizon_s * live_k : 0.0f;
    const float kdown = (float)k * p.kill_time_s;
    const float dlive = live0 - live_k;
    const float rem = clean[s];
    const unsigned kbits = K << 1;
    const int a_revert = P + 2;
    const int budget = depth_lim - k;  // actions left next to the kills

    // what moving REVERT g to the front adds to `ongoing`
    float ex[PS_MAX_GROUPS];
#pragma unroll
    for (int g = 0; g < PS_MAX_GROUPS; ++g) ex[g] = g_rdt[g] * dlive;

    ps_key_t wg[PS_MAX_GROUPS];
#pragma unroll
    for (int g = 0; g < PS_MAX_GROUPS; ++g) wg[g] = 0ull;
    ps_key_t wbase = 0ull, wrestore = 0ull;

    // ---- sets without RESTORE: K and the chunk's revert masks ----
    if (budget >= 0) {
      const unsigned r0 = chunk << chunk_bits;
      for (unsigned i = (unsigned)lane; i < (1u << chunk_bits);
           i += NERRF_WAVE) {
        const unsigned R = r0 + i;  // < 2^G <= 2^16
        if (__popc(R) > budget) continue;
        const unsigned lo = R & (PS_HALF - 1), hi = PS_HALF + (R >> 8);
        const float dts = t_dt[lo] + t_dt[hi];
        const float fps = t_fp[lo] + t_fp[hi];
        const float uns = t_un[lo] + t_un[hi];
        const float og = rate * dts * live_k + hz_og;
        const float wdown = p.downtime_weight * (kdown + dts + hz_dn);
        const float wfp = p.fp_weight * fps;
        const unsigned mask = kbits | (R << a_revert);
        ps_offer(wbase, ps_key(ps_reward(uns + fminf(og, rem), wdown, wfp), mask));
#pragma unroll
        for (int g = 0; g < PS_MAX_GROUPS; ++g) {
          if ((R >> g) & 1u) {
            const float loss = uns + fminf(og + ex[g], rem);
            ps_offer(wg[g], ps_key(ps_reward(loss, wdown, wfp), mask));
          }
        }
      }
    }

    // ---- sets with RESTORE: {K, RESTORE} and {K, RESTORE, g}, g first ----
    ps_key_t wfront = 0ull;  // lane g < G: {K, RESTORE, g}
    if (chunk == 0u && budget >= 1 && lane <= G) {
      const unsigned rbit = 1u << (P + 1);
      const float og = rdt_restore * live_k + hz_og;
      if (lane == G) {
        const float wdown =
            p.downtime_weight * (kdown + p.restore_time_s + hz_dn);
        const unsigned mask = kbits | rbit;
        ps_offer(wbase, ps_key(ps_reward(fminf(og, rem) + p.restore_loss_mb,
                                         wdown, 0.0f), mask));
        ps_offer(wrestore,
                 ps_key(ps_reward(fminf(og + rdt_restore * dlive, rem) +
                                      p.restore_loss_mb, wdown, 0.0f), mask));
      } else if (budget >= 2) {  // lane < G <= 16
        const float dt = g_dt[lane];
        const float wdown =
            p.downtime_weight * (kdown + dt + p.restore_time_s + hz_dn);
        const float loss =
            fminf(g_rdt[lane] * live0 + og, rem) + p.restore_loss_mb;
        wfront = ps_key(ps_reward(loss, wdown, p.fp_weight * g_fp[lane]),
                        kbits | rbit | (1u << (a_revert + lane)));
      }
    }

    // ---- one row per unit ----
    ps_key_t* row = rows + ((long)s * n_units + unit) * PS_SLOTS;
#pragma unroll
    for (int g = 0; g < PS_MAX_GROUPS; ++g) {
      ps_key_t v = ps_wave_max(wg[g]);
      ps_offer(v, __shfl(wfront, g, NERRF_WAVE));
      if (lane == 0) row[g] = v;
    }
    {
      const ps_key_t vb = ps_wave_max(wbase), vr = ps_wave_max(wrestore);
      if (lane == 0) {
        row[PS_SLOT_BASE] = vb;
        row[PS_SLOT_RESTORE] = vr;
      }
    }
  }
}

// One wave per (state, first action a >= 1): the best key of its slot over
// the state's rows; a KILL p reads the kills-first slot of the rows whose K
// holds p.  out[s, 0], the empty plan, is key 0.
__global__ __launch_bounds__(NERRF_WAVE) void plan_subsets_reduce_kernel(
    const ps_key_t* __restrict__ rows,  // [S, n_units, PS_SLOTS]
    int P, int G, int chunk_log, long n_items,  // n_items = S * n
    ps_key_t* __restrict__ out) {               // [S, n + 1]
  const int lane = (int)__builtin_amdgcn_workitem_id_x();
  const int n = P + 1 + G;
  const int n_units = (1 << P) << chunk_log;
  for (long it = (long)__builtin_amdgcn_workgroup_id_x(); it < n_items;
       it += (long)gridDim.x) {
    const long s = it / n;
    const int a = 1 + (int)(it - s * n);
    const bool is_kill = a <= P;
    const int slot = is_kill ? PS_SLOT_BASE
                             : (a == P + 1 ? PS_SLOT_RESTORE : a - (P + 2));
    ps_key_t best = 0ull;
    for (int u = lane; u < n_units; u += NERRF_WAVE) {
      const unsigned K = (unsigned)u >> chunk_log;
      if (is_kill && !((K >> (a - 1)) & 1u)) continue;
      ps_offer(best, rows[(s * n_units + u) * PS_SLOTS + slot]);
    }
    best = ps_wave_max(best);
    if (lane == 0) {
      out[s * (n + 1) + a] = best;
      if (a == 1) out[s * (n + 1)] = 0ull;
    }
  }
}

}  // namespace

// Caller guarantees: 1 <= P <= 8, 1 <= G <= 16, max_depth >= 1,
// 0 <= chunk_log <= max(G - 6, 0), S * (2^P << chunk_log) <= 2^20,
// rows sized [S, 2^P << chunk_log, 18] and out [S, P + 2 + G] (64-bit).
hipError_t launch_plan_subsets(const float* gscore, const float* gmb,
                               const float* gfiles, const float* proc,
                               const float* clean, const PlannerParamsDev& p,
                               int P, int S, int chunk_log,
                               unsigned long long* rows,
                               unsigned long long* out, hipStream_t s) {
  const int n_units = (1 << P) << chunk_log;
  const int blocks_per_state = (n_units + PS_WAVES - 1) / PS_WAVES;
  const long n_blocks = (long)S * blocks_per_state;
  const int grid = (int)(n_blocks < PS_MAX_GRID ? n_blocks : PS_MAX_GRID);
  plan_subsets_kernel<<<grid, PS_BLOCK, 0, s>>>(
      gscore, gmb, gfiles, proc, clean, p, P, chunk_log, blocks_per_state,
      n_blocks, rows);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const long n_items = (long)S * (P + 1 + p.n_groups);
  const int rgrid = (int)(n_items < PS_MAX_GRID ? n_items : PS_MAX_GRID);
  plan_subsets_reduce_kernel<<<rgrid, NERRF_WAVE, 0, s>>>(
      rows, P, p.n_groups, chunk_log, n_items, out);
  return hipGetLastError();
}

}  // namespace nerrf

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
