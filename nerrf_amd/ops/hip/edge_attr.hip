// Per-file edge attribution — CDNA4 (gfx950).
//
// Reduces the whole scored edge list to one winner per file node: for every
// file, the process whose wanted-direction edge (write: proc -> file, read:
// file -> proc) carries the highest logit, that logit, and how many such
// edges reach the hot threshold.  Nodes [0, n_files) are files, nodes
// [n_files, n_nodes) are processes.
//
// Pass 1 (one thread per edge, grid-stride, at most 1024 x 256 threads): an
// edge is skipped when an endpoint is outside [0, n_nodes), when it does not
// join exactly one file and one process, when it runs the other way, or when
// its logit is NaN — so a bad index is never an address.  Otherwise
//   v   = logit + 0.0f                         (-0.0 -> +0.0)
//   key = orderable(v) << 32 | 0xFFFFFFFF - p  (p = proc node - n_files)
// goes into best[file] by 64-bit atomicMax, and n_hot[file] is bumped when
// v >= thr_logit.  orderable() is the monotone fp32 -> u32 map, so the
// maximum key is the maximum logit by float comparison with ties to the
// lowest process index; key 0 means "no edge" because every non-NaN float
// maps to a non-zero high word.  Integer max and add commute: the result does
// not depend on arrival order.
//
// Pass 2 (one thread per file) decodes best[f] into culprit[f] (process node
// index, -1 without an edge) and best_logit[f] (-inf without an edge).
//
// Edges arrive process-major, so the lanes of a wave hit different files; the
// atomics go out one per lane with no wave-level pre-combine.
#include "common.h"

namespace nerrf {

#define EA_BLOCK 256
#define EA_MAX_BLOCKS 1024

__device__ __forceinline__ unsigned ea_orderable(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float ea_from_orderable(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__launch_bounds__(EA_BLOCK)
__global__ void edge_attr_reduce_kernel(
    const float* __restrict__ logit,  // [E]
    const long* __restrict__ src,     // [E]
    const long* __restrict__ dst,     // [E]
    unsigned long long* __restrict__ best,  // [n_files], zero-initialised
    int* __restrict__ n_hot,                // [n_files], zero-initialised
    long n_edges, long n_files, long n_nodes, bool want_write,
    float thr_logit) {
  const long stride = (long)gridDim.x * EA_BLOCK;
  for (long e = (long)blockIdx.x * EA_BLOCK + threadIdx.x; e < n_edges;
       e += stride) {
    const long s = src[e];
    const long d = dst[e];
    if (s < 0 || s >= n_nodes || d < 0 || d >= n_nodes) continue;
    const bool s_file = s < n_files;
    const bool d_file = d < n_files;
    if (s_file == d_file) continue;      // file-file or proc-proc
    if (d_file != want_write) continue;  // write edges end in a file
    const float x = logit[e];
    if (x != x) continue;  // NaN
    const float v = x + 0.0f;
    const long f = d_file ? d : s;               // in [0, n_files)
    const long p = (d_file ? s : d) - n_files;   // in [0, n_nodes - n_files)
    const unsigned long long key =
        ((unsigned long long)ea_orderable(v) << 32) |
        (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
    atomicMax(best + f, key);
    if (v >= thr_logit) atomicAdd(n_hot + f, 1);
  }
}

__launch_bounds__(EA_BLOCK)
__global__ void edge_attr_decode_kernel(
    const unsigned long long* __restrict__ best,  // [n_files]
    long* __restrict__ culprit,                   // [n_files]
    float* __restrict__ best_logit,               // [n_files]
    long n_files) {
  const long stride = (long)gridDim.x * EA_BLOCK;
  for (long f = (long)blockIdx.x * EA_BLOCK + threadIdx.x; f < n_files;
       f += stride) {
    const unsigned long long key = best[f];
    if (key == 0ull) {
      culprit[f] = -1;
      best_logit[f] = -INFINITY;
    } else {
      culprit[f] = n_files + (long)(0xFFFFFFFFu - (unsigned)key);
      best_logit[f] = ea_from_orderable((unsigned)(key >> 32));
    }
  }
}

static int ea_grid(long n) {
  const long blocks = (n + EA_BLOCK - 1) / EA_BLOCK;
  return (int)(blocks < EA_MAX_BLOCKS ? blocks : EA_MAX_BLOCKS);
}

// best and n_hot must be zero on entry; n_edges > 0 and n_files > 0 (a zero
// grid is a launch error — the binding returns the "no edge" outputs itself).
void launch_edge_attr(const float* logit, const long* src, const long* dst,
                      unsigned long long* best, int* n_hot, long* culprit,
                      float* best_logit, long n_edges, long n_files,
                      long n_nodes, bool want_write, float thr_logit,
                      hipStream_t s) {
  if (n_edges <= 0 || n_files <= 0) return;
  edge_attr_reduce_kernel<<<ea_grid(n_edges), EA_BLOCK, 0, s>>>(
      logit, src, dst, best, n_hot, n_edges, n_files, n_nodes, want_write,
      thr_logit);
  edge_attr_decode_kernel<<<ea_grid(n_files), EA_BLOCK, 0, s>>>(
      best, culprit, best_logit, n_files);
}

}  // namespace nerrf
