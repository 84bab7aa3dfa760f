// Fused LSTM gate pointwise + state update — CDNA4 (gfx950).
//
// Forward:  given pre-activation gates [B, 4H] (= x W_ih + h W_hh + b,
// the GEMMs stay in hipBLASLt), previous (h, c) and a per-row validity mask,
// computes in ONE launch what eager PyTorch does in ~12 elementwise kernels:
//   i,f,o = sigmoid; g = tanh; c' = f*c + i*g; h' = o*tanh(c');
//   masked rows pass (h, c) through unchanged.
// Also writes the post-activation gates (saved for backward).
//
// Backward: the matching fused gate-gradient kernel; the two outer GEMMs
// (grad_gates @ W_hh, grad_gates^T @ h) stay in hipBLASLt.
//
// Counterpart of the "fused LSTM cell" obligation in SURVEY.md §2a;
// validated against nerrf_amd/ops/reference.py::lstm_pointwise_{fwd,bwd}_ref.
#include "common.h"

namespace nerrf {

// xg_stride: row stride (elements) of the xg slice — lets the sequence op
// read gate slabs straight out of a [T, B, 2*4H] dual-direction projection.
// hout_stride: row stride of h_out — lets both directions write straight
// into the [T, B, 2H] concatenated output (no torch.cat afterwards).
// prev_rows: rows of the previous state (hg, c_prev, h_prev).  Rows
// b >= prev_rows start from a zero state (hg = c_prev = h_prev = 0) and read
// none of the three — the packed sequence op runs a step over more rows than
// its predecessor had (reverse direction) without a zero-fill or cat, and
// the hg scratch may hold stale rows of a longer step there.
template <typename T>
__global__ void lstm_pointwise_fwd_kernel(
    const T* __restrict__ hg,         // [B, 4H] = h_prev @ W_hh^T (beta=0 GEMM)
    const T* __restrict__ xg,         // [B(row-stride xg_stride), 4H]
    const T* __restrict__ bias,       // [4H]
    const T* __restrict__ c_prev,     // [B, H]
    const T* __restrict__ h_prev,     // [B(row-stride hprev_stride), H]
    const float* __restrict__ mask,   // [B] or nullptr
    T* __restrict__ h_out,            // [B(row-stride hout_stride), H]
    T* __restrict__ c_out,            // [B, H]
    T* __restrict__ gates_act,        // [B, 4H] or nullptr (inference)
    long batch, int hdim, long xg_stride, long hout_stride,
    long hprev_stride, long prev_rows) {
  const long total = batch * hdim;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const long b = t / hdim;
    const int d = (int)(t % hdim);
    const long g0 = b * 4 * hdim + d;
    const long x0 = b * xg_stride + d;
    const bool has_prev = b < prev_rows;
    float hg_i = 0.0f, hg_f = 0.0f, hg_g = 0.0f, hg_o = 0.0f, cp = 0.0f;
    if (has_prev) {
      hg_i = to_f32(hg[g0]);
      hg_f = to_f32(hg[g0 + hdim]);
      hg_g = to_f32(hg[g0 + 2 * hdim]);
      hg_o = to_f32(hg[g0 + 3 * hdim]);
      cp = to_f32(c_prev[t]);
    }
    const float ip = hg_i + to_f32(xg[x0]) + to_f32(bias[d]);
    const float fp = hg_f + to_f32(xg[x0 + hdim]) + to_f32(bias[d + hdim]);
    const float gp = hg_g + to_f32(xg[x0 + 2 * hdim]) + to_f32(bias[d + 2 * hdim]);
    const float op = hg_o + to_f32(xg[x0 + 3 * hdim]) + to_f32(bias[d + 3 * hdim]);
    const float i = sigmoidf_(ip);
    const float f = sigmoidf_(fp);
    const float g = tanhf(gp);
    const float o = sigmoidf_(op);
    float cn = f * cp + i * g;
    float hn = o * tanhf(cn);
    if (mask != nullptr) {
      const float m = mask[b];
      const float hp = has_prev ? to_f32(h_prev[b * hprev_stride + d]) : 0.0f;
      cn = m * cn + (1.0f - m) * cp;
      hn = m * hn + (1.0f - m) * hp;
    }
    c_out[t] = from_f32<T>(cn);
    h_out[b * hout_stride + d] = from_f32<T>(hn);
    if (gates_act != nullptr) {  // inference skips the backward-only store
      gates_act[g0] = from_f32<T>(i);
      gates_act[g0 + hdim] = from_f32<T>(f);
      gates_act[g0 + 2 * hdim] = from_f32<T>(g);
      gates_act[g0 + 3 * hdim] = from_f32<T>(o);
    }
  }
}

template <typename T>
__global__ void lstm_pointwise_bwd_kernel(
    const T* __restrict__ grad_h,     // [B, H] recurrent grad
    const T* __restrict__ grad_out_t, // [B(row-stride gout_stride), H] or nullptr
    const T* __restrict__ grad_c,     // [B, H]
    const T* __restrict__ gates_act,  // [B, 4H]
    const T* __restrict__ c_prev,     // [B, H]
    const float* __restrict__ mask,   // [B] or nullptr
    T* __restrict__ grad_gates,       // [B(row-stride gg_stride), 4H]
    T* __restrict__ grad_c_prev,      // [B, H]
    T* __restrict__ grad_h_pass,      // [B, H] or nullptr (no mask: all 0)
    long batch, int hdim, long gout_stride, long gg_stride, long in_rows,
    long prev_rows) {
  const long total = batch * hdim;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const long b = t / hdim;
    const int d = (int)(t % hdim);
    const long g0 = b * 4 * hdim + d;
    const long o0 = b * gg_stride + d;
    const float i = to_f32(gates_act[g0]);
    const float f = to_f32(gates_act[g0 + hdim]);
    const float g = to_f32(gates_act[g0 + 2 * hdim]);
    const float o = to_f32(gates_act[g0 + 3 * hdim]);
    const float cp = (b < prev_rows) ? to_f32(c_prev[t]) : 0.0f;
    const float m = (mask != nullptr) ? mask[b] : 1.0f;
    const float tcn = tanhf(f * cp + i * g);  // tanh of UNMASKED c_new
    const bool has_in = b < in_rows;
    float gh_in = has_in ? to_f32(grad_h[t]) : 0.0f;
    if (grad_out_t != nullptr) gh_in += to_f32(grad_out_t[b * gout_stride + d]);
    const float gc_in = has_in ? to_f32(grad_c[t]) : 0.0f;
    const float gh = gh_in * m;
    const float gc = gc_in * m;
    const float d_o = gh * tcn;
    const float d_c = gc + gh * o * (1.0f - tcn * tcn);
    const float d_i = d_c * g;
    const float d_f = d_c * cp;
    const float d_g = d_c * i;
    grad_c_prev[t] = from_f32<T>(d_c * f + gc_in * (1.0f - m));
    if (grad_h_pass != nullptr) grad_h_pass[t] = from_f32<T>(gh_in * (1.0f - m));
    grad_gates[o0] = from_f32<T>(d_i * i * (1.0f - i));
    grad_gates[o0 + hdim] = from_f32<T>(d_f * f * (1.0f - f));
    grad_gates[o0 + 2 * hdim] = from_f32<T>(d_g * (1.0f - g * g));
    grad_gates[o0 + 3 * hdim] = from_f32<T>(d_o * o * (1.0f - o));
  }
}

// ---------------------------------------------------------------------------
// vectorised variants: V adjacent hidden elements per thread so every global
// access is a 8/16-byte load (scalar bf16 is a measured 2-2.5x loss on CDNA4).
// Used whenever hdim % V == 0 (H=256 in production).
// ---------------------------------------------------------------------------

template <typename T, int V>
struct alignas(sizeof(T) * V) VecT {
  T v[V];
};

template <typename T, int V>
__global__ void lstm_pointwise_fwd_vec_kernel(
    const T* __restrict__ hg, const T* __restrict__ xg,
    const T* __restrict__ bias, const T* __restrict__ c_prev,
    const T* __restrict__ h_prev, const float* __restrict__ mask,
    T* __restrict__ h_out, T* __restrict__ c_out, T* __restrict__ gates_act,
    long batch, int hdim, long xg_stride, long hout_stride,
    long hprev_stride, long prev_rows) {
  using VT = VecT<T, V>;
  const int hv = hdim / V;
  const long total = batch * hv;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const long b = t / hv;
    const int dv = (int)(t % hv) * V;
    const long g0 = b * 4 * hdim + dv;
    const long x0 = b * xg_stride + dv;
    const long c0 = b * (long)hdim + dv;
    // rows past the previous state start from zero and read none of it
    const bool has_prev = b < prev_rows;
    VT hg_i, hg_f, hg_g, hg_o, cp_v;
    if (has_prev) {
      hg_i = *reinterpret_cast<const VT*>(hg + g0);
      hg_f = *reinterpret_cast<const VT*>(hg + g0 + hdim);
      hg_g = *reinterpret_cast<const VT*>(hg + g0 + 2 * hdim);
      hg_o = *reinterpret_cast<const VT*>(hg + g0 + 3 * hdim);
      cp_v = *reinterpret_cast<const VT*>(c_prev + c0);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        hg_i.v[j] = hg_f.v[j] = hg_g.v[j] = hg_o.v[j] = cp_v.v[j] =
            from_f32<T>(0.0f);
    }
    const VT xg_i = *reinterpret_cast<const VT*>(xg + x0);
    const VT xg_f = *reinterpret_cast<const VT*>(xg + x0 + hdim);
    const VT xg_g = *reinterpret_cast<const VT*>(xg + x0 + 2 * hdim);
    const VT xg_o = *reinterpret_cast<const VT*>(xg + x0 + 3 * hdim);
    const VT b_i = *reinterpret_cast<const VT*>(bias + dv);
    const VT b_f = *reinterpret_cast<const VT*>(bias + dv + hdim);
    const VT b_g = *reinterpret_cast<const VT*>(bias + dv + 2 * hdim);
    const VT b_o = *reinterpret_cast<const VT*>(bias + dv + 3 * hdim);
    VT hp_v;
    const float m = (mask != nullptr) ? mask[b] : 1.0f;
    if (mask != nullptr) {
      if (has_prev) {
        hp_v = *reinterpret_cast<const VT*>(h_prev + b * hprev_stride + dv);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) hp_v.v[j] = from_f32<T>(0.0f);
      }
    }
    VT ho_v, co_v, ga_i, ga_f, ga_g, ga_o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float i = sigmoidf_(to_f32(hg_i.v[j]) + to_f32(xg_i.v[j]) + to_f32(b_i.v[j]));
      const float f = sigmoidf_(to_f32(hg_f.v[j]) + to_f32(xg_f.v[j]) + to_f32(b_f.v[j]));
      const float g = tanhf(to_f32(hg_g.v[j]) + to_f32(xg_g.v[j]) + to_f32(b_g.v[j]));
      const float o = sigmoidf_(to_f32(hg_o.v[j]) + to_f32(xg_o.v[j]) + to_f32(b_o.v[j]));
      const float cp = to_f32(cp_v.v[j]);
      float cn = f * cp + i * g;
      float hn = o * tanhf(cn);
      if (mask != nullptr) {
        cn = m * cn + (1.0f - m) * cp;
        hn = m * hn + (1.0f - m) * to_f32(hp_v.v[j]);
      }
      co_v.v[j] = from_f32<T>(cn);
      ho_v.v[j] = from_f32<T>(hn);
      ga_i.v[j] = from_f32<T>(i);
      ga_f.v[j] = from_f32<T>(f);
      ga_g.v[j] = from_f32<T>(g);
      ga_o.v[j] = from_f32<T>(o);
    }
    *reinterpret_cast<VT*>(c_out + c0) = co_v;
    *reinterpret_cast<VT*>(h_out + b * hout_stride + dv) = ho_v;
    if (gates_act != nullptr) {
      *reinterpret_cast<VT*>(gates_act + g0) = ga_i;
      *reinterpret_cast<VT*>(gates_act + g0 + hdim) = ga_f;
      *reinterpret_cast<VT*>(gates_act + g0 + 2 * hdim) = ga_g;
      *reinterpret_cast<VT*>(gates_act + g0 + 3 * hdim) = ga_o;
    }
  }
}

// ACC = true additionally folds this launch's bias-gradient partial
// (sum over rows of the grad_gates values just stored) into an f32 slab
// bias_accum[P, 4H], so the sequence backward never re-reads grad_gates for
// gg.sum(0).  It relies on blockDim.x == 256 and 256 % (hdim/V) == 0: the
// column group t % hv of a thread is then the same on every grid-stride
// iteration and its 4*V sums stay in registers (no LDS, no atomics in the
// row loop).  After the loop the threads of a block that share a column
// group combine once (wave shuffle, then LDS) and block p adds the block's
// 4H sums into slab row p with plain coalesced loads/stores: launches on one
// stream are ordered, nobody else touches row p, and the result is bitwise
// reproducible.  Needs gridDim.x <= P and R*4H floats of dynamic LDS (see
// launch_bwd_vec).  ACC = false is the plain kernel.
template <typename T, int V, bool ACC>
__global__ void __launch_bounds__(ACC ? 256 : 1024)
lstm_pointwise_bwd_vec_kernel(
    const T* __restrict__ grad_h, const T* __restrict__ grad_out_t,
    const T* __restrict__ grad_c, const T* __restrict__ gates_act,
    const T* __restrict__ c_prev, const float* __restrict__ mask,
    T* __restrict__ grad_gates, T* __restrict__ grad_c_prev,
    T* __restrict__ grad_h_pass, float* __restrict__ bias_accum,
    long batch, int hdim, long gout_stride, long gg_stride, long in_rows,
    long prev_rows) {
  using VT = VecT<T, V>;
  float s_i[V], s_f[V], s_g[V], s_o[V];
  if constexpr (ACC) {
#pragma unroll
    for (int j = 0; j < V; ++j) s_i[j] = s_f[j] = s_g[j] = s_o[j] = 0.0f;
  }
  const int hv = hdim / V;
  const long total = batch * hv;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const long b = t / hv;
    const int dv = (int)(t % hv) * V;
    const long g0 = b * 4 * hdim + dv;
    const long o0 = b * gg_stride + dv;
    const long c0 = b * (long)hdim + dv;
    const VT ga_i = *reinterpret_cast<const VT*>(gates_act + g0);
    const VT ga_f = *reinterpret_cast<const VT*>(gates_act + g0 + hdim);
    const VT ga_g = *reinterpret_cast<const VT*>(gates_act + g0 + 2 * hdim);
    const VT ga_o = *reinterpret_cast<const VT*>(gates_act + g0 + 3 * hdim);
    // rows >= prev_rows had a zero previous cell state; rows >= in_rows
    // have no incoming recurrent gradient — neither is read there
    VT cp_v, gh_v, gc_v;
    if (b < prev_rows) {
      cp_v = *reinterpret_cast<const VT*>(c_prev + c0);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) cp_v.v[j] = from_f32<T>(0.0f);
    }
    if (b < in_rows) {
      gh_v = *reinterpret_cast<const VT*>(grad_h + c0);
      gc_v = *reinterpret_cast<const VT*>(grad_c + c0);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) gh_v.v[j] = gc_v.v[j] = from_f32<T>(0.0f);
    }
    VT go_v;
    if (grad_out_t != nullptr)
      go_v = *reinterpret_cast<const VT*>(grad_out_t + b * gout_stride + dv);
    const float m = (mask != nullptr) ? mask[b] : 1.0f;
    VT gg_i, gg_f, gg_g, gg_o, gcp_v, ghp_v;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float i = to_f32(ga_i.v[j]);
      const float f = to_f32(ga_f.v[j]);
      const float g = to_f32(ga_g.v[j]);
      const float o = to_f32(ga_o.v[j]);
      const float cp = to_f32(cp_v.v[j]);
      const float tcn = tanhf(f * cp + i * g);
      float gh_in = to_f32(gh_v.v[j]);
      if (grad_out_t != nullptr) gh_in += to_f32(go_v.v[j]);
      const float gc_in = to_f32(gc_v.v[j]);
      const float gh = gh_in * m;
      const float gc = gc_in * m;
      const float d_o = gh * tcn;
      const float d_c = gc + gh * o * (1.0f - tcn * tcn);
      const float d_i = d_c * g;
      const float d_f = d_c * cp;
      const float d_g = d_c * i;
      gcp_v.v[j] = from_f32<T>(d_c * f + gc_in * (1.0f - m));
      ghp_v.v[j] = from_f32<T>(gh_in * (1.0f - m));
      gg_i.v[j] = from_f32<T>(d_i * i * (1.0f - i));
      gg_f.v[j] = from_f32<T>(d_f * f * (1.0f - f));
      gg_g.v[j] = from_f32<T>(d_g * (1.0f - g * g));
      gg_o.v[j] = from_f32<T>(d_o * o * (1.0f - o));
    }
    if constexpr (ACC) {
      // Sum the STORED (rounded) values: what gg.sum(0) would read back.
      // The test on the pointer (never null here, but opaque to the
      // compiler) keeps these adds in a basic block of their own: in one
      // block with the gate arithmetic they change how that arithmetic is
      // contracted and packed, and the stored values then differ from the
      // plain kernel's in the last f32 bit.
      if (bias_accum != nullptr) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          s_i[j] += to_f32(gg_i.v[j]);
          s_f[j] += to_f32(gg_f.v[j]);
          s_g[j] += to_f32(gg_g.v[j]);
          s_o[j] += to_f32(gg_o.v[j]);
        }
      }
    }
    *reinterpret_cast<VT*>(grad_c_prev + c0) = gcp_v;
    if (grad_h_pass != nullptr)  // without a mask it is identically zero
      *reinterpret_cast<VT*>(grad_h_pass + c0) = ghp_v;
    *reinterpret_cast<VT*>(grad_gates + o0) = gg_i;
    *reinterpret_cast<VT*>(grad_gates + o0 + hdim) = gg_f;
    *reinterpret_cast<VT*>(grad_gates + o0 + 2 * hdim) = gg_g;
    *reinterpret_cast<VT*>(grad_gates + o0 + 3 * hdim) = gg_o;
  }
  if constexpr (ACC) {
    // [R, 4H] block partials: one per wave, or per 256/hv thread group
    extern __shared__ float bias_red[];
    const int tid = threadIdx.x;
    const int gdim = 4 * hdim;
    // hv divides 256, so it is a power of two: lanes l and l ^ off share a
    // column group for every off that is a multiple of hv
    for (int off = NERRF_WAVE / 2; off >= hv; off >>= 1) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        s_i[j] += __shfl_xor(s_i[j], off, NERRF_WAVE);
        s_f[j] += __shfl_xor(s_f[j], off, NERRF_WAVE);
        s_g[j] += __shfl_xor(s_g[j], off, NERRF_WAVE);
        s_o[j] += __shfl_xor(s_o[j], off, NERRF_WAVE);
      }
    }
    const bool wide = hv >= NERRF_WAVE;  // no two lanes of a wave share a group
    const int nrep = wide ? 256 / hv : 256 / NERRF_WAVE;
    const int rep = wide ? tid / hv : tid / NERRF_WAVE;
    if (wide || (tid & (NERRF_WAVE - 1)) < hv) {
      float* dst = bias_red + rep * gdim + (tid % hv) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        dst[j] = s_i[j];
        dst[hdim + j] = s_f[j];
        dst[2 * hdim + j] = s_g[j];
        dst[3 * hdim + j] = s_o[j];
      }
    }
    __syncthreads();
    float* row = bias_accum + (long)blockIdx.x * gdim;
    for (int i = tid; i < gdim; i += 256) {
      float acc = bias_red[i];
      for (int r = 1; r < nrep; ++r) acc += bias_red[r * gdim + i];
      row[i] += acc;
    }
  }
}

// ---------------------------------------------------------------------------
// host launchers (they instantiate every kernel variant above).  A launch
// over zero rows is a no-op: a grid of 0 blocks is a launch error.
// ---------------------------------------------------------------------------

static inline int grid_elems(long total, int block) {
  long blocks = (total + block - 1) / block;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

void launch_lstm_pointwise_fwd(const void* hg, const void* xg, const void* bias,
                               const void* c_prev, const void* h_prev,
                               const float* mask, void* h_out, void* c_out,
                               void* gates_act, long batch, int hdim,
                               long xg_stride, long hout_stride,
                               long hprev_stride, long prev_rows, bool bf16,
                               hipStream_t s) {
  if (batch <= 0) return;
  const int block = 256;
  // vectorised path (16-B global accesses) whenever the layout allows
  const int v = bf16 ? 8 : 4;
  const bool vec = hdim % v == 0 && xg_stride % v == 0 &&
                   hout_stride % v == 0 && hprev_stride % v == 0;
  if (bf16) {
    if (vec) {
      const int grid = grid_elems(batch * (hdim / v), block);
      lstm_pointwise_fwd_vec_kernel<__hip_bfloat16, 8><<<grid, block, 0, s>>>(
          (const __hip_bfloat16*)hg, (const __hip_bfloat16*)xg,
          (const __hip_bfloat16*)bias, (const __hip_bfloat16*)c_prev,
          (const __hip_bfloat16*)h_prev, mask, (__hip_bfloat16*)h_out,
          (__hip_bfloat16*)c_out, (__hip_bfloat16*)gates_act, batch, hdim,
          xg_stride, hout_stride, hprev_stride, prev_rows);
      return;
    }
    const int grid = grid_elems(batch * hdim, block);
    lstm_pointwise_fwd_kernel<__hip_bfloat16><<<grid, block, 0, s>>>(
        (const __hip_bfloat16*)hg, (const __hip_bfloat16*)xg,
        (const __hip_bfloat16*)bias, (const __hip_bfloat16*)c_prev,
        (const __hip_bfloat16*)h_prev, mask, (__hip_bfloat16*)h_out,
        (__hip_bfloat16*)c_out, (__hip_bfloat16*)gates_act, batch, hdim,
        xg_stride, hout_stride, hprev_stride, prev_rows);
  } else {
    if (vec) {
      const int grid = grid_elems(batch * (hdim / v), block);
      lstm_pointwise_fwd_vec_kernel<float, 4><<<grid, block, 0, s>>>(
          (const float*)hg, (const float*)xg, (const float*)bias,
          (const float*)c_prev, (const float*)h_prev, mask, (float*)h_out,
          (float*)c_out, (float*)gates_act, batch, hdim, xg_stride,
          hout_stride, hprev_stride, prev_rows);
      return;
    }
    const int grid = grid_elems(batch * hdim, block);
    lstm_pointwise_fwd_kernel<float><<<grid, block, 0, s>>>(
        (const float*)hg, (const float*)xg, (const float*)bias,
        (const float*)c_prev, (const float*)h_prev, mask, (float*)h_out,
        (float*)c_out, (float*)gates_act, batch, hdim, xg_stride, hout_stride,
        hprev_stride, prev_rows);
  }
}

// Vectorised backward launch.  With a bias slab (accum != nullptr,
// accum_rows = P >= 1) the accumulating instantiation runs on
// min(P, blocks needed) blocks — block p owns slab row p, rows beyond the
// grid are not touched.
template <typename T, int V>
static void launch_bwd_vec(const void* grad_h, const void* grad_out_t,
                           const void* grad_c, const void* gates_act,
                           const void* c_prev, const float* mask,
                           void* grad_gates, void* grad_c_prev,
                           void* grad_h_pass, float* accum, long accum_rows,
                           long batch, int hdim, long gout_stride,
                           long gg_stride, long in_rows, long prev_rows,
                           hipStream_t s) {
  const int block = 256;  // the accumulating kernel relies on 256
  const int hv = hdim / V;
  if (accum != nullptr) {
    long blocks = (batch * hv + block - 1) / block;
    if (blocks < 1) blocks = 1;
    const int grid = (int)(blocks < accum_rows ? blocks : accum_rows);
    // one [4H] partial per wave (hv < 64) or per 256/hv thread group
    const int nrep = hv >= NERRF_WAVE ? block / hv : block / NERRF_WAVE;
    const size_t lds = (size_t)nrep * 4 * hdim * sizeof(float);
    lstm_pointwise_bwd_vec_kernel<T, V, true><<<grid, block, lds, s>>>(
        (const T*)grad_h, (const T*)grad_out_t, (const T*)grad_c,
        (const T*)gates_act, (const T*)c_prev, mask, (T*)grad_gates,
        (T*)grad_c_prev, (T*)grad_h_pass, accum, batch, hdim, gout_stride,
        gg_stride, in_rows, prev_rows);
    return;
  }
  const int grid = grid_elems(batch * hv, block);
  lstm_pointwise_bwd_vec_kernel<T, V, false><<<grid, block, 0, s>>>(
      (const T*)grad_h, (const T*)grad_out_t, (const T*)grad_c,
      (const T*)gates_act, (const T*)c_prev, mask, (T*)grad_gates,
      (T*)grad_c_prev, (T*)grad_h_pass, nullptr, batch, hdim, gout_stride,
      gg_stride, in_rows, prev_rows);
}

// Returns true when the bias-gradient partial was folded into bias_accum
// ([accum_rows, 4H] f32).  That needs the vectorised path and
// 256 % (hdim/V) == 0; otherwise the plain kernel runs and the slab is left
// untouched (the caller then reduces grad_gates itself).
bool launch_lstm_pointwise_bwd(const void* grad_h, const void* grad_out_t,
                               const void* grad_c, const void* gates_act,
                               const void* c_prev, const float* mask,
                               void* grad_gates, void* grad_c_prev,
                               void* grad_h_pass, float* bias_accum,
                               long accum_rows, long batch, int hdim,
                               long gout_stride, long gg_stride, long in_rows,
                               long prev_rows, bool bf16, hipStream_t s) {
  if (batch <= 0) return false;
  const int block = 256;
  const int v = bf16 ? 8 : 4;
  const bool vec = hdim % v == 0 && gout_stride % v == 0 && gg_stride % v == 0;
  const bool acc = vec && bias_accum != nullptr && accum_rows >= 1 &&
                   block % (hdim / v) == 0;
  float* accum = acc ? bias_accum : nullptr;
  if (bf16) {
    if (vec) {
      launch_bwd_vec<__hip_bfloat16, 8>(
          grad_h, grad_out_t, grad_c, gates_act, c_prev, mask, grad_gates,
          grad_c_prev, grad_h_pass, accum, accum_rows, batch, hdim,
          gout_stride, gg_stride, in_rows, prev_rows, s);
      return acc;
    }
    const int grid = grid_elems(batch * hdim, block);
    lstm_pointwise_bwd_kernel<__hip_bfloat16><<<grid, block, 0, s>>>(
        (const __hip_bfloat16*)grad_h, (const __hip_bfloat16*)grad_out_t,
        (const __hip_bfloat16*)grad_c, (const __hip_bfloat16*)gates_act,
        (const __hip_bfloat16*)c_prev, mask, (__hip_bfloat16*)grad_gates,
        (__hip_bfloat16*)grad_c_prev, (__hip_bfloat16*)grad_h_pass, batch, hdim,
        gout_stride, gg_stride, in_rows, prev_rows);
  } else {
    if (vec) {
      launch_bwd_vec<float, 4>(
          grad_h, grad_out_t, grad_c, gates_act, c_prev, mask, grad_gates,
          grad_c_prev, grad_h_pass, accum, accum_rows, batch, hdim,
          gout_stride, gg_stride, in_rows, prev_rows, s);
      return acc;
    }
    const int grid = grid_elems(batch * hdim, block);
    lstm_pointwise_bwd_kernel<float><<<grid, block, 0, s>>>(
        (const float*)grad_h, (const float*)grad_out_t, (const float*)grad_c,
        (const float*)gates_act, (const float*)c_prev, mask, (float*)grad_gates,
        (float*)grad_c_prev, (float*)grad_h_pass, batch, hdim, gout_stride,
        gg_stride, in_rows, prev_rows);
  }
  return false;
}

}  // namespace nerrf
