// Packed-inference LSTM recurrent step — CDNA4 (gfx950), bf16, H = 256 only.
//
// Forward-only fused step over the length-sorted packed layout of `SeqPlan`
// (ops/lstm_seq.py): sorted row r is live at step t iff r < n_t, and slab t
// of the packed [N, 2H] layer output sits at rows [off_t, off_t + n_t).
// Geometry is that of lstm_rec_fwd_kernel (lstm_rec_fused.hip): 512 threads,
// BM = 64 rows per block, wave w owns hidden units [32w, 32w + 32) for all
// four gates, v_mfma_f32_16x16x32_bf16 with the sage_fused.hip fragment maps
// (A row = l&15, B out-col = l&15, k-chunk (l>>4)*8; C/D row = (l>>4)*4+r,
// col = l&15), swizzled h tile in LDS, gate-major accumulators dumped to LDS
// and a 16-byte row-major pointwise phase.  What differs:
//
//   row counts, no mask   `rows` live rows this step, `prev_rows` (k) of them
//       have a previous state.  Rows >= k start from zero: neither their
//       h_prev nor their c is ever loaded, so stale or NaN memory there
//       cannot reach the output.  A block whose first row is >= k skips the
//       h-tile staging and the whole h @ W_hh^T MFMA phase (the newly live
//       tail rows of the reverse direction); a block that straddles k
//       zero-fills the tile rows past k.
//   in-place cell state   one [n_0, 256] c buffer per direction, read and
//       written by the same thread at the same 8-element chunk.  h_prev is
//       the previous step's slab of the layer output, h_out this step's; no
//       c history and no activated gates are stored.
//   XPROJ (layer 1)       no xg slab exists: x_t @ W_ih^T (K = 16, zero-
//       padded to the MFMA's 32) is one more k-step into the same f32
//       accumulators.  LDS is at the 160 KiB cap, so the x A-fragments go
//       from global memory straight into registers — lane l holds
//       feats[perm[row0 + rf*16 + (l&15)], t, (l>>4)*8 ..] for l>>4 < 2 and
//       zero otherwise — and stay there across the four gates (16 VGPRs).
//       W_ih fragments stream from L2 like W_hh.  Rows >= rows never
//       dereference perm.
//   XPROJ = false (layer 2)   xg rows come from a strided slab of the packed
//       [N, 2*4H] projection, as in lstm_rec_fwd_kernel.
//
// The host loop (`launch_lstm_packed_dir`) issues one launch per live
// timestep of a direction on one stream: one extension call per direction
// per layer instead of one per step.
//
// Packed f32 VALU ops (v_pk_{add,mul,fma}_f32) are kept out of this file's
// device code.  The attribute has to cover the header inlines as well — a
// callee compiled with the feature does not inline into a caller without
// it — so the push precedes the includes, and the kernel reads its block and
// thread ids through the builtins, not the device-library accessors.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "common.h"

namespace nerrf {

typedef __bf16 pbf16x8 __attribute__((ext_vector_type(8)));
typedef float pf32x4 __attribute__((ext_vector_type(4)));

#define PK_H 256
#define PK_BM 64
#define PK_HROW_B 512   // h tile row bytes (256 * 2)
#define PK_GROW_B 2048  // gate tile row bytes (1024 * 2)
#define PK_E 16         // XPROJ input features

// XOR swizzle for conflict-free ds_read_b128 column-slice reads
__device__ __forceinline__ unsigned pk_swz(unsigned row_byte0, unsigned row,
                                           unsigned byte_col) {
  return row_byte0 + (byte_col ^ ((row & 15u) << 4));
}

template <bool XPROJ>
__launch_bounds__(512)
__global__ void lstm_rec_packed_kernel(
    const __hip_bfloat16* __restrict__ h_prev,  // [k (h_stride), 256] prev slab
    const __hip_bfloat16* __restrict__ w_hh,    // [1024, 256] (out, in)
    const __hip_bfloat16* __restrict__ xg,      // [rows (xg_stride), 1024]; !XPROJ
    const __hip_bfloat16* __restrict__ bias,    // [1024]
    __hip_bfloat16* __restrict__ c,             // [n_0, 256], in place
    __hip_bfloat16* __restrict__ h_out,         // [rows (h_stride), 256] this slab
    const __hip_bfloat16* __restrict__ feats,   // [n_seq, t_max, 16]; XPROJ
    const int* __restrict__ perm,               // [>= rows] sorted row -> sequence
    const __hip_bfloat16* __restrict__ w_ih,    // [1024, 16]; XPROJ
    int t, int t_max, int n_seq, int rows, int prev_rows, long h_stride,
    long xg_stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* h_lds = smem;                         // 32 KB, swizzled
  char* gpre_lds = smem + PK_BM * PK_HROW_B;  // 128 KB, linear bf16

  const int row0 = (int)__builtin_amdgcn_workgroup_id_x() * PK_BM;
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int wave = tid / NERRF_WAVE;
  const int lane = tid % NERRF_WAVE;
  const int j0 = wave * 32;  // this wave's hidden-unit slice
  // block-uniform: does any row of this block have a previous state?
  const bool has_prev = row0 < prev_rows;
  // without a recurrent term and without an x k-step the pre-activations
  // are identically zero: the MFMA phase and the LDS round trip drop out
  const bool has_pre = XPROJ || has_prev;

  // ---- stage h tile: 64 rows x 512 B, swizzled; rows >= k zero-filled ----
  if (has_prev) {
    const int r = tid >> 3;              // 0..63
    const int c0 = tid & 7;              // interleaved: consecutive lanes
    const long grow = (long)(row0 + r);  // read consecutive 16-B chunks
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      const int chunk = c0 + cc * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (grow < prev_rows)
        v = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(h_prev + grow * h_stride) +
            chunk * 16);
      *reinterpret_cast<uint4*>(h_lds + pk_swz(r * PK_HROW_B, r, chunk * 16)) =
          v;
    }
  }

  const int frag_col = lane & 15;
  const int kq = lane >> 4;  // k-chunk index within a 32-wide k-step

  // ---- XPROJ: x A-fragments, global -> registers, held across the gates --
  pbf16x8 xfr[4];
  if constexpr (XPROJ) {
#pragma unroll
    for (int rf = 0; rf < 4; ++rf) {
      xfr[rf] = pbf16x8{};
      const int grow = row0 + rf * 16 + frag_col;
      if (kq < 2 && grow < rows) {
        const int seq = perm[grow];
        // perm's values cannot be checked on the host without a sync: a
        // bad index reads as a zero row, never as an address
        if ((unsigned)seq < (unsigned)n_seq)
          xfr[rf] = *reinterpret_cast<const pbf16x8*>(
              feats + ((long)seq * t_max + t) * PK_E + kq * 8);
      }
    }
  }
  if (has_prev) __syncthreads();

  // ---- MFMA phase, gate-major: one gate's accumulators (8 f32x4) live at
  // a time, dumped to LDS before the next gate (the all-gates-resident
  // variant spills; lstm_rec_fused.hip) ----------------------------------
  if (has_pre) {
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
      pf32x4 acc[4][2];
#pragma unroll
      for (int rf = 0; rf < 4; ++rf)
#pragma unroll
        for (int cf = 0; cf < 2; ++cf)
          acc[rf][cf] = pf32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (XPROJ) {
        // the x k-step: K = 16 in the low half of the 32-wide step; the
        // high half is zero on both operands
        pbf16x8 wfr[2];
#pragma unroll
        for (int cf = 0; cf < 2; ++cf) {
          const int orow = g * PK_H + j0 + cf * 16 + frag_col;
          wfr[cf] = pbf16x8{};
          if (kq < 2)
            wfr[cf] = *reinterpret_cast<const pbf16x8*>(
                w_ih + (long)orow * PK_E + kq * 8);
        }
#pragma unroll
        for (int rf = 0; rf < 4; ++rf)
#pragma unroll
          for (int cf = 0; cf < 2; ++cf)
            acc[rf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xfr[rf], wfr[cf], acc[rf][cf], 0, 0, 0);
      }
      if (has_prev) {
#pragma unroll
        for (int ks = 0; ks < PK_H / 32; ++ks) {
          // B fragments from L2 (w_hh is 0.5 MB, shared by every block)
          pbf16x8 bfr[2];
#pragma unroll
          for (int cf = 0; cf < 2; ++cf) {
            const int orow = g * PK_H + j0 + cf * 16 + frag_col;
            bfr[cf] = *reinterpret_cast<const pbf16x8*>(
                w_hh + (long)orow * PK_H + ks * 32 + kq * 8);
          }
#pragma unroll
          for (int rf = 0; rf < 4; ++rf) {
            const int arow = rf * 16 + frag_col;
            const pbf16x8 afr = *reinterpret_cast<const pbf16x8*>(
                h_lds + pk_swz(arow * PK_HROW_B, arow, ks * 64 + kq * 16));
#pragma unroll
            for (int cf = 0; cf < 2; ++cf)
              acc[rf][cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  afr, bfr[cf], acc[rf][cf], 0, 0, 0);
          }
        }
      }
      // dump this gate's pre-activations to LDS (bf16) so the pointwise
      // phase does 16-B row-major global I/O
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) {
        const int j = j0 + cf * 16 + frag_col;
#pragma unroll
        for (int rf = 0; rf < 4; ++rf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = rf * 16 + kq * 4 + r;
            *reinterpret_cast<__hip_bfloat16*>(
                gpre_lds + row * PK_GROW_B + (g * PK_H + j) * 2) =
                __float2bfloat16(acc[rf][cf][r]);
          }
      }
    }
    __syncthreads();
  }

  // ---- pointwise phase: thread -> (row, 8-col chunk); all global traffic
  // 16-B and row-contiguous.  unroll 1: a 4x unroll spills ----------------
#pragma unroll 1
  for (int p = 0; p < 4; ++p) {
    const int row = p * 16 + (tid >> 5);  // 0..63
    const int ch = (tid & 31) * 8;        // hidden-unit chunk base (8 els)
    const long grow = (long)(row0 + row);
    if (grow >= rows) continue;
    pbf16x8 p_i{}, p_f{}, p_g{}, p_o{};
    if (has_pre) {
      const char* pre_p = gpre_lds + row * PK_GROW_B;
      p_i = *reinterpret_cast<const pbf16x8*>(pre_p + ch * 2);
      p_f = *reinterpret_cast<const pbf16x8*>(pre_p + (PK_H + ch) * 2);
      p_g = *reinterpret_cast<const pbf16x8*>(pre_p + (2 * PK_H + ch) * 2);
      p_o = *reinterpret_cast<const pbf16x8*>(pre_p + (3 * PK_H + ch) * 2);
    }
    pbf16x8 x_i{}, x_f{}, x_g{}, x_o{};
    if constexpr (!XPROJ) {
      const __hip_bfloat16* xrow = xg + grow * xg_stride;
      x_i = *reinterpret_cast<const pbf16x8*>(xrow + ch);
      x_f = *reinterpret_cast<const pbf16x8*>(xrow + PK_H + ch);
      x_g = *reinterpret_cast<const pbf16x8*>(xrow + 2 * PK_H + ch);
      x_o = *reinterpret_cast<const pbf16x8*>(xrow + 3 * PK_H + ch);
    }
    const pbf16x8 b_i = *reinterpret_cast<const pbf16x8*>(bias + ch);
    const pbf16x8 b_f = *reinterpret_cast<const pbf16x8*>(bias + PK_H + ch);
    const pbf16x8 b_g = *reinterpret_cast<const pbf16x8*>(bias + 2 * PK_H + ch);
    const pbf16x8 b_o = *reinterpret_cast<const pbf16x8*>(bias + 3 * PK_H + ch);
    __hip_bfloat16* c_p = c + grow * PK_H + ch;
    pbf16x8 cp_v{};
    if (grow < prev_rows) cp_v = *reinterpret_cast<const pbf16x8*>(c_p);
    pbf16x8 ho_v, co_v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float i = sigmoidf_(__bfloat162float(p_i[e]) +
                                __bfloat162float(x_i[e]) +
                                __bfloat162float(b_i[e]));
      const float f = sigmoidf_(__bfloat162float(p_f[e]) +
                                __bfloat162float(x_f[e]) +
                                __bfloat162float(b_f[e]));
      const float g = tanhf(__bfloat162float(p_g[e]) +
                            __bfloat162float(x_g[e]) +
                            __bfloat162float(b_g[e]));
      const float o = sigmoidf_(__bfloat162float(p_o[e]) +
                                __bfloat162float(x_o[e]) +
                                __bfloat162float(b_o[e]));
      const float cn = f * __bfloat162float(cp_v[e]) + i * g;
      co_v[e] = (__bf16)cn;
      ho_v[e] = (__bf16)(o * tanhf(cn));
    }
    *reinterpret_cast<pbf16x8*>(c_p) = co_v;
    *reinterpret_cast<pbf16x8*>(h_out + grow * h_stride + ch) = ho_v;
  }
}

// ---------------------------------------------------------------------------
// host: one direction of one layer, all live timesteps on stream `s`
// ---------------------------------------------------------------------------

// h_dir: this direction's [N, 256] column slab of the packed layer output
// (row stride h_stride); xg_dir likewise of the projection, or nullptr with
// the XPROJ inputs (feats, perm, w_ih) set.  batch_sizes [t_live] is
// non-increasing and offsets [t_live + 1] its running sum (validated by the
// binding).  The (off, n, prev_off, k) arithmetic is `SeqPlan.steps`.
void launch_lstm_packed_dir(void* h_dir, const void* w_hh, const void* xg_dir,
                            const void* bias, void* c, const void* feats,
                            const int* perm, const void* w_ih, int t_max,
                            int n_seq, const long* batch_sizes,
                            const long* offsets, int t_live, bool reverse,
                            long h_stride, long xg_stride, hipStream_t s) {
  const size_t lds = PK_BM * (PK_HROW_B + PK_GROW_B);  // 160 KB
  auto* h = static_cast<__hip_bfloat16*>(h_dir);
  const auto* xg = static_cast<const __hip_bfloat16*>(xg_dir);
  const bool xproj = xg == nullptr;
  for (int i = 0; i < t_live; ++i) {
    const int t = reverse ? t_live - 1 - i : i;
    const long off = offsets[t];
    const int n = (int)batch_sizes[t];
    if (n == 0) continue;
    long prev_off = 0;
    int k = 0;
    if (reverse) {
      prev_off = offsets[t + 1];
      k = t + 1 < t_live ? (int)batch_sizes[t + 1] : 0;
    } else if (t > 0) {
      prev_off = offsets[t - 1];
      k = n;
    }
    const int grid = (n + PK_BM - 1) / PK_BM;
    const __hip_bfloat16* h_prev = h + prev_off * h_stride;
    __hip_bfloat16* h_out = h + off * h_stride;
    if (xproj)
      lstm_rec_packed_kernel<true><<<grid, 512, lds, s>>>(
          h_prev, (const __hip_bfloat16*)w_hh, nullptr,
          (const __hip_bfloat16*)bias, (__hip_bfloat16*)c, h_out,
          (const __hip_bfloat16*)feats, perm, (const __hip_bfloat16*)w_ih, t,
          t_max, n_seq, n, k, h_stride, 0);
    else
      lstm_rec_packed_kernel<false><<<grid, 512, lds, s>>>(
          h_prev, (const __hip_bfloat16*)w_hh, xg + off * xg_stride,
          (const __hip_bfloat16*)bias, (__hip_bfloat16*)c, h_out, nullptr,
          nullptr, nullptr, t, t_max, n_seq, n, k, h_stride, xg_stride);
  }
}

}  // namespace nerrf

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
