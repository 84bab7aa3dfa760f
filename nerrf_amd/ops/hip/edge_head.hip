// Fused GraphSAGE-T edge head forward — CDNA4 (gfx950), hidden = 128,
// edge_head_hidden = 64, bf16, inference only.
//
// One launch scores the whole edge list.  For edge e with s = src[e],
// d = dst[e]:
//   f     = [ h[s]*h[d] (128), |h[s]-h[d]| (128), ew[e], ets[e] ]     (258)
//   z     = GELU_erf(W1 f + b1)                                       (64)
//   logit = W2 . z + b2                                               (fp32)
// — the edge branch of models/graphsage.GraphSAGET.forward (eager: two
// [E,128] gathers, mul, sub, abs, a [E,258] cat, two GEMMs and a GELU) with
// no [E, *] intermediate in HBM.
//
// Geometry: 4 waves (256 threads), 64-edge tile per block, grid-stride loop
// over tiles so W1[:, :256] is staged into LDS once per block.  Wave w builds
// feature rows [w*16, +16) and owns those rows x all 64 hidden columns of the
// GEMM: 4 accumulators of v_mfma_f32_16x16x32_bf16, 8 k-steps over K = 256.
//
// LDS (64 KB): W1 main block [64 x 256] bf16 and the feature tile [64 x 256]
// bf16, both with the ((row&15)<<4) XOR swizzle on 16-byte chunks of
// sage_fused.hip.  The two tail columns of W1 (ew, ets), b1, W2 and b2 enter
// the fp32 epilogue from registers.
//
// Fragment maps: as sage_fused.hip (A row=l&15 / B col=l&15, k-chunk
// (l>>4)*8; C/D row=(l>>4)*4+r, col=l&15).  Numerics: product and absolute
// difference formed in fp32 and rounded once to bf16, fp32 accumulation,
// erf-exact GELU, fp32 second layer.  src/dst outside [0, N) are a contract
// violation the kernel does not check.
#include "common.h"

namespace nerrf {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define EH_D 128            // node embedding width
#define EH_K (2 * EH_D)     // MFMA reduction length (product | abs-diff)
#define EH_BM 64            // edges per tile
#define EH_HID 64           // edge_head_hidden
#define EH_ROW_B (EH_K * 2) // 512 B per LDS row

__device__ __forceinline__ unsigned eh_swz(unsigned row, unsigned byte_col) {
  return row * EH_ROW_B + (byte_col ^ ((row & 15u) << 4));
}

__device__ __forceinline__ float eh_bf16_lo(unsigned v) {
  return __uint_as_float(v << 16);
}
__device__ __forceinline__ float eh_bf16_hi(unsigned v) {
  return __uint_as_float(v & 0xffff0000u);
}
__device__ __forceinline__ unsigned eh_pack_bf16(float a, float b) {
  __hip_bfloat16 b0 = __float2bfloat16(a);
  __hip_bfloat16 b1 = __float2bfloat16(b);
  return (unsigned)*reinterpret_cast<const unsigned short*>(&b0) |
         ((unsigned)*reinterpret_cast<const unsigned short*>(&b1) << 16);
}

__launch_bounds__(256)
__global__ void edge_head_fwd_kernel(
    const __hip_bfloat16* __restrict__ h,        // [N, 128]
    const long* __restrict__ src,                // [E]
    const long* __restrict__ dst,                // [E]
    const float* __restrict__ ew,                // [E]
    const float* __restrict__ ets,               // [E]
    const __hip_bfloat16* __restrict__ w1_main,  // [64, 256] = W1[:, :256]
    const float* __restrict__ w1_tail,           // [64, 2]   = W1[:, 256:258]
    const __hip_bfloat16* __restrict__ b1,       // [64]
    const __hip_bfloat16* __restrict__ w2,       // [64]
    const __hip_bfloat16* __restrict__ b2,       // [1]
    float* __restrict__ out,                     // [E]
    long n_edges, long n_tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* w_lds = smem;                        // 32 KB (swizzled)
  char* f_lds = smem + EH_HID * EH_ROW_B;    // 32 KB (swizzled)

  const int tid = threadIdx.x;
  const int wave = tid / NERRF_WAVE;
  const int lane = tid % NERRF_WAVE;

  // ---- stage W1[:, :256] (64 rows x 512 B = 2048 16-B chunks), once -------
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int chunk = tid + 256 * j;  // 0..2047, coalesced
    const int wr = chunk >> 5;        // 32 chunks per row
    const int wc = (chunk & 31) * 16;
    *reinterpret_cast<uint4*>(w_lds + eh_swz(wr, wc)) =
        *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(w1_main) + wr * EH_ROW_B + wc);
  }

  // ---- epilogue constants of this lane's 4 hidden columns (fp32) ----------
  float c_b1[4], c_t0[4], c_t1[4], c_w2[4];
#pragma unroll
  for (int cf = 0; cf < 4; ++cf) {
    const int col = cf * 16 + (lane & 15);
    c_b1[cf] = __bfloat162float(b1[col]);
    c_t0[cf] = w1_tail[2 * col];
    c_t1[cf] = w1_tail[2 * col + 1];
    c_w2[cf] = __bfloat162float(w2[col]);
  }
  const float c_b2 = __bfloat162float(b2[0]);

  const int row_grp = wave * 16;  // this wave's 16 rows of the tile
  const int arow = row_grp + (lane & 15);
  const int kbyte = (lane >> 4) * 16;

  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long e0 = tile * EH_BM + row_grp;  // first edge of this wave's rows

    // ---- feature tile: wave w -> rows w*16..+16; lane -> column pair ------
    // lanes 0..15 fetch the 16 endpoint pairs, broadcast by shuffle below
    long s_lane = 0, d_lane = 0;
    if (lane < 16 && e0 + lane < n_edges) {
      s_lane = src[e0 + lane];
      d_lane = dst[e0 + lane];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long s = __shfl(s_lane, r, NERRF_WAVE);
      const long d = __shfl(d_lane, r, NERRF_WAVE);
      unsigned prod = 0u, adiff = 0u;
      if (e0 + r < n_edges) {  // wave-uniform
        const unsigned vs = reinterpret_cast<const unsigned*>(h + s * EH_D)[lane];
        const unsigned vd = reinterpret_cast<const unsigned*>(h + d * EH_D)[lane];
        const float s0 = eh_bf16_lo(vs), s1 = eh_bf16_hi(vs);
        const float d0 = eh_bf16_lo(vd), d1 = eh_bf16_hi(vd);
        prod = eh_pack_bf16(s0 * d0, s1 * d1);
        adiff = eh_pack_bf16(fabsf(s0 - d0), fabsf(s1 - d1));
      }
      *reinterpret_cast<unsigned*>(f_lds + eh_swz(row_grp + r, lane * 4)) = prod;
      *reinterpret_cast<unsigned*>(
          f_lds + eh_swz(row_grp + r, EH_D * 2 + lane * 4)) = adiff;
    }

    // per-row scalars of this lane's 4 C/D rows (loads overlap the MFMAs)
    float r_ew[4], r_ets[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long e = e0 + (lane >> 4) * 4 + r;
      r_ew[r] = (e < n_edges) ? ew[e] : 0.0f;
      r_ets[r] = (e < n_edges) ? ets[e] : 0.0f;
    }
    __syncthreads();  // feature tile (and, first time round, W1) visible

    // ---- MFMA: z[16 x 64] = f[16 x 256] @ W1_main^T -----------------------
    f32x4 acc[4];
#pragma unroll
    for (int cf = 0; cf < 4; ++cf) acc[cf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < EH_K / 32; ++ks) {
      const unsigned koff = ks * 64 + kbyte;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(f_lds + eh_swz(arow, koff));
#pragma unroll
      for (int cf = 0; cf < 4; ++cf) {
        const int o = cf * 16 + (lane & 15);
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(w_lds + eh_swz(o, koff));
        acc[cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[cf], 0, 0, 0);
      }
    }

    // ---- epilogue (fp32): tail columns, bias, GELU, W2 dot, row reduce ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float part = 0.0f;
#pragma unroll
      for (int cf = 0; cf < 4; ++cf) {
        const float zv = acc[cf][r] + c_b1[cf] + r_ew[r] * c_t0[cf] + r_ets[r] * c_t1[cf];
        const float gelu = 0.5f * zv * (1.0f + erff(zv * 0.70710678118654752f));
        part = fmaf(gelu, c_w2[cf], part);
      }
      // sum over the 16 lanes that share l>>4 (the 64 hidden columns)
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) part += __shfl_xor(part, off, NERRF_WAVE);
      const long e = e0 + (lane >> 4) * 4 + r;
      if ((lane & 15) == 0 && e < n_edges) out[e] = part + c_b2;
    }
    __syncthreads();  // tile consumed before the next one overwrites it
  }
}

void launch_edge_head_fwd(const void* h, const long* src, const long* dst,
                          const float* ew, const float* ets,
                          const void* w1_main, const float* w1_tail,
                          const void* b1, const void* w2, const void* b2,
                          float* out, long n_edges, hipStream_t s) {
  if (n_edges <= 0) return;  // a zero grid is a launch error
  const long n_tiles = (n_edges + EH_BM - 1) / EH_BM;
  const int grid = (int)(n_tiles < 8192 ? n_tiles : 8192);
  const size_t lds = (EH_HID + EH_BM) * EH_ROW_B;  // 64 KB
  edge_head_fwd_kernel<<<grid, 256, lds, s>>>(
      (const __hip_bfloat16*)h, src, dst, ew, ets,
      (const __hip_bfloat16*)w1_main, w1_tail, (const __hip_bfloat16*)b1,
      (const __hip_bfloat16*)w2, (const __hip_bfloat16*)b2, out, n_edges,
      n_tiles);
}

}  // namespace nerrf
