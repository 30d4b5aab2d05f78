// Scaffolding shared by the per-rollout line-fill kernels (gram.hip, qr.hip, qr_wide.hip): the
// rounding-sensitive helpers, the removal-bitmap tests, the line's action-id load, the M staging
// and the fixed-order per-sample block sums.  Each helper is the one copy of operations the
// kernels used to repeat in the same order; what differs between kernels on purpose (how the
// bitmap words are prefetched, what is held in registers across the samples) stays in the kernels.
#pragma once
#include "spai_device.h"
#include "spai_status.h"

namespace spai {

// 1/x to ~1 ulp: hardware reciprocal + one Newton step (x finite, non-zero, normal).
__device__ __forceinline__ double rcp_newton(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  const double e = fma(-x, r, 1.0);
  return fma(r, e, r);
}

// 1/sqrt(t) to ~1 ulp: hardware reciprocal square root + one Newton step (t > 0, normal).
__device__ __forceinline__ double rsq_newton(double t) {
  const double r = __builtin_amdgcn_rsq(t);
  const double e = fma(-t * r, r, 1.0);  // 1 - t r^2
  return fma(0.5 * r, e, r);
}

// Sum over the L lanes of a group (L = 4, 8, 16, 32 consecutive lanes), valid on every lane of
// the group with identical bits (each step adds a commutative pair).
template <int L>
__device__ __forceinline__ double group_sum(double v) {
  v += dpp_d<0xB1, 0xf>(v);  // quad_perm [1, 0, 3, 2]
  v += dpp_d<0x4E, 0xf>(v);  // quad_perm [2, 3, 0, 1]
  if constexpr (L >= 8) v += dpp_d<0x141, 0xf>(v);  // row_half_mirror: quad 0 <-> quad 1
  if constexpr (L >= 16) v += dpp_d<0x140, 0xf>(v);  // row_mirror: half-row 0 <-> 1
  if constexpr (L >= 32) v += __shfl_xor(v, 16, kWave);
  static_assert(L == 4 || L == 8 || L == 16 || L == 32, "group size");
  return v;
}

// A slot's removal bit: action id act (-1: no slot) is bit act % 32 of bitmap word act / 32; a
// sample's row holds the words from word_base on.  slot_word is the row-relative word (0 for an
// empty slot: any in-bounds word, masked by slot_kept), slot_kept whether the slot stays in M.
__device__ __forceinline__ int slot_word(int act, int32_t word_base) { return act >= 0 ? (act >> 5) - word_base : 0; }
__device__ __forceinline__ bool slot_kept(int act, uint32_t word) { return (act >= 0) & !((word >> (act & 31)) & 1u); }

// The W action ids of line jj (clamped by the caller: in bounds), -1 past the runtime width wrt
// or on an invalid line.  Every load is issued before any is used (no branch per slot).
template <int W>
__device__ __forceinline__ void load_line_acts(const int32_t* pat_act, int jj, int32_t wrt, bool valid,
                                               int (&act)[W]) {
  int av[W];
#pragma unroll
  for (int p = 0; p < W; ++p) av[p] = pat_act[(int64_t)jj * wrt + min(p, wrt - 1)];
#pragma unroll
  for (int p = 0; p < W; ++p) act[p] = (valid && p < wrt) ? av[p] : -1;
}

// M of sample b for a block of 256 lines (one thread per line, block lb of a shard of nloc lines,
// nvl of them valid; lane, wave: the thread's), staged per WAVE: its 64 lines are one contiguous run of M, so no block
// barrier per sample (a wave's LDS operations complete in order).  s_m: 256 * W values.  No
// branch on m_out: store_m_block drops every store when it is null.
template <int W, typename TM>
__device__ __forceinline__ void stage_m_wave(TM* s_m, const double (&mv)[W], bool valid, int lane, int wave,
                                             int32_t wrt, int nvl, TM* m_out, int b, int64_t nloc, int lb) {
  const int wv = __builtin_amdgcn_readfirstlane(wave);  // wave-uniform: scalar offsets
  TM* sm = s_m + wv * 64 * W;
  if (valid) {
#pragma unroll
    for (int p = 0; p < W; ++p)
      if (p < wrt) sm[lane * wrt + p] = (TM)mv[p];
  }
  __builtin_amdgcn_wave_barrier();
  const int nw = min(max(nvl - wv * 64, 0), 64);
  store_m_block<64, W, TM>(m_out ? m_out + ((int64_t)b * nloc + (int64_t)lb * 256 + wv * 64) * wrt : nullptr, sm,
                           nw * wrt, lane);
  __builtin_amdgcn_wave_barrier();
}

// The same per BLOCK of NT lines through two LDS buffers (sample b writes buffer b & 1 while
// sample b - 1's stores may still read the other): one block barrier per sample.  For the QR
// solves, where the per-wave form costs registers (6 VGPRs spilled at 128, 0.127 vs 0.106 ms at
// C4; the Gram fills gain from it).
// mv: the line's W values, in fp64 or already in M's type.
template <int NT, int W, typename TM, typename TV>
__device__ __forceinline__ void stage_m_block(TM (&s_m)[2][NT * W], const TV* mv /* [W] */, bool valid, int32_t wrt,
                                              int nvl, TM* m_out, int b, int64_t nloc, int lb) {
  const int t = threadIdx.x;
  TM* sm = s_m[b & 1];
  if (valid) {
#pragma unroll
    for (int p = 0; p < W; ++p)
      if (p < wrt) sm[t * wrt + p] = (TM)mv[p];
  }
  __syncthreads();
  store_m_block<NT, W, TM>(m_out ? m_out + ((int64_t)b * nloc + (int64_t)lb * NT) * wrt : nullptr, sm, nvl * wrt);
}

// The fixed-order per-sample block sums of a chunk of nb samples whose first is c0: s_r2[u][t] is
// line t's squared residual for sample c0 + u (0 on an invalid line); wave u % (NT / 64) adds the
// NT / 64 wave columns in order, then the lanes by butterfly (wave_sum), between two barriers.
// THE CONTRACT spai_fill_reduce and the shard tests rely on: partials[sample][block] with 256
// consecutive lines per block, each partial a function of its block's lines alone, so shards
// aligned to 256 lines (distributed.LINE_ALIGN) reproduce one launch's bits on any number of GPUs.
template <int NT, int C>
__device__ __forceinline__ void chunk_block_sums(const double (&s_r2)[C][NT], int lane, int wave, int nb, int c0,
                                                 double* partials, int lb) {
  static_assert(NT == 256, "one block = 256 lines (LINE_ALIGN)");
  __syncthreads();
  for (int u = wave; u < nb; u += NT / 64) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) acc += s_r2[u][q * 64 + lane];
    acc = wave_sum(acc);
    if (lane == 0) partials[(int64_t)(c0 + u) * gridDim.x + lb] = acc;
  }
  __syncthreads();
}

// Host side: the preamble every spai_fill_lines_* entry point opens with, under the entry
// point's own name (the messages are part of the ABI's behaviour).  extra_shape_ok / inputs_ok:
// the entry point's further shape terms and its non-null inputs.  SPAI_OK with *nparts = the
// shard's 256-line blocks, 0 for an empty shard (the entry point then returns SPAI_OK at once).
inline int check_fill_lines(const char* name, int32_t n, int32_t line_begin, int32_t line_end, int32_t W, int32_t B,
                            int32_t words, int32_t word_base, bool extra_shape_ok, int32_t m_dtype,
                            const void* workspace, size_t workspace_bytes, bool inputs_ok, int32_t* nparts) {
  *nparts = 0;
  SPAI_CHECK_ARG(m_dtype == SPAI_DTYPE_F32 || m_dtype == SPAI_DTYPE_F64, "%s: bad m_dtype", name);
  SPAI_CHECK_ARG(n >= 1 && line_begin >= 0 && line_end >= line_begin && line_end <= n && W >= 1 && B >= 1 &&
                     words >= 1 && word_base >= 0 && extra_shape_ok,
                 "%s: bad shape", name);
  SPAI_CHECK_ARG(workspace != nullptr, "%s: null workspace", name);
  if (line_end == line_begin) return SPAI_OK;
  SPAI_CHECK_ARG(inputs_ok, "%s: null input", name);
  *nparts = (line_end - line_begin + 255) / 256;
  SPAI_CHECK_ARG(workspace_bytes >= sizeof(double) * (size_t)*nparts * B, "%s: workspace too small", name);
  return SPAI_OK;
}

}  // namespace spai
