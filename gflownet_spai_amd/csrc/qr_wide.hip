// Least-squares fill of M by Householder QR for wide lines on gfx950: pattern widths W <= 32 over
// A-line widths WA <= 32 with row unions |I| <= 256 (qr.hip stops at 13 / 7 / 96).  The numerical
// recipe is qr.hip's (qr_factor_line + qr_masked_solve); the mapping is a wavefront per line
// instead of a lane per line, because a lane cannot hold a 32 x 32 block.
//
// Factor, once per env (k_qrw_factor): one workgroup per line, thread t = row t of the dense block
// D = A[I, slots] (32 values in registers).  One wave merges the slots' sorted A lines into the
// row list I (lane p owns the cursor of slot p; the next row is a wave minimum), every thread
// looks its row's entries up, then the full Householder QR runs with block reductions for the
// column norms and the reflection's dot products.  The line's record goes to the wide R cache,
// line-major: NQ = W (W + 1) / 2 + W + 1 doubles at rcache[l * NQ] = the packed upper triangle of
// R (row-major: row i at i W - i (i - 1) / 2, entries q = i .. W - 1), then (Q^T e_l)[0 .. W),
// then the tail ||(Q^T e_l)[W ..]||^2 (+ 1 when l is not in I).  W is the pattern's own width.
//
// Solve, per rollout (k_qrw_solve): one half-wave per (line, sample), two samples per wave.  Lane
// q = 1 .. W - 1 of the half holds column q of R in registers x[0 .. q] and lane 0 holds Q^T e
// (column 0 is one number: it takes no reflection and nothing ever updates it).  At column p the
// column is broadcast from lane p to the half-wave, which forms the reflection vector over
// {free rows < p} u {row p}, and every lane q > p (and lane 0) forms its own dot product and update: the same
// operations in the same order as qr_masked_solve, with every register index static.  The rank
// floor 1e-24 ||D[:, p]||^2 is recomputed in lane p (once per line) as 1e-24 sum_i R_ip^2 (Q is orthogonal), so
// the record needs no column norms.  The back-substitution is one half-wave sum per row.
//
// Per-sample partial sums: a block is 256 lines (LINE_ALIGN) on 4 waves, wave w taking lines
// w, w + 4, ...; each wave adds its lines' residuals in ascending order and the four wave sums
// are added in wave order, so a block's partial depends on its lines alone and 256-line-aligned
// shards reproduce one launch's bits (partials[b * nparts + block], as every other fill).
#include <climits>

#include "spai_device.h"
#include "spai_fill.h"
#include "spai_status.h"

namespace spai {
namespace {

constexpr int kWW = 32;         // widest pattern line and widest A line
constexpr int kWRows = 256;     // largest row union |I|
constexpr int kWLines = 256;    // lines per solve block (= distributed.LINE_ALIGN)
constexpr int kWNT = 256;       // threads per solve block
constexpr int kWChunk = 64;     // samples whose block sums are in LDS at once (= the wave: lane u zeroes sample u)

__host__ __device__ constexpr int qrw_nq(int W) { return W * (W + 1) / 2 + W + 1; }
__host__ __device__ constexpr int qrw_row(int i, int W) { return i * W - i * (i - 1) / 2; }  // offset of R[i][i]

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (int)__shfl_xor(v, o, kWave));
  return v;
}

// Row-union size per line for widths up to 32 (max over the lines -> *out): one wave per line, lane
// p < W holds the cursor of slot p's A line (left-packed, ascending), each step consumes the
// smallest row index on every cursor that shows it.
__global__ __launch_bounds__(256) void k_qrw_rows(int32_t n, int32_t wrt, const int32_t* __restrict__ pat_idx,
                                                  int32_t wart, const int32_t* __restrict__ a_idx,
                                                  int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= n) return;  // (whole waves)
  const int kp = lane < wrt ? pat_idx[(int64_t)l * wrt + lane] : -1;
  const int32_t* al = a_idx + (int64_t)max(kp, 0) * wart;
  int h = 0;
  auto next = [&]() {
    const int a = (kp >= 0 && h < wart) ? al[h] : -1;
    return a >= 0 ? a : INT_MAX;
  };
  int cur = next(), rows = 0;
  for (;;) {
    const int rmin = wave_min_i(cur);
    if (rmin == INT_MAX) break;
    if (cur == rmin) {
      ++h;
      cur = next();
    }
    ++rows;
  }
  if (lane == 0) atomicMax(out, rows);
}

// Sums of the values v[lo .. hi) over the NT threads of the block, valid on every thread with
// identical bits: butterfly wave sums, then the waves in order.  red: [NT / 64][NV] doubles of LDS.
template <int NT, int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV], int lo, int hi, double* red) {
  constexpr int NW = NT / 64;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (k >= lo && k < hi) v[k] = wave_sum(v[k]);
  if constexpr (NW > 1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // the previous sums were read
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NV; ++k)
        if (k >= lo && k < hi) red[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (k >= lo && k < hi) {
        double s = red[k];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w * NV + k];
        v[k] = s;
      }
  }
}

// Phase 1: the full Householder QR of line blockIdx.x's block on NT threads (NT = 64: row unions
// up to 64, one wave; NT = 256: up to 256), thread t = row t.
template <int NT>
__global__ __launch_bounds__(NT) void k_qrw_factor(int32_t n, int32_t wrt, const int32_t* __restrict__ pat_idx,
                                                   int32_t wart, const int32_t* __restrict__ a_idx,
                                                   const void* __restrict__ a_val, bool a32,
                                                   double* __restrict__ rcache) {
  __shared__ int sAi[kWW][kWW + 1];  // the slots' A lines (row index, -1: none), padded against bank conflicts
  __shared__ double sAv[kWW][kWW + 1];
  __shared__ int sI[NT];             // the row union, ascending
  __shared__ int sInfo[2];           // rows in I (-1: more than NT), 1 when l is in I
  __shared__ double sRed[(NT / 64) * (kWW + 1)];
  const int t = threadIdx.x, lane = t & 63;
  const int l = blockIdx.x;
  const int NQ = qrw_nq(wrt);
  double* rec = rcache + (int64_t)l * NQ;

  for (int e = t; e < kWW * kWW; e += NT) {
    const int p = e / kWW, s = e % kWW;
    const int kp = p < wrt ? pat_idx[(int64_t)l * wrt + p] : -1;
    const int a = (kp >= 0 && s < wart) ? a_idx[(int64_t)kp * wart + s] : -1;
    sAi[p][s] = a;
    const int64_t ea = (int64_t)kp * wart + s;
    sAv[p][s] = a < 0 ? 0.0 : (a32 ? (double)static_cast<const float*>(a_val)[ea] : static_cast<const double*>(a_val)[ea]);
  }
  if (t < 2) sInfo[t] = 0;
  __syncthreads();
  if (t < 64) {  // one wave merges the sorted A lines into the row list
    const int p = min(lane, kWW - 1);
    int h = 0;
    auto next = [&]() {
      const int a = (lane < kWW && h < wart) ? sAi[p][h] : -1;
      return a >= 0 ? a : INT_MAX;
    };
    int cur = next(), rho = 0;
    for (;;) {
      const int rmin = wave_min_i(cur);
      if (rmin == INT_MAX) break;
      if (rho == NT) {  // more rows than the instance holds (the caller's max_rows was wrong)
        rho = -1;
        break;
      }
      if (lane == 0) sI[rho] = rmin;
      if (cur == rmin) {
        ++h;
        cur = next();
      }
      ++rho;
    }
    if (lane == 0) sInfo[0] = rho;
  }
  __syncthreads();
  const int nrows = sInfo[0];
  const int r = (nrows >= 0 && t < nrows) ? sI[t] : -1;
  double d[kWW], rhs = r == l ? 1.0 : 0.0;
  if (r == l) sInfo[1] = 1;
#pragma unroll
  for (int p = 0; p < kWW; ++p) {  // row r's entry of slot p's A line: lower bound in the sorted line
    double x = 0.0;
    if (r >= 0 && p < wrt) {
      int lo = 0, hi = wart;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int a = sAi[p][mid];
        if ((a >= 0 ? a : INT_MAX) < r) lo = mid + 1;
        else hi = mid;
      }
      if (lo < wart && sAi[p][lo] == r) x = sAv[p][lo];
    }
    d[p] = x;
  }
  __syncthreads();  // sInfo[1]

  // reflection p maps column p onto row p (a column already zero from row p down: none)
#pragma unroll
  for (int p = 0; p < kWW; ++p) {
    if (p < wrt) {
      double sx[2] = {t >= p ? d[p] * d[p] : 0.0, t == p ? d[p] : 0.0};  // the column's norm^2 below row p, D[p][p]
      block_sums<NT, 2>(sx, 0, 2, sRed);
      const double sig = sx[0], xkk = sx[1];
      const double sq = sqrt(sig);
      const double alpha = xkk >= 0.0 ? -sq : sq;
      const double tau = sig > 0.0 ? rcp_newton(sig - alpha * xkk) : 0.0;  // H = I - tau v v^T
      const double v = t >= p ? d[p] - (t == p ? alpha : 0.0) : 0.0;
      double dot[kWW + 1];  // v . column q (q > p) at [q], v . rhs at [wrt]
#pragma unroll
      for (int q = 0; q <= kWW; ++q) dot[q] = (q > p && q <= wrt) ? v * (q < wrt ? d[min(q, kWW - 1)] : rhs) : 0.0;
      block_sums<NT, kWW + 1>(dot, p + 1, wrt + 1, sRed);
#pragma unroll
      for (int q = p + 1; q < kWW; ++q)
        if (q < wrt) d[q] = fma(-dot[q] * tau, v, d[q]);
      {
        double dr = 0.0;  // dot[wrt]: a static select, wrt is not a compile-time index
#pragma unroll
        for (int q = 1; q <= kWW; ++q) dr = q == wrt ? dot[q] : dr;
        rhs = fma(-dr * tau, v, rhs);
      }
      // row p of R and (Q^T e)_p are final now (later reflections act on rows > p)
      if (t == p) {
        const int base = qrw_row(p, wrt);
        rec[base] = sig > 0.0 ? alpha : d[p];
#pragma unroll
        for (int q = p + 1; q < kWW; ++q)
          if (q < wrt) rec[base + (q - p)] = d[q];
        rec[wrt * (wrt + 1) / 2 + p] = rhs;
      }
    }
  }
  double tl[1] = {t >= wrt ? rhs * rhs : 0.0};  // the tail of Q^T e: rows >= W
  block_sums<NT, 1>(tl, 0, 1, sRed);
  if (t == 0) rec[NQ - 1] = nrows < 0 ? __builtin_nan("") : tl[0] + (sInfo[1] ? 0.0 : 1.0);
}

// Phase 2 from the wide R cache: see the file header.  half = the sample of the pair, q = the slot.
template <typename TM>
__global__ __launch_bounds__(kWNT) __attribute__((amdgpu_waves_per_eu(2))) void k_qrw_solve(
    int32_t line_begin, int32_t line_end, int32_t wrt, const int32_t* __restrict__ pat_act,
    const double* __restrict__ rcache, int32_t B, const uint32_t* __restrict__ removed, int32_t words,
    int32_t word_base, TM* __restrict__ m_out, double* __restrict__ partials) {
  constexpr int NW = kWNT / 64;
  __shared__ double s_acc[NW][kWChunk];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, q = lane & 31;
  const int lb = blockIdx.x;
  const int64_t nloc = line_end - line_begin;
  const int blk0 = line_begin + lb * kWLines;
  const int NQ = qrw_nq(wrt), T = wrt * (wrt + 1) / 2;

#pragma unroll 1
  for (int b0 = 0; b0 < B; b0 += kWChunk) {
    const int nb = min(kWChunk, B - b0);
    s_acc[wave][lane] = 0.0;
    __syncthreads();
#pragma unroll 1
    for (int li = wave; li < kWLines; li += NW) {
      const int l = blk0 + li;
      if (l >= line_end) break;  // (wave-uniform)
      const double* rec = rcache + (int64_t)l * NQ;
      // lane q >= 1: column q of R, rows 0 .. q; lane 0: Q^T e (its x[0] is c_0).  Re-read per sample
      // (L1 / L2 hits) instead of held beside the working copy: 64 registers less
      // No per-lane load predicate (32 lane masks would spill the scalar registers): lane q reads
      // "row i, column q" of the packed triangle for every row i < W, which for i > q is the tail
      // of row i - 1, inside the record and finite, and nothing reads x[i > q] of a column lane:
      // lane p forms its reflection from x[0 .. p], the lanes q > p update x[0 .. p], the
      // back-substitution reads x[p] on lanes q > p.  Lanes q >= W read column W - 1 and, with
      // keep = false and m_q = 0, add exact zeros.  Rows i >= W are 0.0 on every lane.
      const int qbase = q == 0 ? T : min(q, wrt - 1);
      auto load_col = [&](const double* rp, double (&xc)[kWW]) {
#pragma unroll
        for (int i = 0; i < kWW; ++i) {
          xc[i] = 0.0;
          if (i < wrt) xc[i] = rp[qbase + (q == 0 ? i : qrw_row(i, wrt) - i)];
        }
      };
      const double r00 = rec[0], tail = rec[NQ - 1];
      double thr = 0.0;  // the rank floor of this lane's column: 1e-24 sum_i R_iq^2
      {
        double x0[kWW];
        load_col(rec, x0);
        double s = q == 0 ? r00 * r00 : 0.0;
#pragma unroll
        for (int i = 0; i < kWW; ++i) s = (q == 0 || i > q) ? s : fma(x0[i], x0[i], s);
        thr = 1e-24 * s;
      }
      const int act = q < wrt ? pat_act[(int64_t)l * wrt + q] : -1;
      const int wofs = slot_word(act, word_base);
#pragma unroll 1
      for (int s0 = 0; s0 < nb; s0 += 2) {
        const int sl = min(s0 + half, nb - 1);  // an odd last pair: both halves solve the last sample
        const bool own = s0 + half < nb;
        const int b = b0 + sl;
        // (slot_kept written out: the bitmap load stays under the act >= 0 test, as the registers were tuned)
        const bool keep = act >= 0 && !((removed[(int64_t)b * words + wofs] >> (act & 31)) & 1u);
        double x[kWW];
        {
          const double* rps = rec;
          asm volatile("" : "+v"(rps));  // opaque per sample: re-read, not held across the samples
          load_col(rps, x);
        }
        // the keep bits of this half's sample (bit p: slot p), known to every lane of the half
        const uint32_t kh = (uint32_t)(__ballot(keep) >> (32 * half));
        // fm[i]: all ones while row i is free, 0 once it is a pivot row; ANDed onto both words of a
        // value it zeroes the pivot rows' entries of a reflection vector
        uint32_t fm[kWW];
#pragma unroll
        for (int i = 0; i < kWW; ++i) fm[i] = ~0u;
        auto free_part = [&](double y, uint32_t mk) {
          const uint64_t u = (uint64_t)__double_as_longlong(y);
          return __longlong_as_double((long long)(((uint64_t)((uint32_t)(u >> 32) & mk) << 32) | ((uint32_t)u & mk)));
        };
        double rd = 0.0;  // lane q: 1 / R_qq after the reflections (0: dropped slot)
        {  // column 0 has no rows above it: its reflection would only flip row 0's sign (skipped)
          const bool pv = (kh & 1u) && r00 * r00 > __shfl(thr, 0, 32);
          fm[0] = pv ? 0u : ~0u;
          if (q == 0) rd = pv ? rcp_newton(r00) : 0.0;
        }
#pragma unroll
        for (int p = 1; p < kWW; ++p) {
          if (p < wrt) {
            // column p (rows 0 .. p) and its rank floor from lane p to the whole half, which then
            // forms the reflection vector redundantly (0 on the pivot rows): no second round trip
            // for tau and the pivot decision, and no copy of the vector beside the broadcast one
            double v[kWW];
#pragma unroll
            for (int i = 0; i <= p; ++i) v[i] = __shfl(x[i], p, 32);
            const double thp = __shfl(thr, p, 32);
            const double xp = v[p];
            double sig = xp * xp;
#pragma unroll
            for (int i = 0; i < p; ++i) {
              v[i] = free_part(v[i], fm[i]);
              sig = fma(v[i], v[i], sig);
            }
            const bool pv = ((kh >> p) & 1u) && sig > thp;  // |R_pp| after the reflection > 1e-12 ||D[:, p]||
            const double rs = rsq_newton(pv ? sig : 1.0);
            const double sq = sig * rs;
            const double alpha = __builtin_copysign(sq, -xp);  // the new R_pp (sign opposite to x_p)
            const double tau = pv ? rcp_newton(fma(sq, __builtin_fabs(xp), sig)) : 0.0;  // 1 / (sig - alpha x_p)
            v[p] = xp - alpha;
            if (q == p) rd = pv ? __builtin_copysign(rs, -xp) : 0.0;  // 1 / alpha
            fm[p] = pv ? 0u : ~0u;
            double a = v[p] * x[p];
#pragma unroll
            for (int i = 0; i < p; ++i) a = fma(v[i], x[i], a);
            a = (q > p || q == 0) ? a * tau : 0.0;  // columns <= p are final
#pragma unroll
            for (int i = 0; i <= p; ++i) x[i] = fma(-a, v[i], x[i]);
          }
        }
        double rsum = tail;  // + (Q^T e)^2 over the free rows (lane 0)
#pragma unroll
        for (int i = 0; i < kWW; ++i) rsum = fma(free_part(x[i], fm[i]), x[i], rsum);
        // back-substitution, row p = W - 1 .. 0: lane 0 brings c_p, lane q > p brings -R_pq m_q
        double mq = 0.0;
#pragma unroll
        for (int p = kWW - 1; p >= 0; --p) {
          if (p < wrt) {
            const double sum = group_sum<32>(q == 0 ? x[p] : (q > p ? -x[p] * mq : 0.0));
            if (q == p) mq = sum * rd;  // 0 for a dropped slot
          }
        }
        if (own) {
          if (m_out != nullptr && q < wrt) m_out[((int64_t)b * nloc + (l - line_begin)) * wrt + q] = (TM)mq;
          if (q == 0) s_acc[wave][sl] += rsum;  // one lane per (wave, sample): the wave's lines in order
        }
      }
    }
    __syncthreads();
    for (int u = t; u < nb; u += kWNT) {
      double acc = s_acc[0][u];
#pragma unroll
      for (int w = 1; w < NW; ++w) acc += s_acc[w][u];
      partials[(int64_t)(b0 + u) * gridDim.x + lb] = acc;
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace spai

using namespace spai;

extern "C" int spai_qr_wide_limits(int32_t* max_w, int32_t* max_wa, int32_t* max_rows) {
  SPAI_CHECK_ARG(max_w && max_wa && max_rows, "spai_qr_wide_limits: null pointer");
  *max_w = kWW;
  *max_wa = kWW;
  *max_rows = kWRows;
  return SPAI_OK;
}

static bool qrw_widths_ok(int32_t W, int32_t WA) { return W >= 1 && W <= kWW && WA >= 1 && WA <= kWW; }

extern "C" int spai_qr_wide_max_rows(int32_t n, int32_t W, const int32_t* pat_idx, int32_t WA, const int32_t* a_idx,
                                     int32_t* max_rows, void* stream) {
  SPAI_CHECK_ARG(n >= 1 && W >= 1 && WA >= 1 && pat_idx && a_idx && max_rows, "spai_qr_wide_max_rows: bad arguments");
  if (!qrw_widths_ok(W, WA)) {
    set_error("spai_qr_wide_max_rows: widths W=%d WA=%d above the compiled %d / %d (row union <= %d)", W, WA, kWW, kWW,
              kWRows);
    return SPAI_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  SPAI_CHECK_HIP(hipMemsetAsync(max_rows, 0, sizeof(int32_t), s));
  k_qrw_rows<<<(n + 3) / 4, 256, 0, s>>>(n, W, pat_idx, WA, a_idx, max_rows);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}

extern "C" size_t spai_qr_wide_cache_bytes(int32_t n, int32_t W) {
  if (n <= 0 || W < 1 || W > kWW) return 0;
  return sizeof(double) * (size_t)qrw_nq(W) * (size_t)n;
}

extern "C" int spai_qr_wide_factor(int32_t n, int32_t W, const int32_t* pat_idx, int32_t WA, const int32_t* a_idx,
                                   const void* a_val, int32_t a_dtype, int32_t max_rows, double* rcache,
                                   size_t rcache_bytes, void* stream) {
  SPAI_CHECK_ARG(n >= 1 && W >= 1 && WA >= 1 && max_rows >= 0 && pat_idx && a_idx && a_val && rcache,
                 "spai_qr_wide_factor: bad arguments");
  SPAI_CHECK_ARG(a_dtype == SPAI_DTYPE_F32 || a_dtype == SPAI_DTYPE_F64, "spai_qr_wide_factor: bad a_dtype");
  if (!qrw_widths_ok(W, WA) || max_rows > kWRows) {
    set_error("spai_qr_wide_factor: widths W=%d WA=%d / %d rows above the compiled %d / %d / %d", W, WA, max_rows,
              kWW, kWW, kWRows);
    return SPAI_ERR_UNSUPPORTED;
  }
  SPAI_CHECK_ARG(rcache_bytes >= spai_qr_wide_cache_bytes(n, W), "spai_qr_wide_factor: rcache too small");
  hipStream_t s = (hipStream_t)stream;
  const bool a32 = a_dtype == SPAI_DTYPE_F32;
  if (max_rows <= 64)  // one wave per line
    k_qrw_factor<64><<<n, 64, 0, s>>>(n, W, pat_idx, WA, a_idx, a_val, a32, rcache);
  else
    k_qrw_factor<kWRows><<<n, kWRows, 0, s>>>(n, W, pat_idx, WA, a_idx, a_val, a32, rcache);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}

extern "C" int spai_fill_lines_qr_wide(int32_t n, int32_t line_begin, int32_t line_end, int32_t W,
                                       const int32_t* pat_act, const double* rcache, size_t rcache_bytes, int32_t B,
                                       const uint32_t* removed, int32_t words, int32_t word_base, void* m_out,
                                       int32_t m_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  int32_t nparts;
  const int st = check_fill_lines("spai_fill_lines_qr_wide", n, line_begin, line_end, W, B, words, word_base, true,
                                  m_dtype, workspace, workspace_bytes, pat_act && rcache && removed, &nparts);
  if (st != SPAI_OK || nparts == 0) return st;
  if (W > kWW) {
    set_error("spai_fill_lines_qr_wide: width W=%d above the compiled %d (A width <= %d, row union <= %d)", W, kWW,
              kWW, kWRows);
    return SPAI_ERR_UNSUPPORTED;
  }
  SPAI_CHECK_ARG(rcache_bytes >= spai_qr_wide_cache_bytes(n, W), "spai_fill_lines_qr_wide: rcache too small");
  double* partials = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (m_dtype == SPAI_DTYPE_F64)
    k_qrw_solve<double><<<nparts, kWNT, 0, s>>>(line_begin, line_end, W, pat_act, rcache, B, removed, words,
                                                word_base, static_cast<double*>(m_out), partials);
  else
    k_qrw_solve<float><<<nparts, kWNT, 0, s>>>(line_begin, line_end, W, pat_act, rcache, B, removed, words,
                                               word_base, static_cast<float*>(m_out), partials);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}
