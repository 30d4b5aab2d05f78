// Batched GMRES(m) on gfx950: B right-hand sides / preconditioners solved in lock step, one
// shared A and a different M per sample (gflownet_spai_amd/gmres.py gmres_batched; the
// specification is gmres._gmres = scipy.sparse.linalg.gmres with the legacy callback, per sample).
//
// Every length-n vector is fp64, laid out [B][n]; the Krylov basis is [B][restart + 1][n].  A
// kernel boundary is the only ordering: reductions are per-block partials written to the
// workspace and summed in a fixed order by the next (small) kernel, no floating-point atomics,
// and the block partition of the rows depends on n only, so sample b's bits do not depend on B
// or on the other samples.  Blocks of an inactive sample return at once.
//
//   k_bspmv        y[b] = Op_b x[b] over row-ELL lines (one thread per row, the sample is
//                  gridDim.y; slot order, fp64 fma, as k_ell_spmv).  Shared or per-sample idx
//                  (batch stride 0 or n W), per-sample fp32 / fp64 values read directly or through
//                  an int32 indirection src [n][W] (a column-oriented pattern applied as a row
//                  gather); optional x scale (the pending 1 / ||w|| of the newest basis vector),
//                  optional y = rhs - Op x, optional per-block partials of ||y||^2.
//   one inner iteration (8 launches, whatever col and B):
//     k_bspmv (t = A v_col), k_bspmv (w = M t, partials of ||w||^2 = h0^2),
//     k_dots (partials of V^T w; scales v_col in place), k_reduce_dots (h1),
//     k_upd_dots (w -= V h1, partials of V^T w in the same sweep), k_reduce_dots (h2),
//     k_upd_norm (w -= V h2 -> v_{col+1} unscaled, partials of ||w||^2),
//     k_givens (per sample: finishes the norms, h = h1 + h2, stored rotations, lartg, S, presid,
//               iteration count, history, exit rules; at the sample's cycle end the back-substitution)
//   one restart cycle = k_bspmv (v_0 = M r) + k_cycle_start + restart x 8 + k_xupdate +
//     k_bspmv (r = rhs - A x) + k_cycle_end (exit rules, ptol control, report): no host sync.
#include "spai_device.h"
#include "spai_status.h"

namespace spai {
namespace {

constexpr int kNT = 256;
constexpr int kMaxRestart = 64;
constexpr int kDotK = 4;  // basis vectors per pass of the dot sweeps
constexpr int kReportWords = 8;  // int64 words of a sample's report ahead of its cycle history
constexpr double kEps = 2.220446049250313e-16;

// flags[field * B + b] (int32) and dstate[b * kDCount + field] (fp64)
enum { F_ALIVE = 0, F_ACTIVE, F_ITER, F_INFO, F_NCOL, F_BREAK, F_CAPPED, F_COUNT = 8 };
enum { D_BNRM = 0, D_ATOL, D_PTOL, D_FACTOR, D_PRESID, D_VSCALE, D_RNORM, kDCount = 8 };

inline int ipt_of(int32_t n) {  // rows per thread of the sweeps: a function of n only
  const int64_t per = ((int64_t)n + kNT - 1) / kNT;
  return per <= 1024 ? 1 : per <= 2048 ? 2 : per <= 4096 ? 4 : 8;
}
inline int32_t nb_of(int32_t n) { return (n + kNT - 1) / kNT; }
inline int32_t g_of(int32_t n) {
  const int64_t r = (int64_t)kNT * ipt_of(n);
  return (int32_t)(((int64_t)n + r - 1) / r);
}

struct Work {
  double *V, *w, *t, *r, *pA, *pB, *pD, *pN, *h1, *h2, *S, *giv, *H, *y, *dstate;
  int32_t* flags;
  size_t bytes;
};

Work carve(void* base, int32_t n, int32_t B, int32_t m) {
  Carve c(base);
  Work k;
  const size_t m1 = (size_t)m + 1, nb = nb_of(n), g = g_of(n), b = (size_t)B;
  k.V = c.take<double>(b * m1 * n);
  k.w = c.take<double>(b * n);
  k.t = c.take<double>(b * n);
  k.r = c.take<double>(b * n);
  k.pA = c.take<double>(b * nb);
  k.pB = c.take<double>(b * nb);
  k.pD = c.take<double>(b * g * m1);
  k.pN = c.take<double>(b * g);
  k.h1 = c.take<double>(b * m1);
  k.h2 = c.take<double>(b * m1);
  k.S = c.take<double>(b * m1);
  k.giv = c.take<double>(b * m * 2);
  k.H = c.take<double>(b * m * m1);
  k.y = c.take<double>(b * m);
  k.dstate = c.take<double>(b * kDCount);
  k.flags = c.take<int32_t>(b * F_COUNT);
  k.bytes = c.off;
  return k;
}

// ------------------------------------------------------------------ batched ELL SpMV
struct SpmvArgs {
  int32_t n, W;
  const int32_t* idx;
  int64_t idx_bs, val_bs;
  const int32_t* src;
  const double* x;
  int64_t x_bs;
  double* y;
  int64_t y_bs;
  const int32_t* active;
  const double* xscale;  // NULL or per-sample scale of x at xscale[b * kDCount]
  const double* minus;   // NULL or [B][n]: y = minus - Op x
  double* part;          // NULL or [B][gridDim.x] partials of ||y||^2
};

template <typename VT, int W>
__global__ __launch_bounds__(kNT) void k_bspmv(SpmvArgs a, const VT* __restrict__ val) {
  const int b = blockIdx.y;
  if (a.active && !a.active[b]) return;
  const int i = blockIdx.x * kNT + threadIdx.x;
  double out = 0.0;
  if (i < a.n) {
    const int32_t* ri = a.idx + b * a.idx_bs + (int64_t)i * W;
    const VT* vb = val + b * a.val_bs;
    const double* x = a.x + b * a.x_bs;
    const double sc = a.xscale ? a.xscale[(int64_t)b * kDCount] : 1.0;
    int32_t c[W];
    VT v[W];
    if (a.src) {
      const int32_t* rs = a.src + (int64_t)i * W;
#pragma unroll
      for (int s = 0; s < W; ++s) c[s] = ri[s], v[s] = vb[rs[s]];
    } else {
#pragma unroll
      for (int s = 0; s < W; ++s) c[s] = ri[s], v[s] = vb[(int64_t)i * W + s];
    }
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < W; ++s)
      if (c[s] >= 0) acc = fma((double)v[s], x[c[s]] * sc, acc);
    out = a.minus ? a.minus[(int64_t)b * a.n + i] - acc : acc;
    a.y[b * a.y_bs + i] = out;
  }
  if (a.part) {
    __shared__ double lds[kNT / 64];
    const double s = block_sum<kNT>(out * out, lds);
    if (threadIdx.x == 0) a.part[(int64_t)b * gridDim.x + blockIdx.x] = s;
  }
}

template <typename VT>
__global__ __launch_bounds__(kNT) void k_bspmv_any(SpmvArgs a, const VT* __restrict__ val) {
  const int b = blockIdx.y;
  if (a.active && !a.active[b]) return;
  const int i = blockIdx.x * kNT + threadIdx.x;
  const int W = a.W;
  double out = 0.0;
  if (i < a.n) {
    const int32_t* ri = a.idx + b * a.idx_bs + (int64_t)i * W;
    const VT* vb = val + b * a.val_bs;
    const double* x = a.x + b * a.x_bs;
    const double sc = a.xscale ? a.xscale[(int64_t)b * kDCount] : 1.0;
    double acc = 0.0;
    for (int s = 0; s < W; ++s) {
      const int32_t c = ri[s];
      if (c < 0) continue;
      const VT v = a.src ? vb[a.src[(int64_t)i * W + s]] : vb[(int64_t)i * W + s];
      acc = fma((double)v, x[c] * sc, acc);
    }
    out = a.minus ? a.minus[(int64_t)b * a.n + i] - acc : acc;
    a.y[b * a.y_bs + i] = out;
  }
  if (a.part) {
    __shared__ double lds[kNT / 64];
    const double s = block_sum<kNT>(out * out, lds);
    if (threadIdx.x == 0) a.part[(int64_t)b * gridDim.x + blockIdx.x] = s;
  }
}

template <typename VT>
void launch_bspmv_t(const SpmvArgs& a, const VT* val, int32_t B, hipStream_t s) {
  const dim3 g(nb_of(a.n), B);
  switch (a.W) {
#define SPAI_W(w) \
  case w: k_bspmv<VT, w><<<g, kNT, 0, s>>>(a, val); break;
    SPAI_W(1) SPAI_W(2) SPAI_W(3) SPAI_W(4) SPAI_W(5) SPAI_W(6) SPAI_W(7) SPAI_W(8) SPAI_W(9) SPAI_W(13)
#undef SPAI_W
    default: k_bspmv_any<VT><<<g, kNT, 0, s>>>(a, val);
  }
}

// One operand of the batched SpMV as the entry points receive it.
struct EllOp {
  int32_t W;
  const int32_t* idx;
  int64_t idx_bs;
  const void* val;
  int32_t dtype;
  int64_t val_bs;
  const int32_t* src;
};

void launch_bspmv(const EllOp& op, int32_t n, int32_t B, const double* x, int64_t x_bs, double* y, int64_t y_bs,
                  const int32_t* active, const double* xscale, const double* minus, double* part, hipStream_t s) {
  SpmvArgs a{n, op.W, op.idx, op.idx_bs, op.val_bs, op.src, x, x_bs, y, y_bs, active, xscale, minus, part};
  if (op.dtype == SPAI_DTYPE_F32)
    launch_bspmv_t(a, static_cast<const float*>(op.val), B, s);
  else
    launch_bspmv_t(a, static_cast<const double*>(op.val), B, s);
}

// partials of ||v[b]||^2 over the 256-row blocks
__global__ __launch_bounds__(kNT) void k_norm2(int32_t n, const double* __restrict__ v, double* __restrict__ part) {
  const int b = blockIdx.y, i = blockIdx.x * kNT + threadIdx.x;
  const double e = i < n ? v[(int64_t)b * n + i] : 0.0;
  __shared__ double lds[kNT / 64];
  const double s = block_sum<kNT>(e * e, lds);
  if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = s;
}

// ------------------------------------------------------------------ CGS2 sweeps
// Block (g, b) owns rows [g R, (g + 1) R), R = 256 IPT; thread t rows g R + j 256 + t.
struct SweepArgs {
  int32_t n, m1, col;
  double* V;        // [B][m1][n]
  double* w;        // [B][n]
  const int32_t* active;
  const double* h;  // [B][m1] coefficients of the update (k_upd_*)
  double* dstate;
  double* part;     // k_dots / k_upd_dots: [B][G][m1]; k_upd_norm: [B][G]
};

// partials of V[:, :col+1]^T w for the rows of this block, one wave sum per k, waves in order
template <int IPT>
__device__ __forceinline__ void block_dots(const SweepArgs& a, double* Vb, const double (&wv)[IPT], int64_t row0,
                                           double scale_col, bool scale) {
  __shared__ double lds[kMaxRestart + 1][kNT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // kDotK basis vectors per pass: their loads are in flight together and their wave sums
  // interleave (a pass's surplus vectors re-read v_col and are dropped)
  for (int k0 = 0; k0 <= a.col; k0 += kDotK) {
    double p[kDotK];
#pragma unroll
    for (int c = 0; c < kDotK; ++c) {
      const int k = k0 + c;
      double* vk = Vb + (int64_t)min(k, a.col) * a.n;
      p[c] = 0.0;
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        const int64_t i = row0 + j * kNT;
        if (i < a.n) {
          double v = vk[i];
          if (scale && k == a.col) {
            v *= scale_col;
            vk[i] = v;
          }
          p[c] = fma(v, wv[j], p[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kDotK; ++c) p[c] = wave_sum_dpp(p[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kDotK; ++c)
        if (k0 + c <= a.col) lds[k0 + c][wave] = p[c];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x <= a.col) {
    const int k = threadIdx.x;
    a.part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * a.m1 + k] = ((lds[k][0] + lds[k][1]) + lds[k][2]) + lds[k][3];
  }
}

template <int IPT>
__global__ __launch_bounds__(kNT) void k_dots(SweepArgs a) {
  const int b = blockIdx.y;
  if (!a.active[b]) return;
  double* Vb = a.V + (int64_t)b * a.m1 * a.n;
  const double* wb = a.w + (int64_t)b * a.n;
  const int64_t row0 = (int64_t)blockIdx.x * kNT * IPT + threadIdx.x;
  double wv[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) wv[j] = row0 + j * kNT < a.n ? wb[row0 + j * kNT] : 0.0;
  block_dots<IPT>(a, Vb, wv, row0, a.dstate[(int64_t)b * kDCount + D_VSCALE], true);
}

template <int IPT>
__device__ __forceinline__ void apply_update(const SweepArgs& a, const double* Vb, double (&wv)[IPT], int64_t row0) {
  const double* hb = a.h + (int64_t)blockIdx.y * a.m1;
#pragma unroll 4
  for (int k = 0; k <= a.col; ++k) {
    const double hk = hb[k];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
      const int64_t i = row0 + j * kNT;
      if (i < a.n) wv[j] = fma(-hk, Vb[(int64_t)k * a.n + i], wv[j]);
    }
  }
}

template <int IPT>
__global__ __launch_bounds__(kNT) void k_upd_dots(SweepArgs a) {
  const int b = blockIdx.y;
  if (!a.active[b]) return;
  double* Vb = a.V + (int64_t)b * a.m1 * a.n;
  double* wb = a.w + (int64_t)b * a.n;
  const int64_t row0 = (int64_t)blockIdx.x * kNT * IPT + threadIdx.x;
  double wv[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) wv[j] = row0 + j * kNT < a.n ? wb[row0 + j * kNT] : 0.0;
  apply_update<IPT>(a, Vb, wv, row0);
#pragma unroll
  for (int j = 0; j < IPT; ++j)
    if (row0 + j * kNT < a.n) wb[row0 + j * kNT] = wv[j];
  block_dots<IPT>(a, Vb, wv, row0, 1.0, false);
}

template <int IPT>
__global__ __launch_bounds__(kNT) void k_upd_norm(SweepArgs a) {
  const int b = blockIdx.y;
  if (!a.active[b]) return;
  double* Vb = a.V + (int64_t)b * a.m1 * a.n;
  const double* wb = a.w + (int64_t)b * a.n;
  const int64_t row0 = (int64_t)blockIdx.x * kNT * IPT + threadIdx.x;
  double wv[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) wv[j] = row0 + j * kNT < a.n ? wb[row0 + j * kNT] : 0.0;
  apply_update<IPT>(a, Vb, wv, row0);
  double* vn = Vb + (int64_t)(a.col + 1) * a.n;  // v_{col+1}, unscaled: its 1 / ||w|| is applied by the next
  double p = 0.0;                                // iteration's k_bspmv (on the fly) and k_dots (in place)
#pragma unroll
  for (int j = 0; j < IPT; ++j)
    if (row0 + j * kNT < a.n) {
      vn[row0 + j * kNT] = wv[j];
      p = fma(wv[j], wv[j], p);
    }
  __shared__ double lds[kNT / 64];
  const double s = block_sum<kNT>(p, lds);
  if (threadIdx.x == 0) a.part[(int64_t)b * gridDim.x + blockIdx.x] = s;
}

// h[b][k] = sum over the G row blocks of part[b][g][k]: lane l sums g = l, l + 64, ... in order,
// then one wave sum; wave w takes k = w, w + 4, ...
__global__ __launch_bounds__(kNT) void k_reduce_dots(int32_t G, int32_t m1, int32_t col, const double* __restrict__ part,
                                                     const int32_t* __restrict__ active, double* __restrict__ h) {
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k <= col; k += kNT / 64) {
    double s = 0.0;
    for (int g = lane; g < G; g += 64) s += part[((int64_t)b * G + g) * m1 + k];
    s = wave_sum(s);
    if (lane == 0) h[(int64_t)b * m1 + k] = s;
  }
}

// sum of `cnt` partials in a fixed order (thread t: t, t + 256, ...; then the block sum)
__device__ __forceinline__ double sum_partials(const double* p, int32_t cnt, double* lds) {
  double s = 0.0;
  for (int g = threadIdx.x; g < cnt; g += kNT) s += p[g];
  return block_sum<kNT>(s, lds);
}

// LAPACK dlartg (3.10+, the one scipy's get_lapack_funcs("lartg") binds): c >= 0, r carries f's sign.
__device__ __forceinline__ void lartg(double f, double g, double& c, double& s, double& r) {
#pragma clang fp contract(off)
  const double safmin = 2.2250738585072014e-308, safmax = 1.0 / safmin;
  const double rtmin = 1.4916681462400413e-154, rtmax = 4.7403759540545887e+153;  // sqrt(safmin), sqrt(safmax / 2)
  const double f1 = fabs(f), g1 = fabs(g);
  if (g == 0.0) {
    c = 1.0, s = 0.0, r = f;
  } else if (f == 0.0) {
    c = 0.0, s = copysign(1.0, g), r = g1;
  } else if (f1 > rtmin && f1 < rtmax && g1 > rtmin && g1 < rtmax) {
    const double d = sqrt(f * f + g * g);
    c = f1 / d;
    r = copysign(d, f);
    s = g / r;
  } else {
    const double u = fmin(safmax, fmax(safmin, fmax(f1, g1)));
    const double fs = f / u, gs = g / u, d = sqrt(fs * fs + gs * gs);
    c = fabs(fs) / d;
    r = copysign(d, f);
    s = gs / r;
    r *= u;
  }
}

struct SmallArgs {
  int32_t B, m, col, maxiter, NB, G;
  const double *pA, *pB, *pN, *h1, *h2;
  double *S, *giv, *H, *y, *dstate;
  int32_t* flags;
  int64_t* report;  // [B][kReportWords + m]
  double rtol, atol;
};

__device__ __forceinline__ void write_report(const SmallArgs& a, int b) {
  int64_t* rp = a.report + (int64_t)b * (kReportWords + a.m);
  for (int f = 0; f < F_COUNT; ++f) rp[f] = a.flags[f * a.B + b];
}

// after ||b|| and ||M b||: tolerances, the samples that are done before the first cycle
__global__ __launch_bounds__(kNT) void k_init(SmallArgs a) {
  const int b = blockIdx.x;
  __shared__ double lds[kNT / 64];
  const double bn = sqrt(sum_partials(a.pA + (int64_t)b * a.NB, a.NB, lds));
  const double mb = sqrt(sum_partials(a.pB + (int64_t)b * a.NB, a.NB, lds));
  if (threadIdx.x != 0) return;
  double* d = a.dstate + (int64_t)b * kDCount;
  const double atol = fmax(a.atol, a.rtol * bn);
  d[D_BNRM] = bn, d[D_ATOL] = atol, d[D_FACTOR] = 1.0, d[D_PRESID] = 0.0, d[D_VSCALE] = 1.0, d[D_RNORM] = bn;
  d[D_PTOL] = bn == 0.0 ? 0.0 : mb * fmin(1.0, atol / bn);
  for (int f = 0; f < F_COUNT; ++f) a.flags[f * a.B + b] = 0;
  a.flags[F_ALIVE * a.B + b] = (bn == 0.0 || bn < atol) ? 0 : 1;  // zero rhs: x = b = 0; ||r0|| < atol: x0
  write_report(a, b);
}

// v_0 = M r / ||M r||: the norm here, the scale applied by the first iteration's consumers
__global__ __launch_bounds__(kNT) void k_cycle_start(SmallArgs a) {
  const int b = blockIdx.x;
  if (!a.flags[F_ALIVE * a.B + b]) return;
  __shared__ double lds[kNT / 64];
  const double tmp = sqrt(sum_partials(a.pA + (int64_t)b * a.NB, a.NB, lds));
  const int m1 = a.m + 1;
  for (int k = threadIdx.x + 1; k < m1; k += kNT) a.S[(int64_t)b * m1 + k] = 0.0;
  if (threadIdx.x != 0) return;
  a.S[(int64_t)b * m1] = tmp;
  a.dstate[(int64_t)b * kDCount + D_VSCALE] = 1.0 / tmp;
  a.flags[F_ACTIVE * a.B + b] = 1;
  a.flags[F_NCOL * a.B + b] = 0;
  a.flags[F_BREAK * a.B + b] = 0;
  a.flags[F_CAPPED * a.B + b] = 0;
}

// The (restart+1)-sized work of one inner iteration of one sample: _gmres's host part.
__global__ __launch_bounds__(kNT) void k_givens(SmallArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, t = threadIdx.x, col = a.col, m = a.m, m1 = a.m + 1;
  if (!a.flags[F_ACTIVE * a.B + b]) return;
  __shared__ double lds[kNT / 64];
  __shared__ double hc[kMaxRestart + 2], gc[kMaxRestart], gs[kMaxRestart], ys[kMaxRestart + 1];
  __shared__ int s_end;
  const double h0sq = sum_partials(a.pA + (int64_t)b * a.NB, a.NB, lds);
  const double hnsq = sum_partials(a.pN + (int64_t)b * a.G, a.G, lds);
  if (t <= col) {
    hc[t] = a.h1[(int64_t)b * m1 + t] + a.h2[(int64_t)b * m1 + t];
    ys[t] = a.S[(int64_t)b * m1 + t];
  }
  if (t < col) gc[t] = a.giv[((int64_t)b * m + t) * 2], gs[t] = a.giv[((int64_t)b * m + t) * 2 + 1];
  __syncthreads();
  if (t == 0) {
    double* d = a.dstate + (int64_t)b * kDCount;
    const double h0 = sqrt(h0sq), h1 = sqrt(hnsq);
    const bool breakdown = h1 <= kEps * h0;
    hc[col + 1] = breakdown ? 0.0 : h1;
    d[D_VSCALE] = breakdown ? 1.0 : 1.0 / h1;
    for (int k = 0; k < col; ++k) {
      const double c = gc[k], s = gs[k], n0 = hc[k], n1 = hc[k + 1];
      hc[k] = c * n0 + s * n1;
      hc[k + 1] = -s * n0 + c * n1;
    }
    double c, s, mag;
    lartg(hc[col], hc[col + 1], c, s, mag);
    a.giv[((int64_t)b * m + col) * 2] = c;
    a.giv[((int64_t)b * m + col) * 2 + 1] = s;
    hc[col] = mag;
    hc[col + 1] = 0.0;
    const double tmp = -s * ys[col];
    ys[col] = c * ys[col];
    a.S[(int64_t)b * m1 + col] = ys[col];
    a.S[(int64_t)b * m1 + col + 1] = tmp;
    const double presid = fabs(tmp);
    d[D_PRESID] = presid;
    const int it = a.flags[F_ITER * a.B + b] + 1;
    a.flags[F_ITER * a.B + b] = it;
    reinterpret_cast<double*>(a.report + (int64_t)b * (kReportWords + m) + kReportWords)[col] = presid / d[D_BNRM];
    const bool capped = it == a.maxiter;
    a.flags[F_BREAK * a.B + b] = breakdown;
    a.flags[F_CAPPED * a.B + b] = capped;
    s_end = capped || presid <= d[D_PTOL] || breakdown || col == m - 1;
    if (mag == 0.0) ys[col] = 0.0;  // (read only when the cycle ends here)
  }
  __syncthreads();
  if (t <= col + 1) a.H[((int64_t)b * m + col) * m1 + t] = hc[t];
  if (!s_end) return;
  // back-substitution for y over the rotated Hessenberg columns H[k][0..k] (column col from hc)
  for (int k = col; k >= 1; --k) {
    __syncthreads();
    double yk = ys[k];
    if (yk != 0.0) {
      const double* Hk = a.H + ((int64_t)b * m + k) * m1;
      yk /= k == col ? hc[k] : Hk[k];
      if (t < k) ys[t] -= yk * (k == col ? hc[t] : Hk[t]);
    }
    __syncthreads();
    if (t == 0) ys[k] = yk;
  }
  __syncthreads();
  if (t == 0 && ys[0] != 0.0) ys[0] /= col == 0 ? hc[0] : a.H[(int64_t)b * m * m1];
  __syncthreads();
  if (t <= col) a.y[(int64_t)b * m + t] = ys[t];
  if (t == 0) {
    a.flags[F_ACTIVE * a.B + b] = 0;
    a.flags[F_NCOL * a.B + b] = col + 1;
  }
}

// x[b] += sum_k y[b][k] V[b][k] over the sample's ncol basis vectors
__global__ __launch_bounds__(kNT) void k_xupdate(int32_t n, int32_t B, int32_t m, const double* __restrict__ V,
                                                 const double* __restrict__ y, const int32_t* __restrict__ flags,
                                                 double* __restrict__ x) {
  const int b = blockIdx.y;
  if (!flags[F_ALIVE * B + b]) return;
  const int i = blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const int ncol = flags[F_NCOL * B + b];
  const double* Vb = V + (int64_t)b * (m + 1) * n;
  double acc = 0.0;
  for (int k = 0; k < ncol; ++k) acc = fma(y[(int64_t)b * m + k], Vb[(int64_t)k * n + i], acc);
  x[(int64_t)b * n + i] += acc;
}

// after r = rhs - A x: _gmres's exit rules and inner-tolerance control, then the report
__global__ __launch_bounds__(kNT) void k_cycle_end(SmallArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x;
  if (!a.flags[F_ALIVE * a.B + b]) return;
  __shared__ double lds[kNT / 64];
  const double rnorm = sqrt(sum_partials(a.pA + (int64_t)b * a.NB, a.NB, lds));
  if (threadIdx.x != 0) return;
  double* d = a.dstate + (int64_t)b * kDCount;
  d[D_RNORM] = rnorm;
  const double atol = d[D_ATOL], presid = d[D_PRESID];
  int alive = 1, info = 0;
  if (a.flags[F_CAPPED * a.B + b]) {
    alive = 0, info = rnorm <= atol ? 0 : a.maxiter;
  } else if (rnorm <= atol) {
    alive = 0;
  } else if (a.flags[F_BREAK * a.B + b]) {
    alive = 0, info = a.maxiter;
  } else {
    if (presid <= d[D_PTOL])
      d[D_FACTOR] = fmax(kEps, 0.25 * d[D_FACTOR]);
    else
      d[D_FACTOR] = fmin(1.0, 1.5 * d[D_FACTOR]);
    d[D_PTOL] = presid * fmin(d[D_FACTOR], atol / rnorm);
  }
  a.flags[F_ALIVE * a.B + b] = alive;
  a.flags[F_INFO * a.B + b] = info;
  write_report(a, b);
}

#define SPAI_SWEEP(kernel, ipt, grid, s, args)                  \
  switch (ipt) {                                                \
    case 1: kernel<1><<<grid, kNT, 0, s>>>(args); break;        \
    case 2: kernel<2><<<grid, kNT, 0, s>>>(args); break;        \
    case 4: kernel<4><<<grid, kNT, 0, s>>>(args); break;        \
    default: kernel<8><<<grid, kNT, 0, s>>>(args);              \
  }

int check_op(const char* fn, const char* which, const EllOp& op, int32_t n) {
  SPAI_CHECK_ARG(op.W >= 1, "%s: bad %s width %d", fn, which, op.W);
  SPAI_CHECK_ARG(op.idx && op.val, "%s: null pointer (%s idx / val)", fn, which);
  SPAI_CHECK_ARG(op.dtype == SPAI_DTYPE_F32 || op.dtype == SPAI_DTYPE_F64, "%s: bad %s dtype %d", fn, which, op.dtype);
  SPAI_CHECK_ARG(op.idx_bs == 0 || op.idx_bs == (int64_t)n * op.W, "%s: %s idx batch stride %lld is neither 0 nor n W",
                 fn, which, (long long)op.idx_bs);
  SPAI_CHECK_ARG(op.val_bs >= 0, "%s: negative %s value batch stride", fn, which);
  SPAI_CHECK_ARG(!(op.src && op.idx_bs != 0), "%s: %s src needs a shared pattern (idx batch stride 0)", fn, which);
  return SPAI_OK;
}

int check_shape(const char* fn, int32_t n, int32_t B, int32_t restart) {
  SPAI_CHECK_ARG(n >= 1, "%s: bad n=%d", fn, n);
  SPAI_CHECK_ARG(B >= 1 && B <= 65535, "%s: bad B=%d (1 .. 65535)", fn, B);
  SPAI_CHECK_ARG(restart >= 1, "%s: bad restart=%d", fn, restart);
  if (restart > kMaxRestart) {
    set_error("%s: restart %d above the compiled limit %d", fn, restart, kMaxRestart);
    return SPAI_ERR_UNSUPPORTED;
  }
  return SPAI_OK;
}

}  // namespace
}  // namespace spai

using namespace spai;

extern "C" size_t spai_gmres_workspace_bytes(int32_t n, int32_t B, int32_t restart) {
  if (n < 1 || B < 1 || restart < 1) return 0;
  return carve(nullptr, n, B, restart).bytes;
}

extern "C" int spai_ell_spmv_batched(int32_t n, int32_t W, int32_t B, const int32_t* idx, int64_t idx_bstride,
                                     const void* val, int32_t val_dtype, int64_t val_bstride, const int32_t* src,
                                     const double* x, double* y, const int32_t* active, void* stream) {
  static const char* fn = "spai_ell_spmv_batched";
  SPAI_CHECK_ARG(n >= 1, "%s: bad n=%d", fn, n);
  SPAI_CHECK_ARG(B >= 1 && B <= 65535, "%s: bad B=%d (1 .. 65535)", fn, B);
  const EllOp op{W, idx, idx_bstride, val, val_dtype, val_bstride, src};
  if (int st = check_op(fn, "operator", op, n)) return st;
  SPAI_CHECK_ARG(x && y, "%s: null pointer (x / y)", fn);
  launch_bspmv(op, n, B, x, n, y, n, active, nullptr, nullptr, nullptr, (hipStream_t)stream);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}

extern "C" int spai_gmres_batched_init(int32_t n, int32_t B, int32_t restart, int32_t maxiter, double rtol, double atol,
                                       int32_t m_W, const int32_t* m_idx, int64_t m_idx_bstride, const void* m_val,
                                       int32_t m_val_dtype, int64_t m_val_bstride, const int32_t* m_src,
                                       const double* rhs, double* x, int64_t* report, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  static const char* fn = "spai_gmres_batched_init";
  if (int st = check_shape(fn, n, B, restart)) return st;
  SPAI_CHECK_ARG(maxiter >= 1, "%s: bad maxiter=%d", fn, maxiter);
  SPAI_CHECK_ARG(rtol >= 0.0 && atol >= 0.0, "%s: rtol and atol must be non-negative", fn);
  const EllOp M{m_W, m_idx, m_idx_bstride, m_val, m_val_dtype, m_val_bstride, m_src};
  if (int st = check_op(fn, "M", M, n)) return st;
  SPAI_CHECK_ARG(rhs && x && report && workspace, "%s: null pointer", fn);
  const Work k = carve(workspace, n, B, restart);
  SPAI_CHECK_ARG(workspace_bytes >= k.bytes, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, k.bytes);
  hipStream_t s = (hipStream_t)stream;
  const size_t vec = (size_t)B * n * sizeof(double);
  SPAI_CHECK_HIP(hipMemsetAsync(x, 0, vec, s));
  SPAI_CHECK_HIP(hipMemcpyAsync(k.r, rhs, vec, hipMemcpyDeviceToDevice, s));
  k_norm2<<<dim3(nb_of(n), B), kNT, 0, s>>>(n, rhs, k.pA);
  launch_bspmv(M, n, B, rhs, n, k.w, n, nullptr, nullptr, nullptr, k.pB, s);
  SmallArgs a{B, restart, 0, maxiter, nb_of(n), g_of(n), k.pA, k.pB, k.pN, k.h1, k.h2, k.S, k.giv, k.H, k.y,
              k.dstate, k.flags, report, rtol, atol};
  k_init<<<B, kNT, 0, s>>>(a);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}

extern "C" int spai_gmres_batched_cycle(int32_t n, int32_t B, int32_t restart, int32_t maxiter, int32_t a_W,
                                        const int32_t* a_idx, const void* a_val, int32_t a_val_dtype, int32_t m_W,
                                        const int32_t* m_idx, int64_t m_idx_bstride, const void* m_val,
                                        int32_t m_val_dtype, int64_t m_val_bstride, const int32_t* m_src,
                                        const double* rhs, double* x, int64_t* report, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  static const char* fn = "spai_gmres_batched_cycle";
  if (int st = check_shape(fn, n, B, restart)) return st;
  SPAI_CHECK_ARG(maxiter >= 1, "%s: bad maxiter=%d", fn, maxiter);
  const EllOp A{a_W, a_idx, 0, a_val, a_val_dtype, 0, nullptr};
  const EllOp M{m_W, m_idx, m_idx_bstride, m_val, m_val_dtype, m_val_bstride, m_src};
  if (int st = check_op(fn, "A", A, n)) return st;
  if (int st = check_op(fn, "M", M, n)) return st;
  SPAI_CHECK_ARG(rhs && x && report && workspace, "%s: null pointer", fn);
  const Work k = carve(workspace, n, B, restart);
  SPAI_CHECK_ARG(workspace_bytes >= k.bytes, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, k.bytes);
  hipStream_t s = (hipStream_t)stream;
  const int32_t m = restart, m1 = restart + 1, NB = nb_of(n), G = g_of(n), ipt = ipt_of(n);
  const int64_t vstride = (int64_t)m1 * n;
  const int32_t *alive = k.flags + F_ALIVE * B, *active = k.flags + F_ACTIVE * B;
  const dim3 gs(G, B);
  SmallArgs a{B, m, 0, maxiter, NB, G, k.pA, k.pB, k.pN, k.h1, k.h2, k.S, k.giv, k.H, k.y,
              k.dstate, k.flags, report, 0.0, 0.0};
  launch_bspmv(M, n, B, k.r, n, k.V, vstride, alive, nullptr, nullptr, k.pA, s);
  k_cycle_start<<<B, kNT, 0, s>>>(a);
  for (int32_t col = 0; col < m; ++col) {
    launch_bspmv(A, n, B, k.V + (int64_t)col * n, vstride, k.t, n, active, k.dstate + D_VSCALE, nullptr, nullptr, s);
    launch_bspmv(M, n, B, k.t, n, k.w, n, active, nullptr, nullptr, k.pA, s);
    SweepArgs sw{n, m1, col, k.V, k.w, active, nullptr, k.dstate, k.pD};
    SPAI_SWEEP(k_dots, ipt, gs, s, sw)
    k_reduce_dots<<<B, kNT, 0, s>>>(G, m1, col, k.pD, active, k.h1);
    sw.h = k.h1;
    SPAI_SWEEP(k_upd_dots, ipt, gs, s, sw)
    k_reduce_dots<<<B, kNT, 0, s>>>(G, m1, col, k.pD, active, k.h2);
    sw.h = k.h2, sw.part = k.pN;
    SPAI_SWEEP(k_upd_norm, ipt, gs, s, sw)
    a.col = col;
    k_givens<<<B, kNT, 0, s>>>(a);
  }
  k_xupdate<<<dim3(NB, B), kNT, 0, s>>>(n, B, m, k.V, k.y, k.flags, x);
  launch_bspmv(A, n, B, x, n, k.r, n, alive, nullptr, rhs, k.pA, s);
  k_cycle_end<<<B, kNT, 0, s>>>(a);
  SPAI_CHECK_LAUNCH();
  return SPAI_OK;
}
