// Kernels of the transposed block solve (Device::panel_rhs_t, axpy_cols_masked, col_abs_sum;
// Engine::solve_rhs_block with trans), gfx950.
//
// panel_rhs_t: S = P^T V_loc with P this rank's rows of a tall panel (rows x n of fp64 / fp32) and
// V a skinny fp64 block in natural row order (k <= 64 columns), of which local row r uses the row
// grow(r) = ((r / m) p + rank) m + r % m.  The reduction runs over the local rows, the output has
// one row per column of P.  P is the memory-bound operand: every element is read exactly once per
// launch, straight from HBM into MFMA A-operand registers.  For D = P^T-fragment * V-fragment the
// 16 lanes of one MFMA K index hold 16 consecutive columns of one row of P, so a row-major P is
// read in whole contiguous segments (16-byte loads where the rows are 16-byte aligned, element
// loads otherwise); V stays in L2 and reaches the waves through LDS, once per workgroup.
//
//   pass 1  grid (column tiles of 64 W, S row slices), W = elements per load: a wave owns 16 W
//           columns of P (W column fragments) and NF = 1 | 2 | 4 fragments of 16 columns of V
//           (v_mfma_{f64,f32}_16x16x4), walks its slice of the rows and stores the partial product,
//           widened to fp64, to part[slice][column of P][column of V]
//   pass 2  S = sum_{slice} part in slice order (+0.0 for an inactive column)
//
// The reduction dimension is the local rows, so a small panel has few column tiles and the rows are
// split over S workgroups (auto, or set_rhs_t_split).  The slices are summed by pass 2 in a fixed
// order: the result is bit-identical from run to run, no floating-point value is accumulated with
// atomics.
//
// Masks, not assumptions: padding rows (global row >= n; they are the tail of the local rows, only
// the last global block row is short), columns >= n of P, columns >= k and inactive columns of V
// are never loaded (their operand is 0), whatever m, n, p, the rank and the leading dimensions are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

// LDS row padding of V (elements) at column width kw: the 4 K lanes of a B-fragment read sit on
// consecutive rows.  fp64: pitch = 16 (mod 32) elements, 128 (mod 256) bytes apart; fp32: pitch = 16
// (mod 64) elements, 64 (mod 256) bytes apart.
template <typename T>
constexpr int rt_lds_pad(int kw) {
  return kw == 16 ? 0 : (sizeof(T) == 4 && kw == 32) ? 48 : 16;
}

// Pass 1.  W = elements each lane loads per row (1: element loads, any alignment; SkinnyMfma<T>::W: one
// 16-byte load, rows 16-byte aligned).  A K step covers 4 local rows: lane (i = lane % 16,
// g = lane / 16) holds P[row + g][c0 + i W + j], j < W, and the j-th MFMA of the step produces the
// output rows {c0 + i W + j : i < 16} -- W interleaved column fragments from one load.
//
// V goes through LDS in chunks of kRtKC local rows, picked by the row map and converted to T once
// per workgroup (every wave of a workgroup needs the same rows of V).  Two buffers, one barrier per
// chunk: chunk c + 1 is fetched into registers before chunk c is multiplied and written to the other
// buffer after it.  `real` = this rank's real local rows (global row < n), a prefix of its rows.
template <typename T, int NF, int W>
__global__ __launch_bounds__(64 * kRtWaves) void panel_rhs_t_kernel(
    const T* __restrict__ P, int64_t ldp, int64_t real, int64_t n, uint32_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, const int32_t* __restrict__ active,
    double* __restrict__ part, int64_t cols_pad, int64_t rchunk) {
  using MF = SkinnyMfma<T>;
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRtWaves;
  constexpr int LDK = KW + rt_lds_pad<T>(KW);  // LDS row pitch (elements)
  constexpr int VPT = kRtKC * KW / NT;       // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRtKC / 4;           // K steps per chunk
  static_assert(NT % KW == 0 && (kRtKC * KW) % NT == 0 && kRtKC % 4 == 0, "chunk shape");
  __shared__ T vs[2][kRtKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  const int64_t cbase = ((int64_t)blockIdx.x * kRtWaves + wave) * (16 * W);  // this wave's columns of P
  const int64_t c0 = cbase + i * W;                                          // this lane's
  const bool cvec = c0 + W <= n;
  const int64_t rbeg = (int64_t)blockIdx.y * rchunk;
  const int64_t rend = rbeg + rchunk < real ? rbeg + rchunk : real;

  // staging: this thread's column of V and its rows of a chunk (row vr0 + q * (NT / KW))
  const int vc = threadIdx.x % KW, vr0 = threadIdx.x / KW;
  const bool vcv = vc < k && (!active || active[vc] != 0);
  double vreg[VPT];
  auto fetch = [&](int64_t rb) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int64_t r = rb + vr0 + q * (NT / KW);
      double v = 0.0;
      if (vcv && r < rend) {
        const uint32_t b = (uint32_t)r / m, e = (uint32_t)r - b * m;  // local rows < 2^31
        v = V[(((int64_t)b * p + rk) * m + e) * ldv + vc];
      }
      vreg[q] = v;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = (T)vreg[q];
  };

  typename MF::acc_t acc[W][NF];
#pragma unroll
  for (int j = 0; j < W; ++j)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[j][nf] = typename MF::acc_t{0, 0, 0, 0};

  fetch(rbeg);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int64_t rb = rbeg; rb < rend; rb += kRtKC, buf ^= 1) {
    const bool more = rb + kRtKC < rend;  // uniform over the workgroup
    if (more) fetch(rb + kRtKC);
    T a[STEPS][W];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int64_t r = rb + st * 4 + g;
      const T* src = P + r * ldp + c0;
      if (W > 1 && cvec && r < rend) {
        const typename MF::vec_t v = *reinterpret_cast<const typename MF::vec_t*>(src);
#pragma unroll
        for (int j = 0; j < W; ++j) a[st][j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j) a[st][j] = (r < rend && c0 + j < n) ? src[j] : T(0);
      }
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      T b[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 + g][nf * 16 + i];
#pragma unroll
      for (int j = 0; j < W; ++j)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[j][nf] = MF::op(a[st][j], b[nf], acc[j][nf]);
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // partial product of this row slice, widened: cols_pad is a whole number of tiles, no mask
  double* out = part + ((int64_t)blockIdx.y * cols_pad + cbase) * KW;
#pragma unroll
  for (int j = 0; j < W; ++j)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        out[(int64_t)(MF::row(lane, q) * W + j) * KW + nf * 16 + i] = (double)acc[j][nf][q];
}

// colmax of the active columns starts from 0 (the integer key of +0.0)
__global__ void axpy_cols_init_kernel(unsigned long long* colmax, int k, const int32_t* __restrict__ active) {
  const int j = threadIdx.x;
  if (j < k && (!active || active[j] != 0)) colmax[j] = 0ull;
}

// out[c] = sum over the real local rows of |X[r][c]|: a workgroup covers 64 columns, its 4 row
// groups walk the rows 4 apart and are summed in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void col_abs_sum_kernel(const T* __restrict__ X, int64_t ldx, int64_t real,
                                                          int64_t n, double* __restrict__ out) {
  const int cl = threadIdx.x & 63, rs = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cl;
  double sum = 0.0;
  if (c < n)
    for (int64_t r = rs; r < real; r += 4) sum += fabs((double)X[r * ldx + c]);
  __shared__ double sh[4][64];
  sh[rs][cl] = sum;
  __syncthreads();
  if (rs == 0 && c < n) out[c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
}

template <typename T, int NF>
void launch_rt(const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int k,
               const int32_t* active, double* part, const RtPlan& pl, hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRtWaves);
  if (pl.vec)
    hipLaunchKernelGGL((panel_rhs_t_kernel<T, NF, SkinnyMfma<T>::W>), grid, block, 0, s, static_cast<const T*>(P), ldp,
                       pl.real, L.n, (uint32_t)L.m, L.p, L.k, V, ldv, k, active, part, pl.cols_pad, pl.rchunk);
  else
    hipLaunchKernelGGL((panel_rhs_t_kernel<T, NF, 1>), grid, block, 0, s, static_cast<const T*>(P), ldp, pl.real,
                       L.n, (uint32_t)L.m, L.p, L.k, V, ldv, k, active, part, pl.cols_pad, pl.rchunk);
}

}  // namespace

void set_rhs_t_split(int s) { g_rt_split = s < 0 ? 0 : s; }
const char* last_rhs_t_kernel() { return g_last_rhs_t_kernel; }

size_t panel_rhs_t_scratch_bytes(DType dt, const void* P, int64_t ldp, const Layout& L, int64_t k) {
  const RtPlan pl = rt_plan(dt, P, ldp, L);
  return sizeof(double) * (size_t)pl.S * (size_t)pl.cols_pad * padded_kw(k);
}

void panel_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                 double* S, int64_t lds, const int32_t* active, void* scratch, hipStream_t s) {
  if (L.n <= 0) return;
  const RtPlan pl = rt_plan(dt, P, ldp, L);
  double* part = static_cast<double*>(scratch);
  set_probe_name<struct RhsTProbe>(g_last_rhs_t_kernel, "rhst%d:%s:%s:s%d", padded_kw(k),
                                   dt == DType::F64 ? "f64" : "f32", pl.vec ? "vec" : "scalar", pl.S);
  with_kw(k, [&](auto KW) {
    constexpr int NF = KW / 16;
    if (dt == DType::F64) launch_rt<double, NF>(P, ldp, L, V, ldv, (int)k, active, part, pl, s);
    else launch_rt<float, NF>(P, ldp, L, V, ldv, (int)k, active, part, pl, s);
    launch_rt_reduce<KW>(part, pl, L, (int)k, S, lds, active, s);
  });
}

// Y = C_in + sign S on the active columns, and their maxima
void axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S, int64_t lds,
                      double sign, int64_t rows, int64_t k, const int32_t* active, double* colmax, hipStream_t s) {
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  if (cm) hipLaunchKernelGGL(axpy_cols_init_kernel, dim3(1), dim3(64), 0, s, cm, (int)k, active);
  if (rows <= 0) return;
  with_kw(k, [&](auto KW) {
    launch_col_epilogue<KW>(DenseTerm{S, lds}, C_in, ldc, Y, ldy, sign, rows, (int)k, active, cm, s);
  });
}

void col_abs_sum(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, hipStream_t s) {
  if (L.n <= 0) return;
  const unsigned grid = (unsigned)((L.n + 63) / 64);
  const int64_t real = L.real_rows();
  if (dt == DType::F64)
    hipLaunchKernelGGL(col_abs_sum_kernel<double>, dim3(grid), dim3(256), 0, s, static_cast<const double*>(X), ldx,
                       real, L.n, out);
  else
    hipLaunchKernelGGL(col_abs_sum_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<const float*>(X), ldx,
                       real, L.n, out);
}

}  // namespace kern
}  // namespace gj
