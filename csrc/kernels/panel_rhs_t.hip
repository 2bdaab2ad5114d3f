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
//           (skinny_cols_kernel with PlainArith, skinny_stream.hpp)
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
#include "skinny_stream.hpp"

namespace gj {
namespace kern {

namespace {

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
    launch_skinny_cols<PlainArith, KW>(dt, P, ldp, L, V, ldv, (int)k, active, part, pl, s);
    launch_rt_reduce<KW>(part, pl, L, (int)k, S, lds, active, s);
  });
}

// Y = C_in + sign S on the active columns, and their maxima
void axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S, int64_t lds,
                      double sign, int64_t rows, int64_t k, const int32_t* active, double* colmax, hipStream_t s) {
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  if (cm) launch_zero_keys(cm, (int)k, active, s);
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
