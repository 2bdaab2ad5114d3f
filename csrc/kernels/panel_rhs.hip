// Kernels of the block right-hand-side solve (Device::panel_rhs, gather_rows_natural,
// copy_cols_masked; Engine::solve_rhs_block), gfx950.
//
// panel_rhs: Y = C_in + sign * P V with P a tall panel (rows x n of fp64 / fp32) and V a skinny
// fp64 block (n x k, k <= 64).  P is the memory-bound operand: every element is read exactly once
// per launch, straight from HBM into MFMA A-operand registers (16-byte loads where the rows are
// 16-byte aligned, element loads otherwise); V stays in L2 and reaches the waves through LDS, once
// per workgroup.
//
//   pass 1  grid (row tiles of 128, S K-slices): a wave owns 32 rows (two 16-row fragments) and
//           NF = 1 | 2 | 4 column fragments of 16 (v_mfma_{f64,f32}_16x16x4), walks its K-slice and
//           stores the partial product, widened to fp64, to part[slice][row][col]
//           (skinny_rows_kernel with PlainArith, skinny_stream.hpp)
//   pass 2  Y = C_in + sign * sum_{slice} part in slice order, and the column maxima
//           (col_epilogue_kernel with the SliceSum source, skinny.hpp)
//
// Where a launch has fewer row tiles than the chip needs to saturate HBM, K is split over S
// workgroups (auto, or set_rhs_splitk).  The slices are summed by pass 2 in a fixed order and the
// column maximum is an integer maximum of bit patterns, so the result is bit-identical from run
// to run; no floating-point value is accumulated with atomics.
//
// Masks, not assumptions: rows >= L.rows, local padding rows (global row >= n), K >= n, columns
// >= k and inactive columns are never loaded (their operand is 0), whatever m, n and the leading
// dimensions are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "skinny_stream.hpp"

namespace gj {
namespace kern {

namespace {

__global__ __launch_bounds__(256) void gather_rows_natural_kernel(double* __restrict__ dst, int64_t ldd,
                                                                  const double* __restrict__ src, int64_t lds,
                                                                  int64_t n, int64_t m, int64_t p, int64_t per,
                                                                  int64_t k) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * k) return;
  const int64_t gr = t / k, j = t % k;
  const int64_t gb = gr / m, e = gr % m;
  dst[gr * ldd + j] = src[((gb % p) * per + (gb / p) * m + e) * lds + j];
}

__global__ __launch_bounds__(256) void copy_cols_masked_kernel(double* __restrict__ dst, int64_t ldd,
                                                               const double* __restrict__ src, int64_t lds,
                                                               int64_t rows, int64_t k,
                                                               const int32_t* __restrict__ mask) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * k) return;
  const int64_t r = t / k, j = t % k;
  if (mask[j] != 0) dst[r * ldd + j] = src[r * lds + j];
}

}  // namespace

void set_rhs_splitk(int s) { g_rhs_splitk = s < 0 ? 0 : s; }
const char* last_rhs_kernel() { return g_last_rhs_kernel; }

size_t panel_rhs_scratch_bytes(const Layout& L, int64_t k) {
  const RhsPlan pl = rhs_plan(L);
  return sizeof(double) * (size_t)pl.S * (size_t)pl.rows_pad * padded_kw(k);
}

void panel_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
               const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign, const int32_t* active,
               double* colmax, void* scratch, hipStream_t s) {
  const RhsPlan pl = rhs_plan(L);
  // 16-byte loads of P need 16-byte aligned rows; the K-slices start on multiples of 16 columns
  const bool vec = rows_16B_aligned(P, ldp, dtype_size(dt));
  double* part = static_cast<double*>(scratch);
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  set_probe_name<struct RhsProbe>(g_last_rhs_kernel, "rhs%d:%s:%s:s%d", padded_kw(k),
                                  dt == DType::F64 ? "f64" : "f32", vec ? "vec" : "scalar", pl.S);
  with_kw(k, [&](auto KW) {
    launch_skinny_rows<PlainArith, KW>(dt, vec, P, ldp, L, V, ldv, (int)k, active, part, pl, cm, s);
    const SliceSum<KW> sum{part, pl.S, pl.rows_pad, L.n, L.m, L.p, L.k};
    launch_col_epilogue<KW>(sum, C_in, ldc, Y, ldy, sign, L.rows, (int)k, active, cm, s);
  });
}

void gather_rows_natural(double* dst, int64_t ldd, const double* src, int64_t lds, const Layout& L, int64_t k,
                         hipStream_t s) {
  const int64_t work = L.n * k;
  if (work <= 0) return;
  hipLaunchKernelGGL(gather_rows_natural_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, dst, ldd,
                     src, lds, L.n, L.m, L.p, L.max_nblk * L.m, k);
}

void copy_cols_masked(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t k,
                      const int32_t* mask, hipStream_t s) {
  const int64_t work = rows * k;
  if (work <= 0) return;
  hipLaunchKernelGGL(copy_cols_masked_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, dst, ldd, src,
                     lds, rows, k, mask);
}

}  // namespace kern
}  // namespace gj
