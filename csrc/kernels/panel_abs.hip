// Kernels of the error bounds of a refined solve (Device::panel_abs_rhs, panel_abs_rhs_t,
// bound_terms; Engine::solve_rhs_block with bounds), gfx950.
//
// panel_abs_rhs / panel_abs_rhs_t are the siblings of panel_rhs / panel_rhs_t on absolute values:
// Y = |C_in| + |P| |V| and S = |P|^T |V_loc|, the same pass-1 kernels (skinny_stream.hpp) with the
// arithmetic AbsArith, the same split plans and pass 2 (skinny.hpp) and the same never-read set: rows
// >= L.rows, local padding rows (global row >= n), columns >= n of P, rows >= n of V and for the
// transposed product the rows of V that other ranks own, and columns >= k.  There is no column mask.
//
// What differs is the arithmetic: fp64 whatever the panel's storage type.  An fp32 element is
// widened exactly, its sign is cleared, and the product runs on v_mfma_f64_16x16x4_f64 (the
// precedent of rank_update.hip); the absolute value of V is taken while staging.  The bound these
// products feed has a right-hand side of about u (|A| |x| + |b|), which underflows fp32 for a small
// b, and its own rounding error must stay an fp64 one.  The fp32 vector path loads 4 floats per lane
// and feeds 4 fp64 K steps; the kernel is memory-bound, the conversions ride along.
//
// The K / row split is summed by a second pass in a fixed order and the column maximum is an
// integer maximum of bit patterns: two launches on the same input give the same bits, no
// floating-point value is accumulated with atomics.  Every term is computed by the MFMA from its
// two factors as they are, so a NaN or an Inf of |P| or |V| reaches every element it is a term of,
// also through a zero factor; masked operands (never read) are 0 on both sides.
//
// Both ops refuse a leading dimension of P whose tile rows would leave 32-bit byte offsets
// (device.hpp).  The transposed product addresses its rows that way; for the plain one, which uses
// 64-bit row addresses, the refusal is the contract alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "skinny_stream.hpp"

namespace gj {
namespace kern {

namespace {

// |P| |V| in fp64 for both dtypes: |V| staged as double, an element of P widened exactly, then the
// sign cleared.
template <typename T_>
struct AbsArith {
  using T = T_;
  using MF = SkinnyMfma<double>;
  static __device__ __forceinline__ double stage(double v) { return fabs(v); }
  static __device__ __forceinline__ double operand(T a) { return fabs((double)a); }
  // rows: the 4 K lanes of a B-fragment read sit W rows apart, and W * pitch = 128 (mod 256) bytes
  // spreads them over the banks
  static constexpr int rows_pad(int W, int kw) { return W == 4 ? 4 : W == 2 ? 8 : (kw == 16 ? 0 : 16); }
  // cols: the K lanes sit on consecutive rows
  static constexpr int cols_pad(int kw) { return kw == 16 ? 0 : 16; }
  // 64-bit row addresses cost the vec builds of the transposed product an occupancy step
  static constexpr bool kRowOffsets32 = true;
};

// G = |R| + nz_eps D (+ safe1 where D <= safe2) and the column maxima of |R| / D (of
// (|R| + safe1) / (D + safe1) where D <= safe2), as keys into berr.  A workgroup covers rpb rows x KW
// columns (thread = column tid % KW, row group tid / KW).
template <int KW>
__global__ __launch_bounds__(256) void bound_terms_kernel(const double* R, int64_t ldr, const double* __restrict__ D,
                                                          int64_t ldd, double* G, int64_t ldg, int64_t rows, int k,
                                                          double nz_eps, double safe1, double safe2,
                                                          unsigned long long* berr, int rpb) {
  constexpr int RG = 256 / KW;
  const int c = threadIdx.x % KW, rs = threadIdx.x / KW;
  const bool on = c < k;
  const int64_t base = (int64_t)blockIdx.x * rpb;
  const int64_t end = base + rpb < rows ? base + rpb : rows;
  unsigned long long key = 0ull;
  if (on)
    for (int64_t r = base + rs; r < end; r += RG) {
      const double ar = fabs(R[r * ldr + c]), d = D[r * ldd + c];
      const bool tiny = d <= safe2;
      double gv = fma(nz_eps, d, ar);  // one rounding
      if (tiny) gv += safe1;
      G[r * ldg + c] = gv;
      const double q = tiny ? (ar + safe1) / (d + safe1) : ar / d;
      const unsigned long long kk = nonneg_key(q);
      key = kk > key ? kk : key;
    }
  block_key_max<KW>(key, on, berr);
}

}  // namespace

const char* last_abs_kernel() { return g_last_abs_kernel; }

void panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                   const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax, void* scratch,
                   hipStream_t s) {
  // the op's contract (device.hpp); the kernel addresses its rows with 64-bit pointers and does not need it
  check_ld_32bit("panel_abs_rhs", ldp, (int64_t)dtype_size(dt), kRhsTileM);
  const RhsPlan pl = rhs_plan(L);
  // 16-byte loads of P need 16-byte aligned rows; the K-slices start on multiples of 16 columns
  const bool vec = rows_16B_aligned(P, ldp, dtype_size(dt));
  double* part = static_cast<double*>(scratch);
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  set_probe_name<struct AbsProbe>(g_last_abs_kernel, "abs%d:%s:%s:s%d", padded_kw(k),
                                  dt == DType::F64 ? "f64" : "f32", vec ? "vec" : "scalar", pl.S);
  with_kw(k, [&](auto KW) {
    launch_skinny_rows<AbsArith, KW>(dt, vec, P, ldp, L, V, ldv, (int)k, nullptr, part, pl, cm, s);
    const SliceSum<KW> sum{part, pl.S, pl.rows_pad, L.n, L.m, L.p, L.k};
    launch_col_epilogue<KW, SliceSum<KW>, true>(sum, C_in, ldc, Y, ldy, 1.0, L.rows, (int)k, nullptr, cm, s);
  });
}

void panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                     double* S, int64_t lds, void* scratch, hipStream_t s) {
  // a chunk's rows are addressed from the chunk's base with 32-bit byte offsets (AbsArith::kRowOffsets32)
  check_ld_32bit("panel_abs_rhs_t", ldp, (int64_t)dtype_size(dt), kRtKC);
  const RtPlan pl = rt_plan(dt, P, ldp, L);
  set_probe_name<struct AbsProbe>(g_last_abs_kernel, "abst%d:%s:%s:s%d", padded_kw(k),
                                  dt == DType::F64 ? "f64" : "f32", pl.vec ? "vec" : "scalar", pl.S);
  if (L.n <= 0) return;
  double* part = static_cast<double*>(scratch);
  with_kw(k, [&](auto KW) {
    launch_skinny_cols<AbsArith, KW>(dt, P, ldp, L, V, ldv, (int)k, nullptr, part, pl, s);
    launch_rt_reduce<KW>(part, pl, L, (int)k, S, lds, nullptr, s);
  });
}

void bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg, int64_t rows,
                 int64_t k, double nz_eps, double safe1, double safe2, double* berr, hipStream_t s) {
  unsigned long long* be = reinterpret_cast<unsigned long long*>(berr);
  launch_zero_keys(be, (int)k, nullptr, s);  // berr of every column starts from the key of +0.0
  if (rows <= 0) return;
  with_kw(k, [&](auto KW) {
    const int rpb = 4 * (256 / KW);
    const unsigned grid = (unsigned)((rows + rpb - 1) / rpb);
    hipLaunchKernelGGL((bound_terms_kernel<KW>), dim3(grid), dim3(256), 0, s, R, ldr, D, ldd, G, ldg, rows, (int)k,
                       nz_eps, safe1, safe2, be, rpb);
  });
}

}  // namespace kern
}  // namespace gj
