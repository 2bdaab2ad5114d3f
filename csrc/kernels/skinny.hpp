// Shared pieces of the skinny-block kernels (panel_rhs.hip, panel_rhs_t.hip, rank_update.hip): a
// tall panel against a skinny fp64 block of at most 64 columns.  The MFMA traits, the NaN-keeping
// magnitude key, the host-side launch helpers and the column epilogue Y = C_in + sign * term with
// its column maxima.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "gj/common.hpp"

namespace gj {
namespace kern {

// v_mfma_{f64,f32}_16x16x4: the accumulator, the 16-byte load of T and the row of accumulator
// element q.  The LDS padding is the choice of each kernel and stays with it.
template <typename T>
struct SkinnyMfma;
template <>
struct SkinnyMfma<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  typedef double vec_t __attribute__((ext_vector_type(2)));
  static constexpr int W = 2;  // elements of a 16-byte load
  static __device__ __forceinline__ acc_t op(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int q) { return (lane >> 4) + 4 * q; }
};
template <>
struct SkinnyMfma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  typedef float vec_t __attribute__((ext_vector_type(4)));
  static constexpr int W = 4;
  static __device__ __forceinline__ acc_t op(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int q) { return 4 * (lane >> 4) + q; }
};

// The order of non-negative doubles for reductions in registers: the bit pattern of a non-negative
// double, NaN (of either sign) as the canonical quiet NaN, which lies above +Inf.  An integer
// maximum over these keeps a NaN that fmax would drop.
__device__ __forceinline__ unsigned long long nonneg_key(double v) {
  v = (v >= 0.0) ? fabs(v) : __longlong_as_double(0x7ff8000000000000ll);  // fabs: -0.0 -> +0.0
  return (unsigned long long)__double_as_longlong(v);
}

// compute units of the current device: cached per process, 256 if the query fails
inline int num_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      ncu = v;
    else
      ncu = 256;
  }
  return ncu;
}

// 16-byte loads of a panel need 16-byte aligned rows
inline bool rows_16B_aligned(const void* ptr, int64_t ld, size_t elem_size) {
  return reinterpret_cast<uintptr_t>(ptr) % 16 == 0 && ((size_t)ld * elem_size) % 16 == 0;
}

// k <= 64 columns -> the compile-time column width the kernels are built for: f(KW) with KW an
// integral_constant of 16, 32 or 64
template <typename F>
inline auto with_kw(int64_t k, F&& f) {
  if (k <= 16) return f(std::integral_constant<int, 16>{});
  if (k <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}
inline int padded_kw(int64_t k) {
  return with_kw(k, [](auto KW) -> int { return KW; });
}

// Formats the probe name of op Op's launch into that op's buffer of this thread and points `last`
// (the op's g_last_*_kernel) at it.
template <typename Op>
__attribute__((format(printf, 2, 3))) inline void set_probe_name(const char*& last, const char* fmt, ...) {
  thread_local char buf[48] = "";
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last = buf;
}

// What the column epilogue adds at (r, c): counts(r) = row r takes the term and enters colmax,
// term(r, c) = the value, read only where the row counts.
// SliceSum: the fixed-order sum of the K-slice partials part[s][r][c]; a padded local row (global
// row >= n) keeps C_in (or 0) and does not enter the maximum.
template <int KW>
struct SliceSum {
  const double* __restrict__ part;
  int S;
  int64_t rows_pad, n, m, p, rk;
  __device__ __forceinline__ bool counts(int64_t r) const { return ((r / m) * p + rk) * m + r % m < n; }
  __device__ __forceinline__ double term(int64_t r, int c) const {
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += part[((int64_t)s * rows_pad + r) * KW + c];
    return sum;
  }
};
// DenseTerm: an element of S; every row counts.
struct DenseTerm {
  const double* __restrict__ S;
  int64_t lds;
  __device__ __forceinline__ bool counts(int64_t) const { return true; }
  __device__ __forceinline__ double term(int64_t r, int c) const { return S[r * lds + c]; }
};

// Y = C_in + sign * term on the active columns c < k of the rows < rows, and the maxima of |Y| of
// the rows that count, as keys (nonneg_key) into colmax, which the caller has set to 0 for the active
// columns.  A workgroup covers rpb rows x KW columns (thread = column tid % KW, row group tid / KW).
template <int KW, typename Src>
__global__ __launch_bounds__(256) void col_epilogue_kernel(Src src, const double* C_in, int64_t ldc, double* Y,
                                                           int64_t ldy, double sign, int64_t rows, int k,
                                                           const int32_t* __restrict__ active,
                                                           unsigned long long* colmax, int rpb) {
  constexpr int RG = 256 / KW;
  const int c = threadIdx.x % KW, rs = threadIdx.x / KW;
  const bool on = c < k && (!active || active[c] != 0);
  const int64_t base = (int64_t)blockIdx.x * rpb;
  const int64_t end = base + rpb < rows ? base + rpb : rows;
  unsigned long long key = 0ull;
  if (on)
    for (int64_t r = base + rs; r < end; r += RG) {
      const bool counts = src.counts(r);
      double y = C_in ? C_in[r * ldc + c] : 0.0;
      if (counts) {
        y += sign * src.term(r, c);
        const unsigned long long kk = nonneg_key(fabs(y));
        key = kk > key ? kk : key;
      }
      Y[r * ldy + c] = y;
    }
  if (!colmax) return;
  __shared__ unsigned long long sh[256];
  sh[threadIdx.x] = key;
  __syncthreads();
  if (rs == 0 && on) {
#pragma unroll
    for (int q = 1; q < RG; ++q) key = sh[q * KW + c] > key ? sh[q * KW + c] : key;
    atomicMax(colmax + c, key);  // an integer maximum: the same bits in any order
  }
}

template <int KW, typename Src>
inline void launch_col_epilogue(const Src& src, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign,
                                int64_t rows, int k, const int32_t* active, unsigned long long* colmax,
                                hipStream_t s) {
  const int rpb = 4 * (256 / KW);
  const unsigned grid = (unsigned)std::max<int64_t>((rows + rpb - 1) / rpb, 1);
  hipLaunchKernelGGL((col_epilogue_kernel<KW, Src>), dim3(grid), dim3(256), 0, s, src, C_in, ldc, Y, ldy, sign, rows,
                     k, active, colmax, rpb);
}

}  // namespace kern
}  // namespace gj
