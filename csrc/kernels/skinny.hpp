// Shared pieces of the skinny-block kernels (panel_rhs.hip, panel_rhs_t.hip, panel_abs.hip,
// rank_update.hip): a tall panel against a skinny fp64 block of at most 64 columns.  The MFMA traits,
// the NaN-keeping magnitude key and its reductions, the host-side launch helpers, the split plans of
// the two streaming products (their pass 1 is skinny_stream.hpp), the column epilogue
// Y = C_in + sign * term with its column maxima and the slice sum of the transposed products.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "gj/common.hpp"
#include "gj/layout.hpp"

namespace gj {
namespace kern {

// v_mfma_{f64,f32}_16x16x4: the operand, the accumulator, the 16-byte piece of T and the row of
// accumulator element q.  The LDS padding is the choice of each kernel and stays with it.
template <typename T>
struct SkinnyMfma;
template <>
struct SkinnyMfma<double> {
  typedef double elem_t;
  typedef double acc_t __attribute__((ext_vector_type(4)));
  typedef double vec_t __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ acc_t op(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int q) { return (lane >> 4) + 4 * q; }
};
template <>
struct SkinnyMfma<float> {
  typedef float elem_t;
  typedef float acc_t __attribute__((ext_vector_type(4)));
  typedef float vec_t __attribute__((ext_vector_type(4)));
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

// Refuses (Status::BadArgs) a leading dimension ld of elements of es bytes where the byte offset of a
// tile's last row (row rows - 1, `cols` columns in) from the tile's base would not fit 32 bits
inline void check_ld_32bit(const char* op, int64_t ld, int64_t es, int rows, int cols = 0) {
  if (ld < 0 || ld > ((int64_t(1) << 31) / es - cols) / (rows - 1))
    throw Error(Status::BadArgs, std::string(op) + ": leading dimension too large for 32-bit tile offsets");
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
// a panel's dtype x (16-byte pieces | elements) -> f(T(0), W): T the element type, W an
// integral_constant of the elements of T a lane moves at once (16 / sizeof(T), or 1)
template <typename F>
inline void with_panel(DType dt, bool vec, F&& f) {
  if (dt == DType::F64) {
    if (vec) f(0.0, std::integral_constant<int, 2>{});
    else f(0.0, std::integral_constant<int, 1>{});
  } else {
    if (vec) f(0.0f, std::integral_constant<int, 4>{});
    else f(0.0f, std::integral_constant<int, 1>{});
  }
}

// The keys of the columns j < k that are active start from 0, the key of +0.0 (one workgroup)
static __global__ void zero_keys_kernel(unsigned long long* keys, int k, const int32_t* __restrict__ active) {
  const int j = threadIdx.x;
  if (j < k && (!active || active[j] != 0)) keys[j] = 0ull;
}
inline void launch_zero_keys(unsigned long long* keys, int k, const int32_t* active, hipStream_t s) {
  hipLaunchKernelGGL(zero_keys_kernel, dim3(1), dim3(64), 0, s, keys, k, active);
}

// The maximum of a workgroup's keys per column into out[c], for a workgroup of 256 threads laid out
// as thread = column tid % KW, row group tid / KW; `on` = this thread's column takes part.  Every
// thread of the workgroup calls it.
template <int KW>
__device__ __forceinline__ void block_key_max(unsigned long long key, bool on, unsigned long long* out) {
  constexpr int RG = 256 / KW;
  const int c = threadIdx.x % KW, rs = threadIdx.x / KW;
  __shared__ unsigned long long sh[256];
  sh[threadIdx.x] = key;
  __syncthreads();
  if (rs == 0 && on) {
#pragma unroll
    for (int q = 1; q < RG; ++q) key = sh[q * KW + c] > key ? sh[q * KW + c] : key;
    atomicMax(out + c, key);  // an integer maximum: the same bits in any order
  }
}

// The shapes and split plans of the two streaming products, shared by each product and its sibling
// of absolute values (skinny_stream.hpp).
constexpr int kRhsMI = 2;                             // 16-row fragments per wave
constexpr int kRhsWaves = 4;                          // waves per workgroup
constexpr int kRhsTileM = 16 * kRhsMI * kRhsWaves;    // 128 rows per workgroup
constexpr int kRhsKC = 32;                            // rows of V per LDS stage
constexpr int kRhsMaxSplit = 64;
constexpr int kRtWaves = 4;       // waves per workgroup, each on its own columns of P
constexpr int kRtKC = 32;         // local rows per LDS stage of V
constexpr int kRtMaxSplit = 64;

inline int g_rhs_splitk = 0;  // set_rhs_splitk
inline int g_rt_split = 0;    // set_rhs_t_split

// P (rows x n) V: row tiles of kRhsTileM and S K-slices of kchunk columns
struct RhsPlan {
  int64_t tiles, rows_pad, kchunk;
  int S;
};
inline RhsPlan rhs_plan(const Layout& L) {
  RhsPlan pl;
  pl.tiles = std::max<int64_t>((L.rows + kRhsTileM - 1) / kRhsTileM, 1);
  pl.rows_pad = pl.tiles * kRhsTileM;
  int64_t S = g_rhs_splitk;
  if (S <= 0) {
    // memory-bound: about two workgroups per CU keep HBM busy; a K-slice of at least 256 columns
    S = (2 * (int64_t)num_cus() + pl.tiles - 1) / pl.tiles;
    S = std::min<int64_t>(S, std::max<int64_t>(L.n / 256, 1));
  }
  S = std::max<int64_t>(1, std::min<int64_t>(S, kRhsMaxSplit));
  // slices start on a multiple of 16 columns (the widest K step, and 16-byte aligned in both dtypes)
  pl.kchunk = (((L.n + S - 1) / S + 15) / 16) * 16;
  pl.S = (int)std::max<int64_t>((L.n + pl.kchunk - 1) / pl.kchunk, 1);  // no empty slice
  return pl;
}

// P^T V over the local rows: column tiles of 64 W (W = elements of P per load) and S row slices of
// rchunk rows
struct RtPlan {
  int64_t tiles, cols_pad, rchunk, real;
  int S, W;
  bool vec;
};
inline RtPlan rt_plan(DType dt, const void* P, int64_t ldp, const Layout& L) {
  RtPlan pl;
  // 16-byte loads of P need 16-byte aligned rows; a lane's columns start on a multiple of W
  pl.vec = rows_16B_aligned(P, ldp, dtype_size(dt));
  pl.W = pl.vec ? (int)(16 / dtype_size(dt)) : 1;
  const int64_t tw = 16 * pl.W * kRtWaves;
  pl.tiles = std::max<int64_t>((L.n + tw - 1) / tw, 1);
  pl.cols_pad = pl.tiles * tw;
  pl.real = L.real_rows();
  int64_t S = g_rt_split;
  if (S <= 0) {
    // memory-bound: about two workgroups per CU keep HBM busy; a slice of at least 128 rows
    S = (2 * (int64_t)num_cus() + pl.tiles - 1) / pl.tiles;
    S = std::min<int64_t>(S, std::max<int64_t>(pl.real / 128, 1));
  }
  S = std::max<int64_t>(1, std::min<int64_t>(S, kRtMaxSplit));
  // slices are whole K steps of 4 rows
  pl.rchunk = std::max<int64_t>((((pl.real + S - 1) / S + 3) / 4) * 4, 4);
  pl.S = (int)std::max<int64_t>((pl.real + pl.rchunk - 1) / pl.rchunk, 1);  // no empty slice
  return pl;
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
// AbsC: |C_in| takes the place of C_in (the products of absolute values, panel_abs.hip).
template <int KW, typename Src, bool AbsC = false>
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
      if (AbsC) y = fabs(y);
      if (counts) {
        y += sign * src.term(r, c);
        const unsigned long long kk = nonneg_key(fabs(y));
        key = kk > key ? kk : key;
      }
      Y[r * ldy + c] = y;
    }
  if (colmax) block_key_max<KW>(key, on, colmax);  // uniform
}

template <int KW, typename Src, bool AbsC = false>
inline void launch_col_epilogue(const Src& src, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign,
                                int64_t rows, int k, const int32_t* active, unsigned long long* colmax,
                                hipStream_t s) {
  const int rpb = 4 * (256 / KW);
  const unsigned grid = (unsigned)std::max<int64_t>((rows + rpb - 1) / rpb, 1);
  hipLaunchKernelGGL((col_epilogue_kernel<KW, Src, AbsC>), dim3(grid), dim3(256), 0, s, src, C_in, ldc, Y, ldy, sign, rows,
                     k, active, colmax, rpb);
}

// Pass 2 of the transposed products: S = sum_{slice} part in slice order (+0.0 for an inactive
// column), one thread per element of S (c < n, j < k).
template <int KW>
__global__ __launch_bounds__(256) void panel_rhs_t_reduce(const double* __restrict__ part, int S, int64_t cols_pad,
                                                          int64_t n, int k, double* __restrict__ out, int64_t lds,
                                                          const int32_t* __restrict__ active) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = t / KW;
  const int j = (int)(t % KW);
  if (c >= n || j >= k) return;
  double sum = 0.0;
  if (!active || active[j] != 0)
    for (int s = 0; s < S; ++s) sum += part[((int64_t)s * cols_pad + c) * KW + j];
  out[c * lds + j] = sum;
}

template <int KW>
inline void launch_rt_reduce(const double* part, const RtPlan& pl, const Layout& L, int k, double* S, int64_t lds,
                             const int32_t* active, hipStream_t s) {
  const int64_t work = L.n * KW;
  hipLaunchKernelGGL((panel_rhs_t_reduce<KW>), dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, part, pl.S,
                     pl.cols_pad, L.n, k, S, lds, active);
}

}  // namespace kern
}  // namespace gj
