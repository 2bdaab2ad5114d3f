// Kernels of the power-of-two equilibration (Device::abs_max_rows, abs_max_cols, scale_pow2;
// SolveOptions::equilibrate), gfx950.
//
// Three one-pass, memory-bound kernels over this rank's real rows x the columns c < n of a panel of
// fp64 / fp32.  A wave always touches a row in whole contiguous segments: lane i holds VW adjacent
// columns (one 16-byte access where the rows are 16-byte aligned, VW = 2 | 4; element accesses
// otherwise, VW = 1), so a wave instruction moves 64 VW consecutive elements of one row.
//
//   rmax   a wave per row (grid-stride over the rows), four segments of the row in flight, the 64
//          running maxima combined by a wave reduction, lane 0 stores out_nat[grow(r)]
//   cmax   grid (column strips of 64 VW, row slices): the four waves of a workgroup walk the slice's
//          rows 4 apart, four rows in flight each, every lane keeping the running maxima of its own
//          columns of ldexp(|x|, rexp[grow(r)]); the waves meet in LDS.  One slice: the result is
//          stored.  More: out is zeroed ahead of the launch and the slices meet in an integer maximum
//          of the bit patterns (non-negative doubles order like their bits) -- exact in any order,
//          so the result does not depend on the split; no floating-point atomic anywhere.
//   scale  a wave owns four consecutive rows and walks its column range once: the segment's column
//          exponents are loaded once for the four rows, x -> ldexp(x, rexp + cexp) in fp64
//          (v_ldexp_f64; an fp32 element is widened, scaled exactly and rounded once), stored in place
//          with the non-temporal policy by default (nothing reads the panel again soon: the rule of
//          rank_update.hip; set_equil_nt switches it for measurements).
//
// In both maxima a NaN or an Inf entry counts as +Inf (Device contract), so no NaN ever enters a
// comparison.  Masks, not assumptions: padding rows (local row >= the real rows, a prefix), columns
// >= n and the exponent entries of other ranks' rows are never loaded, and scale writes nothing
// outside the real rows x n columns.  Rows are addressed with 64-bit offsets; the element offset
// inside a row is 32-bit (the launch refuses an n that does not fit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "skinny.hpp"
#include "wave_ops.hpp"

namespace gj {
namespace kern {

namespace {

constexpr int kEqWaves = 4;  // waves per workgroup
constexpr int kEqUnroll = 4; // row segments (rmax) / rows (cmax, scale) a wave keeps in flight

template <typename T, int VW>
using eq_vec_t = std::conditional_t<VW == 1, T, typename SkinnyMfma<T>::vec_t>;

// |x| as a key of the maxima: NaN and Inf count as +Inf
__device__ __forceinline__ double eq_mag(double x) {
  const double v = fabs(x), inf = __longlong_as_double(0x7ff0000000000000ll);
  return v < inf ? v : inf;
}
__device__ __forceinline__ double eq_max(double a, double b) { return a > b ? a : b; }  // (no NaN operand)

// The VW elements at row[c ..] widened, 0 where the column is >= n (whole = all VW are below n: one access).
template <typename T, int VW, bool NT>
__device__ __forceinline__ void eq_load(const T* __restrict__ row, uint32_t c, uint32_t n, bool on, T (&x)[VW]) {
  if constexpr (VW == 1) {
    x[0] = (on && c < n) ? (NT ? __builtin_nontemporal_load(row + c) : row[c]) : T(0);
  } else {
    using vec_t = eq_vec_t<T, VW>;
    if (on && c + VW <= n) {
      const vec_t v = NT ? __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(row + c))
                         : *reinterpret_cast<const vec_t*>(row + c);
#pragma unroll
      for (int e = 0; e < VW; ++e) x[e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < VW; ++e) x[e] = (on && c + e < n) ? row[c + e] : T(0);
    }
  }
}

__device__ __forceinline__ int64_t eq_grow(int64_t r, int64_t m, int64_t p, int64_t rk) {
  return ((r / m) * p + rk) * m + r % m;
}

// ---- rmax
template <typename T, int VW>
__global__ __launch_bounds__(64 * kEqWaves) void eq_rmax_kernel(const T* __restrict__ X, int64_t ldx, int64_t real,
                                                                uint32_t n, int64_t m, int64_t p, int64_t rk,
                                                                double* __restrict__ out_nat) {
  constexpr uint32_t CH = 64 * VW;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * kEqWaves;
  for (int64_t r = (int64_t)blockIdx.x * kEqWaves + wave; r < real; r += nw) {  // wave-uniform
    const T* row = X + r * ldx;
    double mx = 0.0;
    uint32_t c0 = 0;
    for (; c0 + kEqUnroll * CH <= n; c0 += kEqUnroll * CH) {  // whole segments: no mask
      T x[kEqUnroll][VW];
#pragma unroll
      for (int u = 0; u < kEqUnroll; ++u) eq_load<T, VW, false>(row, c0 + u * CH + lane * VW, n, true, x[u]);
#pragma unroll
      for (int u = 0; u < kEqUnroll; ++u)
#pragma unroll
        for (int e = 0; e < VW; ++e) mx = eq_max(mx, eq_mag((double)x[u][e]));
    }
    for (; c0 < n; c0 += CH) {
      T x[VW];
      eq_load<T, VW, false>(row, c0 + lane * VW, n, true, x);  // a masked element is 0: the maximum's identity
#pragma unroll
      for (int e = 0; e < VW; ++e) mx = eq_max(mx, eq_mag((double)x[e]));
    }
    mx = wave_max_f64(mx);
    if (lane == 0) out_nat[eq_grow(r, m, p, rk)] = mx;
  }
}

// ---- cmax
template <typename T, int VW>
__global__ __launch_bounds__(64 * kEqWaves) void eq_cmax_kernel(const T* __restrict__ X, int64_t ldx, int64_t real,
                                                                uint32_t n, int64_t m, int64_t p, int64_t rk,
                                                                const int32_t* __restrict__ rexp_nat,
                                                                double* __restrict__ out, int64_t rchunk) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t c = (blockIdx.x * 64 + lane) * VW;  // this lane's columns
  const int64_t rbeg = (int64_t)blockIdx.y * rchunk;
  const int64_t rend = rbeg + rchunk < real ? rbeg + rchunk : real;
  double mx[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) mx[e] = 0.0;
  for (int64_t r0 = rbeg + wave; r0 < rend; r0 += kEqWaves * kEqUnroll) {  // wave-uniform
    T x[kEqUnroll][VW];
    int ex[kEqUnroll];
#pragma unroll
    for (int u = 0; u < kEqUnroll; ++u) {
      const int64_t r = r0 + u * kEqWaves;
      const bool on = r < rend;
      eq_load<T, VW, false>(X + (on ? r : rbeg) * ldx, c, n, on, x[u]);
      // (clamped: the scaled value saturates long before, and the sum below cannot wrap)
      ex[u] = (on && rexp_nat) ? max(-100000, min(100000, rexp_nat[eq_grow(r, m, p, rk)])) : 0;
    }
#pragma unroll
    for (int u = 0; u < kEqUnroll; ++u)
#pragma unroll
      for (int e = 0; e < VW; ++e) mx[e] = eq_max(mx[e], ldexp(eq_mag((double)x[u][e]), ex[u]));  // overflow: +Inf
  }
  __shared__ double sh[kEqWaves][64 * VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) sh[wave][lane * VW + e] = mx[e];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    double v = mx[e];
#pragma unroll
    for (int w = 1; w < kEqWaves; ++w) v = eq_max(v, sh[w][lane * VW + e]);
    if (c + e < n) {
      if (gridDim.y == 1) out[c + e] = v;
      else atomicMax(reinterpret_cast<unsigned long long*>(out) + (c + e), (unsigned long long)__double_as_longlong(v));
    }
  }
}

// ---- scale
template <typename T, int VW, bool NT>
__global__ __launch_bounds__(64 * kEqWaves) void eq_scale_kernel(T* __restrict__ X, int64_t ldx, int64_t real,
                                                                 uint32_t n, int64_t m, int64_t p, int64_t rk,
                                                                 const int32_t* __restrict__ rexp_nat,
                                                                 const int32_t* __restrict__ cexp, uint32_t cchunk) {
  constexpr uint32_t CH = 64 * VW;
  using vec_t = eq_vec_t<T, VW>;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t cbeg = blockIdx.y * cchunk;  // a multiple of CH
  const uint32_t cend = cbeg + cchunk < n ? cbeg + cchunk : n;
  const bool cexp_vec = VW > 1 && cexp && reinterpret_cast<uintptr_t>(cexp) % (4 * VW) == 0;
  const int64_t ngroups = (real + kEqUnroll - 1) / kEqUnroll;  // groups of kEqUnroll consecutive rows, one per wave
  for (int64_t g = (int64_t)blockIdx.x * kEqWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kEqWaves) {
    T* row[kEqUnroll];
    bool on[kEqUnroll];
    int er[kEqUnroll];
#pragma unroll
    for (int u = 0; u < kEqUnroll; ++u) {
      const int64_t r = g * kEqUnroll + u;
      on[u] = r < real;
      row[u] = X + (on[u] ? r : 0) * ldx;
      er[u] = (on[u] && rexp_nat) ? max(-100000, min(100000, rexp_nat[eq_grow(r, m, p, rk)])) : 0;
    }
    for (uint32_t c = cbeg + lane * VW; c < cend; c += CH) {
      const bool whole = c + VW <= n;
      int ec[VW];
      if (cexp_vec && whole) {
        typedef int ivec_t __attribute__((ext_vector_type(VW)));
        const ivec_t v = *reinterpret_cast<const ivec_t*>(cexp + c);
#pragma unroll
        for (int e = 0; e < VW; ++e) ec[e] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) ec[e] = (cexp && c + e < n) ? cexp[c + e] : 0;
      }
#pragma unroll
      for (int e = 0; e < VW; ++e) ec[e] = max(-100000, min(100000, ec[e]));
      T x[kEqUnroll][VW];
#pragma unroll
      for (int u = 0; u < kEqUnroll; ++u) eq_load<T, VW, NT>(row[u], c, n, on[u], x[u]);
#pragma unroll
      for (int u = 0; u < kEqUnroll; ++u) {
        if (!on[u]) continue;
        T y[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) y[e] = (T)ldexp((double)x[u][e], er[u] + ec[e]);  // exact in fp64, one rounding
        if constexpr (VW == 1) {
          if (whole) {
            if (NT) __builtin_nontemporal_store(y[0], row[u] + c);
            else row[u][c] = y[0];
          }
        } else {
          if (whole) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < VW; ++e) v[e] = y[e];
            if (NT) __builtin_nontemporal_store(v, reinterpret_cast<vec_t*>(row[u] + c));
            else *reinterpret_cast<vec_t*>(row[u] + c) = v;
          } else {
#pragma unroll
            for (int e = 0; e < VW; ++e)
              if (c + e < n) row[u][c + e] = y[e];
          }
        }
      }
    }
  }
}

int g_eq_col_split = 0;  // set_equil_col_split
int g_eq_nt = 1;         // set_equil_nt

struct EqArgs {
  int64_t real;
  bool vec;
};

EqArgs eq_args(const char* op, DType dt, const void* X, int64_t ldx, const Layout& L) {
  const int64_t es = (int64_t)dtype_size(dt);
  // element offsets inside a row are 32-bit (a segment past the end included)
  if (ldx < 0 || L.n < 0 || L.n > (int64_t(1) << 31) / es - 4 * 64 * 4)
    throw Error(Status::BadArgs, std::string(op) + ": a row of n elements does not fit 32-bit offsets");
  EqArgs a;
  a.real = L.real_rows();
  a.vec = rows_16B_aligned(X, ldx, (size_t)es);
  set_probe_name<struct EqProbe>(g_last_equil_kernel, "eq:%s:%s:%s", op, dt == DType::F64 ? "f64" : "f32",
                                 a.vec ? "vec" : "scalar");
  return a;
}

// f(T, VW) for the dtype and the load width of this launch
template <typename F>
void eq_dispatch(DType dt, bool vec, F&& f) {
  if (dt == DType::F64) {
    if (vec) f(double{}, std::integral_constant<int, 2>{});
    else f(double{}, std::integral_constant<int, 1>{});
  } else {
    if (vec) f(float{}, std::integral_constant<int, 4>{});
    else f(float{}, std::integral_constant<int, 1>{});
  }
}

}  // namespace

void set_equil_col_split(int s) { g_eq_col_split = s < 0 ? 0 : s; }
void set_equil_nt(int on) { g_eq_nt = on ? 1 : 0; }
const char* last_equil_kernel() { return g_last_equil_kernel; }

void abs_max_rows(DType dt, const void* X, int64_t ldx, const Layout& L, double* out_nat, hipStream_t s) {
  const EqArgs a = eq_args("rmax", dt, X, ldx, L);
  if (a.real <= 0 || L.n <= 0) return;
  // memory-bound: about four workgroups per CU, a wave per row
  const int64_t grid = std::min<int64_t>((a.real + kEqWaves - 1) / kEqWaves, 4 * (int64_t)num_cus());
  eq_dispatch(dt, a.vec, [&](auto t, auto VW) {
    using T = decltype(t);
    hipLaunchKernelGGL((eq_rmax_kernel<T, VW>), dim3((unsigned)grid), dim3(64 * kEqWaves), 0, s,
                       static_cast<const T*>(X), ldx, a.real, (uint32_t)L.n, L.m, L.p, L.k, out_nat);
  });
}

void abs_max_cols(DType dt, const void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, double* out,
                  hipStream_t s) {
  const EqArgs a = eq_args("cmax", dt, X, ldx, L);
  if (L.n <= 0) return;
  eq_dispatch(dt, a.vec, [&](auto t, auto VW) {
    using T = decltype(t);
    const int64_t strips = (L.n + 64 * VW - 1) / (64 * VW);
    int64_t S = g_eq_col_split;
    if (S <= 0) {
      // eight workgroups per CU, a slice of at least 16 rows per wave: a workgroup's last step is a
      // barrier and one store per column, so more, shorter slices hide each other's tails (N = 32768
      // fp64: 1756 us at four per CU, 1427 at eight, 1415 at sixteen; profiles/equilibrate.md)
      S = (8 * (int64_t)num_cus() + strips - 1) / strips;
      S = std::min<int64_t>(S, std::max<int64_t>(a.real / (16 * kEqWaves), 1));
    }
    S = std::max<int64_t>(1, std::min<int64_t>(S, 65535));
    const int64_t rchunk = std::max<int64_t>((a.real + S - 1) / S, 1);
    S = std::max<int64_t>((a.real + rchunk - 1) / rchunk, 1);  // no empty slice (a rank without rows: one, writing +0.0)
    if (S > 1) (void)hipMemsetAsync(out, 0, sizeof(double) * (size_t)L.n, s);  // +0.0: the integer maximum's identity
    hipLaunchKernelGGL((eq_cmax_kernel<T, VW>), dim3((unsigned)strips, (unsigned)S), dim3(64 * kEqWaves), 0, s,
                       static_cast<const T*>(X), ldx, a.real, (uint32_t)L.n, L.m, L.p, L.k, rexp_nat, out, rchunk);
  });
}

void scale_pow2(DType dt, void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, const int32_t* cexp,
                hipStream_t s) {
  const EqArgs a = eq_args("scale", dt, X, ldx, L);
  if (a.real <= 0 || L.n <= 0) return;
  eq_dispatch(dt, a.vec, [&](auto t, auto VW) {
    using T = decltype(t);
    constexpr int64_t CH = 64 * VW;
    const int64_t rtiles = (a.real + kEqWaves * kEqUnroll - 1) / (kEqWaves * kEqUnroll);
    const int64_t want = 4 * (int64_t)num_cus();  // about four workgroups per CU
    const int64_t gx = std::min<int64_t>(rtiles, want);
    // few rows: split the columns, in whole segments
    const int64_t segs = (L.n + CH - 1) / CH;
    const int64_t S = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((want + gx - 1) / gx, segs), 65535));
    const int64_t cchunk = ((segs + S - 1) / S) * CH;
    const int64_t gy = (L.n + cchunk - 1) / cchunk;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(64 * kEqWaves);
    if (g_eq_nt)
      hipLaunchKernelGGL((eq_scale_kernel<T, VW, true>), grid, block, 0, s, static_cast<T*>(X), ldx, a.real,
                         (uint32_t)L.n, L.m, L.p, L.k, rexp_nat, cexp, (uint32_t)cchunk);
    else
      hipLaunchKernelGGL((eq_scale_kernel<T, VW, false>), grid, block, 0, s, static_cast<T*>(X), ldx, a.real,
                         (uint32_t)L.n, L.m, L.p, L.k, rexp_nat, cexp, (uint32_t)cchunk);
  });
}

}  // namespace kern
}  // namespace gj
