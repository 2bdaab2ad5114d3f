// Kernels of the extra-precise residual (Device::panel_rhs_dd; Engine::solve_rhs_block with precise),
// gfx950.
//
// panel_rhs_dd: Y = round_fp64(C_in - P V) with P a tall fp64 panel (rows x n) and V a skinny fp64
// block (n x k, k <= 64): the whole sum, C_in included, is carried as an unevaluated (hi, lo) pair
// and rounded once.  Dot2 of Ogita, Rump and Oishi: per term p = a v, e = fma(a, v, -p),
// (s, sigma) = TwoSum(s, p), lo += e + sigma.  The MFMA returns no error term, so this is vector fp64
// code; the error-free transforms need every operation as written, so contraction is off for the
// whole file and the fused multiply-add is spelled out (__builtin_fma).
//
//   pass 1  grid (row tiles of 64 R, S K-slices), 4 waves: a wave owns 16 R rows and all KW = 16 | 32
//           | 64 columns.  The lane map of skinny_rows_kernel: lane (i = lane % 16, g = lane / 16)
//           holds row i's elements P[row][kb + g W + j], j < W, of a K step of 4 W columns and
//           accumulates them against every column, a (hi, lo) pair per column and row in registers
//           (R = 2 rows per lane at 16 and 32 columns, 1 at 64: 256 accumulator registers).  The 4 K
//           lanes of a row are combined by a butterfly of double-double additions (the same bits in
//           all four) and the pair is stored to part[slice][row][col].
//   pass 2  pair = (C_in, 0) - sum_{slice} part in slice order by double-double additions, Y = hi + lo
//           rounded once, and the column maxima.
//
// P is the memory-bound operand: every element is read exactly once per launch, straight from HBM
// into registers (16-byte loads where the rows are 16-byte aligned, element loads otherwise), each
// wave its own rows; V goes through LDS as fp64, unrounded, in chunks staged once per workgroup: two
// buffers, one barrier per chunk.  The K-split is panel_rhs's plan (rhs_plan, set_rhs_splitk), the
// slices are summed in a fixed order and the column maximum is an integer maximum of bit patterns:
// two launches on the same inputs give the same bits, no floating-point value is accumulated with
// atomics.
//
// Masks, not assumptions: rows >= L.rows, local padding rows (global row >= n), K >= n, columns
// >= k and inactive columns are never loaded (their operand is 0).  Every term is computed from its
// two factors as they are, so a NaN of V reaches Y also through a zero of P.  Rows are addressed
// with 64-bit pointers: any leading dimension.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "skinny.hpp"

#pragma clang fp contract(off)

namespace gj {
namespace kern {

namespace {

// one term of Dot2: (s, lo) += a * v
__device__ __forceinline__ void dot2_step(double& s, double& lo, double a, double v) {
  const double p = a * v;
  const double e = __builtin_fma(a, v, -p);
  const double t = s + p;
  const double z = t - s;
  const double sigma = (s - (t - z)) + (p - z);
  s = t;
  lo += e + sigma;
}

// (ah, al) += (bh, bl): TwoSum of the heads, the tails added to its error, renormalised
__device__ __forceinline__ void dd_add(double& ah, double& al, double bh, double bl) {
  const double t = ah + bh;
  const double z = t - ah;
  double e = (ah - (t - z)) + (bh - z);
  e += al + bl;
  ah = t + e;
  al = e - (ah - t);
}

typedef double dd_t __attribute__((ext_vector_type(2)));  // (hi, lo)

template <int KW>
constexpr int dd_rows_per_lane() {
  return KW == 64 ? 1 : 2;
}

template <int NF, int W, int R>
__global__ __launch_bounds__(64 * kRhsWaves) void rhs_dd_kernel(
    const double* __restrict__ P, int64_t ldp, int64_t rows, int64_t n, int64_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, const int32_t* __restrict__ active, dd_t* __restrict__ part,
    int64_t rows_pad, int64_t kchunk, unsigned long long* colmax) {
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRhsWaves;
  constexpr int LDK = KW + 2;              // the 4 K lanes read rows W apart: 16 W bytes further on in the banks
  constexpr int VPT = kRhsKC * KW / NT;    // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRhsKC / (4 * W);  // K steps per chunk
  constexpr int TILE = 16 * R * kRhsWaves;
  static_assert(NT % KW == 0 && (kRhsKC * KW) % NT == 0 && kRhsKC % (4 * W) == 0, "chunk shape");
  __shared__ __attribute__((aligned(16))) double vs[2][kRhsKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  // the column maxima of the active columns start from 0 (pass 2 runs after this whole launch)
  if (colmax && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < k &&
      (!active || active[threadIdx.x] != 0))
    colmax[threadIdx.x] = 0ull;

  const int64_t r0 = (int64_t)blockIdx.x * TILE + wave * (16 * R);
  const double* prow[R];
  bool rv[R];
#pragma unroll
  for (int mi = 0; mi < R; ++mi) {
    const int64_t r = r0 + mi * 16 + i;
    rv[mi] = r < rows && ((r / m) * p + rk) * m + r % m < n;
    prow[mi] = P + (rv[mi] ? r : 0) * ldp;
  }
  const int64_t kbeg = (int64_t)blockIdx.y * kchunk;
  const int64_t kend = kbeg + kchunk < n ? kbeg + kchunk : n;

  // staging: this thread's column of V and its rows of a chunk (row vr0 + q * (NT / KW))
  const int vc = threadIdx.x % KW, vr0 = threadIdx.x / KW;
  const bool vcv = vc < k && (!active || active[vc] != 0);
  double vreg[VPT];
  auto fetch = [&](int64_t kb) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int64_t kr = kb + vr0 + q * (NT / KW);
      vreg[q] = (vcv && kr < kend) ? V[kr * ldv + vc] : 0.0;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = vreg[q];
  };

  double hi[R][KW], lo[R][KW];
#pragma unroll
  for (int mi = 0; mi < R; ++mi)
#pragma unroll
    for (int c = 0; c < KW; ++c) hi[mi][c] = lo[mi][c] = 0.0;

  // this lane's W elements of its R rows at K step `kk`; past the slice they are 0 and never used
  auto load_step = [&](double (&dst)[R][W], int64_t kk) {
#pragma unroll
    for (int mi = 0; mi < R; ++mi) {
      if (W > 1 && rv[mi] && kk + W <= kend) {
        const dd_t v = *reinterpret_cast<const dd_t*>(prow[mi] + kk);
        dst[mi][0] = v[0];
        dst[mi][W - 1] = v[W - 1];
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j) dst[mi][j] = (rv[mi] && kk + j < kend) ? prow[mi][kk + j] : 0.0;
      }
    }
  };

  fetch(kbeg);
  stage(0);
  __syncthreads();
  // P one K step ahead of the arithmetic (step STEPS of a chunk is step 0 of the next); the steps of
  // a chunk are a rolled loop, so that the accumulators and one step's operands are all that lives
  double anext[R][W];
  load_step(anext, kbeg + g * W);
  int buf = 0;
  for (int64_t kb = kbeg; kb < kend; kb += kRhsKC, buf ^= 1) {
    const bool more = kb + kRhsKC < kend;  // uniform over the workgroup
    if (more) fetch(kb + kRhsKC);
#pragma unroll 1
    for (int st = 0; st < STEPS; ++st) {
      double a[R][W];
#pragma unroll
      for (int mi = 0; mi < R; ++mi)
#pragma unroll
        for (int j = 0; j < W; ++j) a[mi][j] = anext[mi][j];
      load_step(anext, kb + (st + 1) * 4 * W + g * W);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double* vrow = &vs[buf][st * 4 * W + g * W + j][0];
#pragma unroll
        for (int c = 0; c < KW; c += 2) {
          const dd_t v = *reinterpret_cast<const dd_t*>(vrow + c);
#pragma unroll
          for (int mi = 0; mi < R; ++mi) {
            dot2_step(hi[mi][c], lo[mi][c], a[mi][j], v[0]);
            dot2_step(hi[mi][c + 1], lo[mi][c + 1], a[mi][j], v[1]);
          }
        }
      }
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // the 4 K lanes of a row, in a fixed order: (g0 + g1) + (g2 + g3), the same bits in all four (a
  // double-double addition is commutative); the lanes g = 0 store.  rows_pad is a whole number of
  // tiles: no row mask
  dd_t* out = part + ((int64_t)blockIdx.y * rows_pad + r0 + i) * KW;
#pragma unroll
  for (int mi = 0; mi < R; ++mi)
#pragma unroll
    for (int c = 0; c < KW; ++c) {
      double h = hi[mi][c], l = lo[mi][c];
      dd_add(h, l, __shfl_xor(h, 16), __shfl_xor(l, 16));
      dd_add(h, l, __shfl_xor(h, 32), __shfl_xor(l, 32));
      if (g == 0) out[(int64_t)mi * 16 * KW + c] = dd_t{h, l};
    }
}

// Pass 2: Y = round(C_in - sum_{slice} part) on the active columns c < k of the rows < rows, and the
// maxima of |Y| over the rows that count (global row < n), as keys into colmax.  A padded local row
// keeps C_in (or 0).  A workgroup covers rpb rows x KW columns (thread = column tid % KW, row group
// tid / KW).
template <int KW>
__global__ __launch_bounds__(256) void rhs_dd_epilogue_kernel(const dd_t* __restrict__ part, int S, int64_t rows_pad,
                                                              int64_t n, int64_t m, int64_t p, int64_t rk,
                                                              const double* C_in, int64_t ldc, double* Y, int64_t ldy,
                                                              int64_t rows, int k, const int32_t* __restrict__ active,
                                                              unsigned long long* colmax, int rpb) {
  constexpr int RG = 256 / KW;
  const int c = threadIdx.x % KW, rs = threadIdx.x / KW;
  const bool on = c < k && (!active || active[c] != 0);
  const int64_t base = (int64_t)blockIdx.x * rpb;
  const int64_t end = base + rpb < rows ? base + rpb : rows;
  unsigned long long key = 0ull;
  if (on)
    for (int64_t r = base + rs; r < end; r += RG) {
      double y = C_in ? C_in[r * ldc + c] : 0.0;
      if (((r / m) * p + rk) * m + r % m < n) {
        double h = y, l = 0.0;
        for (int s = 0; s < S; ++s) {
          const dd_t t = part[((int64_t)s * rows_pad + r) * KW + c];
          dd_add(h, l, -t[0], -t[1]);
        }
        y = h + l;
        const unsigned long long kk = nonneg_key(fabs(y));
        key = kk > key ? kk : key;
      }
      Y[r * ldy + c] = y;
    }
  if (colmax) block_key_max<KW>(key, on, colmax);  // uniform
}

}  // namespace

const char* last_rhs_dd_kernel() { return g_last_rhs_dd_kernel; }

size_t panel_rhs_dd_scratch_bytes(const Layout& L, int64_t k) {
  const RhsPlan pl = rhs_plan(L);
  return sizeof(dd_t) * (size_t)pl.S * (size_t)pl.rows_pad * padded_kw(k);
}

void panel_rhs_dd(const double* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                  const double* C_in, int64_t ldc, double* Y, int64_t ldy, const int32_t* active, double* colmax,
                  void* scratch, hipStream_t s) {
  const RhsPlan pl = rhs_plan(L);
  // 16-byte loads of P need 16-byte aligned rows; the K-slices start on multiples of 16 columns
  const bool vec = rows_16B_aligned(P, ldp, sizeof(double));
  dd_t* part = static_cast<dd_t*>(scratch);
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  set_probe_name<struct RhsDdProbe>(g_last_rhs_dd_kernel, "rhsdd%d:f64:%s:s%d", padded_kw(k), vec ? "vec" : "scalar",
                                    pl.S);
  with_kw(k, [&](auto KW) {
    constexpr int NF = KW / 16, R = dd_rows_per_lane<KW>();
    // rows_pad is a multiple of kRhsTileM = 128 rows, hence of this kernel's tile of 64 R
    const dim3 grid((unsigned)(pl.rows_pad / (16 * R * kRhsWaves)), (unsigned)pl.S), block(64 * kRhsWaves);
    with_panel(DType::F64, vec, [&](auto zero, auto W) {
      if constexpr (std::is_same_v<decltype(zero), double>)  // (with_panel names fp32's widths too)
        hipLaunchKernelGGL((rhs_dd_kernel<NF, W, R>), grid, block, 0, s, P, ldp, L.rows, L.n, L.m, L.p, L.k, V, ldv,
                           (int)k, active, part, pl.rows_pad, pl.kchunk, cm);
    });
    const int rpb = 4 * (256 / KW);
    const unsigned eg = (unsigned)std::max<int64_t>((L.rows + rpb - 1) / rpb, 1);
    hipLaunchKernelGGL((rhs_dd_epilogue_kernel<KW>), dim3(eg), dim3(256), 0, s, part, pl.S, pl.rows_pad, L.n, L.m, L.p,
                       L.k, C_in, ldc, Y, ldy, L.rows, (int)k, active, cm, rpb);
  });
}

}  // namespace kern
}  // namespace gj
