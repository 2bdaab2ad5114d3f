// Pass 1 of the streaming skinny products: P V over row tiles (skinny_rows_kernel: panel_rhs.hip and
// its sibling of absolute values in panel_abs.hip) and P^T V_loc over column tiles (skinny_cols_kernel:
// panel_rhs_t.hip and its sibling).  One body per product; an arithmetic policy carries what differs
// between a product and its sibling and nothing that could reorder a floating-point operation:
//
//   T, MF            the panel's element type and the MFMA traits (MF::elem_t is the LDS element type)
//   stage(double v)  an element of V on its way into LDS
//   operand(T a)     an element of P on its way into the MFMA
//   rows_pad(W, kw)  LDS row padding of V (elements) in the rows kernel
//   cols_pad(kw)     the same in the cols kernel; both measured against bank conflicts per family
//   kRowOffsets32    the cols kernel addresses the rows of a chunk with 32-bit byte offsets from the
//                    chunk's base (fewer registers; the launcher must refuse a leading dimension where
//                    they would not fit) instead of 64-bit row addresses; the rows kernel always uses
//                    the latter (profiles/skinny_stream.md)
//
// P is the memory-bound operand: every element is read exactly once per launch, straight from HBM
// into registers (W elements per lane and load: 1 = element loads, any alignment; 16 / sizeof(T) =
// one 16-byte load, rows 16-byte aligned); V stays in L2 and goes through LDS in chunks, staged once
// per workgroup (every wave of a workgroup needs the same rows of V: without the staging each wave
// fetched them from L2 itself, four times the bytes of P at 64 columns).  Two buffers, one barrier
// per chunk: chunk c + 1 is fetched into registers before chunk c is multiplied and written to the
// other buffer after it.  A workgroup stores the partial product of its slice, widened to fp64; pass 2
// (skinny.hpp) sums the slices in a fixed order.
//
// Masked operands are never loaded and are 0: see the never-read set of each op in its .hip file.
#pragma once

#include "skinny.hpp"

namespace gj {
namespace kern {

// The plain product: V rounded to T while staging, P as loaded, v_mfma_{f64,f32}_16x16x4.
template <typename T_>
struct PlainArith {
  using T = T_;
  using MF = SkinnyMfma<T>;
  static __device__ __forceinline__ T stage(double v) { return (T)v; }
  static __device__ __forceinline__ T operand(T a) { return a; }
  // rows: the 4 K lanes of a B-fragment read sit W rows apart; W * pitch = 128 (mod 256) bytes in fp64
  // (pad 8), 64 (mod 256) bytes in fp32 (pad 4), spreads them over the banks
  static constexpr int rows_pad(int, int) { return sizeof(T) == 8 ? 8 : 4; }
  // cols: the 4 K lanes sit on consecutive rows.  fp64: pitch = 16 (mod 32) elements, 128 (mod 256)
  // bytes apart; fp32: pitch = 16 (mod 64) elements, 64 (mod 256) bytes apart
  static constexpr int cols_pad(int kw) { return kw == 16 ? 0 : (sizeof(T) == 4 && kw == 32) ? 48 : 16; }
  static constexpr bool kRowOffsets32 = false;  // any leading dimension
};

// W elements of a row of P
template <typename T, int W>
using Piece = T __attribute__((ext_vector_type(W)));

// Rows: grid (row tiles of kRhsTileM, K-slices of kchunk columns).  A wave owns 32 rows (two 16-row
// fragments) and NF = 1 | 2 | 4 column fragments of 16.  A K step covers 4 W columns: lane
// (i = lane % 16, g = lane / 16) holds P[row i][kb + g W + j], j < W, and the j-th MFMA of the step
// multiplies the columns {kb + g W + j : g < 4} -- any assignment of K indices to the 4 MFMA K lanes
// is a valid product as long as the B operand uses the same one.
template <typename Arith, int NF, int W>
__global__ __launch_bounds__(64 * kRhsWaves) void skinny_rows_kernel(
    const typename Arith::T* __restrict__ P, int64_t ldp, int64_t rows, int64_t n, int64_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, const int32_t* __restrict__ active,
    double* __restrict__ part, int64_t rows_pad, int64_t kchunk, unsigned long long* colmax) {
  using T = typename Arith::T;
  using MF = typename Arith::MF;
  using E = typename MF::elem_t;
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRhsWaves;
  constexpr int LDK = KW + Arith::rows_pad(W, KW);  // LDS row pitch (elements)
  constexpr int VPT = kRhsKC * KW / NT;             // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRhsKC / (4 * W);           // K steps per chunk
  static_assert(NT % KW == 0 && (kRhsKC * KW) % NT == 0 && kRhsKC % (4 * W) == 0, "chunk shape");
  __shared__ E vs[2][kRhsKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  // the column maxima of the active columns start from 0 (pass 2 runs after this whole launch)
  if (colmax && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < k &&
      (!active || active[threadIdx.x] != 0))
    colmax[threadIdx.x] = 0ull;

  const int64_t r0 = (int64_t)blockIdx.x * kRhsTileM + wave * (16 * kRhsMI);
  const T* prow[kRhsMI];
  bool rv[kRhsMI];
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi) {
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
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = Arith::stage(vreg[q]);
  };

  typename MF::acc_t acc[kRhsMI][NF];
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = typename MF::acc_t{0, 0, 0, 0};

  fetch(kbeg);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int64_t kb = kbeg; kb < kend; kb += kRhsKC, buf ^= 1) {
    const bool more = kb + kRhsKC < kend;  // uniform over the workgroup
    if (more) fetch(kb + kRhsKC);
    T a[STEPS][kRhsMI][W];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int64_t kk = kb + st * 4 * W + g * W;
#pragma unroll
      for (int mi = 0; mi < kRhsMI; ++mi) {
        if (W > 1 && rv[mi] && kk + W <= kend) {
          const Piece<T, W> v = *reinterpret_cast<const Piece<T, W>*>(prow[mi] + kk);
#pragma unroll
          for (int j = 0; j < W; ++j) a[st][mi][j] = v[j];
        } else {
#pragma unroll
          for (int j = 0; j < W; ++j) a[st][mi][j] = (rv[mi] && kk + j < kend) ? prow[mi][kk + j] : T(0);
        }
      }
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        E b[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 * W + g * W + j][nf * 16 + i];
#pragma unroll
        for (int mi = 0; mi < kRhsMI; ++mi) {
          const E av = Arith::operand(a[st][mi][j]);
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::op(av, b[nf], acc[mi][nf]);
        }
      }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // partial product of this K-slice, widened: rows_pad is a whole number of tiles, no row mask
  double* out = part + ((int64_t)blockIdx.y * rows_pad + r0) * KW;
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        out[(int64_t)(mi * 16 + MF::row(lane, q)) * KW + nf * 16 + i] = (double)acc[mi][nf][q];
}

// Cols: grid (column tiles of 64 W, row slices of rchunk local rows).  A wave owns 16 W columns of P
// and NF = 1 | 2 | 4 fragments of 16 columns of V.  A K step covers 4 local rows: lane (i = lane % 16,
// g = lane / 16) holds P[row + g][c0 + i W + j], j < W, and the j-th MFMA of the step produces the
// output rows {c0 + i W + j : i < 16} -- W interleaved column fragments from one load.  For
// D = P^T-fragment * V-fragment the 16 lanes of one MFMA K index hold 16 consecutive columns of one
// row of P, so a row-major P is read in whole contiguous segments.  The rows of V of a chunk are
// picked by the row map.  `real` = this rank's real local rows (global row < n), a prefix of its rows.
template <typename Arith, int NF, int W>
__global__ __launch_bounds__(64 * kRtWaves) void skinny_cols_kernel(
    const typename Arith::T* __restrict__ P, int64_t ldp, int64_t real, int64_t n, uint32_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, const int32_t* __restrict__ active,
    double* __restrict__ part, int64_t cols_pad, int64_t rchunk) {
  using T = typename Arith::T;
  using MF = typename Arith::MF;
  using E = typename MF::elem_t;
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRtWaves;
  constexpr int LDK = KW + Arith::cols_pad(KW);  // LDS row pitch (elements)
  constexpr int VPT = kRtKC * KW / NT;           // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRtKC / 4;               // K steps per chunk
  static_assert(NT % KW == 0 && (kRtKC * KW) % NT == 0 && kRtKC % 4 == 0, "chunk shape");
  __shared__ E vs[2][kRtKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  const int64_t cbase = ((int64_t)blockIdx.x * kRtWaves + wave) * (16 * W);  // this wave's columns of P
  const int64_t c0 = cbase + i * W;                                          // this lane's
  const bool cvec = c0 + W <= n;
  const int64_t rbeg = (int64_t)blockIdx.y * rchunk;
  const int64_t rend = rbeg + rchunk < real ? rbeg + rchunk : real;
  // Arith::kRowOffsets32: this lane's row of a K step as a byte offset from the chunk's first row
  // instead of a 64-bit address per row (the launch checks that the offsets fit 32 bits)
  uint32_t ro[STEPS];
  if constexpr (Arith::kRowOffsets32) {
#pragma unroll
    for (int st = 0; st < STEPS; ++st) ro[st] = (uint32_t)(st * 4 + g) * (uint32_t)ldp * (uint32_t)sizeof(T);
  }

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
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = Arith::stage(vreg[q]);
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
    const char* chunk = reinterpret_cast<const char*>(P + rb * ldp + c0);
    T a[STEPS][W];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int64_t r = rb + st * 4 + g;
      const T* src = P + r * ldp + c0;
      if constexpr (Arith::kRowOffsets32) src = reinterpret_cast<const T*>(chunk + ro[st]);
      if (W > 1 && cvec && r < rend) {
        const Piece<T, W> v = *reinterpret_cast<const Piece<T, W>*>(src);
#pragma unroll
        for (int j = 0; j < W; ++j) a[st][j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j) a[st][j] = (r < rend && c0 + j < n) ? src[j] : T(0);
      }
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      E b[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 + g][nf * 16 + i];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const E av = Arith::operand(a[st][j]);
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[j][nf] = MF::op(av, b[nf], acc[j][nf]);
      }
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

// Pass 1 of the product with arithmetic Arith<T> at column width KW, T and W picked by the panel's
// dtype and alignment (vec: 16-byte aligned rows; the K-slices start on multiples of 16 columns)
template <template <typename> class Arith, int KW>
inline void launch_skinny_rows(DType dt, bool vec, const void* P, int64_t ldp, const Layout& L, const double* V,
                               int64_t ldv, int k, const int32_t* active, double* part, const RhsPlan& pl,
                               unsigned long long* colmax, hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRhsWaves);
  with_panel(dt, vec, [&](auto zero, auto W) {
    using T = decltype(zero);
    hipLaunchKernelGGL((skinny_rows_kernel<Arith<T>, KW / 16, W>), grid, block, 0, s, static_cast<const T*>(P), ldp,
                       L.rows, L.n, L.m, L.p, L.k, V, ldv, k, active, part, pl.rows_pad, pl.kchunk, colmax);
  });
}

template <template <typename> class Arith, int KW>
inline void launch_skinny_cols(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                               int k, const int32_t* active, double* part, const RtPlan& pl, hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRtWaves);
  with_panel(dt, pl.vec, [&](auto zero, auto W) {
    using T = decltype(zero);
    hipLaunchKernelGGL((skinny_cols_kernel<Arith<T>, KW / 16, W>), grid, block, 0, s, static_cast<const T*>(P), ldp,
                       pl.real, L.n, (uint32_t)L.m, L.p, L.k, V, ldv, k, active, part, pl.cols_pad, pl.rchunk);
  });
}

}  // namespace kern
}  // namespace gj
