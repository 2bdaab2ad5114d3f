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
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

// LDS row padding of V (elements): the 4 K lanes of a B-fragment read sit W rows apart; W * pitch =
// 128 (mod 256) bytes in fp64 (pad 8), 64 (mod 256) bytes in fp32 (pad 4), spreads them over the banks
template <typename T>
constexpr int kRhsLdsPad = sizeof(T) == 8 ? 8 : 4;

// Pass 1.  W = elements each lane loads per row and K step (1: element loads, any alignment;
// SkinnyMfma<T>::W: one 16-byte load, rows and K-slices 16-byte aligned).  A K step covers 4 W
// columns: lane (i = lane % 16, g = lane / 16) holds P[row i][kb + g W + j], j < W, and the j-th
// MFMA of the step multiplies the columns {kb + g W + j : g < 4} -- any assignment of K indices to
// the 4 MFMA K lanes is a valid product as long as the B operand uses the same one.
//
// V goes through LDS in chunks of kRhsKC rows, converted to T once per workgroup (every wave of a
// workgroup needs the same rows of V: without the staging each wave fetched them from L2 itself, four
// times the bytes of P at 64 columns).  Two buffers, one barrier per chunk: chunk c + 1 is fetched
// into registers before chunk c is multiplied and written to the other buffer after it.
template <typename T, int NF, int W>
__global__ __launch_bounds__(64 * kRhsWaves) void panel_rhs_kernel(
    const T* __restrict__ P, int64_t ldp, int64_t rows, int64_t n, int64_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, const int32_t* __restrict__ active,
    double* __restrict__ part, int64_t rows_pad, int64_t kchunk, unsigned long long* colmax) {
  using MF = SkinnyMfma<T>;
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRhsWaves;
  constexpr int LDK = KW + kRhsLdsPad<T>;         // LDS row pitch (elements)
  constexpr int VPT = kRhsKC * KW / NT;           // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRhsKC / (4 * W);         // K steps per chunk
  static_assert(NT % KW == 0 && (kRhsKC * KW) % NT == 0 && kRhsKC % (4 * W) == 0, "chunk shape");
  __shared__ T vs[2][kRhsKC][LDK];
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
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = (T)vreg[q];
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
          const typename MF::vec_t v = *reinterpret_cast<const typename MF::vec_t*>(prow[mi] + kk);
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
        T b[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 * W + g * W + j][nf * 16 + i];
#pragma unroll
        for (int mi = 0; mi < kRhsMI; ++mi)
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::op(a[st][mi][j], b[nf], acc[mi][nf]);
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

template <typename T, int NF>
void launch_rhs(const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int k,
                const int32_t* active, double* part, const RhsPlan& pl, unsigned long long* colmax, bool vec,
                hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRhsWaves);
  if (vec)
    hipLaunchKernelGGL((panel_rhs_kernel<T, NF, SkinnyMfma<T>::W>), grid, block, 0, s, static_cast<const T*>(P), ldp,
                       L.rows, L.n, L.m, L.p, L.k, V, ldv, k, active, part, pl.rows_pad, pl.kchunk, colmax);
  else
    hipLaunchKernelGGL((panel_rhs_kernel<T, NF, 1>), grid, block, 0, s, static_cast<const T*>(P), ldp, L.rows,
                       L.n, L.m, L.p, L.k, V, ldv, k, active, part, pl.rows_pad, pl.kchunk, colmax);
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
    constexpr int NF = KW / 16;
    if (dt == DType::F64) launch_rhs<double, NF>(P, ldp, L, V, ldv, (int)k, active, part, pl, cm, vec, s);
    else launch_rhs<float, NF>(P, ldp, L, V, ldv, (int)k, active, part, pl, cm, vec, s);
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
