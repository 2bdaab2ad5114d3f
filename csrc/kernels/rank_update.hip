// Kernel of the low-rank update of a resident panel (Device::rank_update; Engine::update_inverse),
// gfx950.
//
// rank_update: X[r][c] = round(X[r][c] + sign * sum_{j<k} W[wrow(r)][j] Z[c][j]) over this rank's real
// rows and the columns c < n, with W (rows x k) and Z (n x k) skinny fp64 blocks, k <= 64, and X a
// tall panel of fp64 / fp32.  X is the memory-bound operand: one pass, every element read once and
// written once with the non-temporal policy (nothing reads it again soon: the trailing update's
// rule for C, profiles/gemm_cache_policy_r6.md); W and Z stay in L2.
//
//   grid (row tiles of 64, column splits): a wave owns 16 rows (one MFMA row fragment) and keeps
//   their rows of W in registers as v_mfma_f64_16x16x4_f64 A operands, k padded to whole steps of 4
//   with zeros.  A workgroup walks its column tiles of 64; per tile Z's 64 rows go through LDS once
//   for the four waves (fetched one tile ahead), the wave loads its 16 x 64 piece of X, forms the
//   fp64 product from LDS while those loads are in flight, adds, rounds once and stores.
//
// Both dtypes share the fp64 product; F32 differs in the widening load and the rounding store.  A
// column of the tile may sit on any B lane of the MFMA as long as Z's rows are staged by the same
// map, so a lane's VW fragments take VW adjacent columns and X moves in 16-byte pieces where its
// rows are 16-byte aligned (VW = 2 | 4); element loads otherwise (VW = 1).
//
// No atomics and no split of the k sum: an element is computed by one lane in one fixed order, so
// two launches give the same bits whatever the column split.
//
// Masks, not assumptions: padding rows (local row >= the real rows), columns >= n, W's and Z's
// columns >= k, Z's rows >= n and W's rows of padded local rows are never loaded, and X outside
// the real rows x n columns is neither read nor written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

constexpr int kRkuMI = 1;                           // 16-row fragments per wave
constexpr int kRkuWaves = 4;                        // waves per workgroup
constexpr int kRkuTileM = 16 * kRkuMI * kRkuWaves;  // 64 rows per workgroup
constexpr int kRkuNF = 4;                           // 16-column fragments per wave
constexpr int kRkuTileN = 16 * kRkuNF;              // 64 columns per tile

// Column (within a tile) of fragment f's B lane i: (f / VW) * 16 VW + VW i + f % VW, so a lane's VW
// fragments of a group sit side by side.
// KS = K steps of 4 the build holds (k <= 4 KS); ks = the steps this launch runs (uniform).
// Two workgroups per CU at the least (the register bound of the k = 64 build): a tile's loads and
// stores overlap with another workgroup's matrix work.
template <typename T, int KS, int VW>
__global__ __launch_bounds__(64 * kRkuWaves, 2) void rank_update_kernel(
    T* __restrict__ X, int64_t ldx, int64_t real, int64_t n, int64_t m, int64_t p, int64_t rk,
    const double* __restrict__ Wm, int64_t ldw, int w_natural, const double* __restrict__ Z, int64_t ldz, int k,
    int ks, double sign, int64_t ctiles) {
  constexpr int NT = 64 * kRkuWaves;
  constexpr int KW = 4 * KS;
  constexpr int LDK = KW + 4;  // LDS row pitch (doubles): the 16 rows of a B read, 4 K lanes each, spread over the banks
  constexpr int ZPT = kRkuTileN * KW / NT;  // elements of a Z tile per thread
  constexpr int ES = (int)sizeof(T);
  static_assert(NT % KW == 0 && (kRkuTileN * KW) % NT == 0, "Z tile shape");
  static_assert(kRkuNF % VW == 0, "fragment groups");
  using MF = SkinnyMfma<double>;  // both dtypes share the fp64 product
  using vec_t = std::conditional_t<VW == 1, T, typename SkinnyMfma<T>::vec_t>;  // a lane's piece of X
  __shared__ double zs[kRkuTileN][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  // A operands: this lane's row of W per fragment, one element per K step (0 beyond k and for a
  // padding row: its products are never stored)
  const int64_t rt0 = (int64_t)blockIdx.x * kRkuTileM;
  double a[kRkuMI][KS];
#pragma unroll
  for (int mi = 0; mi < kRkuMI; ++mi) {
    const int64_t r = rt0 + wave * (16 * kRkuMI) + mi * 16 + i;
    const bool rv = r < real;
    const int64_t wr = w_natural ? ((r / m) * p + rk) * m + r % m : r;
    const double* wp = Wm + (rv ? wr : 0) * ldw;
#pragma unroll
    for (int st = 0; st < KS; ++st) a[mi][st] = (rv && st < ks && 4 * st + g < k) ? wp[4 * st + g] : 0.0;
  }

  // C rows of this lane: fragment mi, q -> tile row (wave * kRkuMI + mi) * 16 + g + 4 q; byte offsets
  // within the tile fit 32 bits (the launch refuses a leading dimension where they would not)
  bool xrv[kRkuMI][4];
  uint32_t xro[kRkuMI][4];
#pragma unroll
  for (int mi = 0; mi < kRkuMI; ++mi)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tr = wave * (16 * kRkuMI) + mi * 16 + g + 4 * q;
      xrv[mi][q] = rt0 + tr < real;
      xro[mi][q] = (uint32_t)tr * (uint32_t)ldx * ES;
    }

  // staging: this thread's K column of Z and its rows of a tile (LDS row = fragment f * 16 + lane i)
  const int zj = threadIdx.x % KW, zc0 = threadIdx.x / KW;
  const bool zjv = zj < k;

  // Z's rows of a tile are fetched into registers one tile ahead, under the previous tile's MFMAs
  double zreg[ZPT];
  auto fetch_z = [&](int64_t ct) {
#pragma unroll
    for (int q = 0; q < ZPT; ++q) {
      const int64_t c = ct * kRkuTileN + zc0 + q * (NT / KW);
      zreg[q] = (zjv && ct < ctiles && c < n) ? Z[c * ldz + zj] : 0.0;
    }
  };
  fetch_z(blockIdx.y);

  for (int64_t ct = blockIdx.y; ct < ctiles; ct += gridDim.y) {
    const int64_t c0 = ct * kRkuTileN;
    char* xt = reinterpret_cast<char*>(X + rt0 * ldx + c0);

    // this lane's piece of X: VW adjacent columns per group and row
    vec_t xin[kRkuMI][4][kRkuNF / VW];
#pragma unroll
    for (int gr = 0; gr < kRkuNF / VW; ++gr) {
      const uint32_t cc = gr * 16 * VW + VW * i;
      const bool full = c0 + cc + VW <= n;
#pragma unroll
      for (int mi = 0; mi < kRkuMI; ++mi)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const T* src = reinterpret_cast<const T*>(xt + xro[mi][q] + cc * ES);
          if constexpr (VW == 1) {
            xin[mi][q][gr] = (xrv[mi][q] && full) ? __builtin_nontemporal_load(src) : T(0);
          } else {
            vec_t v;
            if (xrv[mi][q] && full) {
              v = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(src));
            } else {
#pragma unroll
              for (int e = 0; e < VW; ++e)
                v[e] = (xrv[mi][q] && c0 + cc + e < n) ? __builtin_nontemporal_load(src + e) : T(0);
            }
            xin[mi][q][gr] = v;
          }
        }
    }

    __syncthreads();  // the previous tile's B reads are done
#pragma unroll
    for (int q = 0; q < ZPT; ++q) {
      const int cc = zc0 + q * (NT / KW);  // tile column -> its fragment and lane
      const int grp = cc / (16 * VW), rem = cc % (16 * VW);
      zs[(grp * VW + rem % VW) * 16 + rem / VW][zj] = zreg[q];
    }
    __syncthreads();
    fetch_z(ct + gridDim.y);

    MF::acc_t acc[kRkuMI][kRkuNF];
#pragma unroll
    for (int mi = 0; mi < kRkuMI; ++mi)
#pragma unroll
      for (int f = 0; f < kRkuNF; ++f) acc[mi][f] = MF::acc_t{0, 0, 0, 0};
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      if (st < ks) {  // uniform
        double b[kRkuNF];
#pragma unroll
        for (int f = 0; f < kRkuNF; ++f) b[f] = zs[f * 16 + i][4 * st + g];
#pragma unroll
        for (int mi = 0; mi < kRkuMI; ++mi)
#pragma unroll
          for (int f = 0; f < kRkuNF; ++f) acc[mi][f] = MF::op(a[mi][st], b[f], acc[mi][f]);
      }
    }

    // widen, add, round once, store
#pragma unroll
    for (int gr = 0; gr < kRkuNF / VW; ++gr) {
      const uint32_t cc = gr * 16 * VW + VW * i;
      const bool full = c0 + cc + VW <= n;
#pragma unroll
      for (int mi = 0; mi < kRkuMI; ++mi)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!xrv[mi][q]) continue;
          T* dst = reinterpret_cast<T*>(xt + xro[mi][q] + cc * ES);
          if constexpr (VW == 1) {
            if (full) __builtin_nontemporal_store((T)((double)xin[mi][q][gr] + sign * acc[mi][gr][q]), dst);
          } else {
            vec_t v;
#pragma unroll
            for (int e = 0; e < VW; ++e) v[e] = (T)((double)xin[mi][q][gr][e] + sign * acc[mi][gr * VW + e][q]);
            if (full) {
              __builtin_nontemporal_store(v, reinterpret_cast<vec_t*>(dst));
            } else {
#pragma unroll
              for (int e = 0; e < VW; ++e)
                if (c0 + cc + e < n) __builtin_nontemporal_store((T)v[e], dst + e);
            }
          }
        }
    }
  }
}

template <typename T, int KS, int VW>
void launch_rku(void* X, int64_t ldx, int64_t real, const Layout& L, const double* W, int64_t ldw, bool w_natural,
                const double* Z, int64_t ldz, int k, double sign, hipStream_t s) {
  const int64_t rtiles = (real + kRkuTileM - 1) / kRkuTileM;
  const int64_t ctiles = (L.n + kRkuTileN - 1) / kRkuTileN;
  // memory-bound: about four workgroups per CU in flight; a workgroup keeps its rows of W in
  // registers over all of its column tiles
  int64_t S = (4 * (int64_t)num_cus() + rtiles - 1) / rtiles;
  S = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S, ctiles), 65535));
  const dim3 grid((unsigned)rtiles, (unsigned)S), block(64 * kRkuWaves);
  hipLaunchKernelGGL((rank_update_kernel<T, KS, VW>), grid, block, 0, s, static_cast<T*>(X), ldx, real, L.n, L.m,
                     L.p, L.k, W, ldw, w_natural ? 1 : 0, Z, ldz, k, (k + 3) / 4, sign, ctiles);
}

template <typename T, int VW>
void launch_rku_k(void* X, int64_t ldx, int64_t real, const Layout& L, const double* W, int64_t ldw, bool w_natural,
                  const double* Z, int64_t ldz, int k, double sign, hipStream_t s) {
  if (k <= 4) launch_rku<T, 1, VW>(X, ldx, real, L, W, ldw, w_natural, Z, ldz, k, sign, s);
  else if (k <= 16) launch_rku<T, 4, VW>(X, ldx, real, L, W, ldw, w_natural, Z, ldz, k, sign, s);
  else if (k <= 32) launch_rku<T, 8, VW>(X, ldx, real, L, W, ldw, w_natural, Z, ldz, k, sign, s);
  else launch_rku<T, 16, VW>(X, ldx, real, L, W, ldw, w_natural, Z, ldz, k, sign, s);
}

}  // namespace

const char* last_rank_update_kernel() { return g_last_rank_update_kernel; }

void rank_update(DType dt, void* X, int64_t ldx, const Layout& L, const double* W, int64_t ldw, bool w_natural,
                 const double* Z, int64_t ldz, int64_t k, double sign, hipStream_t s) {
  const int64_t es = (int64_t)dtype_size(dt);
  // a tile's rows are addressed from the tile's base with 32-bit byte offsets
  check_ld_32bit("rank_update", ldx, es, kRkuTileM, kRkuTileN);
  const int64_t real = L.real_rows();
  // 16-byte pieces of X need 16-byte aligned rows; a lane's columns start on a multiple of the width
  const bool vec = rows_16B_aligned(X, ldx, (size_t)es);
  set_probe_name<struct RkuProbe>(g_last_rank_update_kernel, "rku%d:%s:%s", (int)((k + 3) / 4 * 4),
                                  dt == DType::F64 ? "f64" : "f32", vec ? "vec" : "scalar");
  if (real <= 0 || L.n <= 0) return;
  with_panel(dt, vec, [&](auto zero, auto VW) {
    launch_rku_k<decltype(zero), VW>(X, ldx, real, L, W, ldw, w_natural, Z, ldz, (int)k, sign, s);
  });
}

}  // namespace kern
}  // namespace gj
