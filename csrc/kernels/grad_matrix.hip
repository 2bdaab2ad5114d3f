// Kernel of the gradient matrix of a resident inverse (Device::grad_matrix; Engine::grad_matrix and
// Engine::vjp_inverse), gfx950.
//
// grad_matrix: G[i][j] = (accumulate ? G[i][j] : 0) + alpha * P[j][i] + sign * sum_{c<k} W[i][c] Z[j][c]
// over i, j < n, with P an n x n panel of fp64 / fp32 that enters transposed, W and Z skinny fp64
// blocks (n x k, k <= 64) and G fp64.  G is the memory-bound operand: written once with the
// non-temporal policy (nothing reads it again soon: the trailing update's rule for C,
// profiles/gemm_cache_policy_r6.md; when accumulating it is read the same way); P is read with the
// plain policy, it stays resident; W and Z stay in L2.
//
//   grid (row tiles of 64, column splits): the product half is rank_update.hip's.  A wave owns 16
//   rows of G (one MFMA row fragment) and keeps their rows of W in registers as
//   v_mfma_f64_16x16x4_f64 A operands, k padded to whole steps of 4 with zeros; a workgroup walks
//   its column tiles of 64 and Z's 64 rows of a tile go through LDS once for the four waves.
//
//   The transposed operand: the tile of G at (i0, j0) needs the tile of P at (j0, i0).  It is loaded
//   along P's rows, widened and written to an LDS image pt[row of P][column of P] of pitch kLDP
//   doubles, and read back as pt[column of G][row of G], so that both the global load and the global
//   store run along rows.
//
//   Banks (cdna_hip_programming.md, section 2).  A ds_write_b64 takes 16 contiguous lanes at a
//   time over 32 banks of 4 bytes, i.e. 16 slots of one double: the 16 lanes must hit 16 different
//   slots.  A 16-lane group writes VP rows x 16 / VP pieces of VP doubles, element e of each in
//   one instruction, at the double index rsub * kLDP + VP * piece + e: with kLDP == 1 (mod 16) the
//   slots are rsub + VP * piece, all different.  (Element loads, VP = 1: 16 adjacent doubles.)
//   A ds_read_b64 takes 32 lanes over 64 banks, i.e. 32 slots: the lanes (i < 16, g < 2) read the
//   double index (VW * i + e) * kLDP + g + const; with VW = 2 and kLDP = 65 that is 2 i + g (mod
//   32), with VW = 1 and kLDP = 66 it is 2 i + g again (66 is even, which is harmless to the VP =
//   1 writes): all different.  So neither path has a bank conflict by construction.
//
// alpha == 0 (P never read), k == 0 (W and Z never read) and the dtype are builds; accumulate is a
// launch-uniform branch.  Both dtypes work in fp64; nothing is rounded to the panel's dtype.
//
// 16-byte pieces of P and G where both views have 16-byte aligned rows ("vec": G in pairs of
// doubles; P in pairs of doubles or fours of floats), element accesses otherwise ("scalar").
//
// No atomics and no split of the k sum: an element is computed by one lane in one fixed order, so
// two launches give the same bits whatever the column split.
//
// Masks, not assumptions: P's rows and columns >= n, W's and Z's rows >= n and columns >= k are
// never loaded, G outside n x n is neither read nor written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

constexpr int kGmWaves = 4;            // waves per workgroup, 16 rows of G each
constexpr int kGmTile = 16 * kGmWaves;  // 64 x 64 tiles
constexpr int kGmNF = 4;               // 16-column fragments per wave

// T: P's element type; KS: K steps of 4 the build holds (0: no product, W and Z never read);
// HASP: alpha != 0 (else P is never read); VEC: 16-byte pieces.
template <typename T, int KS, bool HASP, bool VEC>
__global__ __launch_bounds__(64 * kGmWaves, 2) void grad_matrix_kernel(
    const T* __restrict__ P, int64_t ldp, int64_t n, double alpha, const double* __restrict__ Wm, int64_t ldw,
    const double* __restrict__ Z, int64_t ldz, int k, int ks, double sign, int accumulate, double* __restrict__ G,
    int64_t ldg, int64_t ctiles) {
  constexpr int NT = 64 * kGmWaves;
  constexpr int VW = VEC ? 2 : 1;                      // doubles of G a lane moves at once
  constexpr int VP = VEC ? (int)(16 / sizeof(T)) : 1;  // elements of P a lane loads at once
  constexpr int KW = KS > 0 ? 4 * KS : 4;
  constexpr int LDK = KW + 4;              // pitch of Z's image (rank_update.hip)
  constexpr int kLDP = VEC ? 65 : 66;      // pitch of P's image: the bank argument above
  constexpr int ZPT = kGmTile * KW / NT;   // elements of a Z tile per thread
  constexpr int PPASS = 16 / VP;           // passes of the workgroup over P's tile
  constexpr int PCG = 16 / VP;             // pieces per row of a 16-lane group
  using MF = SkinnyMfma<double>;
  using pvec_t = std::conditional_t<VP == 1, T, typename SkinnyMfma<T>::vec_t>;
  using gvec_t = std::conditional_t<VW == 1, double, typename SkinnyMfma<double>::vec_t>;
  static_assert(NT % KW == 0 && (kGmTile * KW) % NT == 0, "Z tile shape");
  __shared__ double zs[KS > 0 ? kGmTile : 1][LDK];
  __shared__ double pt[HASP ? kGmTile : 1][kLDP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * kGmTile;

  // A operands: this lane's row of W, one element per K step (0 beyond k and for a row >= n)
  double a[KS > 0 ? KS : 1];
  if constexpr (KS > 0) {
    const int64_t r = i0 + wave * 16 + i;
    const bool rv = r < n;
    const double* wp = Wm + (rv ? r : 0) * ldw;
#pragma unroll
    for (int st = 0; st < KS; ++st) a[st] = (rv && st < ks && 4 * st + g < k) ? wp[4 * st + g] : 0.0;
  }

  // G rows of this lane: q -> tile row wave * 16 + g + 4 q; byte offsets within a tile fit 32 bits
  bool grv[4];
  uint32_t gro[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tr = wave * 16 + g + 4 * q;
    grv[q] = i0 + tr < n;
    gro[q] = (uint32_t)tr * (uint32_t)ldg * 8u;
  }

  // staging of Z: this thread's K column and its rows of a tile (LDS row = fragment f * 16 + lane i)
  const int zj = threadIdx.x % KW, zc0 = threadIdx.x / KW;
  const bool zjv = zj < k;

  // staging of P: a 16-lane group takes VP rows x PCG pieces of a tile; the workgroup's 16 groups
  // take 4 such units side by side (a whole row of 64) and 4 units down, PPASS times over
  const int l16 = threadIdx.x & 15, g16 = threadIdx.x >> 4;
  const int prow0 = (g16 >> 2) * VP + l16 / PCG;             // + pass * 4 VP
  const int pcol = ((g16 & 3) * PCG + l16 % PCG) * VP;       // first column of the piece
  const bool pcfull = i0 + pcol + VP <= n;

  for (int64_t ct = blockIdx.y; ct < ctiles; ct += gridDim.y) {
    const int64_t j0 = ct * kGmTile;

    // Z's rows of this tile and P's tile (rows j0 .., columns i0 ..) into registers
    double zreg[KS > 0 ? ZPT : 1];
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < ZPT; ++q) {
        const int64_t c = j0 + zc0 + q * (NT / KW);
        zreg[q] = (zjv && c < n) ? Z[c * ldz + zj] : 0.0;
      }
    }
    double preg[HASP ? PPASS : 1][VP];
    if constexpr (HASP) {
      const char* pb = reinterpret_cast<const char*>(P + j0 * ldp + i0);
#pragma unroll
      for (int ps = 0; ps < PPASS; ++ps) {
        const int pr = prow0 + ps * 4 * VP;
        const bool rv = j0 + pr < n;
        const T* src = reinterpret_cast<const T*>(pb + (uint32_t)pr * (uint32_t)ldp * (uint32_t)sizeof(T)) + pcol;
        if constexpr (VP == 1) {
          preg[ps][0] = (rv && pcfull) ? (double)*src : 0.0;
        } else {
          if (rv && pcfull) {
            const pvec_t v = *reinterpret_cast<const pvec_t*>(src);
#pragma unroll
            for (int e = 0; e < VP; ++e) preg[ps][e] = (double)v[e];
          } else {
#pragma unroll
            for (int e = 0; e < VP; ++e) preg[ps][e] = (rv && i0 + pcol + e < n) ? (double)src[e] : 0.0;
          }
        }
      }
    }

    // G's piece of this lane when accumulating: VW adjacent columns per group and row
    char* gt = reinterpret_cast<char*>(G + i0 * ldg + j0);
    gvec_t gin[4][kGmNF / VW];
    if (accumulate) {  // uniform
#pragma unroll
      for (int gr = 0; gr < kGmNF / VW; ++gr) {
        const uint32_t cc = gr * 16 * VW + VW * i;
        const bool full = j0 + cc + VW <= n;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double* src = reinterpret_cast<const double*>(gt + gro[q] + cc * 8u);
          if constexpr (VW == 1) {
            gin[q][gr] = (grv[q] && full) ? __builtin_nontemporal_load(src) : 0.0;
          } else {
            gvec_t v;
            if (grv[q] && full) {
              v = __builtin_nontemporal_load(reinterpret_cast<const gvec_t*>(src));
            } else {
#pragma unroll
              for (int e = 0; e < VW; ++e)
                v[e] = (grv[q] && j0 + cc + e < n) ? __builtin_nontemporal_load(src + e) : 0.0;
            }
            gin[q][gr] = v;
          }
        }
      }
    }

    __syncthreads();  // the previous tile's LDS reads are done
    if constexpr (KS > 0) {
#pragma unroll
      for (int q = 0; q < ZPT; ++q) {
        const int cc = zc0 + q * (NT / KW);  // tile column -> its fragment and lane
        const int grp = cc / (16 * VW), rem = cc % (16 * VW);
        zs[(grp * VW + rem % VW) * 16 + rem / VW][zj] = zreg[q];
      }
    }
    if constexpr (HASP) {
#pragma unroll
      for (int ps = 0; ps < PPASS; ++ps)
#pragma unroll
        for (int e = 0; e < VP; ++e) pt[prow0 + ps * 4 * VP][pcol + e] = preg[ps][e];
    }
    __syncthreads();

    MF::acc_t acc[kGmNF];
#pragma unroll
    for (int f = 0; f < kGmNF; ++f) acc[f] = MF::acc_t{0, 0, 0, 0};
    if constexpr (KS > 0) {
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        if (st < ks) {  // uniform
          double b[kGmNF];
#pragma unroll
          for (int f = 0; f < kGmNF; ++f) b[f] = zs[f * 16 + i][4 * st + g];
#pragma unroll
          for (int f = 0; f < kGmNF; ++f) acc[f] = MF::op(a[st], b[f], acc[f]);
        }
      }
    }

    // alpha * P^T + sign * sum (+ G), store
#pragma unroll
    for (int gr = 0; gr < kGmNF / VW; ++gr) {
      const uint32_t cc = gr * 16 * VW + VW * i;
      const bool full = j0 + cc + VW <= n;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!grv[q]) continue;
        const int tr = wave * 16 + g + 4 * q;
        double v[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          double x = 0.0;
          if constexpr (KS > 0) x = sign * acc[gr * VW + e][q];
          if constexpr (HASP) {
            const double t = alpha * pt[cc + e][tr];
            x = KS > 0 ? t + x : t;
          }
          if (accumulate) {
            if constexpr (VW == 1) x = gin[q][gr] + x;
            else x = gin[q][gr][e] + x;
          }
          v[e] = x;
        }
        double* dst = reinterpret_cast<double*>(gt + gro[q] + cc * 8u);
        if constexpr (VW == 1) {
          if (full) __builtin_nontemporal_store(v[0], dst);
        } else {
          if (full) {
            gvec_t o;
#pragma unroll
            for (int e = 0; e < VW; ++e) o[e] = v[e];
            __builtin_nontemporal_store(o, reinterpret_cast<gvec_t*>(dst));
          } else {
#pragma unroll
            for (int e = 0; e < VW; ++e)
              if (j0 + cc + e < n) __builtin_nontemporal_store(v[e], dst + e);
          }
        }
      }
    }
  }
}

template <typename T, int KS, bool HASP, bool VEC>
void launch_gm(const void* P, int64_t ldp, int64_t n, double alpha, const double* W, int64_t ldw, const double* Z,
               int64_t ldz, int k, double sign, bool accumulate, double* G, int64_t ldg, hipStream_t s) {
  const int64_t tiles = (n + kGmTile - 1) / kGmTile;
  // memory-bound: about four workgroups per CU in flight; a workgroup keeps its rows of W in
  // registers over all of its column tiles
  int64_t S = (4 * (int64_t)num_cus() + tiles - 1) / tiles;
  S = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S, tiles), 65535));
  const dim3 grid((unsigned)tiles, (unsigned)S), block(64 * kGmWaves);
  hipLaunchKernelGGL((grad_matrix_kernel<T, KS, HASP, VEC>), grid, block, 0, s, static_cast<const T*>(P), ldp, n,
                     alpha, W, ldw, Z, ldz, k, (k + 3) / 4, sign, accumulate ? 1 : 0, G, ldg, tiles);
}

template <typename T, bool HASP, bool VEC, typename... A>
void launch_gm_k(int k, A... args) {
  if (k == 0) launch_gm<T, 0, HASP, VEC>(args...);
  else if (k <= 4) launch_gm<T, 1, HASP, VEC>(args...);
  else if (k <= 16) launch_gm<T, 4, HASP, VEC>(args...);
  else if (k <= 32) launch_gm<T, 8, HASP, VEC>(args...);
  else launch_gm<T, 16, HASP, VEC>(args...);
}

template <typename T, bool HASP, typename... A>
void launch_gm_v(bool vec, int k, A... args) {
  if (vec) launch_gm_k<T, HASP, true>(k, args...);
  else launch_gm_k<T, HASP, false>(k, args...);
}

}  // namespace

const char* last_grad_matrix_kernel() { return g_last_grad_matrix_kernel; }

void grad_matrix(DType dt, const void* P, int64_t ldp, int64_t n, double alpha, const double* W, int64_t ldw,
                 const double* Z, int64_t ldz, int64_t k, double sign, bool accumulate, double* G, int64_t ldg,
                 hipStream_t s) {
  const bool hasp = alpha != 0.0;
  const int64_t es = (int64_t)dtype_size(dt);
  // a tile's rows are addressed from the tile's base with 32-bit byte offsets
  check_ld_32bit("grad_matrix", ldg, 8, kGmTile, kGmTile);
  if (hasp) check_ld_32bit("grad_matrix", ldp, es, kGmTile, kGmTile);
  // 16-byte pieces need 16-byte aligned rows of G and, where it is read, of P
  const bool vec = rows_16B_aligned(G, ldg, 8) && (!hasp || rows_16B_aligned(P, ldp, (size_t)es));
  set_probe_name<struct GmProbe>(g_last_grad_matrix_kernel, "gm%d:%s:%s", (int)((k + 3) / 4 * 4),
                                 !hasp ? "nop" : dt == DType::F64 ? "f64" : "f32", vec ? "vec" : "scalar");
  if (n <= 0) return;
  const int kk = (int)k;
  if (!hasp)
    launch_gm_v<double, false>(vec, kk, P, ldp, n, alpha, W, ldw, Z, ldz, kk, sign, accumulate, G, ldg, s);
  else if (dt == DType::F64)
    launch_gm_v<double, true>(vec, kk, P, ldp, n, alpha, W, ldw, Z, ldz, kk, sign, accumulate, G, ldg, s);
  else
    launch_gm_v<float, true>(vec, kk, P, ldp, n, alpha, W, ldw, Z, ldz, kk, sign, accumulate, G, ldg, s);
}

}  // namespace kern
}  // namespace gj
