// Kernels of the error bounds of a refined solve (Device::panel_abs_rhs, panel_abs_rhs_t,
// bound_terms; Engine::solve_rhs_block with bounds), gfx950.
//
// panel_abs_rhs / panel_abs_rhs_t are the siblings of panel_rhs / panel_rhs_t on absolute values:
// Y = |C_in| + |P| |V| and S = |P|^T |V_loc|, with the same streaming structure, the same split plans
// (skinny.hpp) and the same never-read set.  P is the memory-bound operand: every element is read
// exactly once per launch, straight from HBM into registers (16-byte loads where the rows are
// 16-byte aligned, element loads otherwise); |V| reaches the waves through LDS, once per workgroup,
// the absolute value taken while staging.
//
// What differs is the arithmetic: fp64 whatever the panel's storage type.  An fp32 element is
// widened exactly, its sign is cleared, and the product runs on v_mfma_f64_16x16x4_f64 (the
// precedent of rank_update.hip).  The bound these products feed has a right-hand side of about
// u (|A| |x| + |b|), which underflows fp32 for a small b, and its own rounding error must stay an
// fp64 one.  The fp32 vector path loads 4 floats per lane and feeds 4 fp64 K steps; the kernel is
// memory-bound, the conversions ride along.
//
// The K / row split is summed by a second pass in a fixed order and the column maximum is an
// integer maximum of bit patterns: two launches on the same input give the same bits, no
// floating-point value is accumulated with atomics.  Every term is computed by the MFMA from its
// two factors as they are, so a NaN or an Inf of |P| or |V| reaches every element it is a term of,
// also through a zero factor; masked operands (never read) are 0 on both sides.
//
// Rows of P are addressed from a tile's base with 32-bit byte offsets; the launch refuses a leading
// dimension where they would not fit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

using MF = SkinnyMfma<double>;  // both dtypes share the fp64 product

// LDS row padding of |V| (doubles) for the plain product: the 4 K lanes of a B-fragment read sit W
// rows apart, and W * pitch = 128 (mod 256) bytes spreads them over the banks
constexpr int abs_lds_pad(int W, int kw) { return W == 4 ? 4 : W == 2 ? 8 : (kw == 16 ? 0 : 16); }
// the same for the transposed product, whose K lanes sit on consecutive rows
constexpr int abst_lds_pad(int kw) { return kw == 16 ? 0 : 16; }

// a 16-byte piece of a row of P
template <typename T, int W>
struct Piece {
  typedef T type __attribute__((ext_vector_type(W)));
};

// Pass 1 of Y = |C_in| + |P| |V|: the partial product of one row tile and one K-slice.  W = elements
// each lane loads per row and K step (1: element loads, any alignment; 16 / sizeof(T): one 16-byte
// load).  A K step covers 4 W columns: lane (i = lane % 16, g = lane / 16) holds P[row i][kb + g W + j],
// j < W, and the j-th MFMA of the step multiplies the columns {kb + g W + j : g < 4} with the rows of
// |V| of the same indices.
template <typename T, int NF, int W>
__global__ __launch_bounds__(64 * kRhsWaves) void panel_abs_kernel(
    const T* __restrict__ P, int64_t ldp, int64_t rows, int64_t n, int64_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, double* __restrict__ part, int64_t rows_pad, int64_t kchunk,
    unsigned long long* colmax) {
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRhsWaves;
  constexpr int LDK = KW + abs_lds_pad(W, KW);    // LDS row pitch (doubles)
  constexpr int VPT = kRhsKC * KW / NT;           // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRhsKC / (4 * W);         // K steps per chunk
  constexpr int ES = (int)sizeof(T);
  static_assert(NT % KW == 0 && (kRhsKC * KW) % NT == 0 && kRhsKC % (4 * W) == 0, "chunk shape");
  __shared__ double vs[2][kRhsKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  // the column maxima start from 0 (pass 2 runs after this whole launch)
  if (colmax && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < k) colmax[threadIdx.x] = 0ull;

  // this lane's rows: byte offsets from the tile's first row fit 32 bits (checked by the launch)
  const int64_t rt0 = (int64_t)blockIdx.x * kRhsTileM;
  const char* tile = reinterpret_cast<const char*>(P + rt0 * ldp);
  uint32_t ro[kRhsMI];
  bool rv[kRhsMI];
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi) {
    const int tr = wave * (16 * kRhsMI) + mi * 16 + i;
    const int64_t r = rt0 + tr;
    rv[mi] = r < rows && ((r / m) * p + rk) * m + r % m < n;
    ro[mi] = rv[mi] ? (uint32_t)tr * (uint32_t)ldp * ES : 0u;
  }
  const int64_t kbeg = (int64_t)blockIdx.y * kchunk;
  const int64_t kend = kbeg + kchunk < n ? kbeg + kchunk : n;

  // staging: this thread's column of V and its rows of a chunk (row vr0 + q * (NT / KW))
  const int vc = threadIdx.x % KW, vr0 = threadIdx.x / KW;
  const bool vcv = vc < k;
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
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = fabs(vreg[q]);
  };

  MF::acc_t acc[kRhsMI][NF];
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::acc_t{0, 0, 0, 0};

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
        const T* src = reinterpret_cast<const T*>(tile + ro[mi]) + kk;
        if constexpr (W > 1) {
          if (rv[mi] && kk + W <= kend) {
            const typename Piece<T, W>::type v = *reinterpret_cast<const typename Piece<T, W>::type*>(src);
#pragma unroll
            for (int j = 0; j < W; ++j) a[st][mi][j] = v[j];
            continue;
          }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) a[st][mi][j] = (rv[mi] && kk + j < kend) ? src[j] : T(0);
      }
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        double b[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 * W + g * W + j][nf * 16 + i];
#pragma unroll
        for (int mi = 0; mi < kRhsMI; ++mi) {
          const double av = fabs((double)a[st][mi][j]);  // widened exactly, then the sign cleared
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::op(av, b[nf], acc[mi][nf]);
        }
      }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // partial product of this K-slice: rows_pad is a whole number of tiles, no row mask
  double* out = part + ((int64_t)blockIdx.y * rows_pad + rt0 + wave * (16 * kRhsMI)) * KW;
#pragma unroll
  for (int mi = 0; mi < kRhsMI; ++mi)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(int64_t)(mi * 16 + MF::row(lane, q)) * KW + nf * 16 + i] = acc[mi][nf][q];
}

// Pass 1 of S = |P|^T |V_loc|: the partial product of one column tile of P and one slice of the local
// rows.  A K step covers 4 local rows: lane (i, g) holds P[row + g][c0 + i W + j], j < W, and the j-th
// MFMA of the step produces the output rows {c0 + i W + j : i < 16} -- W interleaved column fragments
// from one load.  `real` = this rank's real local rows (global row < n), a prefix of its rows.
template <typename T, int NF, int W>
__global__ __launch_bounds__(64 * kRtWaves) void panel_abs_t_kernel(
    const T* __restrict__ P, int64_t ldp, int64_t real, int64_t n, uint32_t m, int64_t p, int64_t rk,
    const double* __restrict__ V, int64_t ldv, int k, double* __restrict__ part, int64_t cols_pad, int64_t rchunk) {
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * kRtWaves;
  constexpr int LDK = KW + abst_lds_pad(KW);  // LDS row pitch (doubles)
  constexpr int VPT = kRtKC * KW / NT;        // elements of a V chunk per thread (column fixed)
  constexpr int STEPS = kRtKC / 4;            // K steps per chunk
  constexpr int ES = (int)sizeof(T);
  static_assert(NT % KW == 0 && (kRtKC * KW) % NT == 0 && kRtKC % 4 == 0, "chunk shape");
  __shared__ double vs[2][kRtKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;

  const int64_t cbase = ((int64_t)blockIdx.x * kRtWaves + wave) * (16 * W);  // this wave's columns of P
  const int64_t c0 = cbase + i * W;                                          // this lane's
  const bool cvec = c0 + W <= n;
  const int64_t rbeg = (int64_t)blockIdx.y * rchunk;
  const int64_t rend = rbeg + rchunk < real ? rbeg + rchunk : real;
  // this lane's row of a K step, as a byte offset from the chunk's first row (32 bits: the launch checks)
  uint32_t ro[STEPS];
#pragma unroll
  for (int st = 0; st < STEPS; ++st) ro[st] = (uint32_t)(st * 4 + g) * (uint32_t)ldp * ES;

  // staging: this thread's column of V and its rows of a chunk (row vr0 + q * (NT / KW))
  const int vc = threadIdx.x % KW, vr0 = threadIdx.x / KW;
  const bool vcv = vc < k;
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
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = fabs(vreg[q]);
  };

  MF::acc_t acc[W][NF];
#pragma unroll
  for (int j = 0; j < W; ++j)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[j][nf] = MF::acc_t{0, 0, 0, 0};

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
      const bool rvalid = rb + st * 4 + g < rend;
      const T* src = reinterpret_cast<const T*>(chunk + ro[st]);
      if constexpr (W > 1) {
        if (cvec && rvalid) {
          const typename Piece<T, W>::type v = *reinterpret_cast<const typename Piece<T, W>::type*>(src);
#pragma unroll
          for (int j = 0; j < W; ++j) a[st][j] = v[j];
          continue;
        }
      }
#pragma unroll
      for (int j = 0; j < W; ++j) a[st][j] = (rvalid && c0 + j < n) ? src[j] : T(0);
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      double b[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) b[nf] = vs[buf][st * 4 + g][nf * 16 + i];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double av = fabs((double)a[st][j]);  // widened exactly, then the sign cleared
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[j][nf] = MF::op(av, b[nf], acc[j][nf]);
      }
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // partial product of this row slice: cols_pad is a whole number of tiles, no mask
  double* out = part + ((int64_t)blockIdx.y * cols_pad + cbase) * KW;
#pragma unroll
  for (int j = 0; j < W; ++j)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(int64_t)(MF::row(lane, q) * W + j) * KW + nf * 16 + i] = acc[j][nf][q];
}

template <typename T, int NF, int W>
void launch_abs(const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int k, double* part,
                const RhsPlan& pl, unsigned long long* colmax, hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRhsWaves);
  hipLaunchKernelGGL((panel_abs_kernel<T, NF, W>), grid, block, 0, s, static_cast<const T*>(P), ldp, L.rows, L.n,
                     L.m, L.p, L.k, V, ldv, k, part, pl.rows_pad, pl.kchunk, colmax);
}

template <typename T, int NF, int W>
void launch_abs_t(const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int k, double* part,
                  const RtPlan& pl, hipStream_t s) {
  const dim3 grid((unsigned)pl.tiles, (unsigned)pl.S), block(64 * kRtWaves);
  hipLaunchKernelGGL((panel_abs_t_kernel<T, NF, W>), grid, block, 0, s, static_cast<const T*>(P), ldp, pl.real, L.n,
                     (uint32_t)L.m, L.p, L.k, V, ldv, k, part, pl.cols_pad, pl.rchunk);
}

// berr of every column starts from the key of +0.0
__global__ void bound_terms_init_kernel(unsigned long long* berr, int k) {
  if ((int)threadIdx.x < k) berr[threadIdx.x] = 0ull;
}

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
  __shared__ unsigned long long sh[256];
  sh[threadIdx.x] = key;
  __syncthreads();
  if (rs == 0 && on) {
#pragma unroll
    for (int q = 1; q < RG; ++q) key = sh[q * KW + c] > key ? sh[q * KW + c] : key;
    atomicMax(berr + c, key);  // an integer maximum: the same bits in any order
  }
}

}  // namespace

const char* last_abs_kernel() { return g_last_abs_kernel; }

void panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                   const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax, void* scratch,
                   hipStream_t s) {
  const int64_t es = (int64_t)dtype_size(dt);
  // a tile's rows are addressed from the tile's base with 32-bit byte offsets
  if (ldp < 0 || ldp > ((int64_t(1) << 31) / es) / (kRhsTileM - 1))
    throw Error(Status::BadArgs, "panel_abs_rhs: leading dimension too large for 32-bit tile offsets");
  const RhsPlan pl = rhs_plan(L);
  // 16-byte loads of P need 16-byte aligned rows; the K-slices start on multiples of 16 columns
  const bool vec = rows_16B_aligned(P, ldp, (size_t)es);
  double* part = static_cast<double*>(scratch);
  unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmax);
  set_probe_name<struct AbsProbe>(g_last_abs_kernel, "abs%d:%s:%s:s%d", padded_kw(k),
                                  dt == DType::F64 ? "f64" : "f32", vec ? "vec" : "scalar", pl.S);
  with_kw(k, [&](auto KW) {
    constexpr int NF = KW / 16;
    if (dt == DType::F64) {
      if (vec) launch_abs<double, NF, 2>(P, ldp, L, V, ldv, (int)k, part, pl, cm, s);
      else launch_abs<double, NF, 1>(P, ldp, L, V, ldv, (int)k, part, pl, cm, s);
    } else {
      if (vec) launch_abs<float, NF, 4>(P, ldp, L, V, ldv, (int)k, part, pl, cm, s);
      else launch_abs<float, NF, 1>(P, ldp, L, V, ldv, (int)k, part, pl, cm, s);
    }
    const SliceSum<KW> sum{part, pl.S, pl.rows_pad, L.n, L.m, L.p, L.k};
    launch_col_epilogue<KW, SliceSum<KW>, true>(sum, C_in, ldc, Y, ldy, 1.0, L.rows, (int)k, nullptr, cm, s);
  });
}

void panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                     double* S, int64_t lds, void* scratch, hipStream_t s) {
  const int64_t es = (int64_t)dtype_size(dt);
  // a chunk's rows are addressed from the chunk's base with 32-bit byte offsets
  if (ldp < 0 || ldp > ((int64_t(1) << 31) / es) / (kRtKC - 1))
    throw Error(Status::BadArgs, "panel_abs_rhs_t: leading dimension too large for 32-bit tile offsets");
  const RtPlan pl = rt_plan(dt, P, ldp, L);
  set_probe_name<struct AbsProbe>(g_last_abs_kernel, "abst%d:%s:%s:s%d", padded_kw(k),
                                  dt == DType::F64 ? "f64" : "f32", pl.vec ? "vec" : "scalar", pl.S);
  if (L.n <= 0) return;
  double* part = static_cast<double*>(scratch);
  with_kw(k, [&](auto KW) {
    constexpr int NF = KW / 16;
    if (dt == DType::F64) {
      if (pl.vec) launch_abs_t<double, NF, 2>(P, ldp, L, V, ldv, (int)k, part, pl, s);
      else launch_abs_t<double, NF, 1>(P, ldp, L, V, ldv, (int)k, part, pl, s);
    } else {
      if (pl.vec) launch_abs_t<float, NF, 4>(P, ldp, L, V, ldv, (int)k, part, pl, s);
      else launch_abs_t<float, NF, 1>(P, ldp, L, V, ldv, (int)k, part, pl, s);
    }
    launch_rt_reduce<KW>(part, pl, L, (int)k, S, lds, nullptr, s);
  });
}

void bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg, int64_t rows,
                 int64_t k, double nz_eps, double safe1, double safe2, double* berr, hipStream_t s) {
  unsigned long long* be = reinterpret_cast<unsigned long long*>(berr);
  hipLaunchKernelGGL(bound_terms_init_kernel, dim3(1), dim3(64), 0, s, be, (int)k);
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
