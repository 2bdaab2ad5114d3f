// Kernels of the stack ops (Device::batch_pack / batch_unpack / batch_rhs; BatchSolver, gj/batch.hpp),
// gfx950: the layer between a stack of nb small matrices (n <= 1024) and block_inverse's calling
// convention, and the products of the refined solve from the stack of inverses.
//
// pack / unpack are memory-bound one-pass transposes.  A workgroup takes one 64 x 64 tile of one
// matrix: it is loaded along the source's rows, changed in registers (sign, ldexp, conversion) and
// written to an LDS image of pitch 65 elements, then read back transposed and stored along the
// destination's rows, so that both the global load and the global store are coalesced
// (grad_matrix.hip's image).  Banks: the image is written at [row][lane] (adjacent lanes, adjacent
// elements) and read at [lane][column], 65 elements apart: 65 dwords (fp32) or 130 dwords (fp64) per
// lane, i.e. lane (mod 64) or 2 lane (mod 64) over the 32 lanes a 64-bit access serves at a time --
// all different either way.  The norms of batch_pack are a pass of their own (one workgroup per
// matrix, a wave per row, fixed-order sums): the exponent of a matrix needs all of its rows.
//
// batch_rhs: Y_b = C_in_b + sign * M_b V_b with v_mfma_f64_16x16x4_f64 in skinny.hpp's lane map, fp64
// arithmetic for both dtypes of M (an fp32 element is widened exactly in registers).  grid (matrix,
// row tile): a wave owns MI 16-row fragments of one matrix and NF = 1 | 2 | 4 column fragments.  M_b
// is the memory-bound operand: every element goes from global memory straight into the A-operand
// registers exactly once per launch (W elements per lane and load: 16-byte pieces where the rows are
// 16-byte aligned, element loads otherwise).  V_b goes through LDS in stages of kRhsKC rows, two
// buffers, one barrier per stage (skinny_stream.hpp's pipeline).  No K-split: the stack supplies the
// parallelism, so every sum has one fixed order and the epilogue runs from the accumulators.  The
// column maxima are integer maxima of nonneg_key (NaN kept) -- no floating-point atomics; two
// launches give the same bits.
//
// Masks, not assumptions: rows and columns >= n of a matrix, inactive columns and every pitch gap are
// never loaded; nothing outside the documented outputs is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "skinny.hpp"
#include "skinny_stream.hpp"

namespace gj {
namespace kern {

namespace {

constexpr int kBtTile = 64;   // pack / unpack tile
constexpr int kBtPitch = 65;  // LDS pitch of its image (elements)

// ---- norms and exponents: one workgroup per matrix
__global__ __launch_bounds__(256) void batch_norm_kernel(const double* __restrict__ A, int64_t stride_a, int64_t lda,
                                                         int n, double* __restrict__ norm, int32_t* __restrict__ exp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* Ab = A + (int64_t)blockIdx.x * stride_a;
  unsigned long long key = 0ull;
  for (int r = wave; r < n; r += 4) {  // wave-uniform
    const double* row = Ab + (int64_t)r * lda;
    double sum = 0.0;
    for (int c = lane; c < n; c += 64) sum += fabs(row[c]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);  // the same order in every lane
    const unsigned long long kk = nonneg_key(sum);
    key = kk > key ? kk : key;
  }
  __shared__ unsigned long long sh[4];
  if (lane == 0) sh[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) key = sh[w] > key ? sh[w] : key;
    const double v = __longlong_as_double((long long)key);
    int e = 0;
    // equil_exponent (gj/device.hpp): ldexp(v, e) in [1, 2); 0 for a norm that is 0 or not finite
    if (v > 0.0 && v < __longlong_as_double(0x7ff0000000000000ll)) {
      (void)frexp(v, &e);
      e = 1 - e;
    }
    norm[blockIdx.x] = v;
    exp[blockIdx.x] = e;
  }
}

// ---- pack: Lt[c*ldl + b*m + r] = (T)(-ldexp(A_b[r][c], exp[b])), diag(., I) up to m
template <typename T>
__global__ __launch_bounds__(256) void batch_pack_kernel(const double* __restrict__ A, int64_t stride_a, int64_t lda,
                                                         int n, int m, int tiles, T* __restrict__ Lt, int64_t ldl,
                                                         const int32_t* __restrict__ exp) {
  __shared__ T img[kBtTile][kBtPitch];
  const int64_t b = blockIdx.x;
  const int r0 = ((int)blockIdx.y / tiles) * kBtTile, c0 = ((int)blockIdx.y % tiles) * kBtTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const double* Ab = A + b * stride_a;
  const int e = exp[b];
  {
    const int c = c0 + tx;
#pragma unroll 4
    for (int q = 0; q < kBtTile / 4; ++q) {
      const int rl = ty + 4 * q, r = r0 + rl;
      if (r < m && c < m) {
        double v;
        if (r < n && c < n)
          v = -ldexp(Ab[(int64_t)r * lda + c], e);
        else
          v = (r >= n && r == c) ? -1.0 : 0.0;
        img[rl][tx] = (T)v;
      }
    }
  }
  __syncthreads();
  {
    const int r = r0 + tx;
#pragma unroll 4
    for (int q = 0; q < kBtTile / 4; ++q) {
      const int cl = ty + 4 * q, c = c0 + cl;
      if (r < m && c < m) Lt[(int64_t)c * ldl + b * m + r] = img[tx][cl];
    }
  }
}

// ---- unpack: X_b[i][j] = (T)ldexp(inv_t[b*m*m + j*m + i], exp[b]), NaN for an invalid block
template <typename T>
__global__ __launch_bounds__(256) void batch_unpack_kernel(const T* __restrict__ inv_t, int n, int m, int tiles,
                                                           const int32_t* __restrict__ exp,
                                                           const int32_t* __restrict__ valid, T* __restrict__ X,
                                                           int64_t stride_x, int64_t ldx) {
  __shared__ T img[kBtTile][kBtPitch];
  const int64_t b = blockIdx.x;
  const int i0 = ((int)blockIdx.y / tiles) * kBtTile, j0 = ((int)blockIdx.y % tiles) * kBtTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const bool ok = valid[b] != 0;  // uniform
  const int e = exp[b];
  T* Xb = X + b * stride_x;
  if (ok) {
    const T* src = inv_t + b * m * m;
    const int i = i0 + tx;
#pragma unroll 4
    for (int q = 0; q < kBtTile / 4; ++q) {
      const int jl = ty + 4 * q, j = j0 + jl;
      if (i < n && j < n) img[jl][tx] = (T)ldexp((double)src[(int64_t)j * m + i], e);
    }
  }
  __syncthreads();
  {
    const int j = j0 + tx;
    const T nan = (T)__longlong_as_double(0x7ff8000000000000ll);
#pragma unroll 4
    for (int q = 0; q < kBtTile / 4; ++q) {
      const int il = ty + 4 * q, i = i0 + il;
      if (i < n && j < n) Xb[(int64_t)i * ldx + j] = ok ? img[tx][il] : nan;
    }
  }
}

// ---- batch_rhs
// The keys of the active (matrix, column) pairs start from 0, the key of +0.0
__global__ __launch_bounds__(256) void batch_zero_keys_kernel(unsigned long long* __restrict__ keys, int64_t count,
                                                              const int32_t* __restrict__ active) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < count && (!active || active[t] != 0)) keys[t] = 0ull;
}

// T: M's element type; NF: 16-column fragments (KW = 16 NF >= k); W: elements of M per load; a
// workgroup of WAVES waves covers 16 MI WAVES rows of one matrix.  A K step covers 4 W columns of M:
// lane (i = lane % 16, g = lane / 16) holds M[row i][kb + g W + j], j < W, and the j-th MFMA of the step
// multiplies the columns {kb + g W + j : g < 4} against the same rows of V (skinny_rows_kernel's map).
template <typename T, int NF, int W, int WAVES, int MI>
__global__ __launch_bounds__(64 * WAVES) void batch_rhs_kernel(
    const T* __restrict__ M, int64_t stride_m, int64_t ldm, int n, const double* __restrict__ V, int64_t stride_v,
    int64_t ldv, int k, const double* C_in, int64_t stride_c, int64_t ldc, double* Y, int64_t stride_y, int64_t ldy,
    double sign, const int32_t* __restrict__ active, unsigned long long* colmax) {
  using MF = SkinnyMfma<double>;
  constexpr int KW = 16 * NF;
  constexpr int NT = 64 * WAVES;
  constexpr int LDK = KW + (W == 4 ? 4 : 8);  // the 4 K lanes of a B read sit W rows apart: 128 (mod 256) bytes
  constexpr int VPT = kRhsKC * KW / NT;       // elements of a V stage per thread (column fixed)
  constexpr int STEPS = kRhsKC / (4 * W);     // K steps per stage
  static_assert(NT % KW == 0 && (kRhsKC * KW) % NT == 0 && kRhsKC % (4 * W) == 0, "stage shape");
  __shared__ double vs[2][kRhsKC][LDK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.x;
  const T* Mb = M + b * stride_m;
  const double* Vb = V + b * stride_v;
  const int32_t* act = active ? active + b * k : nullptr;

  const int r0 = (int)blockIdx.y * (16 * MI * WAVES) + wave * (16 * MI);
  const T* mrow[MI];
  bool rv[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int r = r0 + mi * 16 + i;
    rv[mi] = r < n;
    mrow[mi] = Mb + (int64_t)(rv[mi] ? r : 0) * ldm;
  }

  // staging: this thread's column of V and its rows of a stage (row vr0 + q * (NT / KW))
  const int vc = threadIdx.x % KW, vr0 = threadIdx.x / KW;
  const bool vcv = vc < k && (!act || act[vc] != 0);
  double vreg[VPT];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
      const int kr = kb + vr0 + q * (NT / KW);
      vreg[q] = (vcv && kr < n) ? Vb[(int64_t)kr * ldv + vc] : 0.0;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < VPT; ++q) vs[buf][vr0 + q * (NT / KW)][vc] = vreg[q];
  };

  MF::acc_t acc[MI][NF];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::acc_t{0, 0, 0, 0};

  fetch(0);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int kb = 0; kb < n; kb += kRhsKC, buf ^= 1) {
    const bool more = kb + kRhsKC < n;  // uniform over the workgroup
    if (more) fetch(kb + kRhsKC);
    T a[STEPS][MI][W];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int kk = kb + st * 4 * W + g * W;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        if (W > 1 && rv[mi] && kk + W <= n) {
          const Piece<T, W> v = *reinterpret_cast<const Piece<T, W>*>(mrow[mi] + kk);
#pragma unroll
          for (int j = 0; j < W; ++j) a[st][mi][j] = v[j];
        } else {
#pragma unroll
          for (int j = 0; j < W; ++j) a[st][mi][j] = (rv[mi] && kk + j < n) ? mrow[mi][kk + j] : T(0);
        }
      }
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        double bv[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) bv[nf] = vs[buf][st * 4 * W + g * W + j][nf * 16 + i];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const double av = (double)a[st][mi][j];  // an fp32 element widened exactly
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mi][nf] = MF::op(av, bv[nf], acc[mi][nf]);
        }
      }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // Y = C_in + sign * acc on the active columns; accumulator element q of lane (i, g) is row g + 4 q of
  // the fragment, column i
  const double* Cb = C_in ? C_in + b * stride_c : nullptr;
  double* Yb = Y + b * stride_y;
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int c = nf * 16 + i;
    const bool on = c < k && (!act || act[c] != 0);
    unsigned long long key = 0ull;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + mi * 16 + MF::row(lane, q);
        if (on && r < n) {
          const double y = (Cb ? Cb[(int64_t)r * ldc + c] : 0.0) + sign * acc[mi][nf][q];
          Yb[(int64_t)r * ldy + c] = y;
          const unsigned long long kk = nonneg_key(fabs(y));
          key = kk > key ? kk : key;
        }
      }
    if (colmax) {  // uniform: the maximum over the wave's four row groups, then over the workgroups
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, d);
        key = o > key ? o : key;
      }
      if (on && g == 0 && r0 < n) atomicMax(colmax + b * k + c, key);  // an integer maximum: any order, same bits
    }
  }
}

template <typename T, int NF, int W, int WAVES, int MI, typename... A>
void launch_brhs(int64_t nb, int n, hipStream_t s, A... args) {
  const int tile = 16 * MI * WAVES;
  const dim3 grid((unsigned)nb, (unsigned)((n + tile - 1) / tile)), block(64 * WAVES);
  hipLaunchKernelGGL((batch_rhs_kernel<T, NF, W, WAVES, MI>), grid, block, 0, s, args...);
}

// the rows a workgroup covers, by the matrix order: 16 (one wave), 64 or 128
template <typename T, int NF, int W, typename... A>
void launch_brhs_shape(int64_t nb, int n, hipStream_t s, A... args) {
  if (n <= 16) launch_brhs<T, NF, W, 1, 1>(nb, n, s, args...);
  else if (n <= 64) launch_brhs<T, NF, W, 4, 1>(nb, n, s, args...);
  else launch_brhs<T, NF, W, 4, 2>(nb, n, s, args...);
}

}  // namespace

const char* last_batch_kernel() { return g_last_batch_kernel; }

void batch_pack(DType dt, const double* A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m, int64_t nb,
                void* Lt, int64_t ldl, double* norm, int32_t* exp, hipStream_t s) {
  set_probe_name<struct BpackProbe>(g_last_batch_kernel, "bpack:%s", dt == DType::F64 ? "f64" : "f32");
  if (nb <= 0) return;
  const int tiles = (int)((m + kBtTile - 1) / kBtTile);
  hipLaunchKernelGGL(batch_norm_kernel, dim3((unsigned)nb), dim3(256), 0, s, A64, stride_a, lda, (int)n, norm, exp);
  const dim3 grid((unsigned)nb, (unsigned)(tiles * tiles));
  if (dt == DType::F64)
    hipLaunchKernelGGL((batch_pack_kernel<double>), grid, dim3(256), 0, s, A64, stride_a, lda, (int)n, (int)m, tiles,
                       static_cast<double*>(Lt), ldl, exp);
  else
    hipLaunchKernelGGL((batch_pack_kernel<float>), grid, dim3(256), 0, s, A64, stride_a, lda, (int)n, (int)m, tiles,
                       static_cast<float*>(Lt), ldl, exp);
}

void batch_unpack(DType dt, const void* inv_t, int64_t n, int64_t m, int64_t nb, const int32_t* exp,
                  const int32_t* valid, void* X, int64_t stride_x, int64_t ldx, hipStream_t s) {
  set_probe_name<struct BunpackProbe>(g_last_batch_kernel, "bunpack:%s", dt == DType::F64 ? "f64" : "f32");
  if (nb <= 0) return;
  const int tiles = (int)((n + kBtTile - 1) / kBtTile);
  const dim3 grid((unsigned)nb, (unsigned)(tiles * tiles));
  if (dt == DType::F64)
    hipLaunchKernelGGL((batch_unpack_kernel<double>), grid, dim3(256), 0, s, static_cast<const double*>(inv_t), (int)n,
                       (int)m, tiles, exp, valid, static_cast<double*>(X), stride_x, ldx);
  else
    hipLaunchKernelGGL((batch_unpack_kernel<float>), grid, dim3(256), 0, s, static_cast<const float*>(inv_t), (int)n,
                       (int)m, tiles, exp, valid, static_cast<float*>(X), stride_x, ldx);
}

void batch_rhs(DType dt, const void* M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb, const double* V,
               int64_t stride_v, int64_t ldv, int64_t k, const double* C_in, int64_t stride_c, int64_t ldc, double* Y,
               int64_t stride_y, int64_t ldy, double sign, const int32_t* active, double* colmax, hipStream_t s) {
  const size_t es = dtype_size(dt);
  // 16-byte pieces of M need 16-byte aligned rows in every matrix of the stack
  const bool vec = rows_16B_aligned(M, ldm, es) && ((size_t)stride_m * es) % 16 == 0;
  set_probe_name<struct BrhsProbe>(g_last_batch_kernel, "brhs%d:%s:%s", padded_kw(k), dt == DType::F64 ? "f64" : "f32",
                                   vec ? "vec" : "scalar");
  if (nb <= 0) return;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(colmax);
  if (keys)
    hipLaunchKernelGGL(batch_zero_keys_kernel, dim3((unsigned)((nb * k + 255) / 256)), dim3(256), 0, s, keys, nb * k,
                       active);
  with_kw(k, [&](auto KW) {
    with_panel(dt, vec, [&](auto zero, auto W) {
      using T = decltype(zero);
      launch_brhs_shape<T, KW / 16, W>(nb, (int)n, s, static_cast<const T*>(M), stride_m, ldm, (int)n, V, stride_v,
                                       ldv, (int)k, C_in, stride_c, ldc, Y, stride_y, ldy, sign, active, keys);
    });
  });
}

}  // namespace kern
}  // namespace gj
