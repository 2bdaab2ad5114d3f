// Sign and log-magnitude of the determinant of a batch of small dense blocks (Device::slogdet_batch;
// Engine::slogdet over the pivot-block inverses H_t it stashed), gfx950.
//
// One workgroup per block, an LU with partial pivoting in fp64 whatever the storage type (an fp32
// block is widened exactly on load).  Only the pivots are wanted, so no multiplier is stored:
//
//   per column c   wave 0 picks the pivot of column c among the rows not yet used: a wave-level
//                  arg-max on the NaN-keeping magnitude key (nonneg_key), the lowest row among equal
//                  keys.  Rows are never moved: a swap exchanges two entries of an index map.  Lane
//                  0 adds log|pivot| and folds the pivot's sign and the swap into the running sign,
//                  in column order.                                                   -- barrier --
//                  every thread: row i of the trailing part -= (a[i][c] / pivot) * pivot row, over
//                  the columns > c (a thread owns a column residue mod 32 of a row residue mod 8, so
//                  a wave walks rows contiguously).                                   -- barrier --
//
//   m <= 128       the block lives in LDS with an odd leading dimension (m | 1), so that the column
//                  walk of the pivot search does not stay on one bank: 128 x 129 x 8 B = 129 KiB of
//                  the CU's 160 KiB, above the 64 KiB default and therefore opted into.
//   m > 128        the same code on an fp64 copy of the block in global scratch (slow and correct,
//                  any m): the launch's workgroups walk the blocks with a grid stride, so the
//                  scratch holds one image per workgroup, not per block.
//
// A block that holds a NaN or an Inf entry gives (NaN, NaN): the widening load looks at every entry
// and no column is worked on.  Otherwise a pivot that is exactly zero ends the block with (0, -inf),
// and one that overflowed to NaN or Inf on the way with (NaN, NaN).
//
// No atomics; one lane accumulates in a fixed order: two launches give the same bits.  The input is
// only read.  Blocks with which[b] == 0 are skipped and their outputs are not written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>

#include "kernels.hpp"
#include "skinny.hpp"

namespace gj {
namespace kern {

namespace {

constexpr int kSldThreads = 256;
constexpr int kSldLdsMax = 128;     // largest m of the LDS form
constexpr int kSldGlobGrid = 512;   // workgroups (and scratch images) of the global form
constexpr int kSldMaxDevices = 64;  // devices whose LDS opt-in is remembered (others: set at every launch)

__host__ __device__ inline int64_t sld_lds_ld(int64_t m) { return m | 1; }
// LDS form: the image, the row map and two state words
inline size_t sld_lds_bytes(int64_t m) { return (size_t)m * sld_lds_ld(m) * 8 + (size_t)(m + 2) * 4; }
// global form: per workgroup the image (ld m) and the row map (+ state words), 8-byte granular
__host__ __device__ inline size_t sld_glob_image_bytes(int64_t m) {
  return (size_t)m * m * 8 + (((size_t)(m + 2) * 4 + 7) & ~(size_t)7);
}

extern __shared__ double sld_smem[];

// state words: st[0] = 0 running, 1 = exactly zero pivot, 2 = non-finite entry or pivot; st[1] = pivot row
template <typename T, bool kLds>
__global__ __launch_bounds__(kSldThreads) void slogdet_kernel(const T* __restrict__ blocks, int64_t stride, int m,
                                                              int64_t nb, const int32_t* __restrict__ which,
                                                              double* __restrict__ sign, double* __restrict__ logabs,
                                                              char* __restrict__ scratch) {
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int tx = tid & 31, ty = tid >> 5;  // trailing update: column residue, row residue
  const int64_t ld = kLds ? sld_lds_ld(m) : (int64_t)m;
  double* a;
  int* perm;
  if constexpr (kLds) {
    a = sld_smem;
    perm = reinterpret_cast<int*>(sld_smem + (int64_t)m * ld);
  } else {
    char* img = scratch + (size_t)blockIdx.x * sld_glob_image_bytes(m);
    a = reinterpret_cast<double*>(img);
    perm = reinterpret_cast<int*>(img + (size_t)m * m * 8);
  }
  int* st = perm + m;

  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    if (which && which[b] == 0) continue;  // uniform
    const T* src = blocks + b * stride;
    if (tid == 0) st[0] = 0;
    __syncthreads();
    bool bad = false;  // a NaN or an Inf among this thread's entries
    for (int e = tid; e < m * m; e += kSldThreads) {  // m <= 2^15: m * m fits an int
      const int r = e / m, c = e - r * m;
      const double v = (double)src[e];
      bad = bad || !(fabs(v) < __builtin_huge_val());
      a[(int64_t)r * ld + c] = v;
    }
    for (int i = tid; i < m; i += kSldThreads) perm[i] = i;
    if (bad) st[0] = 2;  // (every writer stores the same value)
    __syncthreads();

    double sg = 1.0, lg = 0.0;  // lane 0 of wave 0
    int state = st[0];
    for (int c = 0; c < m && state == 0; ++c) {
      if (wave == 0) {
        // arg-max of the keys of column c over the slots >= c; ascending slots per lane and a strict
        // '>' keep the lowest slot among equal keys
        unsigned long long bk = 0ull;
        int bs = m;  // m: this lane saw no slot
        for (int i = c + lane; i < m; i += 64) {
          const unsigned long long k = nonneg_key(fabs(a[(int64_t)perm[i] * ld + c]));
          if (bs == m || k > bk) bk = k, bs = i;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const unsigned long long ok = __shfl_xor(bk, off, 64);
          const int os = __shfl_xor(bs, off, 64);
          if (os < m && (bs == m || ok > bk || (ok == bk && os < bs))) bk = ok, bs = os;
        }
        if (lane == 0) {
          const int pr = perm[bs];
          if (bs != c) {
            perm[bs] = perm[c];
            perm[c] = pr;
            sg = -sg;
          }
          const double piv = a[(int64_t)pr * ld + c];
          const double ap = fabs(piv);
          int s = 0;
          if (!(ap < __builtin_huge_val())) s = 2;  // NaN or Inf
          else if (ap == 0.0) s = 1;
          else {
            lg += log(ap);
            if (piv < 0.0) sg = -sg;
          }
          st[0] = s;
          st[1] = pr;
        }
      }
      __syncthreads();
      state = st[0];
      if (state != 0) break;  // uniform
      const int pr = st[1];
      const double* prow = a + (int64_t)pr * ld;
      const double piv = prow[c];
      for (int i = c + 1 + ty; i < m; i += kSldThreads / 32) {
        double* row = a + (int64_t)perm[i] * ld;
        const double l = row[c] / piv;
        for (int j = c + 1 + tx; j < m; j += 32) row[j] -= l * prow[j];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      sign[b] = state == 0 ? sg : state == 1 ? 0.0 : nan;
      logabs[b] = state == 0 ? lg : state == 1 ? -__builtin_huge_val() : nan;
    }
    __syncthreads();  // the next block's load overwrites the image and the state words
  }
}

template <typename T>
void launch_sld(const void* blocks, int64_t stride, int64_t m, int64_t nb, const int32_t* which, double* sign,
                double* logabs, void* scratch, hipStream_t s) {
  const T* src = static_cast<const T*>(blocks);
  if (m <= kSldLdsMax) {
    // above the 64 KiB default: the opt-in the candidate inverse uses, once per device, and under a
    // lock because the ranks of an in-process job launch from their own threads
    static std::mutex mu;
    static bool attr[kSldMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    const bool tracked = dev >= 0 && dev < kSldMaxDevices;
    std::lock_guard<std::mutex> lk(mu);
    if (!tracked || !attr[dev]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&slogdet_kernel<T, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sld_lds_bytes(kSldLdsMax)) != hipSuccess) {
        (void)hipGetLastError();
        throw Error(Status::BadArgs, "slogdet_batch: dynamic LDS attribute refused");
      }
      if (tracked) attr[dev] = true;
    }
    hipLaunchKernelGGL((slogdet_kernel<T, true>), dim3((unsigned)nb), dim3(kSldThreads), sld_lds_bytes(m), s, src,
                       stride, (int)m, nb, which, sign, logabs, static_cast<char*>(nullptr));
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(nb, kSldGlobGrid);
    hipLaunchKernelGGL((slogdet_kernel<T, false>), dim3(grid), dim3(kSldThreads), 0, s, src, stride, (int)m, nb,
                       which, sign, logabs, static_cast<char*>(scratch));
  }
}

}  // namespace

const char* last_slogdet_kernel() { return g_last_slogdet_kernel; }

size_t slogdet_scratch_bytes(int64_t m, int64_t nb) {
  if (m <= kSldLdsMax || nb <= 0) return 0;
  return (size_t)std::min<int64_t>(nb, kSldGlobGrid) * sld_glob_image_bytes(m);
}

void slogdet_batch(DType dt, const void* blocks, int64_t stride, int64_t m, int64_t nb, const int32_t* which,
                   double* sign, double* logabs, void* scratch, hipStream_t s) {
  if (m < 1 || m > (int64_t(1) << 15) || nb < 0 || nb > 0x7fffffff || stride < m * m)
    throw Error(Status::BadArgs, "slogdet_batch: 1 <= m <= 32768, 0 <= nb < 2^31, stride >= m * m");
  set_probe_name<struct SldProbe>(g_last_slogdet_kernel, "sld:%s:%s", m <= kSldLdsMax ? "lds" : "glob",
                                  dt == DType::F64 ? "f64" : "f32");
  if (nb == 0) return;
  if (m > kSldLdsMax && !scratch) throw Error(Status::BadArgs, "slogdet_batch: m > 128 needs its scratch");
  if (dt == DType::F64) launch_sld<double>(blocks, stride, m, nb, which, sign, logabs, scratch, s);
  else launch_sld<float>(blocks, stride, m, nb, which, sign, logabs, scratch, s);
}

}  // namespace kern
}  // namespace gj
