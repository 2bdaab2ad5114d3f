// Where does a workgroup's LDS allocation sit, as the wave sees it?  (profiles/gemm_phase.md: a
// static priority per co-resident trailing-update workgroup would take its slot from this.)
//
//   hipcc --offload-arch=gfx950 -O2 -o build/lds_slot_probe bench/lds_slot_probe.hip && build/lds_slot_probe
//
// For a few LDS sizes a kernel of 4096 four-wave workgroups, each spinning ~20 us so that a CU's
// residents overlap, records the wave's LDS allocation register (HW_REG_LDS_ALLOC, id 6, all 32
// bits) from its first and last wave with the CU it ran on (HW_ID, XCC_ID); the program prints the
// distinct register values with their counts, and how many distinct values one CU saw.  The base
// field and its granularity are read off the values: size s, residents at base 0, s, 2 s, ...
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#define CHECK(x)                                                                        \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) {                                                             \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

extern __shared__ double dyn_lds[];

__global__ __launch_bounds__(256) void slot_kernel(unsigned* out, long long spin_ticks) {
  const unsigned la = __builtin_amdgcn_s_getreg((31 << 11) | 6);    // LDS_ALLOC, 32 bits
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
  const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // XCC_ID
  dyn_lds[threadIdx.x] = (double)la;                                // (the allocation is used)
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < spin_ticks) {
  }
  if (threadIdx.x == 0 || threadIdx.x == 192) {
    unsigned* o = out + 4 * blockIdx.x + (threadIdx.x ? 3 : 0);
    o[0] = la;
    if (threadIdx.x == 0) {
      o[1] = hw;
      o[2] = xcc + (dyn_lds[1] < 0.0 ? 1u << 31 : 0u);
    }
  }
}

int main() {
  const int nwg = 4096;
  unsigned* d;
  CHECK(hipMalloc(&d, sizeof(unsigned) * 4 * nwg));
  std::vector<unsigned> h(4 * nwg);
  int rate = 0;
  CHECK(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, 0));  // kHz
  const long long ticks = (long long)rate * 20 / 1000;                      // ~20 us
  for (int bytes : {34816, 52224, 16384, 26624}) {
    CHECK(hipFuncSetAttribute((const void*)slot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    CHECK(hipMemset(d, 0xff, sizeof(unsigned) * 4 * nwg));
    hipLaunchKernelGGL(slot_kernel, dim3(nwg), dim3(256), bytes, 0, d, ticks);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d, sizeof(unsigned) * 4 * nwg, hipMemcpyDeviceToHost));
    std::map<unsigned, int> vals;
    std::map<unsigned, std::set<unsigned>> per_cu;
    int differ = 0;
    for (int i = 0; i < nwg; ++i) {
      vals[h[4 * i]]++;
      differ += h[4 * i] != h[4 * i + 3];
      per_cu[((h[4 * i + 2] & 0xf) << 8) | ((h[4 * i + 1] >> 8) & 0xff)].insert(h[4 * i]);
    }
    size_t most = 0;
    for (const auto& c : per_cu) most = c.second.size() > most ? c.second.size() : most;
    std::printf("LDS %5d B: %zu CUs, at most %zu distinct values on one CU, waves 0 / 3 of a workgroup differ in %d; values:",
                bytes, per_cu.size(), most, differ);
    for (const auto& v : vals) std::printf(" %08x x%d", v.first, v.second);
    std::printf("\n");
  }
  CHECK(hipFree(d));
  return 0;
}
