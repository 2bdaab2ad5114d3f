// HostDevice: plain C++ reference executor of the Device interface.
//
// Used for `gj --device cpu` (the reference's CPU-only "plumbing" configuration), for CPU tests of
// the distributed protocol, and as an oracle.  It is never chosen implicitly for a GPU run.
// Streams/events are no-ops: every op completes before it returns.
#include <chrono>
#include "gj/host_device.hpp"

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gj/gen.hpp"

namespace gj {

// GEMM launch census (gj/device.hpp)
std::atomic<bool> g_gemm_census_on{false};
namespace {
std::mutex g_gemm_census_mu;
std::map<std::string, int64_t> g_gemm_census;
}  // namespace
void gemm_census_enable(bool on) {
  std::lock_guard<std::mutex> lk(g_gemm_census_mu);
  if (on) g_gemm_census.clear();
  g_gemm_census_on.store(on, std::memory_order_relaxed);
}
void gemm_census_add(const char* name) {
  std::lock_guard<std::mutex> lk(g_gemm_census_mu);
  ++g_gemm_census[name];
}
std::map<std::string, int64_t> gemm_census_counts() {
  std::lock_guard<std::mutex> lk(g_gemm_census_mu);
  return g_gemm_census;
}

namespace {

template <typename F>
void parallel_for(int64_t n, int nthreads, F f) {
  if (n <= 0) return;
  int nt = (int)std::min<int64_t>(nthreads, n);
  if (nt <= 1) {
    for (int64_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int w = 0; w < nt; ++w)
    th.emplace_back([=, &f] {
      for (int64_t i = w; i < n; i += nt) f(i);
    });
  for (auto& t : th) t.join();
}

template <typename T>
T* tp(void* p) {
  return static_cast<T*>(p);
}
template <typename T>
const T* tp(const void* p) {
  return static_cast<const T*>(p);
}

template <typename T>
void gemm_t(GemmOp op, ALayout al, int64_t M, int64_t N, int64_t K, const T* A, int64_t lda,
            const T* B, int64_t ldb, T* C, int64_t ldc, int nthreads, const GemmExtra& ex) {
  if (ex.owner_phys) {  // owner-predicated (GemmExtra::owner_phys)
    const int64_t g = *ex.owner_phys;
    if (g < 0 || g % ex.owner_p != ex.owner_k) return;
  }
  parallel_for(M, nthreads, [&](int64_t il) {
    const int64_t i = ex.rsel_m > 0 ? ex.rsel_row(il) : il;  // GemmExtra::rsel: physical row
    bool zrow = false;
    for (int z = 0; z < ex.nzr; ++z) zrow |= (i >= ex.zr[z] && i < ex.zr[z] + ex.zh);
    std::vector<double> acc(N, 0.0);
    for (int64_t k = 0; k < K; ++k) {
      // (no shortcut for a == 0: 0 * NaN and 0 * Inf are NaN, as on the matrix cores -- Device::gemm)
      const double a = (al == ALayout::RowMajor) ? (double)A[i * lda + k] : (double)A[k * lda + i];
      const T* b = B + k * ldb;
      for (int64_t j = 0; j < N; ++j)
        if (!(j >= ex.skip_c0 && j < ex.skip_c1)) acc[j] += a * (double)b[j];
    }
    T* c = C + i * ldc;
    const T* ci = ex.c_in ? static_cast<const T*>(ex.c_in) + i * ex.ldc_in : c;  // GemmExtra::c_in
    const auto skip = [&](int64_t j) { return j >= ex.skip_c0 && j < ex.skip_c1; };  // GemmExtra::skip_c0/c1
    if (op == GemmOp::Acc) {
      for (int64_t j = 0; j < N; ++j)
        if (!skip(j)) c[j] = (T)((zrow || (j >= ex.zc0 && j < ex.zc1) ? 0.0 : (double)ci[j]) + acc[j]);
    } else {
      for (int64_t j = 0; j < N; ++j)
        if (!skip(j)) c[j] = (T)acc[j];
    }
    if (ex.tneg) {
      const int64_t nt = ex.tneg_cols > 0 ? std::min(ex.tneg_cols, N) : N;
      for (int64_t j = 0; j < nt; ++j)
        if (!skip(j)) static_cast<T*>(ex.tneg)[j * ex.ldtneg + i] = -c[j];
    }
  });
}

// In-place Gauss-Jordan sweep on W (m x m, row-major) with partial pivoting over not-yet-used rows.
// Returns false when singular (|pivot| < thresh, or an Inf / NaN pivot).  prow[k] = pivot row of column k.
// The sweep runs in double whatever the block's type: `limit` is the largest finite value of that
// type, and a value beyond it -- an overflow of the sweep in the block's own precision, which the
// GPU kernels run in -- ends the sweep like a singular pivot (fp64: never taken, Inf > DBL_MAX aside).
inline bool sweep_inverse(std::vector<double>& W, int64_t m, double thresh, std::vector<int64_t>& prow,
                          double limit) {
  std::vector<char> used(m, 0);
  for (int64_t k = 0; k < m; ++k) {
    int64_t r = -1;
    double best = -1.0;
    for (int64_t i = 0; i < m; ++i) {
      if (used[i]) continue;
      const double a = std::fabs(W[i * m + k]);
      if (a != a) {  // a NaN is the column maximum, like the GPU's integer key: singular below
        best = a;
        r = i;
        break;
      }
      if (a > best) {
        best = a;
        r = i;
      }
    }
    if (!(best >= thresh && best < HUGE_VAL)) return false;  // NaN and Inf pivots included
    used[r] = 1;
    prow[k] = r;
    const double inv = 1.0 / W[r * m + k];
    for (int64_t j = 0; j < m; ++j) {
      W[r * m + j] *= inv;
      if (std::fabs(W[r * m + j]) > limit) return false;
    }
    W[r * m + k] = inv;
    for (int64_t i = 0; i < m; ++i) {
      if (i == r) continue;
      const double f = W[i * m + k];
      if (f == 0.0) continue;
      for (int64_t j = 0; j < m; ++j) {
        W[i * m + j] -= f * W[r * m + j];
        if (std::fabs(W[i * m + j]) > limit) return false;
      }
      W[i * m + k] = -f * inv;
    }
  }
  return true;
}

}  // namespace

HostDevice::HostDevice(int nthreads) {
  nthreads_ = nthreads > 0 ? nthreads : (int)std::max(1u, std::thread::hardware_concurrency());
}

std::string HostDevice::describe() const {
  return "host(" + std::to_string(nthreads_) + " threads)";
}

// GJ_TEST_ALLOC_NTH=<n> (fault injection, tests only): the n-th allocation of the process fails.
void* HostDevice::alloc(size_t bytes) {
  static std::atomic<int64_t> count{0};
  static const int64_t nth = [] {
    const char* e = std::getenv("GJ_TEST_ALLOC_NTH");
    return e ? std::atoll(e) : 0;
  }();
  if (++count == nth) throw Error(Status::NoMemory, "injected (GJ_TEST_ALLOC_NTH)");
  void* p = nullptr;
  if (posix_memalign(&p, 64, std::max<size_t>(bytes, 64)) != 0 || !p)
    throw Error(Status::NoMemory, "host allocation failed");
  return p;
}
void HostDevice::release(void* p) { std::free(p); }
void* HostDevice::alloc_pinned(size_t bytes) { return alloc(bytes); }
void HostDevice::release_pinned(void* p) { std::free(p); }
size_t HostDevice::free_memory() const { return ~size_t(0); }
void HostDevice::memset0(void* p, size_t bytes, int) { std::memset(p, 0, bytes); }
void HostDevice::memset2d(void* p, size_t pitch, size_t w, size_t h, int) {
  for (size_t r = 0; r < h; ++r) std::memset(static_cast<char*>(p) + r * pitch, 0, w);
}
void HostDevice::copy(void* dst, const void* src, size_t bytes, int) {
  if (dst != src) std::memmove(dst, src, bytes);
}
void HostDevice::copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t w, size_t h,
                        int) {
  for (size_t r = 0; r < h; ++r)
    std::memmove(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, w);
}

// Events carry the host time at which they were recorded (all work before them is complete).
int HostDevice::create_event(bool) {
  ev_time_.push_back(0.0);
  return nev_++;
}
void HostDevice::record(int ev, int) {
  ev_time_[ev] = std::chrono::duration<double, std::milli>(
                     std::chrono::steady_clock::now().time_since_epoch()).count();
}
void HostDevice::wait(int, int) {}
void HostDevice::sync_event(int) {}
void HostDevice::sync_stream(int) {}
void HostDevice::sync_all() {}
float HostDevice::event_ms(int a, int b) { return (float)(ev_time_[b] - ev_time_[a]); }

void HostDevice::generate(DType dt, void* X, const Layout& L, GenSpec g, int) {
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const int64_t gr = L.global_row(r);
    for (int64_t j = 0; j < L.npad; ++j) {
      const double v = gen_value((int)g.kind, g.seed, L.n, gr, j);
      if (dt == DType::F64)
        tp<double>(X)[r * L.npad + j] = v;
      else
        tp<float>(X)[r * L.npad + j] = (float)v;
    }
  });
}

void HostDevice::widen(DType dt, double* dst, int64_t ldd, const void* X, int64_t ldx, int64_t rows,
                       int64_t cols, int) {
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t j = 0; j < cols; ++j)
      dst[r * ldd + j] = dt == DType::F64 ? tp<double>(X)[r * ldx + j] : (double)tp<float>(X)[r * ldx + j];
}

void HostDevice::upload_convert(DType dt, void* X, int64_t ldx, const double* src, int64_t src_ld,
                                int64_t rows, int64_t cols, int) {
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t j = 0; j < cols; ++j) {
      if (dt == DType::F64)
        tp<double>(X)[r * ldx + j] = src[r * src_ld + j];
      else
        tp<float>(X)[r * ldx + j] = (float)src[r * src_ld + j];
    }
}

void HostDevice::extract_neg_t(DType dt, void* Lt, int64_t ldl, const void* X, int64_t ldx,
                               int64_t rows, int64_t col0, int64_t m, int) {
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t c = 0; c < m; ++c) {
      if (dt == DType::F64)
        tp<double>(Lt)[c * ldl + r] = -tp<double>(X)[r * ldx + col0 + c];
      else
        tp<float>(Lt)[c * ldl + r] = -tp<float>(X)[r * ldx + col0 + c];
    }
}

void HostDevice::add_diag(DType dt, void* A, int64_t ld, int64_t nd, double alpha, int) {
  for (int64_t i = 0; i < nd; ++i) {
    if (dt == DType::F64)
      tp<double>(A)[i * ld + i] += alpha;
    else
      tp<float>(A)[i * ld + i] += (float)alpha;
  }
}

void HostDevice::block_inverse(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                               int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                               int) {
  (void)nlive;
  const int64_t m = L.m;
  const double limit =
      dt == DType::F64 ? std::numeric_limits<double>::max() : (double)std::numeric_limits<float>::max();
  parallel_for(L.nblk, nthreads_, [&](int64_t b) {
    const int64_t g = L.global_block(b);
    if (used[g]) {
      valid[b] = 0;
      scores[b] = 0;
      return;
    }
    std::vector<double> W(m * m);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = 0; j < m; ++j)
        W[i * m + j] = (dt == DType::F64) ? -tp<double>(Lt)[j * ldl + b * m + i]
                                          : -(double)tp<float>(Lt)[j * ldl + b * m + i];
    std::vector<int64_t> prow(m);
    const bool ok = sweep_inverse(W, m, thresh, prow, limit);
    double sc = 0.0;
    if (ok)
      for (int64_t i = 0; i < m; ++i) {
        double s = 0.0;
        // the norm of the inverse as inv_t holds it: fp32 sums the rounded entries, like the GPU
        for (int64_t j = 0; j < m; ++j)
          s += std::fabs(dt == DType::F64 ? W[i * m + j] : (double)(float)W[i * m + j]);
        sc = max_keep_nan(sc, s);  // a NaN row sum must reach the test below (std::max drops it)
      }
    // a non-finite score: an entry of the block or of its sweep was NaN or Inf (Device::block_inverse)
    if (!ok || !std::isfinite(sc)) {
      valid[b] = 0;
      scores[b] = 0;
      return;
    }
    valid[b] = 1;
    scores[b] = sc;
    // Y[k][prow[u]] = W[prow[k]][u]; inv_t[j*m + i] = Y[i][j]
    for (int64_t k = 0; k < m; ++k)
      for (int64_t u = 0; u < m; ++u) {
        const double y = W[prow[k] * m + u];
        const int64_t idx = b * m * m + prow[u] * m + k;
        if (dt == DType::F64)
          tp<double>(inv_t)[idx] = y;
        else
          tp<float>(inv_t)[idx] = (float)y;
      }
  });
}

// The fused candidate-inverse + selection launch of the GPU (Device::block_inverse_select), for the
// same kernel family range (16 < m <= 128), so the CPU executes the GPU's op sequence.
bool HostDevice::block_inverse_select(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                                      int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                                      const PivotSelectArgs& sel, int s) {
  if (L.m <= 16 || L.m > 128 || L.nblk <= 0) return false;
  block_inverse(dt, Lt, ldl, inv_t, scores, valid, used, L, thresh, nlive, s);
  pivot_local(scores, valid, used, sel.pos, L, sel.rec, s);
  if (sel.single)
    pivot_global(sel.rec, 1, sel.t, sel.pos_w, sel.phys_at, sel.used_w, sel.seq, sel.out, sel.host_out, s);
  return true;
}

void HostDevice::candidate_maxabs(DType dt, const void* Lt, int64_t ldl, double* scores, int32_t* valid,
                                  const int32_t* used, const Layout& L, double thresh, int) {
  const int64_t m = L.m;
  for (int64_t b = 0; b < L.nblk; ++b) {
    if (used[L.global_block(b)]) {
      valid[b] = 0;
      scores[b] = 0;
      continue;
    }
    double mx = 0.0;
    for (int64_t c = 0; c < m; ++c)
      for (int64_t i = 0; i < m; ++i) {
        const int64_t idx = c * ldl + b * m + i;
        const double v = dt == DType::F64 ? tp<double>(Lt)[idx] : (double)tp<float>(Lt)[idx];
        mx = max_keep_nan(mx, std::fabs(v));  // a NaN entry invalidates the candidate
      }
    scores[b] = -mx;
    valid[b] = (mx >= thresh && std::isfinite(mx)) ? 1 : 0;
  }
}

void HostDevice::gather_candidate(DType dt, void* sel, const void* Lt, int64_t ldl, const PivotRec* rec,
                                  const Layout& L, int) {
  const int64_t m = L.m;
  const bool ok = rec->valid != 0;
  const int64_t b = ok ? rec->phys / L.p : 0;
  for (int64_t c = 0; c < m; ++c)
    for (int64_t i = 0; i < m; ++i) {
      const int64_t src = c * ldl + b * m + i, dst = c * m + i;
      if (dt == DType::F64)
        tp<double>(sel)[dst] = ok ? tp<double>(Lt)[src] : (c == i ? -1.0 : 0.0);
      else
        tp<float>(sel)[dst] = ok ? tp<float>(Lt)[src] : (c == i ? -1.0f : 0.0f);
    }
}

void HostDevice::commit_candidate(DType dt, void* inv_t, const void* inv1, const int32_t* valid1, const double* score1, double growth, PivotRec* rec,
                                  const Layout& L, int) {
  // growth guard: ||inv(W)||_inf * max|W| (score1 * -rec->score) above the bound counts as singular
  if (!rec->valid || !valid1[0] || (growth > 0 && !(score1[0] * -rec->score <= growth))) {
    rec->valid = 0;
    return;
  }
  const size_t blk = (size_t)L.m * L.m * dtype_size(dt);
  std::memcpy(static_cast<char*>(inv_t) + (size_t)(rec->phys / L.p) * blk, inv1, blk);
}

void HostDevice::pivot_local(const double* scores, const int32_t* valid, const int32_t* used,
                             const int32_t* pos, const Layout& L, PivotRec* out, int) {
  PivotRec best = pivot_invalid();
  for (int64_t b = 0; b < L.nblk; ++b) {
    const int64_t g = L.global_block(b);
    if (used[g] || !valid[b]) continue;
    PivotRec c;
    c.score = scores[b];
    c.logical = pos[g];
    c.phys = (int32_t)g;
    c.valid = 1;
    c.pad_ = 0;
    if (pivot_better(c, best, (int32_t)L.p)) best = c;
  }
  *out = best;
}

void HostDevice::pivot_global(const PivotRec* recs, int32_t p, int32_t t, int32_t* pos,
                              int32_t* phys_at, int32_t* used, int32_t* seq, PivotResult* out,
                              PivotResult* host_out, int) {
  PivotRec best = pivot_invalid();
  for (int32_t q = 0; q < p; ++q)
    if (pivot_better(recs[q], best, p)) best = recs[q];
  PivotResult r{};
  r.step = t;
  if (best.valid) {
    r.found = 1;
    r.phys = best.phys;
    r.owner = best.phys % p;
    r.logical = best.logical;
    r.score = best.score;
    pivot_commit(t, best.phys, pos, phys_at, used, seq);
  } else {
    seq[t] = -1;  // as the GPU kernel: the step's owner-predicated launches stay no-ops
    r.found = 0;
    r.phys = -1;
    r.owner = -1;
    r.logical = -1;
  }
  *out = r;
  if (host_out) *host_out = r;
}

void HostDevice::owner_edits(DType dt, void* At, int64_t ldl, const int32_t* phys, int64_t p, int64_t k,
                             int64_t j, int64_t m, void* lrow, void* ht, const void* inv, const PieceMove& mv,
                             int s) {
  const int64_t g = *phys;
  if (g < 0 || g % p != k) return;
  if (mv.w > 0) take_rows(dt, mv.dst, mv.ldd, mv.X, mv.ldx, phys, p, k, mv.col0, mv.w, m, s);
  if (mv.eye) {
    const size_t es = dtype_size(dt);
    for (int64_t r = 0; r < m; ++r)
      for (int64_t c = 0; c < m; ++c) {
        char* e = static_cast<char*>(mv.eye) + (r * mv.ld_eye + c) * (int64_t)es;
        if (dt == DType::F64) *reinterpret_cast<double*>(e) = r == c ? 1.0 : 0.0;
        else *reinterpret_cast<float*>(e) = r == c ? 1.0f : 0.0f;
      }
  }
  const int64_t row0 = (g / p) * m;
  auto run = [&](auto* a, auto* lr, auto* h, const auto* iv) {
    using T = std::remove_pointer_t<decltype(a)>;
    for (int64_t kk = 0; kk < (j + 1) * m; ++kk)
      for (int64_t c = 0; c < m; ++c) {
        T& x = a[kk * ldl + row0 + c];
        if (kk < j * m) lr[kk * m + c] = x;
        x = (kk - j * m == c) ? T(1) : T(0);
      }
    for (int64_t e = 0; e < m * m; ++e) h[e] = iv[(g / p) * m * m + e];
  };
  if (dt == DType::F64)
    run(static_cast<double*>(At), static_cast<double*>(lrow), static_cast<double*>(ht), static_cast<const double*>(inv));
  else
    run(static_cast<float*>(At), static_cast<float*>(lrow), static_cast<float*>(ht), static_cast<const float*>(inv));
}

void HostDevice::take_rows(DType dt, void* dst, int64_t ldd, void* X, int64_t ldx, const int32_t* phys, int64_t p,
                           int64_t k, int64_t col0, int64_t w, int64_t m, int) {
  const int64_t g = *phys;
  if (g < 0 || g % p != k || w <= 0) return;
  const size_t es = dtype_size(dt);
  const int64_t row0 = (g / p) * m;
  for (int64_t r = 0; r < m; ++r) {
    char* src = static_cast<char*>(X) + ((row0 + r) * ldx + col0) * (int64_t)es;
    std::memcpy(static_cast<char*>(dst) + r * ldd * (int64_t)es, src, (size_t)w * es);
    std::memset(src, 0, (size_t)w * es);
  }
}

void HostDevice::sum_slices(DType dt, void* dst, const void* src, int64_t count, int64_t nslices, int) {
  auto run = [&](auto* d, const auto* x) {
    using T = std::remove_pointer_t<decltype(d)>;
    for (int64_t i = 0; i < count; ++i) {
      T acc = x[i];
      for (int64_t q = 1; q < nslices; ++q) acc += x[q * count + i];
      d[i] = acc;
    }
  };
  if (dt == DType::F64) run(static_cast<double*>(dst), static_cast<const double*>(src));
  else run(static_cast<float*>(dst), static_cast<const float*>(src));
}

void HostDevice::zero_unless_owner(DType dt, void* buf, int64_t count, const int32_t* phys, int64_t p, int64_t k,
                                   int) {
  const int64_t g = *phys;
  if (g >= 0 && g % p == k) return;
  std::memset(buf, 0, (size_t)count * dtype_size(dt));
}

void HostDevice::h_block(DType dt, void* R, int64_t ldr, const void* Ht, int64_t m, int) {
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < m; ++j) {
      if (dt == DType::F64)
        tp<double>(R)[i * ldr + j] = tp<double>(Ht)[j * m + i];
      else
        tp<float>(R)[i * ldr + j] = tp<float>(Ht)[j * m + i];
    }
}

void HostDevice::gemm(DType dt, GemmOp op, ALayout al, int64_t M, int64_t N, int64_t K,
                      const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                      int, const GemmExtra& ex) {
  note_gemm_kernel("host");
  if (M <= 0 || N <= 0) return;
  if (dt == DType::F64)
    gemm_t<double>(op, al, M, N, K, tp<double>(A), lda, tp<double>(B), ldb, tp<double>(C), ldc,
                   nthreads_, ex);
  else
    gemm_t<float>(op, al, M, N, K, tp<float>(A), lda, tp<float>(B), ldb, tp<float>(C), ldc,
                  nthreads_, ex);
}

void HostDevice::permute_blocks(DType dt, void* dst, int64_t ldd, const void* X, int64_t ldx,
                                int64_t nblk, int64_t m, int64_t Nr, const int32_t* dst_blk,
                                const int32_t* colsrc, int) {
  const size_t es = dtype_size(dt);
  parallel_for(nblk * m, nthreads_, [&](int64_t row) {
    const int64_t b = row / m, r = row % m;
    char* d = static_cast<char*>(dst) + ((int64_t)dst_blk[b] * m + r) * ldd * es;
    const char* s = static_cast<const char*>(X) + (b * m + r) * ldx * es;
    for (int64_t c = 0; c < Nr; ++c)
      std::memcpy(d + c * m * es, s + (int64_t)colsrc[c] * m * es, m * es);
  });
}

void HostDevice::row_abs_max_minus_i(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                                     int) {
  double mx = 0.0;
  for (int64_t r = 0; r < L.rows; ++r) {
    const int64_t gr = L.global_row(r);
    if (gr >= L.n) continue;
    double s = 0.0;
    for (int64_t j = 0; j < L.n; ++j) {
      const double v = dt == DType::F64 ? tp<double>(X)[r * ldx + j] : (double)tp<float>(X)[r * ldx + j];
      s += std::fabs(v - (j == gr ? 1.0 : 0.0));
    }
    mx = max_keep_nan(mx, s);
  }
  out[0] = mx;
}

void HostDevice::hash_rows(const void* base, int64_t ld_bytes, int64_t width_bytes, int64_t rows,
                           uint64_t* parts, int) {
  const int64_t ww = width_bytes / 4;
  uint64_t h = 0;
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t w = 0; w < ww; ++w) {
      uint32_t v;
      std::memcpy(&v, static_cast<const char*>(base) + r * ld_bytes + 4 * w, 4);
      h += hash_term(v, (uint64_t)(r * ww + w));
    }
  parts[0] = h;
  for (int g = 1; g < kHashParts; ++g) parts[g] = 0;
}

void HostDevice::row_abs_max(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                             int) {
  double mx = 0.0;
  for (int64_t r = 0; r < L.rows; ++r) {
    if (L.global_row(r) >= L.n) continue;
    double s = 0.0;
    for (int64_t j = 0; j < L.n; ++j)
      s += std::fabs(dt == DType::F64 ? tp<double>(X)[r * ldx + j] : (double)tp<float>(X)[r * ldx + j]);
    mx = max_keep_nan(mx, s);
  }
  out[0] = mx;
}

void HostDevice::residual(DType dt, const void* A, const void* Full, const Layout& L, double* out,
                          int) {
  const int64_t np = L.npad;
  std::vector<double> rowres(L.rows, 0.0);
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const int64_t gr = L.global_row(r);
    if (gr >= L.n) return;
    std::vector<double> acc(L.n, 0.0);
    for (int64_t k = 0; k < L.n; ++k) {
      const double a = dt == DType::F64 ? tp<double>(A)[r * np + k] : (double)tp<float>(A)[r * np + k];
      if (a == 0.0) continue;
      for (int64_t j = 0; j < L.n; ++j)
        acc[j] += a * (dt == DType::F64 ? tp<double>(Full)[k * np + j]
                                        : (double)tp<float>(Full)[k * np + j]);
    }
    double s = 0.0;
    for (int64_t j = 0; j < L.n; ++j) s += std::fabs(acc[j] - (j == gr ? 1.0 : 0.0));
    rowres[r] = s;
  });
  double mx = 0.0;
  for (double v : rowres) mx = max_keep_nan(mx, v);
  out[0] = mx;
}


void HostDevice::panel_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                           int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign,
                           const int32_t* active, double* colmax, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "panel_rhs: 1 <= k <= 64 columns");
  g_last_rhs_kernel = "host";
  std::vector<double> rowmax((size_t)std::max<int64_t>(L.rows, 1) * k, 0.0);
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const bool real = L.global_row(r) < L.n;
    for (int64_t j = 0; j < k; ++j) {
      if (active && active[j] == 0) continue;
      double y = C_in ? C_in[r * ldc + j] : 0.0;
      if (real) {
        double prod;
        if (dt == DType::F64) {
          double acc = 0.0;
          for (int64_t c = 0; c < L.n; ++c) acc += tp<double>(P)[r * ldp + c] * V[c * ldv + j];
          prod = acc;
        } else {  // V rounded to fp32, fp32 accumulation, the product widened
          float acc = 0.0f;
          for (int64_t c = 0; c < L.n; ++c) acc += tp<float>(P)[r * ldp + c] * (float)V[c * ldv + j];
          prod = (double)acc;
        }
        y += sign * prod;
        rowmax[(size_t)(r * k + j)] = std::fabs(y);
      }
      Y[r * ldy + j] = y;
    }
  });
  if (!colmax) return;
  for (int64_t j = 0; j < k; ++j) {
    if (active && active[j] == 0) continue;
    double mx = 0.0;
    for (int64_t r = 0; r < L.rows; ++r) mx = max_keep_nan(mx, rowmax[(size_t)(r * k + j)]);
    colmax[j] = mx;
  }
}

// Dot2 (Ogita, Rump, Oishi): the pair starts as (C_in, 0), every term -P[r][c] V[c][j] enters by an exact
// product (fma) and a TwoSum whose errors collect in lo; one rounding at the end.  The error-free
// transforms need every operation as written: no contraction in this function.
void HostDevice::panel_rhs_dd(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                              int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy,
                              const int32_t* active, double* colmax, int) {
#pragma clang fp contract(off)
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "panel_rhs_dd: 1 <= k <= 64 columns");
  GJ_REQUIRE(dt == DType::F64, "panel_rhs_dd: the panel is fp64");
  g_last_rhs_dd_kernel = "host";
  std::vector<double> rowmax((size_t)std::max<int64_t>(L.rows, 1) * k, 0.0);
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
#pragma clang fp contract(off)
    const bool real = L.global_row(r) < L.n;
    for (int64_t j = 0; j < k; ++j) {
      if (active && active[j] == 0) continue;
      double y = C_in ? C_in[r * ldc + j] : 0.0;
      if (real) {
        double s = y, lo = 0.0;
        for (int64_t c = 0; c < L.n; ++c) {
          const double a = -tp<double>(P)[r * ldp + c], v = V[c * ldv + j];
          const double pr = a * v;
          const double e = std::fma(a, v, -pr);
          const double t = s + pr;
          const double z = t - s;
          const double sigma = (s - (t - z)) + (pr - z);
          s = t;
          lo += e + sigma;
        }
        y = s + lo;
        rowmax[(size_t)(r * k + j)] = std::fabs(y);
      }
      Y[r * ldy + j] = y;
    }
  });
  if (!colmax) return;
  for (int64_t j = 0; j < k; ++j) {
    if (active && active[j] == 0) continue;
    double mx = 0.0;
    for (int64_t r = 0; r < L.rows; ++r) mx = max_keep_nan(mx, rowmax[(size_t)(r * k + j)]);
    colmax[j] = mx;
  }
}

void HostDevice::gather_rows_natural(double* dst, int64_t ldd, const double* src, int64_t lds, const Layout& L,
                                     int64_t k, int) {
  const int64_t per = L.max_nblk * L.m;
  for (int64_t g = 0; g < L.n; ++g) {
    const int64_t gb = g / L.m, e = g % L.m;
    std::memcpy(dst + g * ldd, src + ((gb % L.p) * per + (gb / L.p) * L.m + e) * lds, sizeof(double) * (size_t)k);
  }
}

void HostDevice::copy_cols_masked(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t k,
                                  const int32_t* mask, int) {
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t j = 0; j < k; ++j)
      if (mask[j] != 0) dst[r * ldd + j] = src[r * lds + j];
}

void HostDevice::panel_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                             int64_t k, double* S, int64_t lds, const int32_t* active, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "panel_rhs_t: 1 <= k <= 64 columns");
  g_last_rhs_t_kernel = "host";
  parallel_for(L.n, nthreads_, [&](int64_t c) {
    for (int64_t j = 0; j < k; ++j) {
      double sum = 0.0;
      if (!active || active[j] != 0) {
        if (dt == DType::F64) {
          for (int64_t r = 0; r < L.rows; ++r) {
            const int64_t g = L.global_row(r);
            if (g < L.n) sum += tp<double>(P)[r * ldp + c] * V[g * ldv + j];
          }
        } else {  // V rounded to fp32, fp32 accumulation, the product widened
          float acc = 0.0f;
          for (int64_t r = 0; r < L.rows; ++r) {
            const int64_t g = L.global_row(r);
            if (g < L.n) acc += tp<float>(P)[r * ldp + c] * (float)V[g * ldv + j];
          }
          sum = (double)acc;
        }
      }
      S[c * lds + j] = sum;
    }
  });
}

void HostDevice::axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S,
                                  int64_t lds, double sign, int64_t rows, int64_t k, const int32_t* active,
                                  double* colmax, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "axpy_cols_masked: 1 <= k <= 64 columns");
  for (int64_t j = 0; j < k; ++j) {
    if (active && active[j] == 0) continue;
    double mx = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
      const double y = (C_in ? C_in[r * ldc + j] : 0.0) + sign * S[r * lds + j];
      Y[r * ldy + j] = y;
      mx = max_keep_nan(mx, std::fabs(y));
    }
    if (colmax) colmax[j] = mx;
  }
}

void HostDevice::col_abs_sum(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, int) {
  parallel_for(L.n, nthreads_, [&](int64_t c) {
    double sum = 0.0;
    for (int64_t r = 0; r < L.rows; ++r) {
      if (L.global_row(r) >= L.n) continue;
      sum += std::fabs(dt == DType::F64 ? tp<double>(X)[r * ldx + c] : (double)tp<float>(X)[r * ldx + c]);
    }
    out[c] = sum;
  });
}

void HostDevice::panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                               int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax,
                               int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "panel_abs_rhs: 1 <= k <= 64 columns");
  g_last_abs_kernel = "host";
  std::vector<double> rowmax((size_t)std::max<int64_t>(L.rows, 1) * k, 0.0);
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const bool real = L.global_row(r) < L.n;
    for (int64_t j = 0; j < k; ++j) {
      double y = C_in ? std::fabs(C_in[r * ldc + j]) : 0.0;
      if (real) {
        double acc = 0.0;  // fp64 for both dtypes
        for (int64_t c = 0; c < L.n; ++c)
          acc += std::fabs(dt == DType::F64 ? tp<double>(P)[r * ldp + c] : (double)tp<float>(P)[r * ldp + c]) *
                 std::fabs(V[c * ldv + j]);
        y += acc;
        rowmax[(size_t)(r * k + j)] = y;
      }
      Y[r * ldy + j] = y;
    }
  });
  if (!colmax) return;
  for (int64_t j = 0; j < k; ++j) {
    double mx = 0.0;
    for (int64_t r = 0; r < L.rows; ++r) mx = max_keep_nan(mx, rowmax[(size_t)(r * k + j)]);
    colmax[j] = mx;
  }
}

void HostDevice::panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                                 int64_t k, double* S, int64_t lds, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "panel_abs_rhs_t: 1 <= k <= 64 columns");
  g_last_abs_kernel = "host";
  parallel_for(L.n, nthreads_, [&](int64_t c) {
    for (int64_t j = 0; j < k; ++j) {
      double sum = 0.0;  // fp64 for both dtypes
      for (int64_t r = 0; r < L.rows; ++r) {
        const int64_t g = L.global_row(r);
        if (g >= L.n) continue;
        sum += std::fabs(dt == DType::F64 ? tp<double>(P)[r * ldp + c] : (double)tp<float>(P)[r * ldp + c]) *
               std::fabs(V[g * ldv + j]);
      }
      S[c * lds + j] = sum;
    }
  });
}

void HostDevice::bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg,
                             int64_t rows, int64_t k, double nz_eps, double safe1, double safe2, double* berr, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "bound_terms: 1 <= k <= 64 columns");
  for (int64_t j = 0; j < k; ++j) {
    double mx = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
      const double ar = std::fabs(R[r * ldr + j]), d = D[r * ldd + j];
      const bool tiny = d <= safe2;
      double g = std::fma(nz_eps, d, ar);  // one rounding
      if (tiny) g += safe1;
      G[r * ldg + j] = g;
      mx = max_keep_nan(mx, tiny ? (ar + safe1) / (d + safe1) : ar / d);
    }
    berr[j] = mx;
  }
}

void HostDevice::rank_update(DType dt, void* X, int64_t ldx, const Layout& L, const double* W, int64_t ldw,
                             bool w_natural, const double* Z, int64_t ldz, int64_t k, double sign, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "rank_update: 1 <= k <= 64 columns");
  g_last_rank_update_kernel = "host";
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const int64_t g = L.global_row(r);
    if (g >= L.n) return;
    const double* w = W + (w_natural ? g : r) * ldw;
    for (int64_t c = 0; c < L.n; ++c) {
      double sum = 0.0;  // fp64 for both dtypes, then one rounding
      for (int64_t j = 0; j < k; ++j) sum += w[j] * Z[c * ldz + j];
      if (dt == DType::F64)
        tp<double>(X)[r * ldx + c] += sign * sum;
      else
        tp<float>(X)[r * ldx + c] = (float)((double)tp<float>(X)[r * ldx + c] + sign * sum);
    }
  });
}

void HostDevice::grad_matrix(DType dt, const void* P, int64_t ldp, int64_t n, double alpha, const double* W,
                             int64_t ldw, const double* Z, int64_t ldz, int64_t k, double sign, bool accumulate,
                             double* G, int64_t ldg, int) {
  GJ_REQUIRE(n >= 0 && k >= 0 && k <= kMaxRhs, "grad_matrix: n >= 0 and 0 <= k <= 64 columns");
  g_last_grad_matrix_kernel = "host";
  parallel_for(n, nthreads_, [&](int64_t i) {
    for (int64_t j = 0; j < n; ++j) {
      double v = 0.0;  // fp64 for both dtypes, nothing rounded to dt
      if (k > 0) {
        double sum = 0.0;
        for (int64_t c = 0; c < k; ++c) sum += W[i * ldw + c] * Z[j * ldz + c];
        v = sign * sum;
      }
      if (alpha != 0.0) {
        const double t = alpha * (dt == DType::F64 ? tp<double>(P)[j * ldp + i] : (double)tp<float>(P)[j * ldp + i]);
        v = k > 0 ? t + v : t;
      }
      G[i * ldg + j] = accumulate ? G[i * ldg + j] + v : v;
    }
  });
}

void HostDevice::slogdet_batch(DType dt, const void* blocks, int64_t stride, int64_t m, int64_t nb,
                               const int32_t* which, double* sign, double* logabs, int) {
  GJ_REQUIRE(m >= 1 && nb >= 0 && stride >= m * m, "slogdet_batch: m >= 1, nb >= 0, stride >= m * m");
  g_last_slogdet_kernel = "host";
  parallel_for(nb, nthreads_, [&](int64_t b) {
    if (which && which[b] == 0) return;
    std::vector<double> a((size_t)(m * m));  // the fp64 copy: the input is not written
    bool bad = false;  // a NaN or an Inf entry: (NaN, NaN) whatever the pivots would do
    for (int64_t e = 0; e < m * m; ++e) {
      a[(size_t)e] = dt == DType::F64 ? tp<double>(blocks)[b * stride + e] : (double)tp<float>(blocks)[b * stride + e];
      bad = bad || !std::isfinite(a[(size_t)e]);
    }
    if (bad) {
      sign[b] = logabs[b] = std::numeric_limits<double>::quiet_NaN();
      return;
    }
    std::vector<int64_t> perm((size_t)m);
    for (int64_t i = 0; i < m; ++i) perm[(size_t)i] = i;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double sg = 1.0, lg = 0.0;
    for (int64_t c = 0; c < m; ++c) {
      // the largest magnitude of column c over the unused rows, NaN above everything, the first among equals
      int64_t ps = c;
      double pa = std::fabs(a[(size_t)(perm[(size_t)c] * m + c)]);
      for (int64_t i = c + 1; i < m && !std::isnan(pa); ++i) {
        const double v = std::fabs(a[(size_t)(perm[(size_t)i] * m + c)]);
        if (std::isnan(v) || v > pa) pa = v, ps = i;
      }
      if (ps != c) std::swap(perm[(size_t)ps], perm[(size_t)c]), sg = -sg;
      const double* prow = &a[(size_t)(perm[(size_t)c] * m)];
      const double piv = prow[c];
      if (!std::isfinite(piv)) {
        sg = lg = nan;
        break;
      }
      if (piv == 0.0) {
        sg = 0.0;
        lg = -std::numeric_limits<double>::infinity();
        break;
      }
      lg += std::log(std::fabs(piv));
      if (piv < 0.0) sg = -sg;
      for (int64_t i = c + 1; i < m; ++i) {
        double* row = &a[(size_t)(perm[(size_t)i] * m)];
        const double l = row[c] / piv;
        for (int64_t j = c + 1; j < m; ++j) row[j] -= l * prow[j];
      }
    }
    sign[b] = sg;
    logabs[b] = lg;
  });
}

// |x| as a key of the equilibration maxima: NaN and Inf count as +Inf
static inline double equil_mag(double x) {
  const double v = std::fabs(x);
  return v < std::numeric_limits<double>::infinity() ? v : std::numeric_limits<double>::infinity();
}

void HostDevice::abs_max_rows(DType dt, const void* X, int64_t ldx, const Layout& L, double* out_nat, int) {
  g_last_equil_kernel = "host";
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const int64_t g = L.global_row(r);
    if (g >= L.n) return;
    double mx = 0.0;
    for (int64_t c = 0; c < L.n; ++c)
      mx = std::max(mx, equil_mag(dt == DType::F64 ? tp<double>(X)[r * ldx + c] : (double)tp<float>(X)[r * ldx + c]));
    out_nat[g] = mx;
  });
}

void HostDevice::abs_max_cols(DType dt, const void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat,
                              double* out, int) {
  g_last_equil_kernel = "host";
  parallel_for(L.n, nthreads_, [&](int64_t c) {
    double mx = 0.0;
    for (int64_t r = 0; r < L.rows; ++r) {
      const int64_t g = L.global_row(r);
      if (g >= L.n) continue;
      const double v = equil_mag(dt == DType::F64 ? tp<double>(X)[r * ldx + c] : (double)tp<float>(X)[r * ldx + c]);
      mx = std::max(mx, std::ldexp(v, rexp_nat ? (int)rexp_nat[g] : 0));  // overflow: +Inf
    }
    out[c] = mx;
  });
}

void HostDevice::scale_pow2(DType dt, void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat,
                            const int32_t* cexp, int) {
  g_last_equil_kernel = "host";
  parallel_for(L.rows, nthreads_, [&](int64_t r) {
    const int64_t g = L.global_row(r);
    if (g >= L.n) return;
    const int64_t re = rexp_nat ? (int64_t)rexp_nat[g] : 0;
    for (int64_t c = 0; c < L.n; ++c) {
      const int64_t e64 = re + (cexp ? (int64_t)cexp[c] : 0);
      const int e = (int)std::max<int64_t>(-100000, std::min<int64_t>(100000, e64));  // (saturated either way)
      // exact in fp64 for an fp32 element within any exponents an fp32 panel can produce; one rounding
      if (dt == DType::F64)
        tp<double>(X)[r * ldx + c] = std::ldexp(tp<double>(X)[r * ldx + c], e);
      else
        tp<float>(X)[r * ldx + c] = (float)std::ldexp((double)tp<float>(X)[r * ldx + c], e);
    }
  });
}

void HostDevice::batch_pack(DType dt, const double* A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m,
                            int64_t nb, void* Lt, int64_t ldl, double* norm, int32_t* exp, int) {
  GJ_REQUIRE(n >= 1 && m >= n && nb >= 0 && lda >= n && ldl >= nb * m,
             "batch_pack: 1 <= n <= m, nb >= 0, lda >= n, ldl >= nb * m");
  g_last_batch_kernel = "host";
  parallel_for(nb, nthreads_, [&](int64_t b) {
    const double* A = A64 + b * stride_a;
    double mx = 0.0;
    for (int64_t r = 0; r < n; ++r) {
      double sum = 0.0;
      for (int64_t c = 0; c < n; ++c) sum += std::fabs(A[r * lda + c]);
      mx = max_keep_nan(mx, sum);
    }
    const int e = equil_exponent(mx);
    norm[b] = mx;
    exp[b] = e;
    for (int64_t c = 0; c < m; ++c)
      for (int64_t r = 0; r < m; ++r) {
        const double v = (r < n && c < n) ? -std::ldexp(A[r * lda + c], e) : (r < n || c < n) ? 0.0 : r == c ? -1.0 : 0.0;
        if (dt == DType::F64)
          tp<double>(Lt)[c * ldl + b * m + r] = v;
        else
          tp<float>(Lt)[c * ldl + b * m + r] = (float)v;
      }
  });
}

void HostDevice::batch_unpack(DType dt, const void* inv_t, int64_t n, int64_t m, int64_t nb, const int32_t* exp,
                              const int32_t* valid, void* X, int64_t stride_x, int64_t ldx, int) {
  GJ_REQUIRE(n >= 1 && m >= n && nb >= 0 && ldx >= n, "batch_unpack: 1 <= n <= m, nb >= 0, ldx >= n");
  g_last_batch_kernel = "host";
  parallel_for(nb, nthreads_, [&](int64_t b) {
    const bool ok = valid[b] != 0;
    const int e = exp[b];
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < n; ++j) {
        const int64_t src = b * m * m + j * m + i, dst = b * stride_x + i * ldx + j;
        if (dt == DType::F64)
          tp<double>(X)[dst] = ok ? std::ldexp(tp<double>(inv_t)[src], e) : std::numeric_limits<double>::quiet_NaN();
        else
          tp<float>(X)[dst] =
              ok ? (float)std::ldexp((double)tp<float>(inv_t)[src], e) : std::numeric_limits<float>::quiet_NaN();
      }
  });
}

void HostDevice::batch_rhs(DType dt, const void* M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb,
                           const double* V, int64_t stride_v, int64_t ldv, int64_t k, const double* C_in,
                           int64_t stride_c, int64_t ldc, double* Y, int64_t stride_y, int64_t ldy, double sign,
                           const int32_t* active, double* colmax, int) {
  GJ_REQUIRE(k >= 1 && k <= kMaxRhs, "batch_rhs: 1 <= k <= 64 columns");
  GJ_REQUIRE(n >= 1 && nb >= 0, "batch_rhs: n >= 1, nb >= 0");
  g_last_batch_kernel = "host";
  parallel_for(nb, nthreads_, [&](int64_t b) {
    const double* Vb = V + b * stride_v;
    const double* Cb = C_in ? C_in + b * stride_c : nullptr;
    double* Yb = Y + b * stride_y;
    for (int64_t j = 0; j < k; ++j) {
      if (active && active[b * k + j] == 0) continue;
      double mx = 0.0;
      for (int64_t r = 0; r < n; ++r) {
        double acc = 0.0;  // fp64 for both dtypes
        for (int64_t c = 0; c < n; ++c)
          acc += (dt == DType::F64 ? tp<double>(M)[b * stride_m + r * ldm + c]
                                   : (double)tp<float>(M)[b * stride_m + r * ldm + c]) *
                 Vb[c * ldv + j];
        const double y = (Cb ? Cb[r * ldc + j] : 0.0) + sign * acc;
        Yb[r * ldy + j] = y;
        mx = max_keep_nan(mx, std::fabs(y));
      }
      if (colmax) colmax[b * k + j] = mx;
    }
  });
}

}  // namespace gj
