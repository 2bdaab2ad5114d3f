// BatchSolver: inverses, refined solves and determinants of a stack of small matrices on one device
// (gj/batch.hpp for the contract).
#include "gj/batch.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

#include "gj/column_rule.hpp"

namespace gj {

namespace {
// nb matrices of rows x width_bytes, rows pitch bytes and matrices stride bytes apart, into / out of a
// contiguous image: one copy where the layouts allow it, one per matrix otherwise
void copy_stack(Device& dev, void* dst, size_t dstride, size_t dpitch, const void* src, size_t sstride, size_t spitch,
                size_t width_bytes, int64_t rows, int64_t nb) {
  if (nb <= 0) return;
  if (dstride == (size_t)rows * dpitch && sstride == (size_t)rows * spitch) {
    dev.copy2d(dst, dpitch, src, spitch, width_bytes, (size_t)(rows * nb), S_MAIN);
    return;
  }
  for (int64_t b = 0; b < nb; ++b)
    dev.copy2d(static_cast<char*>(dst) + b * dstride, dpitch, static_cast<const char*>(src) + b * sstride, spitch,
               width_bytes, (size_t)rows, S_MAIN);
}
}  // namespace

BatchSolver::BatchSolver(Device& dev, DType dt, int64_t n, int64_t nb, double eps, size_t workspace_bytes)
    : dev_(dev), dt_(dt), n_(n), nb_(nb), m_(std::max(n, kMinBlock)), eps_(eps),
      ws_(workspace_bytes ? workspace_bytes : kDefaultWorkspace) {
  GJ_REQUIRE(n >= 1 && n <= kMaxOrder, "BatchSolver: 1 <= n <= 1024 (a larger matrix is the engine's: gj.factor)");
  GJ_REQUIRE(nb >= 1 && nb < (int64_t(1) << 31) / m_, "BatchSolver: 1 <= nb and nb * max(n, 16) < 2^31");
  const size_t es = dtype_size(dt_);
  // The working set of a chunk of cb matrices: the packed panel, inv_t and block_inverse's scratch for
  // that layout.  The largest cb that fits (at least 1), and a panel of at most 1 GiB.
  auto need = [&](int64_t cb) {
    return 2 * (size_t)cb * m_ * m_ * es + dev_.block_inverse_scratch_bytes(dt_, Layout::make(cb * m_, m_, 1, 0), -1);
  };
  const int64_t cap = std::max<int64_t>(1, (int64_t)((size_t(1) << 30) / ((size_t)m_ * m_ * es)));
  int64_t lo = 1, hi = std::min(nb_, cap);
  while (lo < hi) {  // need() grows with cb
    const int64_t mid = (lo + hi + 1) / 2;
    if (need(mid) <= ws_) lo = mid;
    else hi = mid - 1;
  }
  chunk_ = lo;
  const size_t nn = (size_t)n_ * n_;
  a64_ = DevBuf<double>::device(dev_, (size_t)nb_ * nn, "batch.a64");
  inv_ = DevBuf<void>::device(dev_, (size_t)nb_ * nn * es, "batch.inv");
  dnorm_ = DevBuf<double>::device(dev_, (size_t)nb_, "batch.norm");
  dexp_ = DevBuf<int32_t>::device(dev_, (size_t)nb_, "batch.exp");
  dvalid_ = DevBuf<int32_t>::device(dev_, (size_t)nb_, "batch.valid");
}

void BatchSolver::factor(const double* A, int64_t stride_a, int64_t lda) {
  GJ_REQUIRE(A && lda >= n_, "BatchSolver::factor: A with lda >= n");
  const size_t es = dtype_size(dt_);
  const int64_t n = n_, m = m_, nn = n * n;
  factored_ = false;
  copy_stack(dev_, a64_, (size_t)nn * 8, (size_t)n * 8, A, (size_t)stride_a * 8, (size_t)lda * 8, (size_t)n * 8, n, nb_);

  const int64_t cb0 = chunk_;
  auto Lt = DevBuf<void>::device(dev_, (size_t)cb0 * m * m * es, "batch.Lt");
  auto inv_t = DevBuf<void>::device(dev_, (size_t)cb0 * m * m * es, "batch.inv_t");
  auto scores = DevBuf<double>::device(dev_, (size_t)nb_, "batch.scores");
  auto used = DevBuf<int32_t>::device(dev_, (size_t)cb0, "batch.used");
  DrainOnExit drain{dev_};  // after the buffers: runs before they go
  dev_.memset0(used, sizeof(int32_t) * cb0, S_MAIN);
  dev_.prepare_block_inverse(dt_, Layout::make(cb0 * m, m, 1, 0), -1);
  for (int64_t b0 = 0; b0 < nb_; b0 += cb0) {
    const int64_t cb = std::min(cb0, nb_ - b0);
    const Layout L = Layout::make(cb * m, m, 1, 0);
    dev_.batch_pack(dt_, a64_.get() + b0 * nn, nn, n, n, m, cb, Lt, cb * m, dnorm_.get() + b0, dexp_.get() + b0, S_MAIN);
    dev_.block_inverse(dt_, Lt, cb * m, inv_t, scores.get() + b0, dvalid_.get() + b0, used, L, eps_, -1, S_MAIN);
    dev_.batch_unpack(dt_, inv_t, n, m, cb, dexp_.get() + b0, dvalid_.get() + b0, static_cast<char*>(inv_.get()) + b0 * nn * es, nn,
                      n, S_MAIN);
  }
  valid_.assign((size_t)nb_, 0);
  exp_.assign((size_t)nb_, 0);
  norm_.assign((size_t)nb_, 0.0);
  inorm_.assign((size_t)nb_, 0.0);
  dev_.copy(valid_.data(), dvalid_, sizeof(int32_t) * nb_, S_MAIN);
  dev_.copy(exp_.data(), dexp_, sizeof(int32_t) * nb_, S_MAIN);
  dev_.copy(norm_.data(), dnorm_, sizeof(double) * nb_, S_MAIN);
  dev_.copy(inorm_.data(), scores, sizeof(double) * nb_, S_MAIN);
  dev_.sync_stream(S_MAIN);
  // scores[b] = ||inv(As_b)||_inf; inv(A_b) = 2^e_b inv(As_b)
  for (int64_t b = 0; b < nb_; ++b)
    inorm_[(size_t)b] = valid_[(size_t)b] ? std::ldexp(inorm_[(size_t)b], exp_[(size_t)b]) : 0.0;
  factored_ = true;
}

void BatchSolver::inverse(void* X, int64_t stride_x, int64_t ldx) const {
  GJ_REQUIRE(factored_, "BatchSolver::inverse: factor() first");
  GJ_REQUIRE(X && ldx >= n_, "BatchSolver::inverse: X with ldx >= n");
  const size_t es = dtype_size(dt_);
  copy_stack(dev_, X, (size_t)stride_x * es, (size_t)ldx * es, inv_.get(), (size_t)n_ * n_ * es, (size_t)n_ * es,
             (size_t)n_ * es, n_, nb_);
  dev_.sync_stream(S_MAIN);
}

void BatchSolver::slogdet(double* sign, double* logabs) {
  GJ_REQUIRE(factored_, "BatchSolver::slogdet: factor() first");
  auto out = DevBuf<double>::device(dev_, 2 * (size_t)nb_, "batch.det");
  DrainOnExit drain{dev_};
  dev_.prepare_slogdet(n_, nb_);
  dev_.slogdet_batch(DType::F64, a64_, n_ * n_, n_, nb_, nullptr, out.get(), out.get() + nb_, S_MAIN);
  dev_.copy(sign, out, sizeof(double) * nb_, S_MAIN);
  dev_.copy(logabs, out.get() + nb_, sizeof(double) * nb_, S_MAIN);
  dev_.sync_stream(S_MAIN);
}

// X comes back stack-interleaved, X[(r * nb + b) * k + j]: the layout of the work buffers, in which a
// matrix's columns are columns b * k + j of one n-row array -- batch_rhs addresses it by its strides,
// and one copy_cols_masked with the (matrix, column) flags serves the whole stack.
BatchSolveInfo BatchSolver::solve(const double* B, int64_t stride_b, int64_t ldb, double* X, int64_t k, int max_refine,
                                  double tol) {
  GJ_REQUIRE(factored_, "BatchSolver::solve: factor() first");
  GJ_REQUIRE(B && X && k >= 1 && ldb >= k, "BatchSolver::solve: k >= 1 columns, ldb >= k");
  if (max_refine < 0) max_refine = dt_ == DType::F64 ? 2 : 10;
  const int64_t n = n_, nb = nb_, nn = n * n;
  const int64_t kw = std::min<int64_t>(k, Device::kMaxRhs);
  BatchSolveInfo out;
  out.k = k;
  out.converged.assign((size_t)(nb * k), 0);
  out.steps.assign((size_t)(nb * k), 0);
  out.residual.assign((size_t)(nb * k), std::numeric_limits<double>::quiet_NaN());
  out.backward_error.assign((size_t)(nb * k), std::numeric_limits<double>::quiet_NaN());

  std::vector<DevBuf<void>> held;
  DrainOnExit drain{dev_};  // after `held`: runs before the buffers go
  auto dbuf = [&](size_t bytes, const char* name) {
    held.push_back(DevBuf<void>::device(dev_, std::max<size_t>(bytes, 1), name));
    return held.back().get();
  };
  auto pbuf = [&](size_t bytes) {
    held.push_back(DevBuf<void>::pinned(dev_, std::max<size_t>(bytes, 1)));
    return held.back().get();
  };
  const size_t NW = (size_t)nb * kw;
  const double* Bd = B;
  const int64_t sb = stride_b, lb = ldb;
  double* Xd = X;
  double* x = static_cast<double*>(dbuf(NW * n * 8, "batch.x"));
  double* r = static_cast<double*>(dbuf(NW * n * 8, "batch.r"));
  double* best = static_cast<double*>(dbuf(NW * n * 8, "batch.best"));
  double* dnorm = static_cast<double*>(dbuf(2 * NW * 8, "batch.colnorm"));  // ||r_j|| | ||x_j||
  int32_t* dflag = static_cast<int32_t*>(dbuf(2 * NW * 4, "batch.flags"));  // active | save-mask
  double* hnorm = static_cast<double*>(pbuf(2 * NW * 8));
  int32_t* hflag = static_cast<int32_t*>(pbuf(2 * NW * 4));
  dev_.memset0(dnorm, 2 * NW * 8, S_MAIN);
  const void* inv = inv_.get();

  for (int64_t c0 = 0; c0 < k; c0 += kw) {
    const int64_t kg = std::min<int64_t>(kw, k - c0);
    const int64_t N = nb * kg;  // (matrix, column) pairs of the group = columns of the work arrays
    const double* Bg = Bd + c0;
    // the columns of the valid matrices are active
    dev_.host_access(hflag, sizeof(int32_t) * 2 * NW, true);
    for (int64_t b = 0; b < nb; ++b)
      for (int64_t j = 0; j < kg; ++j) hflag[b * kg + j] = valid_[(size_t)b] ? 1 : 0;
    dev_.copy(dflag, hflag, sizeof(int32_t) * N, S_MAIN);
    // ||b_j|| per (matrix, column).  On the GPU from the op that is there: Y = B + A 0 is B (a valid
    // matrix is finite) and its column maxima are the norms -- one pass over A instead of B's way to the host.
    std::vector<double> bn((size_t)N, 0.0);
    if (dev_.on_gpu()) {
      dev_.memset0(x, (size_t)N * n * 8, S_MAIN);
      dev_.batch_rhs(DType::F64, a64_, nn, n, n, nb, x, kg, N, kg, Bg, sb, lb, r, kg, N, 1.0, dflag, dnorm, S_MAIN);
      dev_.copy(hnorm, dnorm, sizeof(double) * N, S_MAIN);
      dev_.sync_stream(S_MAIN);
      dev_.host_access(hnorm, sizeof(double) * 2 * NW, false);
      for (int64_t b = 0; b < nb; ++b)
        if (valid_[(size_t)b])
          for (int64_t j = 0; j < kg; ++j) bn[(size_t)(b * kg + j)] = hnorm[b * kg + j];
    } else {
      const double* bh = B + c0;
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t i = 0; i < n; ++i)
          for (int64_t j = 0; j < kg; ++j)
            bn[(size_t)(b * kg + j)] =
                std::max(bn[(size_t)(b * kg + j)], std::fabs(bh[b * stride_b + i * ldb + j]));
    }
    for (double& v : bn)
      if (v == 0) v = 1;

    // x_0 = inv(A) b in the stack's dtype, every column (an invalid matrix's inverse is NaN, so is its x)
    dev_.batch_rhs(dt_, inv, nn, n, n, nb, Bg, sb, lb, kg, nullptr, 0, 0, x, kg, N, 1.0, nullptr, dnorm + N, S_MAIN);

    std::vector<ColumnRule> rule((size_t)N);
    std::vector<RhsResult> rr((size_t)N);
    for (int64_t b = 0; b < nb; ++b)
      if (!valid_[(size_t)b])
        for (int64_t j = 0; j < kg; ++j) rule[(size_t)(b * kg + j)].active = false;
    for (int it = 0;; ++it) {
      // r = b - A x in fp64 against the kept copy of A
      dev_.batch_rhs(DType::F64, a64_, nn, n, n, nb, x, kg, N, kg, Bg, sb, lb, r, kg, N, -1.0, dflag, dnorm, S_MAIN);
      dev_.copy(hnorm, dnorm, sizeof(double) * N, S_MAIN);
      dev_.copy(hnorm + N, dnorm + N, sizeof(double) * N, S_MAIN);
      dev_.sync_stream(S_MAIN);
      dev_.host_access(hnorm, sizeof(double) * 2 * NW, false);
      out.sweeps = std::max(out.sweeps, it + 1);
      // the per-column decision
      dev_.host_access(hflag, sizeof(int32_t) * 2 * NW, true);
      bool any = false;
      for (int64_t b = 0; b < nb; ++b)
        for (int64_t j = 0; j < kg; ++j) {
          const int64_t c = b * kg + j;
          ColumnRule& cr = rule[(size_t)c];
          hflag[N + c] = cr.active && cr.step(rr[(size_t)c], it, hnorm[c], hnorm[N + c], norm_[(size_t)b],
                                              bn[(size_t)c], max_refine, tol);
          if (it == 0 && !valid_[(size_t)b]) hflag[N + c] = 1;  // its NaN iterate is the one returned
          hflag[c] = cr.active;
          any = any || cr.active;
        }
      dev_.copy(dflag, hflag, sizeof(int32_t) * 2 * N, S_MAIN);
      dev_.copy_cols_masked(best, N, x, N, n, N, dflag + N, S_MAIN);
      if (!any) break;
      // x += inv(A) r for the columns still active (the stack's dtype, added in fp64)
      dev_.batch_rhs(dt_, inv, nn, n, n, nb, r, kg, N, kg, x, kg, N, x, kg, N, 1.0, dflag, dnorm + N, S_MAIN);
    }
    // every column's returned iterate is in `best`: rows of nb * kg into rows of nb * k, at column c0
    dev_.copy2d(Xd + c0, (size_t)k * 8, best, (size_t)kg * 8, (size_t)kg * 8, (size_t)(n * nb), S_MAIN);
    dev_.sync_stream(S_MAIN);
    for (int64_t b = 0; b < nb; ++b)
      for (int64_t j = 0; j < kg; ++j) {
        if (!valid_[(size_t)b]) continue;
        const RhsResult& q = rr[(size_t)(b * kg + j)];
        const size_t o = (size_t)(b * k + c0 + j);
        out.converged[o] = q.converged ? 1 : 0;
        out.steps[o] = q.steps;
        out.residual[o] = q.residual;
        out.backward_error[o] = q.backward_error;
      }
  }
  return out;
}

}  // namespace gj
