// What works from the resident inverse after Engine::solve(): A x = b, A X = B and A^T X = B with
// iterative refinement in fp64, and the low-rank update of the inverse.  One column rule
// (ColumnRule), one staging of A's rows (Engine::stage_rows_f64) and one block driver
// (Engine::solve_rhs_block_impl) serve every path -- see gj/engine.hpp for the contracts.
#include "gj/engine.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <limits>

#include "gj/column_rule.hpp"

namespace gj {

namespace {
// full n-vector (double, host) -> padded device vector of the engine dtype
DevBuf<void> upload_vector(Device& dev, DType dt, const double* v, int64_t n, int64_t npad) {
  const auto st = DevBuf<double>::device(dev, (size_t)npad);
  dev.memset0(st, sizeof(double) * npad, S_MAIN);
  dev.copy(st, v, sizeof(double) * n, S_MAIN);
  auto d = DevBuf<void>::device(dev, dtype_size(dt) * npad);
  dev.upload_convert(dt, d, 1, st, 1, npad, 1, S_MAIN);
  dev.sync_stream(S_MAIN);
  return d;
}

// local product y = P * v  (P: this rank's rows of a panel, v: full padded vector) -> host doubles
std::vector<double> local_matvec(Device& dev, DType dt, const void* P, const Layout& L, const void* vd) {
  const size_t es = dtype_size(dt);
  std::vector<double> y((size_t)L.rows, 0.0);
  if (L.rows == 0) return y;
  const auto yd = DevBuf<void>::device(dev, es * L.rows);
  dev.gemm(dt, GemmOp::Store, ALayout::RowMajor, L.rows, 1, L.npad, P, L.npad, vd, 1, yd, 1, S_MAIN);
  std::vector<char> h(es * L.rows);
  dev.copy(h.data(), yd, es * L.rows, S_MAIN);
  dev.sync_stream(S_MAIN);
  for (int64_t i = 0; i < L.rows; ++i)
    y[i] = dt == DType::F64 ? reinterpret_cast<double*>(h.data())[i] : (double)reinterpret_cast<float*>(h.data())[i];
  return y;
}

// device / pinned buffers of one call, released together (after the device went idle)
struct BufSet {
  Device& dev;
  std::vector<DevBuf<void>> held;
  DrainOnExit drain{dev};  // after `held`: runs before the buffers go
  explicit BufSet(Device& d) : dev(d) {}
  template <typename T>
  T* get(size_t count, bool zero = true) {
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    held.push_back(DevBuf<void>::device(dev, bytes));
    if (zero) dev.memset0(held.back(), bytes, S_MAIN);
    return static_cast<T*>(held.back().get());
  }
  template <typename T>
  T* get_pinned(size_t count) {
    held.push_back(DevBuf<void>::pinned(dev, sizeof(T) * std::max<size_t>(count, 1)));
    return static_cast<T*>(held.back().get());
  }
};
}  // namespace

void Engine::apply_inverse(const double* b, double* x) {
  GJ_REQUIRE(solved_, "apply_inverse: solve() first");
  const int64_t m = L_.m, n = L_.n, p = L_.p;
  std::vector<double> mine = local_matvec(dev_, opt_.dtype, out_, L_, upload_vector(dev_, opt_.dtype, b, n, L_.npad));
  const int64_t per = L_.max_nblk * m;
  mine.resize((size_t)per, 0.0);
  std::vector<double> all((size_t)per * p);
  comm_.host_allgather(dev_, mine.data(), all.data(), sizeof(double) * per);
  for (int64_t q = 0; q < p; ++q)
    for (int64_t j = 0; j < rows_owned(L_.Nr, p, q); ++j)
      for (int64_t r = 0; r < m; ++r) {
        const int64_t gi = (j * p + q) * m + r;
        if (gi < n) x[gi] = all[(size_t)q * per + j * m + r];
      }
}

double Engine::axb_residual(const double* x, const double* b) {
  const int64_t m = L_.m, n = L_.n;
  const std::vector<double> y = local_matvec(dev_, opt_.dtype, X_, L_, upload_vector(dev_, opt_.dtype, x, n, L_.npad));
  double local = 0.0;
  for (int64_t i = 0; i < L_.rows; ++i) {
    const int64_t gi = L_.global_block(i / m) * m + i % m;
    if (gi < n) local = std::max(local, std::fabs(y[i] - b[gi]));
  }
  return comm_.host_max(dev_, local);
}

// This rank's rows of A in fp64 into Aw (ld npad), from the generator, from an fp64 device array or
// from host rows.  Enqueues on MAIN; does not wait.
void Engine::stage_rows_f64(double* Aw, const GenSpec* gen, const double* host_rows, const void* dev_rows,
                            int64_t ld) {
  if (gen) {
    dev_.generate(DType::F64, Aw, L_, *gen, S_MAIN);
  } else if (dev_rows) {  // zero + identity padding, then the real rows device-to-device
    GenSpec z;
    z.kind = GenKind::Zero;
    dev_.generate(DType::F64, Aw, L_, z, S_MAIN);
    const int64_t real = real_local_rows();
    if (real > 0) dev_.copy2d(Aw, L_.npad * 8, dev_rows, ld * 8, L_.n * 8, real, S_MAIN);
  } else {
    upload_rows_into(Aw, DType::F64, host_rows, ld);
  }
}

// ---------------------------------------------------------------- A x = b
// x = inv(A) b, then iterative refinement with the residual in fp64:
//   r_k = b - A x_k  (A in fp64: regenerated, or re-uploaded from the caller's fp64 rows;
//                     fp64 MFMA GEMV, the full vector all-gathered)
//   x_{k+1} = x_k + X r_k   (X = the computed inverse, engine dtype)
// It converges when ||I - X A|| < 1; each step gains about -log10 ||I - X A|| digits.  Stops at
// the normwise backward error ||r|| / (||A|| ||x|| + ||b||) <= tol (inf-norms), after max_refine
// steps, or when the residual stops shrinking
// (refinement cannot converge: reported, not hidden).
RhsResult Engine::solve_rhs_device(const double* b, double* x, const void* dev_rows_f64, int64_t ld,
                                   int max_refine, double tol) {
  GJ_REQUIRE(dev_rows_f64 || real_local_rows() == 0, "solve_rhs_device: the matrix rows are needed");
  return solve_rhs_impl(b, x, nullptr, nullptr, dev_rows_f64, ld, max_refine, tol);
}

RhsResult Engine::solve_rhs(const double* b, double* x, const GenSpec* gen, const double* host_rows,
                            int64_t ld, int max_refine, double tol) {
  GJ_REQUIRE(gen || host_rows || real_local_rows() == 0,
             "solve_rhs: the matrix (generator or rows) is needed for the fp64 residual");
  return solve_rhs_impl(b, x, gen, host_rows, nullptr, ld, max_refine, tol);
}

RhsResult Engine::solve_rhs_impl(const double* b, double* x, const GenSpec* gen, const double* host_rows,
                                const void* dev_rows, int64_t ld, int max_refine, double tol) {
  GJ_REQUIRE(solved_, "solve_rhs: solve() first");
  const int64_t m = L_.m, n = L_.n;
  RhsResult rr;
  const auto Aw = DevBuf<double>::device(dev_, (size_t)std::max<int64_t>(L_.rows, 1) * L_.npad);
  stage_rows_f64(Aw, gen, host_rows, dev_rows, ld);
  dev_.sync_stream(S_MAIN);
  double bn = 0;
  for (int64_t i = 0; i < n; ++i) bn = std::max(bn, std::fabs(b[i]));
  if (bn == 0) bn = 1;
  dev_.row_abs_max(DType::F64, Aw, L_.npad, L_, dscratch_, S_MAIN);  // ||A||_inf (fp64)
  dev_.copy(dhost_, dscratch_, sizeof(double), S_MAIN);
  dev_.sync_stream(S_MAIN);
  const double an = comm_.host_max(dev_, L_.nblk > 0 ? dhost_[0] : 0.0);
  apply_inverse(b, x);
  std::vector<double> r((size_t)n), d((size_t)n);
  std::vector<double> best_x(x, x + n);  // the iterate to return
  ColumnRule rule;
  for (int it = 0;; ++it) {
    // r = b - A x (this rank's rows, fp64), all-gathered to the full vector
    const std::vector<double> y =
        local_matvec(dev_, DType::F64, Aw, L_, upload_vector(dev_, DType::F64, x, n, L_.npad));
    const int64_t per = L_.max_nblk * m;
    std::vector<double> mine((size_t)per, 0.0), all((size_t)per * L_.p);
    for (int64_t i = 0; i < L_.rows; ++i) {
      const int64_t gi = L_.global_block(i / m) * m + i % m;
      if (gi < n) mine[(size_t)i] = b[gi] - y[(size_t)i];
    }
    comm_.host_allgather(dev_, mine.data(), all.data(), sizeof(double) * per);
    double rn = 0;
    for (int64_t q = 0; q < L_.p; ++q)
      for (int64_t j = 0; j < rows_owned(L_.Nr, L_.p, q); ++j)
        for (int64_t e = 0; e < m; ++e) {
          const int64_t gi = (j * L_.p + q) * m + e;
          if (gi < n) {
            r[(size_t)gi] = all[(size_t)q * per + j * m + e];
            rn = std::max(rn, std::fabs(r[(size_t)gi]));
          }
        }
    double xn = 0;
    for (int64_t i = 0; i < n; ++i) xn = std::max(xn, std::fabs(x[i]));
    if (rule.step(rr, it, rn, xn, an, bn, max_refine, tol)) best_x.assign(x, x + n);
    if (!rule.active) break;
    apply_inverse(r.data(), d.data());
    for (int64_t i = 0; i < n; ++i) x[i] += d[(size_t)i];
  }
  std::copy(best_x.begin(), best_x.end(), x);
  return rr;
}

// ---------------------------------------------------------------- A X = B, a block of columns
RhsBlockResult Engine::solve_rhs_block(const double* B, int64_t ldb, double* X, int64_t ldx, int64_t k,
                                       const GenSpec* gen, const double* host_rows, const void* dev_rows_f64,
                                       int64_t ld, int max_refine, double tol, bool trans, bool bounds,
                                       bool precise) {
  return solve_rhs_block_impl(B, ldb, X, ldx, k, false, gen, host_rows, dev_rows_f64, ld, max_refine, tol, trans,
                              bounds, precise);
}

RhsBlockResult Engine::solve_rhs_block_device(const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx,
                                              int64_t k, const GenSpec* gen, const double* host_rows,
                                              const void* dev_rows_f64, int64_t ld, int max_refine, double tol,
                                              bool trans, bool bounds, bool precise) {
  return solve_rhs_block_impl(B_dev, ldb, X_dev, ldx, k, true, gen, host_rows, dev_rows_f64, ld, max_refine, tol,
                              trans, bounds, precise);
}

// What A X = B and A^T X = B differ in, for the block driver.  Vb / Vx / Vr hold B, the iterate and
// the residual in natural row order (n rows, ld kw) on every rank; a product reads one of them.
struct Engine::BlockPath {
  BufSet bufs;
  explicit BlockPath(Device& d) : bufs(d) {}
  double an = 0;                                  // the ||A|| of the backward error
  double *Vb = nullptr, *Vx = nullptr, *Vr = nullptr;
  // what a product adds to (b, x) and writes (x, r), and the best iterate: xrows rows, ld kw
  double *b = nullptr, *x = nullptr, *r = nullptr, *best = nullptr;
  int64_t xrows = 0;
  std::function<void(int64_t kg)> begin_group;    // before a group's B is staged (may be empty)
  std::function<void()> stage_b;                  // b from Vb (may be empty)
  // dst = C + sign * (P or P^T) V for the columns `act`, colmax = their column norms; `nat` is the
  // natural-order buffer that mirrors dst
  std::function<void(DType dt, const void* P, const double* V, int64_t kg, const double* C, double* dst,
                     double* nat, double sign, const int32_t* act, double* colmax)>
      product;
  // precise (A X = B only): r = b - A x from the doubled sum, gathered into Vr, colmax = ||r_j||; the
  // correction d = inv(A) r in the engine dtype into a buffer of its own, colmax = ||d_j||; x += d,
  // gathered into Vx, colmax = ||x_j|| -- each for the columns `act`
  std::function<void(int64_t kg, const int32_t* act, double* colmax)> residual_dd, correction, advance;
  int norm_sets = 2;  // column-norm vectors (Device::kMaxRhs doubles each) all_ranks makes global
  std::function<const double*(const double* norms)> all_ranks;  // the column norms over all ranks
  std::function<const double*()> result;          // `best` in natural row order
  // The error bounds of a group whose columns have all stopped: xhat = result() (natural order), r
  // holds b - A xhat unless redo_r says to compute it again; colmax[j] = this rank's max_i F_ij with
  // F = |inv(A)| (|r| + nz_eps D), D = |A| |xhat| + |b|, and berr[j] = its max_i |r_i| / D_i (device,
  // Device::kMaxRhs doubles each).  Uses x, r and Vr, which the loop has left.
  std::function<void(int64_t kg, const double* xhat, bool redo_r, double* colmax, double* berr)> bounds;
};

namespace {
// xGERFS's constants at order n
struct BoundConst {
  double nz_eps, safe1, safe2;
  // precise: the residual comes from Dot2, whose rounding term is gamma^2 (|A| |x| + |b|); the factor 4
  // covers double-double additions of relative error 2 u^2
  explicit BoundConst(int64_t n, bool precise = false)
      : nz_eps(precise ? 4 * ((double)(n + 2) * 0x1p-53) * ((double)(n + 2) * 0x1p-53) : (double)(n + 1) * 0x1p-53),
        safe1((double)(n + 1) * std::numeric_limits<double>::min()),
        safe2(safe1 / 0x1p-53) {}
};
}  // namespace

// A X = B: a product is this rank's rows of it (Device::panel_rhs), all-gathered into natural order.
void Engine::block_path_plain(BlockPath& f, const double* Aw, int64_t kw, bool precise) {
  BufSet& bufs = f.bufs;
  const int64_t m = L_.m, n = L_.n, p = L_.p;
  const int64_t per = L_.max_nblk * m;  // rows every rank sends to an all-gather
  dev_.row_abs_max(DType::F64, Aw, L_.npad, L_, dscratch_, S_MAIN);  // ||A||_inf (fp64)
  dev_.copy(dhost_, dscratch_, sizeof(double), S_MAIN);
  dev_.sync_stream(S_MAIN);
  f.an = comm_.host_max(dev_, L_.nblk > 0 ? dhost_[0] : 0.0);

  const size_t loc = (size_t)per * kw, nat = (size_t)std::max<int64_t>(n, 1) * kw;
  double* Vb = f.Vb = bufs.get<double>(nat);
  f.Vx = bufs.get<double>(nat);
  f.Vr = bufs.get<double>(nat);
  double* Bloc = f.b = bufs.get<double>(loc);  // this rank's rows of B / X / R / the best iterate
  f.x = bufs.get<double>(loc);
  f.r = bufs.get<double>(loc);
  f.best = bufs.get<double>(loc);
  f.xrows = L_.rows;
  double* gath = bufs.get<double>(loc * (size_t)p);

  auto gather_natural = [this, gath, loc, kw](double* dst, const double* src_loc) {
    comm_.allgather(dev_, src_loc, gath, loc * sizeof(double), S_MAIN);
    dev_.gather_rows_natural(dst, kw, gath, kw, L_, kw, S_MAIN);
  };
  f.stage_b = [this, Vb, Bloc, m, n, kw] {
    for (int64_t b = 0; b < L_.nblk; ++b) {
      const int64_t g0 = L_.global_block(b) * m;
      if (g0 < n)
        dev_.copy(Bloc + b * m * kw, Vb + g0 * kw, sizeof(double) * (size_t)(std::min<int64_t>(m, n - g0) * kw),
                  S_MAIN);
    }
  };
  f.product = [this, gather_natural, kw](DType dt, const void* P, const double* V, int64_t kg, const double* C,
                                         double* dst, double* natural, double sign, const int32_t* act,
                                         double* colmax) {
    dev_.panel_rhs(dt, P, L_.npad, L_, V, kw, kg, C, C ? kw : 0, dst, kw, sign, act, colmax, S_MAIN);
    gather_natural(natural, dst);
  };
  if (precise) {
    f.norm_sets = 3;
    double* d = bufs.get<double>(loc);
    f.residual_dd = [this, gather_natural, Aw, kw, b = f.b, r = f.r, Vx = f.Vx, Vr = f.Vr](
                        int64_t kg, const int32_t* act, double* colmax) {
      dev_.panel_rhs_dd(DType::F64, Aw, L_.npad, L_, Vx, kw, kg, b, kw, r, kw, act, colmax, S_MAIN);
      gather_natural(Vr, r);
    };
    f.correction = [this, kw, d, Vr = f.Vr](int64_t kg, const int32_t* act, double* colmax) {
      dev_.panel_rhs(opt_.dtype, out_, L_.npad, L_, Vr, kw, kg, nullptr, 0, d, kw, 1.0, act, colmax, S_MAIN);
    };
    f.advance = [this, gather_natural, kw, d, x = f.x, Vx = f.Vx](int64_t kg, const int32_t* act, double* colmax) {
      dev_.axpy_cols_masked(x, kw, x, kw, d, kw, 1.0, real_local_rows(), kg, act, colmax, S_MAIN);
      gather_natural(Vx, x);
    };
  }
  // (a NaN from any rank wins)
  f.all_ranks = [this, p, sets = (size_t)f.norm_sets, mine = std::vector<double>(),
                 all = std::vector<double>((size_t)f.norm_sets * Device::kMaxRhs * p)](const double* norms) mutable {
    mine.assign(norms, norms + sets * Device::kMaxRhs);
    comm_.host_allgather(dev_, mine.data(), all.data(), sizeof(double) * mine.size());
    for (int64_t q = 0; q < p; ++q)
      for (size_t e = 0; e < mine.size(); ++e)
        mine[e] = q == 0 ? all[e] : max_keep_nan(mine[e], all[(size_t)q * mine.size() + e]);
    return (const double*)mine.data();
  };
  f.result = [gather_natural, Vx = f.Vx, best = f.best] {
    gather_natural(Vx, best);
    return (const double*)Vx;
  };
  f.bounds = [this, gather_natural, Aw, kw, n, precise, b = f.b, D = f.x, r = f.r, Vr = f.Vr](
                 int64_t kg, const double* xhat, bool redo_r, double* colmax, double* berr) {
    const BoundConst c(n, precise);
    dev_.panel_abs_rhs(DType::F64, Aw, L_.npad, L_, xhat, kw, kg, b, kw, D, kw, nullptr, S_MAIN);
    if (redo_r && precise)
      dev_.panel_rhs_dd(DType::F64, Aw, L_.npad, L_, xhat, kw, kg, b, kw, r, kw, nullptr, nullptr, S_MAIN);
    else if (redo_r)
      dev_.panel_rhs(DType::F64, Aw, L_.npad, L_, xhat, kw, kg, b, kw, r, kw, -1.0, nullptr, nullptr, S_MAIN);
    // G over r, on the real rows (a prefix of the local rows)
    dev_.bound_terms(r, kw, D, kw, r, kw, real_local_rows(), kg, c.nz_eps, c.safe1, c.safe2, berr, S_MAIN);
    gather_natural(Vr, r);
    dev_.panel_abs_rhs(opt_.dtype, out_, L_.npad, L_, Vr, kw, kg, nullptr, 0, D, kw, colmax, S_MAIN);
  };
}

// A^T X = B: every product is P_loc^T V_loc summed over the ranks, so B, X and R live in natural row
// order on every rank, identical bit for bit, and so are the column norms each rank computes.
void Engine::block_path_trans(BlockPath& f, const double* Aw, int64_t kw) {
  BufSet& bufs = f.bufs;
  const int64_t n = L_.n;
  // ||A^T||_inf = ||A||_1: the column sums of every rank's rows, summed over the ranks
  double* csum = bufs.get<double>((size_t)std::max<int64_t>(n, 1));
  dev_.col_abs_sum(DType::F64, Aw, L_.npad, L_, csum, S_MAIN);
  comm_.allreduce_sum(dev_, csum, (size_t)n, DType::F64, S_MAIN);
  std::vector<double> hsum((size_t)n);
  dev_.copy(hsum.data(), csum, sizeof(double) * (size_t)n, S_MAIN);
  comm_.drain(dev_, S_MAIN);
  for (double v : hsum) f.an = max_keep_nan(f.an, v);

  const size_t nat = (size_t)std::max<int64_t>(n, 1) * kw;
  f.b = f.Vb = bufs.get<double>(nat);
  f.x = f.Vx = bufs.get<double>(nat);
  f.r = f.Vr = bufs.get<double>(nat);
  double* Sp = bufs.get<double>(nat);  // a product: this rank's term, then the sum over the ranks
  double* best = f.best = bufs.get<double>(nat);
  f.xrows = n;

  f.begin_group = [this, Sp, nat, kw](int64_t kg) {
    if (kg < kw) dev_.memset0(Sp, sizeof(double) * nat, S_MAIN);  // the columns past kg enter the sum as 0
  };
  f.product = [this, Sp, nat, n, kw](DType dt, const void* P, const double* V, int64_t kg, const double* C,
                                     double* dst, double*, double sign, const int32_t* act, double* colmax) {
    dev_.panel_rhs_t(dt, P, L_.npad, L_, V, kw, kg, Sp, kw, act, S_MAIN);
    comm_.allreduce_sum(dev_, Sp, nat, DType::F64, S_MAIN);
    dev_.axpy_cols_masked(dst, kw, C, kw, Sp, kw, sign, n, kg, act, colmax, S_MAIN);
  };
  f.result = [best] { return (const double*)best; };
  // every step gives the same bits on every rank: B, xhat and r are whole and identical, the products
  // are sums over the ranks
  f.bounds = [this, Aw, Sp, nat, kw, n, b = f.b, D = f.x, r = f.r](int64_t kg, const double* xhat, bool redo_r,
                                                                    double* colmax, double* berr) {
    const BoundConst c(n);
    dev_.panel_abs_rhs_t(DType::F64, Aw, L_.npad, L_, xhat, kw, kg, Sp, kw, S_MAIN);
    comm_.allreduce_sum(dev_, Sp, nat, DType::F64, S_MAIN);
    // D = |b| + |A^T| |xhat|: bound_terms' G with nz_eps = 1 and no safe2 row (berr is overwritten below)
    dev_.bound_terms(b, kw, Sp, kw, D, kw, n, kg, 1.0, 0.0, -1.0, berr, S_MAIN);
    if (redo_r) {
      dev_.panel_rhs_t(DType::F64, Aw, L_.npad, L_, xhat, kw, kg, Sp, kw, nullptr, S_MAIN);
      comm_.allreduce_sum(dev_, Sp, nat, DType::F64, S_MAIN);
      dev_.axpy_cols_masked(r, kw, b, kw, Sp, kw, -1.0, n, kg, nullptr, nullptr, S_MAIN);
    }
    dev_.bound_terms(r, kw, D, kw, r, kw, n, kg, c.nz_eps, c.safe1, c.safe2, berr, S_MAIN);
    dev_.panel_abs_rhs_t(opt_.dtype, out_, L_.npad, L_, r, kw, kg, Sp, kw, S_MAIN);
    comm_.allreduce_sum(dev_, Sp, nat, DType::F64, S_MAIN);
    dev_.axpy_cols_masked(D, kw, nullptr, kw, Sp, kw, 1.0, n, kg, nullptr, colmax, S_MAIN);
  };
}

RhsBlockResult Engine::solve_rhs_block_impl(const double* B, int64_t ldb, double* X, int64_t ldx, int64_t k,
                                           bool on_device, const GenSpec* gen, const double* host_rows,
                                           const void* dev_rows, int64_t ld, int max_refine, double tol,
                                           bool trans, bool bounds, bool precise) {
  GJ_REQUIRE(solved_, "solve_rhs_block: solve() first");
  GJ_REQUIRE(!(trans && precise),
             "solve_rhs_block: precise is not available with trans (the transposed residual is a sum over the "
             "ranks and needs a doubled all-reduce)");
  GJ_REQUIRE(k >= 1 && ldb >= k && ldx >= k, "solve_rhs_block: k >= 1 columns, ldb >= k and ldx >= k");
  GJ_REQUIRE(gen || host_rows || dev_rows || real_local_rows() == 0,
             "solve_rhs_block: the matrix (generator or rows) is needed for the fp64 residual");
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t n = L_.n;
  const int64_t kw = std::min<int64_t>(k, Device::kMaxRhs);  // widest group = every buffer's leading dimension
  constexpr int64_t K = Device::kMaxRhs;
  RhsBlockResult out;
  out.col.resize((size_t)k);
  BlockPath f(dev_);
  BufSet& bufs = f.bufs;
  // A's local rows in fp64, once per call
  double* Aw = bufs.get<double>((size_t)std::max<int64_t>(L_.rows, 1) * L_.npad, false);
  stage_rows_f64(Aw, gen, host_rows, dev_rows, ld);
  if (trans)
    block_path_trans(f, Aw, kw);
  else
    block_path_plain(f, Aw, kw, precise);
  const int64_t NS = f.norm_sets;
  double* dnorm = bufs.get<double>(NS * K);   // ||r_j|| | ||x_j|| (| ||d_j||, precise)
  int32_t* dflag = bufs.get<int32_t>(2 * K);  // active | save-mask
  double* hnorm = bufs.get_pinned<double>(NS * K);
  int32_t* hflag = bufs.get_pinned<int32_t>(2 * K);
  std::vector<double> hb;  // a device-resident B's columns on the host, for ||b_j|| only

  for (int64_t c0 = 0; c0 < k; c0 += kw) {
    const int64_t kg = std::min<int64_t>(kw, k - c0);
    if (f.begin_group) f.begin_group(kg);
    // B's columns of this group: natural order on the device, ||b_j||
    dev_.copy2d(f.Vb, kw * 8, B + c0, ldb * 8, kg * 8, n, S_MAIN);
    if (f.stage_b) f.stage_b();
    std::vector<double> bn((size_t)kg, 0.0);
    const double* bh = B + c0;
    int64_t ldh = ldb;
    if (on_device) {
      hb.resize((size_t)n * kw);
      dev_.copy(hb.data(), f.Vb, sizeof(double) * (size_t)n * kw, S_MAIN);
      dev_.sync_stream(S_MAIN);
      bh = hb.data();
      ldh = kw;
    }
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < kg; ++j) bn[(size_t)j] = std::max(bn[(size_t)j], std::fabs(bh[i * ldh + j]));
    for (double& v : bn)
      if (v == 0) v = 1;

    // x_0 = inv(A) b in the engine dtype, every column active
    dev_.host_access(hflag, sizeof(int32_t) * 2 * K, true);
    for (int64_t j = 0; j < K; ++j) hflag[j] = j < kg ? 1 : 0;
    dev_.copy(dflag, hflag, sizeof(int32_t) * K, S_MAIN);
    f.product(opt_.dtype, out_, f.Vb, kg, nullptr, f.x, f.Vx, 1.0, nullptr, dnorm + K);

    std::vector<ColumnRule> rule((size_t)kg);
    RhsResult* rr = out.col.data() + c0;
    for (int it = 0;; ++it) {
      if (precise) {  // r = b - A x from the doubled sum and the correction d = inv(A) r it would get
        f.residual_dd(kg, dflag, dnorm);
        f.correction(kg, dflag, dnorm + 2 * K);
      } else {  // r = b - A x in fp64, the whole residual on every rank
        f.product(DType::F64, Aw, f.Vx, kg, f.b, f.r, f.Vr, -1.0, dflag, dnorm);
      }
      dev_.copy(hnorm, dnorm, sizeof(double) * NS * K, S_MAIN);
      comm_.drain(dev_, S_MAIN);
      dev_.host_access(hnorm, sizeof(double) * NS * K, false);
      const double* norms = f.all_ranks ? f.all_ranks(hnorm) : hnorm;
      out.sweeps = std::max(out.sweeps, it + 1);
      // the per-column decision
      dev_.host_access(hflag, sizeof(int32_t) * 2 * K, true);
      bool any = false;
      for (int64_t j = 0; j < kg; ++j) {
        ColumnRule& c = rule[(size_t)j];
        if (precise)
          hflag[K + j] = c.active && c.step_precise(rr[j], it, norms[j], norms[K + j], norms[2 * K + j], f.an,
                                                    bn[(size_t)j], max_refine, n);
        else
          hflag[K + j] = c.active && c.step(rr[j], it, norms[j], norms[K + j], f.an, bn[(size_t)j], max_refine, tol);
        hflag[j] = c.active;
        any = any || c.active;
      }
      dev_.copy(dflag, hflag, sizeof(int32_t) * 2 * K, S_MAIN);
      dev_.copy_cols_masked(f.best, kw, f.x, kw, f.xrows, kg, dflag + K, S_MAIN);
      if (!any) break;
      // x += inv(A) r for the columns still active (engine dtype, added in fp64)
      if (precise)
        f.advance(kg, dflag, dnorm + K);
      else
        f.product(opt_.dtype, out_, f.Vr, kg, f.x, f.x, f.Vx, 1.0, dflag, dnorm + K);
    }
    // every column's returned iterate is in `best`
    const double* xhat = f.result();
    dev_.copy2d(X + c0, ldx * 8, xhat, kw * 8, kg * 8, n, S_MAIN);
    if (bounds) {
      bool redo_r = false;
      for (const ColumnRule& c : rule) redo_r = redo_r || c.stale_r;
      f.bounds(kg, xhat, redo_r, dnorm, dnorm + K);
      dev_.copy(hnorm, dnorm, sizeof(double) * NS * K, S_MAIN);
      comm_.drain(dev_, S_MAIN);
      dev_.host_access(hnorm, sizeof(double) * NS * K, false);
      const double* norms = f.all_ranks ? f.all_ranks(hnorm) : hnorm;
      for (int64_t j = 0; j < kg; ++j) {
        const double xn = rule[(size_t)j].ret_xn;
        rr[j].ferr = xn == 0 ? norms[j] : norms[j] / xn;  // (LAPACK's rule for x = 0)
        rr[j].berr = norms[K + j];
      }
    }
    comm_.drain(dev_, S_MAIN);
  }
  out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return out;
}

// ---------------------------------------------------------------- ||A|| and ||inv(A)||, 1 and inf
CondResult Engine::cond(const GenSpec* gen, const double* host_rows, const void* dev_rows, int64_t ld) {
  GJ_REQUIRE(solved_, "cond: solve() first");
  GJ_REQUIRE(gen || host_rows || dev_rows || real_local_rows() == 0,
             "cond: the matrix (generator or rows) is needed for its norms");
  const int64_t n = L_.n;
  BufSet bufs(dev_);
  double* Aw = bufs.get<double>((size_t)std::max<int64_t>(L_.rows, 1) * L_.npad, false);
  stage_rows_f64(Aw, gen, host_rows, dev_rows, ld);
  double* csum = bufs.get<double>(2 * (size_t)std::max<int64_t>(n, 1));  // column sums of A | of inv(A)
  double* rmax = bufs.get<double>(2);                                    // row-sum maxima of A, of inv(A)
  dev_.col_abs_sum(DType::F64, Aw, L_.npad, L_, csum, S_MAIN);
  dev_.col_abs_sum(opt_.dtype, out_, L_.npad, L_, csum + n, S_MAIN);
  comm_.allreduce_sum(dev_, csum, 2 * (size_t)n, DType::F64, S_MAIN);
  dev_.row_abs_max(DType::F64, Aw, L_.npad, L_, rmax, S_MAIN);
  dev_.row_abs_max(opt_.dtype, out_, L_.npad, L_, rmax + 1, S_MAIN);
  std::vector<double> h(2 * (size_t)n + 2);
  dev_.copy(h.data(), csum, sizeof(double) * 2 * (size_t)n, S_MAIN);
  dev_.copy(h.data() + 2 * n, rmax, sizeof(double) * 2, S_MAIN);
  comm_.drain(dev_, S_MAIN);
  CondResult c;
  for (int64_t j = 0; j < n; ++j) {
    c.a_norm1 = max_keep_nan(c.a_norm1, h[(size_t)j]);
    c.inv_norm1 = max_keep_nan(c.inv_norm1, h[(size_t)(n + j)]);
  }
  c.a_norminf = comm_.host_max(dev_, L_.nblk > 0 ? h[(size_t)(2 * n)] : 0.0);
  c.inv_norminf = comm_.host_max(dev_, L_.nblk > 0 ? h[(size_t)(2 * n + 1)] : 0.0);
  return c;
}

// ---------------------------------------------------------------- inv(A + U V^T) from inv(A)
namespace {
struct SmallInverse {
  bool singular = false;
  double min_pivot = 0;
  std::vector<double> inv;  // inv(C), k x k (zeros when singular)
  double cond1 = 0;         // ||C||_1 ||inv(C)||_1 (0 when the LU already refused)
  // slogdet(C) from the LU's pivots and row swaps (0, -inf at a zero pivot; NaN, NaN at a non-finite one)
  double sign = 1.0, logabs = 0.0;
};

// C = I + T (k x k, row-major) by an LU with partial pivoting in fp64, inv(C) column by column.
// Singular: a pivot that is non-finite or |pivot| <= eps * scale, or a non-finite inverse.
SmallInverse invert_small(const std::vector<double>& T, int64_t k, double eps, double scale) {
  SmallInverse out;
  double c1 = 0.0;
  std::vector<double> C(T);
  for (int64_t i = 0; i < k; ++i) C[(size_t)(i * k + i)] += 1.0;
  for (int64_t j = 0; j < k; ++j) {
    double s = 0.0;
    for (int64_t i = 0; i < k; ++i) s += std::fabs(C[(size_t)(i * k + j)]);
    c1 = max_keep_nan(c1, s);
  }
  std::vector<int64_t> perm((size_t)k);
  for (int64_t i = 0; i < k; ++i) perm[(size_t)i] = i;
  bool singular = !std::isfinite(scale);
  if (singular) out.sign = out.logabs = std::numeric_limits<double>::quiet_NaN();
  double minpiv = std::numeric_limits<double>::infinity();
  for (int64_t c = 0; c < k && !singular; ++c) {
    int64_t pr = c;
    for (int64_t i = c + 1; i < k; ++i)
      if (std::fabs(C[(size_t)(i * k + c)]) > std::fabs(C[(size_t)(pr * k + c)])) pr = i;
    if (pr != c) {
      for (int64_t j = 0; j < k; ++j) std::swap(C[(size_t)(c * k + j)], C[(size_t)(pr * k + j)]);
      std::swap(perm[(size_t)c], perm[(size_t)pr]);
      out.sign = -out.sign;
    }
    const double piv = C[(size_t)(c * k + c)];
    if (!std::isfinite(piv)) {
      out.sign = out.logabs = std::numeric_limits<double>::quiet_NaN();
    } else if (piv == 0.0) {
      out.sign = 0.0;
      out.logabs = -std::numeric_limits<double>::infinity();
    } else {
      out.logabs += std::log(std::fabs(piv));
      if (piv < 0.0) out.sign = -out.sign;
    }
    if (!std::isfinite(piv) || std::fabs(piv) <= eps * scale) {
      singular = true;
      minpiv = std::isfinite(piv) ? std::min(minpiv, std::fabs(piv) / scale) : 0.0;
      break;
    }
    minpiv = std::min(minpiv, std::fabs(piv) / scale);
    for (int64_t i = c + 1; i < k; ++i) {
      const double l = C[(size_t)(i * k + c)] / piv;
      C[(size_t)(i * k + c)] = l;
      for (int64_t j = c + 1; j < k; ++j) C[(size_t)(i * k + j)] -= l * C[(size_t)(c * k + j)];
    }
  }
  std::vector<double>& Ci = out.inv;
  Ci.assign((size_t)k * k, 0.0);
  if (!singular) {
    std::vector<double> y((size_t)k);
    for (int64_t e = 0; e < k; ++e) {  // C x = e_e: L y = P e_e, U x = y
      for (int64_t i = 0; i < k; ++i) {
        double v = perm[(size_t)i] == e ? 1.0 : 0.0;
        for (int64_t j = 0; j < i; ++j) v -= C[(size_t)(i * k + j)] * y[(size_t)j];
        y[(size_t)i] = v;
      }
      for (int64_t i = k - 1; i >= 0; --i) {
        double v = y[(size_t)i];
        for (int64_t j = i + 1; j < k; ++j) v -= C[(size_t)(i * k + j)] * Ci[(size_t)(j * k + e)];
        Ci[(size_t)(i * k + e)] = v / C[(size_t)(i * k + i)];
      }
    }
    double ci1 = 0.0;
    for (int64_t j = 0; j < k; ++j) {
      double s = 0.0;
      for (int64_t i = 0; i < k; ++i) s += std::fabs(Ci[(size_t)(i * k + j)]);
      ci1 = max_keep_nan(ci1, s);
    }
    out.cond1 = c1 * ci1;
    if (!std::isfinite(ci1)) singular = true;
  }
  out.singular = singular;
  out.min_pivot = minpiv;
  return out;
}
}  // namespace

// (Device::copy2d takes host and device sources alike, as in solve_rhs_block_device)
UpdateResult Engine::update_inverse_device(const double* U_dev, int64_t ldu, const double* V_dev, int64_t ldv,
                                           int64_t k) {
  return update_inverse(U_dev, ldu, V_dev, ldv, k);
}

UpdateResult Engine::update_inverse(const double* U, int64_t ldu, const double* V, int64_t ldv, int64_t k) {
  GJ_REQUIRE(solved_, "update_inverse: solve() first");
  GJ_REQUIRE(k >= 1 && k <= Device::kMaxRhs, "update_inverse: 1 <= k <= 64 columns (apply a larger update in pieces)");
  GJ_REQUIRE(U && V && ldu >= k && ldv >= k, "update_inverse: U and V are n x k, ldu >= k and ldv >= k");
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t n = L_.n, rows = L_.rows;
  UpdateResult out;
  out.k = k;
  // the determinant follows the panel: take det(A) from the stash before the first update moves on
  if (opt_.track_det && !det_cached_) slogdet();
  BufSet bufs(dev_);
  const size_t nat = (size_t)std::max<int64_t>(n, 1) * k, loc = (size_t)std::max<int64_t>(rows, 1) * k;
  double* Ud = bufs.get<double>(nat);    // U, V, Z = X^T V: natural row order, ld k
  double* Vd = bufs.get<double>(nat);
  double* Z = bufs.get<double>(nat);
  double* Wl = bufs.get<double>(loc);    // this rank's rows of W = X U, then of W inv(C)
  double* Wc = bufs.get<double>(loc);
  double* Cd = bufs.get<double>((size_t)k * k);  // V^T X U, then inv(C)
  dev_.copy2d(Ud, k * 8, U, ldu * 8, k * 8, n, S_MAIN);
  dev_.copy2d(Vd, k * 8, V, ldv * 8, k * 8, n, S_MAIN);
  dev_.panel_rhs(opt_.dtype, out_, L_.npad, L_, Ud, k, k, nullptr, k, Wl, k, 1.0, nullptr, nullptr, S_MAIN);
  dev_.panel_rhs_t(opt_.dtype, out_, L_.npad, L_, Vd, k, k, Z, k, nullptr, S_MAIN);
  comm_.allreduce_sum(dev_, Z, nat, DType::F64, S_MAIN);
  // T = Z^T U = V^T X U, the same bits on every rank (Z and U are); C = I + T is formed on the host
  dev_.gemm(DType::F64, GemmOp::Store, ALayout::KMajor, k, k, n, Z, k, Ud, k, Cd, k, S_MAIN);
  std::vector<double> T((size_t)k * k);
  dev_.copy(T.data(), Cd, sizeof(double) * (size_t)k * k, S_MAIN);
  comm_.drain(dev_, S_MAIN);

  double tmax = 0.0;
  for (double v : T) tmax = max_keep_nan(tmax, std::fabs(v));
  const SmallInverse ci = invert_small(T, k, opt_.eps, std::isfinite(tmax) ? std::max(1.0, tmax) : tmax);
  out.min_pivot = ci.min_pivot;
  out.sign_c = ci.sign;
  out.logabsdet_c = ci.logabs;
  // one outcome for all ranks, before anything is written
  if (comm_.host_max(dev_, ci.singular ? 1.0 : 0.0) > 0) {
    out.status = Status::Singular;
    out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return out;
  }
  out.cond1 = ci.cond1;
  dev_.copy(Cd, ci.inv.data(), sizeof(double) * (size_t)k * k, S_MAIN);
  if (rows > 0)
    dev_.gemm(DType::F64, GemmOp::Store, ALayout::RowMajor, rows, k, k, Wl, k, Cd, k, Wc, k, S_MAIN);
  dev_.rank_update(opt_.dtype, out_, L_.npad, L_, Wc, k, false, Z, k, k, -1.0, S_MAIN);
  comm_.drain(dev_, S_MAIN);  // (ci.inv is read by the copy until here)
  if (det_cached_) {  // det(A + U V^T) = det(C) det(A)
    det_.sign *= ci.sign;
    det_.logabsdet += ci.logabs;
  }
  out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return out;
}

}  // namespace gj
