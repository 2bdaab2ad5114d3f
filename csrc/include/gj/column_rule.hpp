// The stopping rule of one right-hand side of a refined solve, shared by every solve path
// (solver/refine.cpp: Engine::solve_rhs, Engine::solve_rhs_block; solver/batch.cpp: BatchSolver::solve).
// Internal to the solver sources.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>

#include "gj/engine.hpp"

namespace gj {

// The refinement rule of one right-hand side, the same for every solve path: converged at backward
// error <= tol; the best iterate so far is remembered (a diverging refinement, e.g. an fp32 inverse
// with ||I - XA|| near 1, must not hand back a worse x than it was given); stopped when the budget
// is spent or the residual did not halve, and then the best iterate is the one returned, with its
// own residual and the full history.
struct ColumnRule {
  RhsResult best;  // the report of the best iterate
  double best_rn = 1e300, prev = 1e300;
  bool active = true;  // false: the column has stopped, r is its final report
  // for the error bounds of the returned iterate: its ||x||, and whether the residual last computed
  // (the current iterate's) is the returned iterate's own
  double ret_xn = 0, best_xn = 0;
  bool stale_r = false;
  // Iterate `it` has ||b - A x|| = rn and ||x|| = xn: updates the report r.  True: this iterate is
  // the one to return unless a later step says so again, the caller keeps a copy of it.
  bool step(RhsResult& r, int it, double rn, double xn, double an, double bn, int max_refine, double tol) {
    r.history.push_back(rn / bn);
    r.residual = rn;
    r.backward_error = rn / (an * xn + bn);
    ret_xn = xn;
    if (r.backward_error <= tol) {
      r.converged = true;
      active = false;
      return true;
    }
    bool save = false;
    if (rn < best_rn) {
      best_rn = rn;
      best = r;
      best_xn = xn;
      save = true;
    }
    if (it >= max_refine || (it > 0 && rn > 0.5 * prev)) {  // budget spent / not contracting
      if (rn > best_rn) {  // the best iterate (already saved), with its own residual (history kept)
        best.history = r.history;
        r = best;
        ret_xn = best_xn;
        stale_r = true;
      } else {  // (also a NaN residual: neither better nor worse, the current iterate stands)
        save = true;
      }
      active = false;
    } else {
      prev = rn;
      r.steps = it + 1;
    }
    return save;
  }

  // The rule of extra-precise refinement (solve_rhs_block with precise; LAPACK's xGERFSX): it looks at
  // the correction, not at the residual.  Iterate `it` has ||b - A x|| = rn (from the doubled
  // residual), ||x|| = xn and ||inv(A) (b - A x)|| = dn, the size of the correction it would get and
  // the estimate of its error.  Converged at dn <= 2^-53 xn: the correction is not applied.  Stopped
  // when the budget is spent, when dn did not halve (LAPACK's rthresh) or when dn is NaN; then the
  // iterate with the smallest dn is the one returned (a NaN dn: the current one).  Otherwise the column
  // stays active and the caller adds the correction.  At the stop the report gets dx_ratio and err_est.
  // Returns whether to keep a copy of this iterate, as step does.
  double best_dn = std::numeric_limits<double>::infinity(), prev_dn = 0, max_ratio = 0;
  bool step_precise(RhsResult& r, int it, double rn, double xn, double dn, double an, double bn, int max_refine,
                    int64_t n) {
    r.history.push_back(rn / bn);
    r.residual = rn;
    r.backward_error = rn / (an * xn + bn);
    r.dx_rel = xn == 0 ? dn : dn / xn;
    ret_xn = xn;
    if (it > 0) max_ratio = max_keep_nan(max_ratio, dn / prev_dn);
    bool save = false;
    if (dn < best_dn) {
      best_dn = dn;
      best = r;
      best_xn = xn;
      save = true;
    }
    const bool nan = dn != dn;
    if (dn <= 0x1p-53 * xn) {
      r.converged = true;
      save = true;
      active = false;
    } else if (nan || it >= max_refine || (it > 0 && dn > 0.5 * prev_dn)) {
      if (!nan && dn > best_dn) {  // the best iterate (already saved), with its own report (history kept)
        best.history = r.history;
        r = best;
        ret_xn = best_xn;
        stale_r = true;
      } else {
        save = true;
      }
      active = false;
    } else {
      prev_dn = dn;
      r.steps = it + 1;
    }
    if (!active) {
      r.dx_ratio = max_ratio;
      const double floor_ = std::max(10.0, std::sqrt((double)n)) * 0x1p-53;
      r.err_est = max_ratio < 1 ? max_keep_nan(floor_, r.dx_rel / (1 - max_ratio))
                                : std::numeric_limits<double>::infinity();
    }
    return save;
  }
};

}  // namespace gj
