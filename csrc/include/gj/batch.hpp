// A stack of small matrices: inverses, refined solves and determinants of nb matrices of one order
// n <= 1024 on one device (one rank, no Comm).
//
// factor() feeds Device::block_inverse -- one workgroup per matrix -- through batch_pack / batch_unpack:
// every matrix is brought to ||.||_inf in [1, 2) by an exact power of two (equil_exponent), so that the
// launch's single absolute pivot threshold `eps` is the engine's per-matrix rule |pivot| < eps ||A||_inf,
// and the inverse comes back as ldexp(inv(As_b), e_b): the inverse of A_b as the sweep on the scaled
// matrix gives it, bit for bit.  A matrix below order 16 enters as diag(As_b, I) of order 16, the
// smallest block the candidate-inverse kernels are run at.  The stack is processed in chunks whose
// working set (the packed panel, the transposed inverses and block_inverse's scratch) stays under
// `workspace_bytes`.
//
// solve() never returns a bare inv @ B: X = inv B, then R = B - A X in fp64 against the kept fp64 copy of
// A and X += inv R, every product by Device::batch_rhs, every (matrix, column) stopped by ColumnRule
// (gj/column_rule.hpp) -- the rule of every other solve path.
#pragma once

#include <cstdint>
#include <vector>

#include "gj/buffer.hpp"
#include "gj/device.hpp"

namespace gj {

// The last solve's report, one entry per (matrix, column): index b * k + j.
struct BatchSolveInfo {
  int64_t k = 0;
  std::vector<int32_t> converged, steps;
  std::vector<double> residual, backward_error;
  int sweeps = 0;
};

class BatchSolver {
 public:
  // 256 MiB: the whole stack of every shape up to 4096 matrices of order 128 in one chunk, and a few
  // matrices per chunk at order 1024, next to what the stack itself takes.
  static constexpr size_t kDefaultWorkspace = size_t(256) << 20;
  static constexpr int64_t kMaxOrder = 1024;
  static constexpr int64_t kMinBlock = 16;

  // workspace_bytes = 0: kDefaultWorkspace.  A chunk never has fewer than one matrix.
  BatchSolver(Device& dev, DType dt, int64_t n, int64_t nb, double eps, size_t workspace_bytes = 0);

  // Every operand below is memory of the solver's device (host memory on the host executors).
  // A: nb matrices of n x n fp64, rows lda and matrices stride_a elements apart.  Keeps an fp64 copy and
  // the inverses (dtype dt, contiguous).
  void factor(const double* A, int64_t stride_a, int64_t lda);

  // X_b = inverse of A_b in dtype dt (NaN for an invalid matrix), rows ldx, matrices stride_x apart
  void inverse(void* X, int64_t stride_x, int64_t ldx) const;
  // A_b X_b = B_b for k >= 1 columns, in groups of Device::kMaxRhs.  B: fp64, rows ldb and matrices
  // stride_b elements apart.  X (fp64, nb * n * k elements) comes back stack-interleaved,
  // X[(r * nb + b) * k + j] = X_b[r][j]: the layout of the work arrays, in which the columns of the whole
  // stack are the columns of one n-row array and one masked copy serves every matrix.  max_refine < 0:
  // 2 steps for an fp64 stack, 10 for fp32.  Columns of invalid matrices start inactive and return NaN.
  BatchSolveInfo solve(const double* B, int64_t stride_b, int64_t ldb, double* X, int64_t k, int max_refine,
                       double tol);
  // Device::slogdet_batch on the kept fp64 copy: host arrays of nb doubles
  void slogdet(double* sign, double* logabs);

  int64_t n() const { return n_; }
  int64_t nb() const { return nb_; }
  int64_t m() const { return m_; }
  DType dtype() const { return dt_; }
  int64_t chunk() const { return chunk_; }  // matrices per chunk
  const std::vector<int32_t>& valid() const { return valid_; }
  const std::vector<int32_t>& exponents() const { return exp_; }
  const std::vector<double>& norms() const { return norm_; }          // ||A_b||_inf
  const std::vector<double>& inverse_norms() const { return inorm_; }  // ||inv(A_b)||_inf (0 when invalid)
  const void* inverses_device() const { return inv_.get(); }
  const double* a64_device() const { return a64_.get(); }

 private:
  Device& dev_;
  DType dt_;
  int64_t n_, nb_, m_, chunk_ = 1;
  double eps_;
  size_t ws_;
  bool factored_ = false;
  DevBuf<double> a64_;    // nb x n x n, the residual's operand
  DevBuf<void> inv_;      // nb x n x n of dt
  DevBuf<double> dnorm_;  // nb
  DevBuf<int32_t> dexp_, dvalid_;
  std::vector<int32_t> valid_, exp_;
  std::vector<double> norm_, inorm_;
};

}  // namespace gj
