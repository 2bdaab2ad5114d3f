// Gradients from the resident inverse after Engine::solve(): the gradient matrix alpha inv(A)^T +
// sign W Z^T of a solve or of log|det A| (Engine::grad_matrix) and the vector-Jacobian product of
// A -> inv(A) (Engine::vjp_inverse).  Neither inverts anything again -- see gj/engine.hpp for the
// contracts.
#include "gj/engine.hpp"

#include <algorithm>

namespace gj {

namespace {
// work space of a gradient call: a failed allocation is Status::NoBlockMemory, like the
// elimination's work space
DevBuf<void> work_buffer(Device& dev, size_t bytes, const char* label) {
  try {
    return DevBuf<void>::device(dev, std::max<size_t>(bytes, 1), label);
  } catch (const Error& e) {
    if (e.status() != Status::NoMemory) throw;
    throw Error(Status::NoBlockMemory, std::string("not enough memory for the gradient's work space: ") + e.what());
  }
}
}  // namespace

void Engine::grad_matrix_device(double alpha, const double* W_dev, int64_t ldw, const double* Z_dev, int64_t ldz,
                                int64_t k, double sign, bool accumulate, double* G_dev, int64_t ldg) {
  GJ_REQUIRE(L_.p == 1, "grad_matrix: one rank only (a distributed gradient needs a distributed transpose)");
  GJ_REQUIRE(solved_, "grad_matrix: solve() first");
  GJ_REQUIRE(k >= 0 && k <= Device::kMaxRhs, "grad_matrix: 0 <= k <= 64 columns (apply a wider product in pieces)");
  GJ_REQUIRE(G_dev && ldg >= L_.n && (k == 0 || (W_dev && Z_dev && ldw >= k && ldz >= k)),
             "grad_matrix: G is n x n (ldg >= n), W and Z are n x k (ldw >= k, ldz >= k)");
  GJ_REQUIRE(sign == 1.0 || sign == -1.0, "grad_matrix: sign is +1 or -1");
  dev_.grad_matrix(opt_.dtype, out_, L_.npad, L_.n, alpha, W_dev, ldw, Z_dev, ldz, k, sign, accumulate, G_dev, ldg,
                   S_MAIN);
  comm_.drain(dev_, S_MAIN);
}

void Engine::grad_matrix(double alpha, const double* W, int64_t ldw, const double* Z, int64_t ldz, int64_t k,
                         double sign, bool accumulate, double* G, int64_t ldg) {
  GJ_REQUIRE(L_.p == 1, "grad_matrix: one rank only (a distributed gradient needs a distributed transpose)");
  GJ_REQUIRE(solved_, "grad_matrix: solve() first");
  GJ_REQUIRE(k >= 0 && k <= Device::kMaxRhs, "grad_matrix: 0 <= k <= 64 columns (apply a wider product in pieces)");
  GJ_REQUIRE(G && ldg >= L_.n && (k == 0 || (W && Z && ldw >= k && ldz >= k)),
             "grad_matrix: G is n x n (ldg >= n), W and Z are n x k (ldw >= k, ldz >= k)");
  if (!dev_.on_gpu()) {  // host memory is the host executor's own
    grad_matrix_device(alpha, W, ldw, Z, ldz, k, sign, accumulate, G, ldg);
    return;
  }
  const int64_t n = L_.n;
  const size_t nk = (size_t)std::max<int64_t>(n * k, 1), nn = (size_t)std::max<int64_t>(n * n, 1);
  auto Wd = work_buffer(dev_, 8 * nk, "grad W");
  auto Zd = work_buffer(dev_, 8 * nk, "grad Z");
  auto Gd = work_buffer(dev_, 8 * nn, "grad G");
  DrainOnExit drain{dev_};
  if (k > 0 && n > 0) {
    dev_.copy2d(Wd, k * 8, W, ldw * 8, k * 8, n, S_MAIN);
    dev_.copy2d(Zd, k * 8, Z, ldz * 8, k * 8, n, S_MAIN);
  }
  if (accumulate && n > 0) dev_.copy2d(Gd, n * 8, G, ldg * 8, n * 8, n, S_MAIN);
  grad_matrix_device(alpha, static_cast<const double*>(Wd.get()), k, static_cast<const double*>(Zd.get()), k, k, sign,
                     accumulate, static_cast<double*>(Gd.get()), n);
  if (n > 0) dev_.copy2d(G, ldg * 8, Gd, n * 8, n * 8, n, S_MAIN);
  comm_.drain(dev_, S_MAIN);
}

void Engine::vjp_inverse_device(const double* Gbar_dev, int64_t ldg, double* out_dev, int64_t ldo) {
  GJ_REQUIRE(L_.p == 1, "vjp_inverse: one rank only (a distributed gradient needs a distributed transpose)");
  GJ_REQUIRE(solved_, "vjp_inverse: solve() first");
  GJ_REQUIRE(Gbar_dev && out_dev && ldg >= L_.n && ldo >= L_.n, "vjp_inverse: Gbar and out are n x n (ldg, ldo >= n)");
  const int64_t n = L_.n, npad = L_.npad;
  const DType dt = opt_.dtype;
  const size_t bytes = dtype_size(dt) * (size_t)std::max<int64_t>(n, 1) * (size_t)npad;
  auto B1 = work_buffer(dev_, bytes, "vjp Gbar / N");
  auto B2 = work_buffer(dev_, bytes, "vjp M");
  DrainOnExit drain{dev_};
  if (n == 0) return;
  // X = inv(A) is the result panel (p = 1: rows in natural order); only its n x n corner is used
  dev_.upload_convert(dt, B1, npad, Gbar_dev, ldg, n, n, S_MAIN);
  // M = Gbar^T X: Gbar as the K-major A operand
  dev_.gemm(dt, GemmOp::Store, ALayout::KMajor, n, n, n, B1, npad, out_, npad, B2, npad, S_MAIN);
  // N = X M
  dev_.gemm(dt, GemmOp::Store, ALayout::RowMajor, n, n, n, out_, npad, B2, npad, B1, npad, S_MAIN);
  // out = -N^T
  dev_.grad_matrix(dt, B1, npad, n, -1.0, nullptr, 0, nullptr, 0, 0, 1.0, false, out_dev, ldo, S_MAIN);
  comm_.drain(dev_, S_MAIN);
}

void Engine::vjp_inverse(const double* Gbar, int64_t ldg, double* out, int64_t ldo) {
  GJ_REQUIRE(L_.p == 1, "vjp_inverse: one rank only (a distributed gradient needs a distributed transpose)");
  GJ_REQUIRE(solved_, "vjp_inverse: solve() first");
  GJ_REQUIRE(Gbar && out && ldg >= L_.n && ldo >= L_.n, "vjp_inverse: Gbar and out are n x n (ldg, ldo >= n)");
  if (!dev_.on_gpu()) {
    vjp_inverse_device(Gbar, ldg, out, ldo);
    return;
  }
  const int64_t n = L_.n;
  auto Gd = work_buffer(dev_, 8 * (size_t)std::max<int64_t>(n * n, 1), "vjp staging");  // Gbar, then out
  DrainOnExit drain{dev_};
  if (n == 0) return;
  dev_.copy2d(Gd, n * 8, Gbar, ldg * 8, n * 8, n, S_MAIN);
  vjp_inverse_device(static_cast<const double*>(Gd.get()), n, static_cast<double*>(Gd.get()), n);
  dev_.copy2d(out, ldo * 8, Gd, n * 8, n * 8, n, S_MAIN);
  comm_.drain(dev_, S_MAIN);
}

}  // namespace gj
