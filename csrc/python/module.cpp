// Python bindings (pybind11) of the native framework: devices, communicators, the engine and the
// in-process runner.  The module is built in-tree as mpi_jordan_crazy_acceleration_amd/_C*.so and
// shares the HIP runtime / RCCL already loaded by torch (the package imports torch first).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <thread>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <tuple>

#include "gj/async_host_device.hpp"
#include "gj/batch.hpp"
#include "gj/comms.hpp"
#include "gj/engine.hpp"
#include "gj/hip_device.hpp"
#include "gj/host_device.hpp"
#include "gj/io.hpp"
#include "gj/race_check.hpp"
#include "gj/runner.hpp"
#include "../kernels/kernels.hpp"

namespace py = pybind11;
using namespace gj;

namespace {

DType parse_dtype(const std::string& s) {
  if (s == "fp64" || s == "float64" || s == "f64" || s == "double") return DType::F64;
  if (s == "fp32" || s == "float32" || s == "f32" || s == "float") return DType::F32;
  throw std::invalid_argument("dtype must be fp64 or fp32");
}

GenKind parse_gen(const std::string& s) {
  if (s == "absdiff") return GenKind::AbsDiff;
  if (s == "hilbert") return GenKind::Hilbert;
  if (s == "identity") return GenKind::Identity;
  if (s == "random") return GenKind::Random;
  if (s == "randshift") return GenKind::RandomShifted;
  if (s == "zero") return GenKind::Zero;
  throw std::invalid_argument("unknown generator " + s);
}

// Communicator implemented in Python (torch.distributed, gloo) — host memory only.
class PyComm : public Comm {
 public:
  PyComm(py::object impl, int rank, int size) : impl_(std::move(impl)), r_(rank), n_(size) {}
  int size() const override { return n_; }
  int rank() const override { return r_; }
  std::string describe() const override { return "python(" + std::to_string(n_) + ")"; }
  void allgather(Device& dev, const void* send, void* recv, size_t bytes, int s) override {
    check(dev);
    call(s, "allgather", bytes, -1, [&] { impl_.attr("allgather")((uintptr_t)send, (uintptr_t)recv, bytes); });
  }
  void bcast(Device& dev, void* buf, size_t bytes, int root, int s) override {
    check(dev);
    call(s, "broadcast", bytes, root, [&] { impl_.attr("bcast")((uintptr_t)buf, bytes, root); });
  }
  void allreduce_max(Device& dev, double* buf, size_t count, int s) override {
    check(dev);
    call(s, "allreduce(max)", count * 8, -1, [&] { impl_.attr("allreduce_max")((uintptr_t)buf, count); });
  }
  void group_p2p(Device& dev, const std::vector<P2POp>& ops, int s) override {
    check(dev);
    size_t tot = 0;
    for (const auto& op : ops) tot += op.bytes;
    call(s, "grouped send/recv", tot, -1, [&] {
      py::list l;
      for (const auto& op : ops) l.append(py::make_tuple((uintptr_t)op.ptr, op.bytes, op.peer, op.send));
      impl_.attr("group_p2p")(l);
    });
  }
  void barrier(Device&) override {
    call(S_SIDE, "barrier", 0, -1, [&] { impl_.attr("barrier")(); });
  }
  double host_max(Device&, double v) override {
    double out = 0;
    call(S_SIDE, "host max", 8, -1, [&] { out = impl_.attr("host_max")(v).cast<double>(); });
    return out;
  }
  void host_allgather(Device&, const void* send, void* recv, size_t bytes) override {
    call(S_SIDE, "host allgather", bytes, -1,
         [&] { impl_.attr("allgather")((uintptr_t)send, (uintptr_t)recv, bytes); });
  }

 private:
  static void check(Device& dev) {
    if (dev.on_gpu()) throw std::runtime_error("PyComm works on host memory only (use RcclComm on GPUs)");
  }
  // A Python-side failure (gloo timeout, a peer that closed its connection) becomes a
  // communication error of the engine, converted while the GIL is held, naming the collective.
  template <class F>
  void call(int s, const char* kind, size_t bytes, int root, F&& f) {
    note(s, kind, bytes, root);
    py::gil_scoped_acquire g;
    try {
      f();
    } catch (py::error_already_set& e) {
      const std::string msg = e.what();
      throw Error(Status::CommError, "torch.distributed failed in the " + last_op(s) + ": " + msg);
    }
  }
  py::object impl_;
  int r_, n_;
};

PivotRule parse_pivot(const std::string& v) {
  if (v == "block-min-inv-norm" || v == "min-inv-norm") return PivotRule::MinInvNorm;
  if (v == "partial") return PivotRule::Partial;
  throw std::invalid_argument("pivot: block-min-inv-norm | partial");
}

// SolveStats::equil as reports carry it: {applied, row_exp_range, col_exp_range}
py::dict equil_to_dict(const SolveStats::Equil& q) {
  py::dict d;
  d["applied"] = q.applied;
  d["row_exp_range"] = py::make_tuple(q.row_exp_min, q.row_exp_max);
  d["col_exp_range"] = py::make_tuple(q.col_exp_min, q.col_exp_max);
  return d;
}

py::dict stats_to_dict(const SolveStats& st) {
  py::dict d;
  d["status"] = (int)st.status;
  if (st.equil.enabled) d["equilibrate"] = equil_to_dict(st.equil);
  d["singular_step"] = st.singular_step;
  d["seconds"] = st.seconds;
  d["host_wait_ms"] = st.host_wait_ms;
  d["pivots"] = st.pivots;
  d["offdiag_pivots"] = st.offdiag_pivots;
  d["pivot_fallbacks"] = st.pivot_fallbacks;
  d["bcast_bytes"] = st.bcast_bytes;
  {
    static const char* kinds[SolveStats::kNumCommKinds] = {"pivot_rows", "panel_pieces", "pivot_records"};
    py::dict cb;
    for (int k = 0; k < SolveStats::kNumCommKinds; ++k) {
      py::dict e;
      e["bytes"] = st.comm_bytes[k];
      e["calls"] = st.comm_calls[k];
      cb[kinds[k]] = e;
    }
    d["comm_bytes"] = cb;
  }
  if (st.profiled) {
    py::dict ph;
    for (int i = 0; i < kNumPhases; ++i) {
      py::dict e;
      e["ms"] = st.phase_ms[i];
      e["calls"] = st.phase_calls[i];
      ph[phase_name(i)] = e;
    }
    d["phases"] = ph;
  }
  return d;
}

// GemmExtra's owner predicate from None or (address of the int32 pivot | None, p, k)
void set_owner(GemmExtra& ex, const py::object& owner) {
  if (owner.is_none()) return;
  const py::tuple t = owner.cast<py::tuple>();
  if (t.size() != 3) throw std::invalid_argument("owner: (phys, p, k)");
  ex.owner_phys = t[0].is_none() ? nullptr : reinterpret_cast<const int32_t*>(t[0].cast<uintptr_t>());
  ex.owner_p = t[1].cast<int64_t>();
  ex.owner_k = t[2].cast<int64_t>();
  if (ex.owner_p <= 0) throw std::invalid_argument("owner: p > 0");
}

py::array_t<double> to_array(const std::vector<double>& v, int64_t r, int64_t c) {
  py::array_t<double> a({r, c});
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), sizeof(double) * r * c);
  return a;
}

}  // namespace

// bounds: the solve was asked for ferr / berr (the keys are absent otherwise); precise: likewise for
// dx_rel / dx_ratio / err_est
static py::dict rhs_info(const RhsResult& rr, bool bounds = false, bool precise = false) {
  py::dict info;
  info["residual"] = rr.residual;
  info["backward_error"] = rr.backward_error;
  info["history"] = rr.history;
  info["steps"] = rr.steps;
  info["converged"] = rr.converged;
  if (bounds) {
    info["ferr"] = rr.ferr;
    info["berr"] = rr.berr;
  }
  if (precise) {
    info["dx_rel"] = rr.dx_rel;
    info["dx_ratio"] = rr.dx_ratio;
    info["err_est"] = rr.err_est;
  }
  return info;
}

// Engine::Policy as Engine.policy and run_local's policy_ranks show it (the engine adds bcast,
// bcast_tuning and comm)
static py::dict policy_to_dict(const Engine::Policy& pl) {
  py::dict d;
  d["depth"] = pl.depth;
  d["chunk_cols"] = pl.chunk_cols;
  d["nchunks"] = pl.nchunks;
  d["reserve_cus"] = pl.reserve_cus;
  d["block_inverse"] = pl.block_inverse;
  d["comm_small_tiles"] = pl.comm_small_tiles;
  d["dense_gemm"] = pl.dense_gemm;
  d["look_ahead_rows"] = pl.la_side ? "SIDE" : "COMM";
  d["pivot"] = pl.pivot;
  if (!pl.fault_injection.empty()) d["fault_injection"] = pl.fault_injection;
  d["env_overrides"] = pl.env_overrides;
  d["gemm_tile"] = pl.gemm_tile;
  d["split"] = pl.split;
  d["lat_wide"] = pl.lat_wide;
  d["skip_cols"] = pl.skip_cols;
  d["lat_reg"] = pl.lat_reg;
  d["chunk_skip"] = pl.chunk_skip;
  d["first_depth"] = pl.first_depth;
  d["main_cnt"] = pl.main_cnt;
  d["gemm_phase"] = pl.gemm_phase;
  return d;
}

// max_refine < 0: the default budget of refinement steps, by the engine dtype
// (precise: LAPACK's ithresh -- the rule stops a column by its correction long before, and two
// corrections need not reach 2^-53 from an error of kappa u)
static int refine_budget(const Engine& eng, int max_refine, bool precise = false) {
  return max_refine >= 0 ? max_refine : (eng.options().dtype == DType::F64 && !precise) ? 2 : 10;
}

// Device-side time of a launch: `reps` back-to-back run(i), i < reps, on one stream between two
// timing events (no host work in between; the caller has warmed up); microseconds per call.
template <typename F>
static double time_launches(Device& d, int stream, int reps, F&& run) {
  const int e0 = d.create_event(true), e1 = d.create_event(true);
  d.record(e0, stream);
  for (int i = 0; i < reps; ++i) run(i);
  d.record(e1, stream);
  d.sync_stream(stream);
  return 1e3 * d.event_ms(e0, e1) / std::max(reps, 1);
}

PYBIND11_MODULE(_C, mod) {
  mod.doc() = "MI355X-native block Gauss-Jordan inversion: native engine, HIP kernels, RCCL comm";

  // gj::Error -> GJError (a RuntimeError) carrying the engine status (2 = no memory for the matrix,
  // 6 = communication failure, 7 = no memory for the work space, ...).
  static py::object gj_error = py::reinterpret_steal<py::object>(
      PyErr_NewException("mpi_jordan_crazy_acceleration_amd._C.GJError", PyExc_RuntimeError, nullptr));
  mod.attr("GJError") = gj_error;
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (const Error& e) {
      py::object inst = gj_error(e.what());
      inst.attr("status") = (int)e.status();
      PyErr_SetObject(gj_error.ptr(), inst.ptr());
    }
  });

  mod.def("version", [] { return std::string("0.1.0"); });
  mod.def("device_count", [] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
  });
  mod.def("rccl_unique_id", [] { return py::bytes(RcclComm::unique_id()); });
  mod.def("layout_real_rows",
          [](int64_t n, int64_t m, int64_t p, int64_t k) { return Layout::make(n, m, p, k).real_rows(); },
          "Layout::real_rows(): rank k's local rows whose global row is < n");
  mod.def("set_block_inverse_variant", [](const std::string& v) {
    kern::set_block_inverse_variant(kern::block_inverse_variant_id(v.c_str()));
  });
  mod.def("set_block_inverse_probe", [](uintptr_t p) { kern::set_block_inverse_probe(reinterpret_cast<int32_t*>(p)); },
          "test probe: device int32 buffer (nblk x m) receiving each candidate's pivot row per column; 0 = off");
  mod.def("set_gemm_variant", [](const std::string& v) { kern::set_gemm_variant(kern::gemm_variant_id(v.c_str())); });
  mod.def("set_glds_peel", [](bool on) { kern::set_glds_peel(on ? 1 : 0); },
          "fp64 LDS-DMA trailing-update kernel: the peeled, stage-unrolled main loop (GJ_GLDS_PEEL)");
  mod.def("set_glds_covl", [](bool on) { kern::set_glds_covl(on ? 1 : 0); },
          "fp64 LDS-DMA kernel: C loads overlapped with the first K slices (GJ_GLDS_COVL)");
  mod.def("set_glds_build", [](int b) { kern::set_glds_build(b); },
          "fp64 LDS-DMA trailing-update build for every launch: 23 | 25 | 33 | 43 | 1623, 0 = auto (GJ_GLDS_BUILD)");
  mod.def("set_glds_tile", [](int bn) { kern::set_glds_tile(bn); },
          "fp64 LDS-DMA trailing-update tile width for the 4-per-CU builds: 64 | 128 for every launch, 0 = per "
          "launch (the engine's choice; GJ_GLDS_TILE)");
  mod.def("set_lat_kernel", [](int mode) { kern::set_lat_kernel(mode); },
          "fp64 latency GEMMs on the register-fed small kernel: 1 / 0 for every launch, -1 per launch "
          "(GemmExtra::lat_reg; GJ_LAT_KERNEL)");
  mod.def("last_gemm_kernel", [] { return std::string(kern::last_gemm_kernel()); },
          "test probe: family / build name of the kernel this thread's last Device.gemm / gemm_batch ran "
          "('host' on the host executor)");
  mod.def("gemm_census", [](bool on) { gemm_census_enable(on); },
          "test probe: count every Device.gemm / gemm_batch launch of the process by its last_gemm_kernel name; True "
          "clears the counts and starts, False stops and keeps them (off by default)");
  mod.def("gemm_census_counts", [] { return gemm_census_counts(); }, "the census: {kernel name: launches}");
  mod.def("plan_policy",
          [](int64_t n, int64_t m, int p, int rank, const std::string& dtype, bool on_gpu, int depth,
             int64_t chunk_cols, int reserve_cus, int granted_cus) {
            Engine::PolicyPlan pl =
                Engine::plan_policy(n, m, p, rank, parse_dtype(dtype), on_gpu, depth, chunk_cols, reserve_cus);
            pl.grant(granted_cus >= 0 ? granted_cus : pl.reserve_request);
            py::dict d;
            d["depth"] = pl.depth;
            d["first_depth"] = pl.depth;
            d["nchunks"] = (int)pl.chunk_begin.size();
            int64_t w = 0;
            for (size_t c = 0; c < pl.chunk_begin.size(); ++c) w = std::max(w, (pl.chunk_end[c] - pl.chunk_begin[c]) * m);
            d["chunk_cols"] = w;
            d["chunk_begin"] = pl.chunk_begin;
            d["chunk_end"] = pl.chunk_end;
            d["reserve_request"] = pl.reserve_request;
            d["reserve_cus"] = pl.reserve_cus;
            d["dense_gemm"] = pl.dense_gemm;
            d["gemm_tile"] = pl.gemm_tile;
            d["skip_cols"] = pl.skip_cols;
            d["chunk_skip"] = pl.chunk_skip;
            d["lat_reg"] = pl.lat_reg;
            d["lat_wide"] = pl.lat_wide;
            return d;
          },
          py::arg("n"), py::arg("m"), py::arg("p") = 1, py::arg("rank") = 0, py::arg("dtype") = "fp64",
          py::arg("on_gpu") = true, py::arg("depth") = 0, py::arg("chunk_cols") = 0, py::arg("reserve_cus") = -1,
          py::arg("granted_cus") = -1,
          "Engine::plan_policy: what an engine of this shape chooses with no GJ_* override, under Engine.policy's "
          "keys (plus chunk_begin / chunk_end in block columns and reserve_request); granted_cus: the CUs the "
          "device sets aside, -1 = all that are asked for.  No device is touched.");
  mod.def("set_rhs_splitk", [](int s) { kern::set_rhs_splitk(s); },
          "test hook: K-split of the following Device.panel_rhs launches on the GPU (0 = auto, s >= 1 forces s)");
  mod.def("last_rhs_kernel", [] { return std::string(kern::last_rhs_kernel()); },
          "test probe: 'rhs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>' of this thread's last Device.panel_rhs "
          "('host' on the host executor)");
  mod.def("last_rhs_dd_kernel", [] { return std::string(kern::last_rhs_dd_kernel()); },
          "test probe: 'rhsdd<16|32|64>:f64:<vec|scalar>:s<split>' of this thread's last Device.panel_rhs_dd "
          "('host' on the host executors); the split is that of set_rhs_splitk");
  mod.def("set_rhs_t_split", [](int v) { kern::set_rhs_t_split(v); },
          "test hook: row split of the following Device.panel_rhs_t launches on the GPU (0 = auto, s >= 1 forces s)");
  mod.def("last_rhs_t_kernel", [] { return std::string(kern::last_rhs_t_kernel()); },
          "test probe: 'rhst<16|32|64>:<f64|f32>:<vec|scalar>:s<split>' of this thread's last Device.panel_rhs_t "
          "('host' on the host executor)");
  mod.def("last_abs_kernel", [] { return std::string(kern::last_abs_kernel()); },
          "test probe: 'abs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>' of this thread's last Device.panel_abs_rhs, "
          "'abst...' of its last panel_abs_rhs_t ('host' on the host executors); the splits are those of "
          "set_rhs_splitk / set_rhs_t_split");
  mod.def("last_rank_update_kernel",[] { return std::string(kern::last_rank_update_kernel()); },
          "test probe: 'rku<k padded to 4>:<f64|f32>:<vec|scalar>' of this thread's last Device.rank_update "
          "('host' on the host executor)");
  mod.def("last_grad_matrix_kernel", [] { return std::string(kern::last_grad_matrix_kernel()); },
          "test probe: 'gm<k padded to 4>:<f64|f32|nop>:<vec|scalar>' of this thread's last Device.grad_matrix "
          "('host' on the host executor)");
  mod.def("last_slogdet_kernel", [] { return std::string(kern::last_slogdet_kernel()); },
          "test probe: 'sld:<lds|glob>:<f64|f32>' of this thread's last Device.slogdet_batch ('host' on the "
          "host executor)");
  mod.def("last_equil_kernel", [] { return std::string(kern::last_equil_kernel()); },
          "test probe: 'eq:<rmax|cmax|scale>:<f64|f32>:<vec|scalar>' of this thread's last Device.abs_max_rows / "
          "abs_max_cols / scale_pow2 ('host' on the host executor)");
  mod.def("last_batch_kernel", [] { return std::string(kern::last_batch_kernel()); },
          "test probe: 'bpack:<f64|f32>', 'bunpack:<f64|f32>' or 'brhs<16|32|64>:<f64|f32>:<vec|scalar>' of this "
          "thread's last Device.batch_pack / batch_unpack / batch_rhs ('host' on the host executors)");
  mod.def("set_equil_col_split", [](int v) { kern::set_equil_col_split(v); },
          "test hook: row split of the following Device.abs_max_cols launches on the GPU (0 = auto, s >= 1 forces s)");
  mod.def("set_equil_nt", [](bool on) { kern::set_equil_nt(on ? 1 : 0); },
          "Device.scale_pow2 on the GPU: panel accesses with the non-temporal policy (default) or plain (measurements)");
  mod.def("set_lat_glds", [](bool on) { kern::set_lat_glds(on ? 1 : 0); },
          "every latency GEMM of >= 1024 rows on the LDS-DMA kernel (tests; the engine sets it per launch)");

  // Kernel-level entry points (raw pointers; used by the per-kernel numerics tests and
  // mpi_jordan_crazy_acceleration_amd.ops).  Every op runs on the MAIN stream and is waited for.
  using U = uintptr_t;
  auto lay = [](int64_t n, int64_t m, int64_t p, int64_t k) { return Layout::make(n, m, p, k); };
  py::class_<Device, std::shared_ptr<Device>>(mod, "Device")
      .def_property_readonly("on_gpu", &Device::on_gpu)
      .def("describe", &Device::describe)
      .def("sync", &Device::sync_all, py::call_guard<py::gil_scoped_release>())
      .def("gemm",
           [](Device& d, const std::string& dt, const std::string& op, bool a_kmajor, int64_t M,
              int64_t N, int64_t K, U A, int64_t lda, U B, int64_t ldb, U C, int64_t ldc, int64_t zc0,
              int64_t zc1, std::vector<int64_t> zero_rows, int64_t zh, U tneg, int64_t ldtneg, bool latency,
              int64_t tneg_cols, bool dense, U c_in, int64_t ldc_in, std::vector<int64_t> row_blocks,
              int64_t row_block_m, int64_t skip_c0, int64_t skip_c1, py::object owner, bool lat_wide,
              bool lat_reg, int glds_build, int glds_tile, int c_nt) {
             GemmExtra ex;
             set_owner(ex, owner);
             ex.lat_wide = lat_wide;
             ex.lat_reg = lat_reg;
             ex.glds_build = glds_build;
             ex.glds_tile = glds_tile;
             ex.c_nt = c_nt;
             ex.dense = dense;
             ex.skip_c0 = skip_c0;
             ex.skip_c1 = skip_c1;
             ex.c_in = (const void*)c_in;
             ex.ldc_in = ldc_in;
             if (row_block_m > 0) {  // GemmExtra::rsel from a list of selected row blocks
               ex.rsel_m = row_block_m;
               for (int64_t b : row_blocks) {
                 if (b < 0 || b >= 64 * GemmExtra::kRselWords) throw std::invalid_argument("row block out of range");
                 ex.rsel[b / 64] |= uint64_t(1) << (b % 64);
               }
               if (M != ex.rsel_count() * row_block_m) throw std::invalid_argument("M != selected rows");
             }
             ex.tneg = (void*)tneg;
             ex.ldtneg = ldtneg;
             ex.tneg_cols = tneg_cols;
             ex.latency = latency;
             ex.zc0 = zc0;
             ex.zc1 = zc1;
             if (zero_rows.size() > (size_t)GemmExtra::kMaxZeroRows) throw std::invalid_argument("too many zero rows");
             ex.nzr = (int)zero_rows.size();
             for (size_t i = 0; i < zero_rows.size(); ++i) ex.zr[i] = zero_rows[i];
             ex.zh = zh;
             d.gemm(parse_dtype(dt), op == "store" ? GemmOp::Store : GemmOp::Acc,
                    a_kmajor ? ALayout::KMajor : ALayout::RowMajor, M, N, K, (const void*)A, lda,
                    (const void*)B, ldb, (void*)C, ldc, S_MAIN, ex);
             d.sync_stream(S_MAIN);
           },
           py::arg("dtype"), py::arg("op"), py::arg("a_kmajor"), py::arg("M"), py::arg("N"), py::arg("K"),
           py::arg("A"), py::arg("lda"), py::arg("B"), py::arg("ldb"), py::arg("C"), py::arg("ldc"),
           py::arg("zc0") = 0, py::arg("zc1") = 0, py::arg("zero_rows") = std::vector<int64_t>(),
           py::arg("zh") = 0, py::arg("tneg") = U(0), py::arg("ldtneg") = 0, py::arg("latency") = false,
           py::arg("tneg_cols") = 0, py::arg("dense") = false, py::arg("c_in") = U(0), py::arg("ldc_in") = 0,
           py::arg("row_blocks") = std::vector<int64_t>(), py::arg("row_block_m") = 0, py::arg("skip_c0") = 0,
           py::arg("skip_c1") = 0, py::arg("owner") = py::none(), py::arg("lat_wide") = false,
           py::arg("lat_reg") = false, py::arg("glds_build") = 0, py::arg("glds_tile") = 0, py::arg("c_nt") = -1)
      .def("gemm_batch",
           // product: (op, M, N, K, A, lda, B, ldb, C, ldc[, lat_reg[, owner]]), owner as in gemm
           [](Device& d, const std::string& dt, const std::vector<py::tuple>& ps) {
             std::vector<GemmDesc> v(ps.size());
             for (size_t i = 0; i < ps.size(); ++i) {
               const py::tuple& t = ps[i];
               if (t.size() < 10 || t.size() > 12) throw std::invalid_argument("gemm_batch: 10 to 12 fields per product");
               GemmDesc& g = v[i];
               g.op = t[0].cast<std::string>() == "store" ? GemmOp::Store : GemmOp::Acc;
               g.M = t[1].cast<int64_t>(); g.N = t[2].cast<int64_t>(); g.K = t[3].cast<int64_t>();
               g.A = (const void*)t[4].cast<U>(); g.lda = t[5].cast<int64_t>();
               g.B = (const void*)t[6].cast<U>(); g.ldb = t[7].cast<int64_t>();
               g.C = (void*)t[8].cast<U>(); g.ldc = t[9].cast<int64_t>();
               if (t.size() > 10) g.ex.lat_reg = t[10].cast<bool>();
               if (t.size() > 11) set_owner(g.ex, t[11]);
             }
             d.gemm_batch(parse_dtype(dt), v.data(), (int)v.size(), S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dtype"), py::arg("products"))
      .def("generate",
           [lay](Device& d, const std::string& dt, U X, int64_t n, int64_t m, int64_t p, int64_t k,
                 const std::string& kind, uint64_t seed) {
             GenSpec g;
             g.kind = parse_gen(kind);
             g.seed = seed;
             d.generate(parse_dtype(dt), (void*)X, lay(n, m, p, k), g, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("extract_neg_t",
           [](Device& d, const std::string& dt, U Lt, int64_t ldl, U X, int64_t ldx, int64_t rows,
              int64_t col0, int64_t m) {
             d.extract_neg_t(parse_dtype(dt), (void*)Lt, ldl, (const void*)X, ldx, rows, col0, m, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("block_inverse",
           [lay](Device& d, const std::string& dt, U Lt, int64_t ldl, U inv_t, U scores, U valid,
                 U used, int64_t n, int64_t m, int64_t p, int64_t k, double thresh, int64_t nlive) {
             d.block_inverse(parse_dtype(dt), (const void*)Lt, ldl, (void*)inv_t, (double*)scores,
                             (int32_t*)valid, (const int32_t*)used, lay(n, m, p, k), thresh, nlive, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("Lt"), py::arg("ldl"), py::arg("inv_t"), py::arg("scores"), py::arg("valid"),
           py::arg("used"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"), py::arg("thresh"),
           py::arg("nlive") = -1)
      // pivot selection kernels (tests): local argmin of one rank's candidates -> 32-B record at rec
      .def("pivot_local",
           [lay](Device& d, U scores, U valid, U used, U pos, int64_t n, int64_t m, int64_t p, int64_t k, U rec) {
             d.pivot_local((const double*)scores, (const int32_t*)valid, (const int32_t*)used,
                           (const int32_t*)pos, lay(n, m, p, k), (PivotRec*)rec, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // one rank: argmin + book-keeping (pos / phys_at / used / seq) + result record, one launch
      .def("pivot_select_single",
           [lay](Device& d, U scores, U valid, int64_t n, int64_t m, int t, U pos, U phys_at, U used, U seq,
                 U rec, U out) {
             d.pivot_select_single((const double*)scores, (const int32_t*)valid, lay(n, m, 1, 0), (int32_t)t,
                                   (int32_t*)pos, (int32_t*)phys_at, (int32_t*)used, (int32_t*)seq,
                                   (PivotRec*)rec, (PivotResult*)out, nullptr, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // p ranks' gathered records -> winner, book-keeping, *out and the pinned host mirror (returned
      // as (step, found, phys, owner, logical, score), read after the stream completes)
      .def("pivot_global",
           [](Device& d, U recs, int p, int t, U pos, U phys_at, U used, U seq, U out) {
             const auto mirror = DevBuf<PivotResult>::pinned_coherent(d, 1);
             PivotResult* h = mirror;
             h->step = -1;
             d.pivot_global((const PivotRec*)recs, (int32_t)p, (int32_t)t, (int32_t*)pos, (int32_t*)phys_at,
                            (int32_t*)used, (int32_t*)seq, (PivotResult*)out, h, S_MAIN);
             d.sync_stream(S_MAIN);
             return py::make_tuple(h->step, h->found, h->phys, h->owner, h->logical, h->score);
           })
      // block_inverse with the selection run by the launch's last workgroup (PivotSelectArgs; `used`
      // doubles as used_w, as in Engine::select).  `done` is the caller's device counter (0 between
      // launches).  p == 1: the whole selection, with a pinned host mirror read after the stream
      // completes.  Returns (fused, mirror (step, found, phys, owner, logical, score) or None);
      // fused == False: nothing was enqueued.
      .def("block_inverse_select",
           [lay](Device& d, const std::string& dt, U Lt, int64_t ldl, U inv_t, U scores, U valid, U used,
                 int64_t n, int64_t m, int64_t p, int64_t k, double thresh, int64_t nlive, int t, U pos,
                 U phys_at, U seq, U rec, U out, U done) {
             DevBuf<PivotResult> pinned;
             if (p == 1) pinned = DevBuf<PivotResult>::pinned_coherent(d, 1);
             PivotResult* h = pinned;
             if (h) {
               std::memset(h, 0, sizeof(PivotResult));
               h->step = -1;
             }
             PivotSelectArgs sel;
             sel.done = (int32_t*)done;
             sel.t = (int32_t)t;
             sel.pos = (const int32_t*)pos;
             sel.pos_w = (int32_t*)pos;
             sel.phys_at = (int32_t*)phys_at;
             sel.used_w = (int32_t*)used;
             sel.seq = (int32_t*)seq;
             sel.rec = (PivotRec*)rec;
             sel.out = (PivotResult*)out;
             sel.host_out = h;
             sel.single = p == 1 ? 1 : 0;
             const bool fused =
                 d.block_inverse_select(parse_dtype(dt), (const void*)Lt, ldl, (void*)inv_t, (double*)scores,
                                        (int32_t*)valid, (const int32_t*)used, lay(n, m, p, k), thresh, nlive, sel,
                                        S_MAIN);
             d.sync_stream(S_MAIN);
             py::object mirror = py::none();
             if (h) mirror = py::make_tuple(h->step, h->found, h->phys, h->owner, h->logical, h->score);
             return py::make_tuple(fused, mirror);
           },
           py::arg("dt"), py::arg("Lt"), py::arg("ldl"), py::arg("inv_t"), py::arg("scores"), py::arg("valid"),
           py::arg("used"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"), py::arg("thresh"),
           py::arg("nlive"), py::arg("t"), py::arg("pos"), py::arg("phys_at"), py::arg("seq"), py::arg("rec"),
           py::arg("out"), py::arg("done"))
      // Device-side latency of the batched block inverse: `reps` back-to-back launches on one
      // stream between two timing events (no host work in between); returns microseconds per call.
      .def("time_block_inverse",
           [lay](Device& d, const std::string& dt, U Lt, int64_t ldl, U inv_t, U scores, U valid,
                 U used, int64_t n, int64_t m, int64_t p, int64_t k, double thresh, int reps, int64_t nlive) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.block_inverse(t, (const void*)Lt, ldl, (void*)inv_t, (double*)scores, (int32_t*)valid,
                               (const int32_t*)used, L, thresh, nlive, S_SIDE);
             };
             run(0);
             return time_launches(d, S_SIDE, reps, run);
           },
           py::arg("dt"), py::arg("Lt"), py::arg("ldl"), py::arg("inv_t"), py::arg("scores"), py::arg("valid"),
           py::arg("used"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"), py::arg("thresh"),
           py::arg("reps"), py::arg("nlive") = -1)
      // Device-side time of panel_rhs (Y = P V, every column active, column maxima on), and of the
      // plain GEMM C = A B (row-major A, M x N x K) it is measured against: `reps` back-to-back
      // launches between two timing events after one warm-up launch; microseconds per call.
      .def("time_panel_rhs",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U Y, int64_t ldy, U colmax, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.panel_rhs(t, (const void*)P, ldp, L, (const double*)V, ldv, ncols, nullptr, 0, (double*)Y, ldy, 1.0,
                           nullptr, (double*)colmax, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      // The same timing of panel_rhs_dd (Y = -P V from the double-double sum, P fp64)
      .def("time_panel_rhs_dd",
           [lay](Device& d, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k, U V, int64_t ldv,
                 int64_t ncols, U Y, int64_t ldy, U colmax, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             auto run = [&](int) {
               d.panel_rhs_dd(DType::F64, (const void*)P, ldp, L, (const double*)V, ldv, ncols, nullptr, 0, (double*)Y,
                              ldy, nullptr, (double*)colmax, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      // The same timing of panel_rhs_t (S = P^T V, every column active) and of the K-major GEMM it is
      // measured against (C = At^T B with At = P: M = n, K = the rows of P).
      .def("time_panel_rhs_t",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U S, int64_t lds, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.panel_rhs_t(t, (const void*)P, ldp, L, (const double*)V, ldv, ncols, (double*)S, lds, nullptr,
                             S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      // The same timings of their siblings on absolute values (Y = |P| |V| with column maxima, S = |P|^T |V|)
      .def("time_panel_abs_rhs",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U Y, int64_t ldy, U colmax, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.panel_abs_rhs(t, (const void*)P, ldp, L, (const double*)V, ldv, ncols, nullptr, 0, (double*)Y, ldy,
                               (double*)colmax, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("time_panel_abs_rhs_t",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U S, int64_t lds, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.panel_abs_rhs_t(t, (const void*)P, ldp, L, (const double*)V, ldv, ncols, (double*)S, lds, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      // The same timing of rank_update (X -= / += W Z^T in turn, so that X stays bounded), W in local order
      .def("time_rank_update",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U W, int64_t ldw, U Z, int64_t ldz, int64_t ncols, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, p, k);
             const DType t = parse_dtype(dt);
             auto run = [&](int i) {
               d.rank_update(t, (void*)X, ldx, L, (const double*)W, ldw, false, (const double*)Z, ldz, ncols,
                             i % 2 ? 1.0 : -1.0, S_MAIN);
             };
             run(0);
             run(1);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("time_gemm_store_kmajor",
           [](Device& d, const std::string& dt, int64_t M, int64_t N, int64_t K, U A, int64_t lda, U B, int64_t ldb,
              U C, int64_t ldc, int reps) {
             py::gil_scoped_release rel;
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.gemm(t, GemmOp::Store, ALayout::KMajor, M, N, K, (const void*)A, lda, (const void*)B, ldb, (void*)C,
                      ldc, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("time_gemm_store",
           [](Device& d, const std::string& dt, int64_t M, int64_t N, int64_t K, U A, int64_t lda, U B, int64_t ldb,
              U C, int64_t ldc, int reps) {
             py::gil_scoped_release rel;
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.gemm(t, GemmOp::Store, ALayout::RowMajor, M, N, K, (const void*)A, lda, (const void*)B, ldb, (void*)C,
                      ldc, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("permute_blocks",
           [](Device& d, const std::string& dt, U dst, int64_t ldd, U X, int64_t ldx, int64_t nblk,
              int64_t m, int64_t Nr, U dst_blk, U colsrc) {
             d.permute_blocks(parse_dtype(dt), (void*)dst, ldd, (const void*)X, ldx, nblk, m, Nr,
                              (const int32_t*)dst_blk, (const int32_t*)colsrc, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("row_abs_max",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p,
                 int64_t k, U out) {
             d.row_abs_max(parse_dtype(dt), (const void*)X, ldx, lay(n, m, p, k), (double*)out, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("residual",
           [lay](Device& d, const std::string& dt, U A, U Full, int64_t n, int64_t m, int64_t p,
                 int64_t k, U out) {
             d.residual(parse_dtype(dt), (const void*)A, (const void*)Full, lay(n, m, p, k),
                        (double*)out, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("row_abs_max_minus_i",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p,
                 int64_t k, U out) {
             d.row_abs_max_minus_i(parse_dtype(dt), (const void*)X, ldx, lay(n, m, p, k), (double*)out, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // owner-side edits of a pivot step; the PieceMove fields default to "none"
      .def("owner_edits",
           [](Device& d, const std::string& dt, U At, int64_t ldl, U phys, int64_t p, int64_t k, int64_t j,
              int64_t m, U lrow, U ht, U inv, U dst, int64_t ldd, U X, int64_t ldx, int64_t col0, int64_t w,
              U eye, int64_t ld_eye) {
             PieceMove mv;
             mv.dst = (void*)dst;
             mv.ldd = ldd;
             mv.X = (void*)X;
             mv.ldx = ldx;
             mv.col0 = col0;
             mv.w = w;
             mv.eye = (void*)eye;
             mv.ld_eye = ld_eye;
             d.owner_edits(parse_dtype(dt), (void*)At, ldl, (const int32_t*)phys, p, k, j, m, (void*)lrow,
                           (void*)ht, (const void*)inv, mv, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("At"), py::arg("ldl"), py::arg("phys"), py::arg("p"), py::arg("k"), py::arg("j"),
           py::arg("m"), py::arg("lrow"), py::arg("ht"), py::arg("inv"), py::arg("dst") = U(0), py::arg("ldd") = 0,
           py::arg("X") = U(0), py::arg("ldx") = 0, py::arg("col0") = 0, py::arg("w") = 0, py::arg("eye") = U(0),
           py::arg("ld_eye") = 0)
      .def("take_rows",
           [](Device& d, const std::string& dt, U dst, int64_t ldd, U X, int64_t ldx, U phys, int64_t p, int64_t k,
              int64_t col0, int64_t w, int64_t m) {
             d.take_rows(parse_dtype(dt), (void*)dst, ldd, (void*)X, ldx, (const int32_t*)phys, p, k, col0, w, m,
                         S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("sum_slices",
           [](Device& d, const std::string& dt, U dst, U src, int64_t count, int64_t nslices) {
             d.sum_slices(parse_dtype(dt), (void*)dst, (const void*)src, count, nslices, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("zero_unless_owner",
           [](Device& d, const std::string& dt, U buf, int64_t count, U phys, int64_t p, int64_t k) {
             d.zero_unless_owner(parse_dtype(dt), (void*)buf, count, (const int32_t*)phys, p, k, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("h_block",
           [](Device& d, const std::string& dt, U R, int64_t ldr, U Ht, int64_t m) {
             d.h_block(parse_dtype(dt), (void*)R, ldr, (const void*)Ht, m, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // 64-bit partial sums into the kHashParts words at parts
      .def("hash_rows",
           [](Device& d, U base, int64_t ld_bytes, int64_t width_bytes, int64_t rows, U parts) {
             d.hash_rows((const void*)base, ld_bytes, width_bytes, rows, (uint64_t*)parts, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def_property_readonly_static("kHashParts", [](py::object) { return (int)Device::kHashParts; })
      // Y = C_in + sign * P V for a block of right-hand sides; 0 = a null pointer
      .def("panel_rhs",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U C_in, int64_t ldc, U Y, int64_t ldy, double sign, U active,
                 U colmax) {
             py::gil_scoped_release rel;
             d.panel_rhs(parse_dtype(dt), (const void*)P, ldp, lay(n, m, p, k), (const double*)V, ldv, ncols,
                         (const double*)C_in, ldc, (double*)Y, ldy, sign, (const int32_t*)active, (double*)colmax,
                         S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("V"), py::arg("ldv"), py::arg("ncols"), py::arg("C_in"), py::arg("ldc"), py::arg("Y"),
           py::arg("ldy"), py::arg("sign"), py::arg("active") = U(0), py::arg("colmax") = U(0))
      // Y = round(C_in - P V) from a double-double sum, P fp64; 0 = a null pointer
      .def("panel_rhs_dd",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U C_in, int64_t ldc, U Y, int64_t ldy, U active, U colmax) {
             py::gil_scoped_release rel;
             d.panel_rhs_dd(parse_dtype(dt), (const void*)P, ldp, lay(n, m, p, k), (const double*)V, ldv, ncols,
                            (const double*)C_in, ldc, (double*)Y, ldy, (const int32_t*)active, (double*)colmax, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("V"), py::arg("ldv"), py::arg("ncols"), py::arg("C_in"), py::arg("ldc"), py::arg("Y"),
           py::arg("ldy"), py::arg("active") = U(0), py::arg("colmax") = U(0))
      // S = P^T V over this rank's real rows (its term of the transposed product); 0 = a null pointer
      .def("panel_rhs_t",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U S, int64_t lds, U active) {
             py::gil_scoped_release rel;
             d.panel_rhs_t(parse_dtype(dt), (const void*)P, ldp, lay(n, m, p, k), (const double*)V, ldv, ncols,
                           (double*)S, lds, (const int32_t*)active, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("V"), py::arg("ldv"), py::arg("ncols"), py::arg("S"), py::arg("lds"), py::arg("active") = U(0))
      // Y = |C_in| + |P| |V| in fp64 whatever dt is; 0 = a null pointer
      .def("panel_abs_rhs",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U C_in, int64_t ldc, U Y, int64_t ldy, U colmax) {
             py::gil_scoped_release rel;
             d.panel_abs_rhs(parse_dtype(dt), (const void*)P, ldp, lay(n, m, p, k), (const double*)V, ldv, ncols,
                             (const double*)C_in, ldc, (double*)Y, ldy, (double*)colmax, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("V"), py::arg("ldv"), py::arg("ncols"), py::arg("C_in"), py::arg("ldc"), py::arg("Y"),
           py::arg("ldy"), py::arg("colmax") = U(0))
      // S = |P|^T |V| over this rank's real rows, in fp64 whatever dt is
      .def("panel_abs_rhs_t",
           [lay](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, int64_t m, int64_t p, int64_t k,
                 U V, int64_t ldv, int64_t ncols, U S, int64_t lds) {
             py::gil_scoped_release rel;
             d.panel_abs_rhs_t(parse_dtype(dt), (const void*)P, ldp, lay(n, m, p, k), (const double*)V, ldv, ncols,
                               (double*)S, lds, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("V"), py::arg("ldv"), py::arg("ncols"), py::arg("S"), py::arg("lds"))
      // G = |R| + nz_eps D (+ safe1 where D <= safe2), berr[j] = max_r |R| / D (xGERFS)
      .def("bound_terms",
           [](Device& d, U R, int64_t ldr, U D, int64_t ldd, U G, int64_t ldg, int64_t rows, int64_t ncols,
              double nz_eps, double safe1, double safe2, U berr) {
             py::gil_scoped_release rel;
             d.bound_terms((const double*)R, ldr, (const double*)D, ldd, (double*)G, ldg, rows, ncols, nz_eps, safe1,
                           safe2, (double*)berr, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("R"), py::arg("ldr"), py::arg("D"), py::arg("ldd"), py::arg("G"), py::arg("ldg"), py::arg("rows"),
           py::arg("ncols"), py::arg("nz_eps"), py::arg("safe1"), py::arg("safe2"), py::arg("berr"))
      // X += sign * W Z^T over this rank's real rows and the columns < n, rounded once (in place)
      .def("rank_update",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U W, int64_t ldw, bool w_natural, U Z, int64_t ldz, int64_t ncols, double sign) {
             py::gil_scoped_release rel;
             d.rank_update(parse_dtype(dt), (void*)X, ldx, lay(n, m, p, k), (const double*)W, ldw, w_natural,
                           (const double*)Z, ldz, ncols, sign, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("X"), py::arg("ldx"), py::arg("n"), py::arg("m"), py::arg("p"), py::arg("k"),
           py::arg("W"), py::arg("ldw"), py::arg("w_natural"), py::arg("Z"), py::arg("ldz"), py::arg("ncols"),
           py::arg("sign"))
      // G (+)= alpha * P^T + sign * W Z^T over n x n, in fp64 (P of dtype dt; 0 = null where never read)
      .def("grad_matrix",
           [](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, double alpha, U W, int64_t ldw, U Z,
              int64_t ldz, int64_t ncols, double sign, bool accumulate, U G, int64_t ldg) {
             py::gil_scoped_release rel;
             d.grad_matrix(parse_dtype(dt), (const void*)P, ldp, n, alpha, (const double*)W, ldw, (const double*)Z,
                           ldz, ncols, sign, accumulate, (double*)G, ldg, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("P"), py::arg("ldp"), py::arg("n"), py::arg("alpha"), py::arg("W"), py::arg("ldw"),
           py::arg("Z"), py::arg("ldz"), py::arg("ncols"), py::arg("sign"), py::arg("accumulate"), py::arg("G"),
           py::arg("ldg"))
      // The same timing of grad_matrix (the same launch `reps` times: G is only written unless accumulating)
      .def("time_grad_matrix",
           [](Device& d, const std::string& dt, U P, int64_t ldp, int64_t n, double alpha, U W, int64_t ldw, U Z,
              int64_t ldz, int64_t ncols, double sign, bool accumulate, U G, int64_t ldg, int reps) {
             py::gil_scoped_release rel;
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               d.grad_matrix(t, (const void*)P, ldp, n, alpha, (const double*)W, ldw, (const double*)Z, ldz, ncols,
                             sign, accumulate, (double*)G, ldg, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      // (sign, log|det|) of nb blocks of m x m (dtype dt, stride elements apart); which: int32[nb] or 0
      .def("slogdet_batch",
           [](Device& d, const std::string& dt, U blocks, int64_t stride, int64_t m, int64_t nb, U which, U sign,
              U logabs) {
             py::gil_scoped_release rel;
             d.slogdet_batch(parse_dtype(dt), (const void*)blocks, stride, m, nb, (const int32_t*)which,
                             (double*)sign, (double*)logabs, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("blocks"), py::arg("stride"), py::arg("m"), py::arg("nb"), py::arg("which"),
           py::arg("sign"), py::arg("logabs"))
      .def("slogdet_scratch_bytes", [](Device& d, int64_t m, int64_t nb) { return d.slogdet_scratch_bytes(m, nb); })
      // the stack ops (BatchSolver's): pack / unpack around block_inverse, and the stack's products
      .def("batch_pack",
           [](Device& d, const std::string& dt, U A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m, int64_t nb,
              U Lt, int64_t ldl, U norm, U exp) {
             py::gil_scoped_release rel;
             d.batch_pack(parse_dtype(dt), (const double*)A64, stride_a, lda, n, m, nb, (void*)Lt, ldl, (double*)norm,
                          (int32_t*)exp, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("A64"), py::arg("stride_a"), py::arg("lda"), py::arg("n"), py::arg("m"),
           py::arg("nb"), py::arg("Lt"), py::arg("ldl"), py::arg("norm"), py::arg("exp"))
      .def("batch_unpack",
           [](Device& d, const std::string& dt, U inv_t, int64_t n, int64_t m, int64_t nb, U exp, U valid, U X,
              int64_t stride_x, int64_t ldx) {
             py::gil_scoped_release rel;
             d.batch_unpack(parse_dtype(dt), (const void*)inv_t, n, m, nb, (const int32_t*)exp, (const int32_t*)valid,
                            (void*)X, stride_x, ldx, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("inv_t"), py::arg("n"), py::arg("m"), py::arg("nb"), py::arg("exp"),
           py::arg("valid"), py::arg("X"), py::arg("stride_x"), py::arg("ldx"))
      .def("batch_rhs",
           [](Device& d, const std::string& dt, U M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb, U V,
              int64_t stride_v, int64_t ldv, int64_t ncols, U C_in, int64_t stride_c, int64_t ldc, U Y, int64_t stride_y,
              int64_t ldy, double sign, U active, U colmax) {
             py::gil_scoped_release rel;
             d.batch_rhs(parse_dtype(dt), (const void*)M, stride_m, ldm, n, nb, (const double*)V, stride_v, ldv, ncols,
                         (const double*)C_in, stride_c, ldc, (double*)Y, stride_y, ldy, sign, (const int32_t*)active,
                         (double*)colmax, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("dt"), py::arg("M"), py::arg("stride_m"), py::arg("ldm"), py::arg("n"), py::arg("nb"), py::arg("V"),
           py::arg("stride_v"), py::arg("ldv"), py::arg("ncols"), py::arg("C_in"), py::arg("stride_c"),
           py::arg("ldc"), py::arg("Y"), py::arg("stride_y"), py::arg("ldy"), py::arg("sign"),
           py::arg("active") = U(0), py::arg("colmax") = U(0))
      // device time per launch (microseconds) of the stack ops, for bench/bench_batched.py
      .def("time_batch_op",
           [](Device& d, const std::string& which, const std::string& dt, U A, U B, U C, U e, U v, int64_t n, int64_t m,
              int64_t nb, int64_t ncols, int reps) {
             py::gil_scoped_release rel;
             const DType t = parse_dtype(dt);
             auto run = [&](int) {
               if (which == "pack")  // A: fp64 stack, B: Lt, C: norm
                 d.batch_pack(t, (const double*)A, n * n, n, n, m, nb, (void*)B, nb * m, (double*)C, (int32_t*)e, S_MAIN);
               else if (which == "unpack")  // A: inv_t, B: X
                 d.batch_unpack(t, (const void*)A, n, m, nb, (const int32_t*)e, (const int32_t*)v, (void*)B, n * n, n,
                                S_MAIN);
               else  // A: M, B: V, C: Y
                 d.batch_rhs(t, (const void*)A, n * n, n, n, nb, (const double*)B, n * ncols, ncols, ncols, nullptr, 0, 0,
                             (double*)C, n * ncols, ncols, 1.0, nullptr, nullptr, S_MAIN);
             };
             run(0);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("axpy_cols_masked",
           [](Device& d, U Y, int64_t ldy, U C_in, int64_t ldc, U S, int64_t lds, double sign, int64_t rows,
              int64_t ncols, U active, U colmax) {
             py::gil_scoped_release rel;
             d.axpy_cols_masked((double*)Y, ldy, (const double*)C_in, ldc, (const double*)S, lds, sign, rows, ncols,
                                (const int32_t*)active, (double*)colmax, S_MAIN);
             d.sync_stream(S_MAIN);
           },
           py::arg("Y"), py::arg("ldy"), py::arg("C_in"), py::arg("ldc"), py::arg("S"), py::arg("lds"),
           py::arg("sign"), py::arg("rows"), py::arg("ncols"), py::arg("active") = U(0), py::arg("colmax") = U(0))
      .def("col_abs_sum",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U out) {
             py::gil_scoped_release rel;
             d.col_abs_sum(parse_dtype(dt), (const void*)X, ldx, lay(n, m, p, k), (double*)out, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // the equilibration ops (rexp_nat / cexp: int32 device arrays or 0)
      .def("abs_max_rows",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U out_nat) {
             py::gil_scoped_release rel;
             d.abs_max_rows(parse_dtype(dt), (const void*)X, ldx, lay(n, m, p, k), (double*)out_nat, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("abs_max_cols",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U rexp_nat, U out) {
             py::gil_scoped_release rel;
             d.abs_max_cols(parse_dtype(dt), (const void*)X, ldx, lay(n, m, p, k), (const int32_t*)rexp_nat,
                            (double*)out, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("scale_pow2",
           [lay](Device& d, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m, int64_t p, int64_t k,
                 U rexp_nat, U cexp) {
             py::gil_scoped_release rel;
             d.scale_pow2(parse_dtype(dt), (void*)X, ldx, lay(n, m, p, k), (const int32_t*)rexp_nat,
                          (const int32_t*)cexp, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // device time per launch (microseconds) of the three equilibration ops: which = rmax | cmax | scale
      // (scale alternates the sign of the exponents, so that X stays bounded)
      .def("time_equil",
           [lay](Device& d, const std::string& which, const std::string& dt, U X, int64_t ldx, int64_t n, int64_t m,
                 U rexp, U cexp, U rexp_neg, U cexp_neg, U out, int reps) {
             py::gil_scoped_release rel;
             const Layout L = lay(n, m, 1, 0);
             const DType t = parse_dtype(dt);
             auto run = [&](int i) {
               if (which == "rmax") d.abs_max_rows(t, (const void*)X, ldx, L, (double*)out, S_MAIN);
               else if (which == "cmax") d.abs_max_cols(t, (const void*)X, ldx, L, (const int32_t*)rexp, (double*)out, S_MAIN);
               else if (i % 2 == 0) d.scale_pow2(t, (void*)X, ldx, L, (const int32_t*)rexp, (const int32_t*)cexp, S_MAIN);
               else d.scale_pow2(t, (void*)X, ldx, L, (const int32_t*)rexp_neg, (const int32_t*)cexp_neg, S_MAIN);
             };
             run(0);
             run(1);
             return time_launches(d, S_MAIN, reps, run);
           })
      .def("gather_rows_natural",
           [lay](Device& d, U dst, int64_t ldd, U src, int64_t lds, int64_t n, int64_t m, int64_t p, int64_t ncols) {
             d.gather_rows_natural((double*)dst, ldd, (const double*)src, lds, lay(n, m, p, 0), ncols, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("copy_cols_masked",
           [](Device& d, U dst, int64_t ldd, U src, int64_t lds, int64_t rows, int64_t ncols, U mask) {
             d.copy_cols_masked((double*)dst, ldd, (const double*)src, lds, rows, ncols, (const int32_t*)mask, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("widen",
           [](Device& d, const std::string& dt, U dst, int64_t ldd, U X, int64_t ldx, int64_t rows, int64_t cols) {
             d.widen(parse_dtype(dt), (double*)dst, ldd, (const void*)X, ldx, rows, cols, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("upload_convert",
           [](Device& d, const std::string& dt, U X, int64_t ldx, U src, int64_t src_ld, int64_t rows,
              int64_t cols) {
             d.upload_convert(parse_dtype(dt), (void*)X, ldx, (const double*)src, src_ld, rows, cols, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("add_diag",
           [](Device& d, const std::string& dt, U A, int64_t ld, int64_t nd, double alpha) {
             d.add_diag(parse_dtype(dt), (void*)A, ld, nd, alpha, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      // partial pivoting: candidate scores, the chosen block copied out, its inverse committed
      .def("candidate_maxabs",
           [lay](Device& d, const std::string& dt, U Lt, int64_t ldl, U scores, U valid, U used, int64_t n,
                 int64_t m, int64_t p, int64_t k, double thresh) {
             d.candidate_maxabs(parse_dtype(dt), (const void*)Lt, ldl, (double*)scores, (int32_t*)valid,
                                (const int32_t*)used, lay(n, m, p, k), thresh, S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("gather_candidate",
           [lay](Device& d, const std::string& dt, U sel, U Lt, int64_t ldl, U rec, int64_t n, int64_t m,
                 int64_t p, int64_t k) {
             d.gather_candidate(parse_dtype(dt), (void*)sel, (const void*)Lt, ldl, (const PivotRec*)rec,
                                lay(n, m, p, k), S_MAIN);
             d.sync_stream(S_MAIN);
           })
      .def("commit_candidate",
           [lay](Device& d, const std::string& dt, U inv_t, U inv1, U valid1, U score1, double growth, U rec,
                 int64_t n, int64_t m, int64_t p, int64_t k) {
             d.commit_candidate(parse_dtype(dt), (void*)inv_t, (const void*)inv1, (const int32_t*)valid1,
                                (const double*)score1, growth, (PivotRec*)rec, lay(n, m, p, k), S_MAIN);
             d.sync_stream(S_MAIN);
           });
  mod.def("hip_device", [](int idx) { return std::shared_ptr<Device>(new HipDevice(idx)); });
  mod.def("host_device", [](int nthreads) { return std::shared_ptr<Device>(new HostDevice(nthreads)); },
          py::arg("nthreads") = 0);
  // the asynchronous host executor (its own worker threads per stream), for per-op tests
  mod.def("async_host_device", [](int nthreads) { return std::shared_ptr<Device>(new AsyncHostDevice(nthreads)); },
          py::arg("nthreads") = 1);

  // A host executor under the schedule checker (gj/race_check.hpp), for drivers that take a Device:
  // returns (device, checker); async: the asynchronous executor (its own worker threads per stream).
  py::class_<HbChecker, std::shared_ptr<HbChecker>>(mod, "HbChecker")
      .def("races", &HbChecker::races)
      .def("ops", &HbChecker::ops)
      .def("reports", &HbChecker::reports);
  mod.def("race_check_host_device",
          [](bool async, int nthreads) {
            auto hb = std::make_shared<HbChecker>();
            std::unique_ptr<Device> inner;
            if (async) inner.reset(new AsyncHostDevice(nthreads));
            else inner.reset(new HostDevice(nthreads));
            std::shared_ptr<Device> dev(new RaceCheckDevice(std::move(inner), hb, "batch"));
            return py::make_tuple(dev, hb);
          },
          py::arg("async") = true, py::arg("nthreads") = 1);

  // A stack of small matrices (gj/batch.hpp).  Pointers are integers: memory of the solver's device
  // (host memory on the host executors).
  struct PyBatch {
    std::shared_ptr<Device> dev;  // outlives the solver
    std::unique_ptr<BatchSolver> bs;
    BatchSolveInfo last;
  };
  py::class_<PyBatch>(mod, "BatchSolver")
      .def(py::init([](std::shared_ptr<Device> dev, const std::string& dt, int64_t n, int64_t nb, double eps,
                       size_t workspace_bytes) {
             auto p = std::make_unique<PyBatch>();
             p->dev = dev;
             p->bs = std::make_unique<BatchSolver>(*dev, parse_dtype(dt), n, nb, eps, workspace_bytes);
             return p;
           }),
           py::arg("device"), py::arg("dtype"), py::arg("n"), py::arg("nb"), py::arg("eps") = 1e-15,
           py::arg("workspace_bytes") = 0)
      .def("factor",
           [](PyBatch& b, U A, int64_t stride_a, int64_t lda) {
             py::gil_scoped_release rel;
             b.bs->factor((const double*)A, stride_a, lda);
           },
           py::arg("A"), py::arg("stride_a"), py::arg("lda"))
      .def("inverse",
           [](PyBatch& b, U X, int64_t stride_x, int64_t ldx) {
             py::gil_scoped_release rel;
             b.bs->inverse((void*)X, stride_x, ldx);
           },
           py::arg("X"), py::arg("stride_x"), py::arg("ldx"))
      .def("solve",
           [](PyBatch& b, U B, int64_t stride_b, int64_t ldb, U X, int64_t ncols, int max_refine,
              double tol) {
             BatchSolveInfo r;
             {
               py::gil_scoped_release rel;
               r = b.bs->solve((const double*)B, stride_b, ldb, (double*)X, ncols, max_refine, tol);
             }
             const int64_t nb = b.bs->nb();
             auto arr = [&](const auto& v, auto zero) {
               using T = decltype(zero);
               py::array_t<T> a({nb, ncols});
               std::copy(v.begin(), v.end(), a.mutable_data());
               return a;
             };
             py::dict d;
             d["converged"] = arr(r.converged, int32_t(0));
             d["steps"] = arr(r.steps, int32_t(0));
             d["residual"] = arr(r.residual, 0.0);
             d["backward_error"] = arr(r.backward_error, 0.0);
             d["sweeps"] = r.sweeps;
             return d;
           },
           py::arg("B"), py::arg("stride_b"), py::arg("ldb"), py::arg("X"), py::arg("ncols"),
           py::arg("max_refine") = -1, py::arg("tol") = 1e-15,
           "A_b X_b = B_b, refined in fp64; X comes back stack-interleaved, X[(r * nb + b) * ncols + j]")
      .def("slogdet",
           [](PyBatch& b) {
             const int64_t nb = b.bs->nb();
             py::array_t<double> sg(nb), lg(nb);
             {
               py::gil_scoped_release rel;
               b.bs->slogdet(sg.mutable_data(), lg.mutable_data());
             }
             return py::make_tuple(sg, lg);
           })
      .def_property_readonly("n", [](PyBatch& b) { return b.bs->n(); })
      .def_property_readonly("nb", [](PyBatch& b) { return b.bs->nb(); })
      .def_property_readonly("m", [](PyBatch& b) { return b.bs->m(); })
      .def_property_readonly("chunk", [](PyBatch& b) { return b.bs->chunk(); })
      .def_property_readonly("valid", [](PyBatch& b) { return py::array_t<int32_t>(b.bs->valid().size(), b.bs->valid().data()); })
      .def_property_readonly("exponents", [](PyBatch& b) { return py::array_t<int32_t>(b.bs->exponents().size(), b.bs->exponents().data()); })
      .def_property_readonly("norms", [](PyBatch& b) { return py::array_t<double>(b.bs->norms().size(), b.bs->norms().data()); })
      .def_property_readonly("inverse_norms", [](PyBatch& b) { return py::array_t<double>(b.bs->inverse_norms().size(), b.bs->inverse_norms().data()); })
      .def_property_readonly("inverses_ptr", [](PyBatch& b) { return (U)b.bs->inverses_device(); })
      .def_property_readonly("a64_ptr", [](PyBatch& b) { return (U)b.bs->a64_device(); });

  py::class_<Comm,std::shared_ptr<Comm>>(mod, "Comm")
      .def_property_readonly("size", &Comm::size)
      .def_property_readonly("rank", &Comm::rank)
      .def("describe", &Comm::describe)
      .def("bcast_report", &Comm::bcast_report)
      .def("tune_bcast",
           [](Comm& c, std::shared_ptr<Device> dev, size_t bytes) {
             py::gil_scoped_release r;
             c.tune_bcast(*dev, bytes);
             return c.bcast_report();
           },
           py::arg("device"), py::arg("bytes"));
  mod.def("self_comm", [] { return std::shared_ptr<Comm>(new SelfComm()); });
  mod.def("rccl_comm",
          [](std::vector<py::bytes> ids, int nranks, int rank, int device, bool one_comm) {
            std::vector<std::string> s;
            for (auto& b : ids) s.push_back(std::string(b));
            py::gil_scoped_release rel;
            return std::shared_ptr<Comm>(new RcclComm(s, nranks, rank, device, one_comm));
          },
          py::arg("ids"), py::arg("nranks"), py::arg("rank"), py::arg("device"), py::arg("one_comm") = false,
          "one_comm: the SIDE and COMM roles share one communicator (every rank must pass the same value; "
          "parallel.dist.agree_comm_mode decides it)");
  mod.def("shadow_comm", [](int p, double bw_gbs, double lat_us, int channels, int lds_kib, bool direct) {
            CostModel cm;
            cm.bw_gbs = bw_gbs;
            cm.lat_us = lat_us;
            cm.channels = channels;
            cm.lds_kib = lds_kib;
            cm.direct = direct;
            return std::shared_ptr<Comm>(new ShadowComm(p, cm));
          },
          py::arg("p"), py::arg("bw_gbs") = 0.0, py::arg("lat_us") = 0.0, py::arg("channels") = 16,
          py::arg("lds_kib") = 20, py::arg("direct") = false,
          "rank 0 of a p-rank job alone on one device (critical-path timing emulation); bw_gbs > 0 "
          "adds the communication-cost model (lat_us + bytes/bw on `channels` spin workgroups)");
  mod.def("shadow_reset", [](std::shared_ptr<Comm> c) {
    auto* sc = dynamic_cast<ShadowComm*>(c.get());
    GJ_REQUIRE(sc != nullptr, "shadow_reset: not a shadow communicator");
    sc->reset();
  });
  // One broadcast of `bytes` from `root` through a shadow communicator on the host (cost accounting
  // only: tests of the per-link model).
  mod.def("shadow_bcast_probe", [](std::shared_ptr<Comm> c, size_t bytes, int root) {
    auto* sc = dynamic_cast<ShadowComm*>(c.get());
    GJ_REQUIRE(sc != nullptr, "shadow_bcast_probe: not a shadow communicator");
    HostDevice dev(1);
    std::vector<char> buf(bytes);
    sc->bcast(dev, buf.data(), bytes, root, S_COMM);
  });
  mod.def("shadow_modelled_us", [](std::shared_ptr<Comm> c) {
    auto* sc = dynamic_cast<ShadowComm*>(c.get());
    GJ_REQUIRE(sc != nullptr, "shadow_modelled_us: not a shadow communicator");
    return sc->modelled_us();
  });
  // Two virtual ranks on the host enter collectives with different roots (rank 1 passes root_b):
  // returns the error message the loopback consistency check raised on each rank ("" = none).
  mod.def("loopback_mismatch_probe", [](int root_b) {
    auto hub = std::make_shared<LoopbackHub>(2);
    std::vector<std::string> msg(2);
    std::vector<std::thread> th;
    for (int r = 0; r < 2; ++r)
      th.emplace_back([&, r] {
        HostDevice dev(1);
        LoopbackComm c(hub, r);
        double buf[4] = {double(r), 0, 0, 0};
        try {
          c.bcast(dev, buf, sizeof(buf), r == 1 ? root_b : 0, S_COMM);
        } catch (const std::exception& e) {
          msg[r] = e.what();
        }
      });
    for (auto& t : th) t.join();
    return msg;
  });
  // len(values) virtual ranks on the host, each calling host_max with its own value on a
  // LoopbackComm (async_: AsyncLoopbackComm) group: returns what every rank got back.
  mod.def("loopback_host_max", [](std::vector<double> values, bool async_) {
    const int p = (int)values.size();
    if (p < 1) throw std::invalid_argument("loopback_host_max: no values");
    auto hub = std::make_shared<LoopbackHub>(p);
    std::vector<double> got(p, 0.0);
    std::vector<std::string> err(p);
    {
      py::gil_scoped_release rel;
      std::vector<std::thread> th;
      for (int r = 0; r < p; ++r)
        th.emplace_back([&, r] {
          HostDevice dev(1);
          try {
            if (async_) {
              AsyncLoopbackComm c(hub, r);
              got[r] = c.host_max(dev, values[r]);
            } else {
              LoopbackComm c(hub, r);
              got[r] = c.host_max(dev, values[r]);
            }
          } catch (const std::exception& e) {
            err[r] = e.what();
            hub->fail(err[r]);
          }
        });
      for (auto& t : th) t.join();
    }
    for (const auto& e : err)
      if (!e.empty()) throw std::runtime_error("loopback_host_max: " + e);
    return got;
  }, py::arg("values"), py::arg("async_") = false);
  // p virtual ranks on the host (LoopbackComm) invert a well-conditioned n x n matrix, then every rank
  // calls Engine::grad_matrix and Engine::vjp_inverse: returns each rank's pair of status codes (0 = the
  // call returned; both are single-rank operations and must refuse p > 1 with BadArgs).
  mod.def("loopback_grad_probe", [](int p, int64_t n, int64_t m) {
    if (p < 1 || n < 1) throw std::invalid_argument("loopback_grad_probe: p >= 1, n >= 1");
    auto hub = std::make_shared<LoopbackHub>(p);
    std::vector<std::pair<int, int>> got(p, {-1, -1});
    std::vector<std::string> err(p);
    {
      py::gil_scoped_release rel;
      std::vector<std::thread> th;
      for (int r = 0; r < p; ++r)
        th.emplace_back([&, r] {
          HostDevice dev(1);
          try {
            LoopbackComm c(hub, r);
            Engine eng(dev, c, n, m, SolveOptions());
            GenSpec g;
            g.kind = GenKind::RandomShifted;
            g.seed = 3;
            eng.generate(g);
            if (eng.solve().status != Status::Ok) throw std::runtime_error("the inversion failed");
            std::vector<double> G((size_t)(n * n), 0.0), O((size_t)(n * n), 0.0);
            auto status_of = [&](auto&& f) {
              try {
                f();
                return (int)Status::Ok;
              } catch (const Error& e) {
                return (int)e.status();
              }
            };
            got[r].first = status_of([&] { eng.grad_matrix(1.0, nullptr, 0, nullptr, 0, 0, 1.0, false, G.data(), n); });
            got[r].second = status_of([&] { eng.vjp_inverse(G.data(), n, O.data(), n); });
          } catch (const std::exception& e) {
            err[r] = e.what();
            hub->fail(err[r]);
          }
        });
      for (auto& t : th) t.join();
    }
    for (const auto& e : err)
      if (!e.empty()) throw std::runtime_error("loopback_grad_probe: " + e);
    return got;
  }, py::arg("p"), py::arg("n"), py::arg("m"));
  mod.attr("kHashParts") = (int)Device::kHashParts;
  mod.def("py_comm", [](py::object impl, int rank, int size) {
    return std::shared_ptr<Comm>(new PyComm(std::move(impl), rank, size));
  });

  // Engine keeps its device and communicator alive.
  struct PyEngine {
    std::shared_ptr<Device> dev;
    std::shared_ptr<Comm> comm;
    std::unique_ptr<Engine> eng;
  };
  py::class_<PyEngine>(mod, "Engine")
      .def(py::init([](std::shared_ptr<Device> dev, std::shared_ptr<Comm> comm, int64_t n, int64_t m,
                       const std::string& dtype, int64_t chunk_cols, double eps, bool sync_debug,
                       int depth, bool profile, double comm_timeout_s, const std::string& pivot,
                       double pivot_growth, bool track_det, bool equilibrate) {
             SolveOptions o;
             o.track_det = track_det;
             o.equilibrate = equilibrate;
             o.pivot_growth = pivot_growth;
             o.dtype = parse_dtype(dtype);
             o.depth = depth;
             o.pivot = parse_pivot(pivot);
             o.profile = profile;
             o.comm_timeout_s = comm_timeout_s;
             o.chunk_cols = chunk_cols;
             o.eps = eps;
             o.sync_debug = sync_debug;
             auto* pe = new PyEngine();
             pe->dev = dev;
             pe->comm = comm;
             pe->eng.reset(new Engine(*dev, *comm, n, m, o));
             return pe;
           }),
           py::arg("device"), py::arg("comm"), py::arg("n"), py::arg("m"), py::arg("dtype") = "fp64",
           py::arg("chunk_cols") = 0, py::arg("eps") = kDefaultEps, py::arg("sync_debug") = false,
           py::arg("depth") = 0, py::arg("profile") = false, py::arg("comm_timeout_s") = 600.0,
           py::arg("pivot") = "block-min-inv-norm", py::arg("pivot_growth") = -1.0,
           py::arg("track_det") = false, py::arg("equilibrate") = false)
      .def("equil_exponents",
           [](PyEngine& e) -> py::object {
             if (!e.eng->options().equilibrate) return py::none();
             const auto rc = e.eng->equil_exponents();
             const std::vector<int32_t>&r = rc.first, &c = rc.second;
             py::dict d;
             d["applied"] = e.eng->equil_applied();
             d["row_exp"] = py::array_t<int32_t>((py::ssize_t)r.size(), r.data());
             d["col_exp"] = py::array_t<int32_t>((py::ssize_t)c.size(), c.data());
             return d;
           },
           "the last solve's equilibration {applied, row_exp, col_exp} (int32 arrays, the same on every rank); "
           "None for an engine built without equilibrate=True")
      .def("slogdet",
           [](PyEngine& e) {
             DetResult dr;
             {
               py::gil_scoped_release rel;
               dr = e.eng->slogdet();
             }
             py::dict d;
             d["status"] = (int)dr.status;
             d["sign"] = dr.sign;
             d["logabsdet"] = dr.logabsdet;
             d["seconds"] = dr.seconds;
             return d;
           },
           "sign and log|det| of the matrix the result panel inverts (Engine::slogdet; collective): valid after a "
           "successful solve() of an engine built with track_det=True, else status 5 (BadArgs)")
      .def_property_readonly("layout",
                             [](PyEngine& e) {
                               const Layout& L = e.eng->layout();
                               py::dict d;
                               d["n"] = L.n; d["m"] = L.m; d["p"] = L.p; d["k"] = L.k;
                               d["Nr"] = L.Nr; d["npad"] = L.npad; d["nblk"] = L.nblk;
                               d["rows"] = L.rows; d["real_rows"] = e.eng->real_local_rows();
                               d["depth"] = e.eng->depth();
                               d["bcast"] = e.eng->bcast_algo();
                               return d;
                             })
      .def_property_readonly("policy",
                             [](PyEngine& e) {
                               py::dict d = policy_to_dict(e.eng->policy());
                               d["bcast"] = e.eng->bcast_algo();
                               d["bcast_tuning"] = e.comm->bcast_report();
                               d["comm"] = e.comm->describe();
                               return d;
                             })
      .def("generate",
           [](PyEngine& e, const std::string& kind, uint64_t seed) {
             GenSpec g;
             g.kind = parse_gen(kind);
             g.seed = seed;
             py::gil_scoped_release rel;
             e.eng->generate(g);
           },
           py::arg("kind") = "absdiff", py::arg("seed") = 0)
      .def("upload_local_rows",
           [](PyEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> a) {
             const int64_t real = e.eng->real_local_rows(), n = e.eng->layout().n;
             if (a.ndim() != 2 || a.shape(0) != real || a.shape(1) != n)
               throw std::invalid_argument("expected (real_rows, n) float64 array");
             const double* p = a.data();
             py::gil_scoped_release rel;
             e.eng->upload_local_rows(p, n);
           })
      .def("upload_rows_device",
           [](PyEngine& e, uintptr_t ptr, int64_t ld) {
             if (ld < e.eng->layout().n) throw std::invalid_argument("ld < n");
             py::gil_scoped_release rel;
             e.eng->upload_rows_device(reinterpret_cast<const void*>(ptr), ld);
           },
           py::arg("ptr"), py::arg("ld"))
      .def("download_rows_device",
           [](PyEngine& e, uintptr_t ptr, int64_t ld) {
             if (ld < e.eng->layout().n) throw std::invalid_argument("ld < n");
             py::gil_scoped_release rel;
             e.eng->download_rows_device(reinterpret_cast<void*>(ptr), ld);
           },
           py::arg("ptr"), py::arg("ld"))
      .def("solve_rhs_device",
           [](PyEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> b, uintptr_t rows,
              int64_t ld, int max_refine, double tol) {
             const int64_t n = e.eng->layout().n;
             if (b.ndim() != 1 || b.shape(0) != n) throw std::invalid_argument("b must be an n-vector");
             if (ld < n) throw std::invalid_argument("ld < n");
             max_refine = refine_budget(*e.eng, max_refine);
             py::array_t<double> x(n);
             RhsResult rr;
             {
               py::gil_scoped_release rel;
               rr = e.eng->solve_rhs_device(b.data(), x.mutable_data(), reinterpret_cast<const void*>(rows), ld,
                                            max_refine, tol);
             }
             return py::make_tuple(x, rhs_info(rr));
           },
           py::arg("b"), py::arg("rows_f64"), py::arg("ld"), py::arg("max_refine") = -1, py::arg("tol") = 1e-15,
           "A x = b after solve(): x = inv(A) b by the native GEMV, refined in fp64 against this rank's rows "
           "of A given as an fp64 device array (Engine::solve_rhs_device); returns (x, info)")
      .def("solve_rhs_block",
           [](PyEngine& e, py::object B, py::object gen, py::object rows, uintptr_t rows_f64, int64_t ld,
              uintptr_t b_dev, int64_t ldb, uintptr_t x_dev, int64_t ldx, int64_t ncols, int max_refine,
              double tol, bool trans, bool bounds, bool precise) {
             const int64_t n = e.eng->layout().n;
             if (trans && precise) throw std::invalid_argument("precise is not available with trans");
             max_refine = refine_budget(*e.eng, max_refine, precise);
             GenSpec g;
             const GenSpec* gp = nullptr;
             if (!gen.is_none()) {
               const py::tuple t = gen.cast<py::tuple>();
               g.kind = parse_gen(t[0].cast<std::string>());
               g.seed = t[1].cast<uint64_t>();
               gp = &g;
             }
             py::array_t<double, py::array::c_style | py::array::forcecast> hr;
             const double* hrp = nullptr;
             int64_t ldr = ld;
             if (!rows.is_none()) {
               hr = rows.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
               if (hr.ndim() != 2 || hr.shape(0) != e.eng->real_local_rows() || hr.shape(1) != n)
                 throw std::invalid_argument("rows must be (real_rows, n) float64");
               hrp = hr.data();
               ldr = n;
             } else if (rows_f64 && ld < n) {
               throw std::invalid_argument("ld < n");
             }
             RhsBlockResult br;
             py::object xo = py::none();
             if (b_dev) {  // B and X in device memory (fp64, n x ncols)
               if (!x_dev || ncols < 1 || ldb < ncols || ldx < ncols)
                 throw std::invalid_argument("device B / X: ncols >= 1, ldb >= ncols, ldx >= ncols");
               py::gil_scoped_release rel;
               br = e.eng->solve_rhs_block_device(reinterpret_cast<const double*>(b_dev), ldb,
                                                  reinterpret_cast<double*>(x_dev), ldx, ncols, gp, hrp,
                                                  reinterpret_cast<const void*>(rows_f64), ldr, max_refine, tol,
                                                  trans, bounds, precise);
             } else {
               auto b = B.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
               if (b.ndim() != 2 || b.shape(0) != n || b.shape(1) < 1)
                 throw std::invalid_argument("B must be an (n, k) array, k >= 1");
               const int64_t k = b.shape(1);
               py::array_t<double> x({n, k});
               {
                 py::gil_scoped_release rel;
                 br = e.eng->solve_rhs_block(b.data(), k, x.mutable_data(), k, k, gp, hrp,
                                             reinterpret_cast<const void*>(rows_f64), ldr, max_refine, tol, trans,
                                             bounds, precise);
               }
               xo = x;
             }
             py::list infos;
             for (const RhsResult& rc : br.col) infos.append(rhs_info(rc, bounds, precise));
             py::dict meta;
             meta["sweeps"] = br.sweeps;
             meta["seconds"] = br.seconds;
             return py::make_tuple(xo, infos, meta);
           },
           py::arg("B") = py::none(), py::arg("gen") = py::none(), py::arg("rows") = py::none(),
           py::arg("rows_f64") = 0, py::arg("ld") = 0, py::arg("b_dev") = 0, py::arg("ldb") = 0,
           py::arg("x_dev") = 0, py::arg("ldx") = 0, py::arg("ncols") = 0, py::arg("max_refine") = -1,
           py::arg("tol") = 1e-15, py::arg("trans") = false, py::arg("bounds") = false, py::arg("precise") = false,
           "A X = B (trans: A^T X = B) after solve() for a block of right-hand sides (Engine::solve_rhs_block): every "
           "column refined "
           "in fp64 against A given as gen=(kind, seed), rows (this rank's fp64 rows, host) or rows_f64 / ld (an "
           "fp64 device array).  B: an (n, k) host array -> returns (X, infos, meta); or b_dev / x_dev device "
           "pointers (fp64, n x ncols) -> X is written in place and returned as None.  bounds: every info also "
           "carries 'ferr' and 'berr' of the returned column (RhsResult).  precise: extra-precise refinement, the "
           "residual accumulated in twice the working precision and the columns stopped by the size of their "
           "correction (tol is not used); every info also carries 'dx_rel', 'dx_ratio' and 'err_est'; not with "
           "trans (ValueError)")
      .def("cond",
           [](PyEngine& e, py::object gen, py::object rows, uintptr_t rows_f64, int64_t ld) {
             const int64_t n = e.eng->layout().n;
             GenSpec g;
             const GenSpec* gp = nullptr;
             if (!gen.is_none()) {
               const py::tuple t = gen.cast<py::tuple>();
               g.kind = parse_gen(t[0].cast<std::string>());
               g.seed = t[1].cast<uint64_t>();
               gp = &g;
             }
             py::array_t<double, py::array::c_style | py::array::forcecast> hr;
             const double* hrp = nullptr;
             int64_t ldr = ld;
             if (!rows.is_none()) {
               hr = rows.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
               if (hr.ndim() != 2 || hr.shape(0) != e.eng->real_local_rows() || hr.shape(1) != n)
                 throw std::invalid_argument("rows must be (real_rows, n) float64");
               hrp = hr.data();
               ldr = n;
             } else if (rows_f64 && ld < n) {
               throw std::invalid_argument("ld < n");
             }
             CondResult c;
             {
               py::gil_scoped_release rel;
               c = e.eng->cond(gp, hrp, reinterpret_cast<const void*>(rows_f64), ldr);
             }
             py::dict o;
             o["a_norm1"] = c.a_norm1;
             o["a_norminf"] = c.a_norminf;
             o["inv_norm1"] = c.inv_norm1;
             o["inv_norminf"] = c.inv_norminf;
             return o;
           },
           py::arg("gen") = py::none(), py::arg("rows") = py::none(), py::arg("rows_f64") = 0, py::arg("ld") = 0,
           "the 1- and inf-norms of A (gen / rows / rows_f64 as in solve_rhs_block) and of the resident inverse "
           "(Engine::cond; collective)")
      .def("update_inverse",
           [](PyEngine& e, py::object Uo, py::object Vo, uintptr_t u_dev, int64_t ldu, uintptr_t v_dev, int64_t ldv,
              int64_t ncols) {
             const int64_t n = e.eng->layout().n;
             UpdateResult ur;
             if (u_dev || v_dev) {  // U and V in device memory (fp64, n x ncols)
               if (!u_dev || !v_dev || ncols < 1 || ldu < ncols || ldv < ncols)
                 throw std::invalid_argument("device U / V: both pointers, ncols >= 1, ldu >= ncols, ldv >= ncols");
               py::gil_scoped_release rel;
               ur = e.eng->update_inverse_device(reinterpret_cast<const double*>(u_dev), ldu,
                                                 reinterpret_cast<const double*>(v_dev), ldv, ncols);
             } else {
               auto u = Uo.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
               auto v = Vo.cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
               if (u.ndim() != 2 || u.shape(0) != n || u.shape(1) < 1 || v.ndim() != 2 || v.shape(0) != n ||
                   v.shape(1) != u.shape(1))
                 throw std::invalid_argument("U and V must be (n, k) arrays, k >= 1");
               const int64_t k = u.shape(1);
               py::gil_scoped_release rel;
               ur = e.eng->update_inverse(u.data(), k, v.data(), k, k);
             }
             py::dict info;
             info["status"] = (int)ur.status;
             info["k"] = ur.k;
             info["min_pivot"] = ur.min_pivot;
             info["cond1"] = ur.cond1;
             info["seconds"] = ur.seconds;
             info["sign_c"] = ur.sign_c;
             info["logabsdet_c"] = ur.logabsdet_c;
             return info;
           },
           py::arg("U") = py::none(), py::arg("V") = py::none(), py::arg("u_dev") = 0, py::arg("ldu") = 0,
           py::arg("v_dev") = 0, py::arg("ldv") = 0, py::arg("ncols") = 0,
           "inv(A) -> inv(A + U V^T) in the result panel (Engine::update_inverse; collective): U, V (n, k) host "
           "arrays, or u_dev / v_dev device pointers (fp64, n x ncols).  status 1 = refused as singular, nothing "
           "written.  Later solve_rhs* / residual_* calls must be given the rows of A + U V^T")
      .def("grad_matrix",
           [](PyEngine& e, double alpha, U W, int64_t ldw, U Z, int64_t ldz, int64_t ncols, double sign,
              bool accumulate, U G, int64_t ldg, bool device) {
             py::gil_scoped_release rel;
             if (device)
               e.eng->grad_matrix_device(alpha, (const double*)W, ldw, (const double*)Z, ldz, ncols, sign, accumulate,
                                         (double*)G, ldg);
             else
               e.eng->grad_matrix(alpha, (const double*)W, ldw, (const double*)Z, ldz, ncols, sign, accumulate,
                                  (double*)G, ldg);
           },
           py::arg("alpha"), py::arg("W") = 0, py::arg("ldw") = 0, py::arg("Z") = 0, py::arg("ldz") = 0,
           py::arg("ncols") = 0, py::arg("sign") = 1.0, py::arg("accumulate") = false, py::arg("G") = 0,
           py::arg("ldg") = 0, py::arg("device") = false,
           "G (+)= alpha * inv(A)^T + sign * W Z^T from the resident inverse (Engine::grad_matrix; one rank): G "
           "(n x n), W and Z (n x ncols, 0 <= ncols <= 64) are addresses of fp64 arrays with leading dimensions "
           "ldg, ldw, ldz -- host memory, or device memory with device=True")
      .def("vjp_inverse",
           [](PyEngine& e, U Gbar, int64_t ldg, U out, int64_t ldo, bool device) {
             py::gil_scoped_release rel;
             if (device)
               e.eng->vjp_inverse_device((const double*)Gbar, ldg, (double*)out, ldo);
             else
               e.eng->vjp_inverse((const double*)Gbar, ldg, (double*)out, ldo);
           },
           py::arg("Gbar"), py::arg("ldg"), py::arg("out"), py::arg("ldo"), py::arg("device") = false,
           "out = -inv(A)^T Gbar inv(A)^T, the vector-Jacobian product of A -> inv(A), from the resident inverse "
           "(Engine::vjp_inverse; one rank): addresses of fp64 n x n arrays in host memory, or in device memory "
           "with device=True; the products run in the engine dtype")
      .def("solve_rhs_rows",
           [](PyEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> b,
              py::array_t<double, py::array::c_style | py::array::forcecast> rows, int max_refine, double tol) {
             const int64_t n = e.eng->layout().n;
             if (b.ndim() != 1 || b.shape(0) != n) throw std::invalid_argument("b must be an n-vector");
             if (rows.ndim() != 2 || rows.shape(0) != e.eng->real_local_rows() || rows.shape(1) != n)
               throw std::invalid_argument("rows must be (real_rows, n) float64");
             max_refine = refine_budget(*e.eng, max_refine);
             py::array_t<double> x(n);
             RhsResult rr;
             {
               py::gil_scoped_release rel;
               rr = e.eng->solve_rhs(b.data(), x.mutable_data(), nullptr, rows.data(), n, max_refine, tol);
             }
             return py::make_tuple(x, rhs_info(rr));
           },
           py::arg("b"), py::arg("rows"), py::arg("max_refine") = -1, py::arg("tol") = 1e-15,
           "A x = b after solve(): x = inv(A) b, refined in fp64 against this rank's fp64 rows of A on the host "
           "(Engine::solve_rhs); returns (x, info)")
      .def("solve_rhs_generated",
           [](PyEngine& e, const std::string& kind, uint64_t seed,
              py::array_t<double, py::array::c_style | py::array::forcecast> b, int max_refine, double tol) {
             const int64_t n = e.eng->layout().n;
             if (b.ndim() != 1 || b.shape(0) != n) throw std::invalid_argument("b must be an n-vector");
             max_refine = refine_budget(*e.eng, max_refine);
             GenSpec g;
             g.kind = parse_gen(kind);
             g.seed = seed;
             py::array_t<double> x(n);
             RhsResult rr;
             {
               py::gil_scoped_release rel;
               rr = e.eng->solve_rhs(b.data(), x.mutable_data(), &g, nullptr, 0, max_refine, tol);
             }
             return py::make_tuple(x, rhs_info(rr));
           },
           py::arg("kind"), py::arg("seed"), py::arg("b"), py::arg("max_refine") = -1, py::arg("tol") = 1e-15,
           "A x = b after solve() of the generated matrix (kind, seed): x = inv(A) b, refined in fp64 against A "
           "regenerated in fp64 (Engine::solve_rhs); returns (x, info) -- BASELINE config 5 as a solve")
      .def("input_panel_ptr", [](PyEngine& e) { return (uintptr_t)e.eng->input_panel(); })
      .def("result_panel_ptr", [](PyEngine& e) { return (uintptr_t)e.eng->result_panel(); })
      .def("norm_inf", [](PyEngine& e) {
        py::gil_scoped_release rel;
        return e.eng->norm_inf();
      })
      .def("input_norm_inf", [](PyEngine& e) { return e.eng->input_norm_inf(); },
           "||A||_inf of the last solve's input")
      .def("result_norm_inf",
           [](PyEngine& e) {
             py::gil_scoped_release rel;
             return e.eng->result_norm_inf();
           },
           "||inv(A)||_inf of the last solve's result (collective)")
      .def("set_profile", [](PyEngine& e, bool on) { e.eng->set_profile(on); },
           "per-phase device timers for the following solves (between solves only)")
      .def("solve", [](PyEngine& e) {
        SolveStats st;
        {
          py::gil_scoped_release rel;
          st = e.eng->solve();
        }
        return stats_to_dict(st);
      })
      .def("download_local_rows", [](PyEngine& e) {
        const int64_t real = e.eng->real_local_rows(), n = e.eng->layout().n;
        py::array_t<double> a({real, n});
        double* p = a.mutable_data();
        {
          py::gil_scoped_release rel;
          e.eng->download_local_rows(p, n);
        }
        return a;
      })
      .def("corner", [](PyEngine& e, int nm, int which) {
        std::vector<double> c;
        {
          py::gil_scoped_release rel;
          c = e.eng->corner(nm, which);
        }
        return to_array(c, nm, nm);
      })
      .def("residual_generated",
           [](PyEngine& e, const std::string& kind, uint64_t seed) {
             GenSpec g;
             g.kind = parse_gen(kind);
             g.seed = seed;
             py::gil_scoped_release rel;
             return e.eng->residual_generated(g);
           },
           py::arg("kind") = "absdiff", py::arg("seed") = 0)
      .def("load_file",
           [](PyEngine& e, const std::string& path, int nthreads) {
             py::gil_scoped_release rel;
             return (int)e.eng->load_file(path, nthreads);
           },
           py::arg("path"), py::arg("nthreads") = 0,
           "collective: this rank's rows of a matrix file; returns 0, 3 (cannot open) or 4 (cannot read)")
      .def("residual_file",
           [](PyEngine& e, const std::string& path, int nthreads) {
             Status s = Status::Ok;
             double r;
             {
               py::gil_scoped_release rel;
               r = e.eng->residual_file(path, nthreads, &s);
             }
             return py::make_tuple((int)s, r);
           },
           py::arg("path"), py::arg("nthreads") = 0)
      .def("residual_rows", [](PyEngine& e, py::array_t<double, py::array::c_style | py::array::forcecast> a) {
        const int64_t real = e.eng->real_local_rows(), n = e.eng->layout().n;
        if (a.ndim() != 2 || a.shape(0) != real || a.shape(1) != n)
          throw std::invalid_argument("expected (real_rows, n) float64 array");
        const double* p = a.data();
        py::gil_scoped_release rel;
        return e.eng->residual_rows(p, n);
      });

  // geometry of the schedule checker (tests): regions as (base, pitch, width, height) in bytes
  auto region = [](py::tuple t) {
    MemRegion r;
    r.base = reinterpret_cast<const char*>((uintptr_t)t[0].cast<int64_t>());
    r.pitch = t[1].cast<int64_t>();
    r.width = t[2].cast<int64_t>();
    r.height = t[3].cast<int64_t>();
    return r;
  };
  mod.def("_regions_overlap", [region](py::tuple a, py::tuple b) { return regions_overlap(region(a), region(b)); });
  mod.def("_region_covers", [region](py::tuple a, py::tuple b) { return region_covers(region(a), region(b)); });

  mod.def("run_local", [](py::dict d) {
    RunConfig c;
    c.n = d["n"].cast<int64_t>();
    c.m = d["m"].cast<int64_t>();
    if (d.contains("ranks")) c.ranks = d["ranks"].cast<int>();
    if (d.contains("device")) c.gpu = d["device"].cast<std::string>() == "gpu";
    if (d.contains("comm")) c.comm = d["comm"].cast<std::string>();
    if (d.contains("jitter_us")) c.jitter_us = d["jitter_us"].cast<double>();
    if (d.contains("gen")) c.gen.kind = parse_gen(d["gen"].cast<std::string>());
    if (d.contains("seed")) c.gen.seed = d["seed"].cast<uint64_t>();
    if (d.contains("file")) c.file = d["file"].cast<std::string>();
    if (d.contains("dtype")) c.solve.dtype = parse_dtype(d["dtype"].cast<std::string>());
    if (d.contains("chunk_cols")) c.solve.chunk_cols = d["chunk_cols"].cast<int64_t>();
    if (d.contains("eps")) c.solve.eps = d["eps"].cast<double>();
    if (d.contains("sync_debug")) c.solve.sync_debug = d["sync_debug"].cast<bool>();
    if (d.contains("verify")) c.solve.verify = d["verify"].cast<bool>();
    if (d.contains("one_comm")) c.one_comm = d["one_comm"].cast<bool>();
    if (d.contains("depth")) c.solve.depth = d["depth"].cast<int>();
    if (d.contains("pivot")) c.solve.pivot = parse_pivot(d["pivot"].cast<std::string>());
    if (d.contains("pivot_growth")) c.solve.pivot_growth = d["pivot_growth"].cast<double>();
    if (d.contains("profile")) c.solve.profile = d["profile"].cast<bool>();
    if (d.contains("rhs")) c.rhs = d["rhs"].cast<std::string>();
    if (d.contains("nrhs")) c.nrhs = d["nrhs"].cast<int>();
    if (c.nrhs < 1) throw std::invalid_argument("nrhs must be >= 1");
    if (d.contains("trans")) c.trans = d["trans"].cast<bool>();
    if (d.contains("bounds")) c.bounds = d["bounds"].cast<bool>();
    if (d.contains("precise")) c.precise = d["precise"].cast<bool>();
    if (c.trans && c.precise) throw std::invalid_argument("precise is not available with trans");
    if (d.contains("cond")) c.cond = d["cond"].cast<bool>();
    if (d.contains("keep_solution")) c.keep_solution = d["keep_solution"].cast<bool>();
    if (d.contains("comm_timeout_s")) c.solve.comm_timeout_s = d["comm_timeout_s"].cast<double>();
    if (d.contains("residual")) {
      const std::string r = d["residual"].cast<std::string>();
      c.residual = r == "never" ? ResidualMode::Never : r == "compat" ? ResidualMode::Compat : ResidualMode::Always;
    }
    if (d.contains("print_max")) c.print_max = d["print_max"].cast<int>();
    if (d.contains("keep_inverse")) c.keep_inverse = d["keep_inverse"].cast<bool>();
    if (d.contains("host_threads")) c.host_threads = d["host_threads"].cast<int>();
    if (d.contains("repeats")) c.repeats = d["repeats"].cast<int>();
    if (d.contains("refine")) c.refine = d["refine"].cast<int>();
    if (d.contains("refine_tol")) c.refine_tol = d["refine_tol"].cast<double>();
    if (d.contains("race_check")) c.race_check = d["race_check"].cast<bool>();
    if (d.contains("det")) c.solve.track_det = d["det"].cast<bool>();
    if (d.contains("equilibrate")) c.solve.equilibrate = d["equilibrate"].cast<bool>();
    py::array_t<double, py::array::c_style | py::array::forcecast> inp;
    if (d.contains("input") && !d["input"].is_none()) {
      inp = d["input"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      if (inp.ndim() != 2 || inp.shape(0) != c.n || inp.shape(1) != c.n)
        throw std::invalid_argument("input must be (n, n)");
      c.input = inp.data();
    }
    py::array_t<double, py::array::c_style | py::array::forcecast> rhs_in;
    if (d.contains("rhs_input") && !d["rhs_input"].is_none()) {
      rhs_in = d["rhs_input"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      if (rhs_in.size() != c.n * c.nrhs) throw std::invalid_argument("rhs_input must have n * nrhs entries");
      c.rhs_input = rhs_in.data();
    }
    py::array_t<double, py::array::c_style | py::array::forcecast> upd_u, upd_v;
    if (d.contains("update_u") && !d["update_u"].is_none()) {
      upd_u = d["update_u"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      upd_v = d["update_v"].cast<py::array_t<double, py::array::c_style | py::array::forcecast>>();
      if (upd_u.ndim() != 2 || upd_u.shape(0) != c.n || upd_u.shape(1) < 1 || upd_u.shape(1) > Device::kMaxRhs ||
          upd_v.ndim() != 2 || upd_v.shape(0) != c.n || upd_v.shape(1) != upd_u.shape(1))
        throw std::invalid_argument("update_u / update_v must be (n, k) arrays, 1 <= k <= 64");
      c.update_u = upd_u.data();
      c.update_v = upd_v.data();
      c.update_k = upd_u.shape(1);
    }
    RunReport r;
    {
      py::gil_scoped_release rel;
      r = run_local(c);
    }
    py::dict o;
    o["status"] = (int)r.status;
    o["message"] = r.message;
    o["glob_time"] = r.glob_time;
    o["best_time"] = r.best_time;
    o["residual_computed"] = r.residual_computed;
    o["residual"] = r.residual;
    o["residual_fp64"] = r.residual_fp64;
    o["nm"] = r.nm;
    o["corner_a"] = to_array(r.corner_a, r.corner_a.empty() ? 0 : r.nm, r.corner_a.empty() ? 0 : r.nm);
    o["corner_inv"] = to_array(r.corner_inv, r.corner_inv.empty() ? 0 : r.nm, r.corner_inv.empty() ? 0 : r.nm);
    if (c.keep_inverse && r.status == Status::Ok) o["inverse"] = to_array(r.inverse, c.n, c.n);
    o["stats"] = stats_to_dict(r.stats);
    {
      py::list pr;
      for (const Engine::Policy& pl : r.policy_ranks) pr.append(policy_to_dict(pl));
      o["policy_ranks"] = pr;
    }
    o["device"] = r.device_desc;
    o["comm"] = r.comm_desc;
    o["gflops_nominal"] = r.gflops_nominal;
    if (c.race_check) {
      o["race_count"] = r.race_count;
      o["races"] = r.races;
      o["race_ops"] = r.race_ops;
    }
    if (r.updated) {
      py::dict u;
      u["k"] = r.update.k;
      u["min_pivot"] = r.update.min_pivot;
      u["cond1"] = r.update.cond1;
      u["seconds"] = r.update.seconds;
      o["update"] = u;
    }
    if (c.solve.equilibrate) o["equilibrate"] = equil_to_dict(r.stats.equil);
    if (r.det_computed) {
      o["slogdet"] = std::vector<double>{r.det.sign, r.det.logabsdet};
      o["slogdet_ranks"] = to_array(r.det_ranks, c.ranks, 2);
    }
    if (r.cond_computed) {
      py::dict cd;
      cd["one"] = r.cond.a_norm1 * r.cond.inv_norm1;
      cd["inf"] = r.cond.a_norminf * r.cond.inv_norminf;
      o["cond"] = cd;
    }
    if (r.rhs_solved) {
      o["axb_residual"] = r.rhs_residual;
      o["axb_seconds"] = r.rhs_seconds;
      o["axb_history"] = r.rhs_history;
      o["refine_steps"] = r.rhs_steps;
      o["refine_converged"] = r.rhs_converged;
      o["axb_backward_error"] = r.rhs_backward_error;
      o["x_head"] = r.x_head;
      if (c.keep_solution) o["x"] = to_array(r.x, c.n, r.nrhs);
      if (r.trans) o["trans"] = true;
      if (r.precise) o["precise"] = true;
      if (r.nrhs > 1 || r.trans || r.bounds || r.precise) {
        py::list cols;
        for (const RhsResult& rc : r.rhs_cols) cols.append(rhs_info(rc, r.bounds, r.precise));
        o["axb_columns"] = cols;
      }
    }
    return o;
  });

  mod.def("read_matrix_file", [](const std::string& path, int64_t n) {
    std::vector<double> v;
    Status s;
    {
      py::gil_scoped_release rel;
      s = read_matrix_file(path, n, v);
    }
    if (s == Status::CannotOpen) throw std::runtime_error("cannot open " + path);
    if (s == Status::CannotRead) throw std::runtime_error("cannot read " + path);
    return to_array(v, n, n);
  }, py::arg("path"), py::arg("n"));
  mod.def("read_matrix_rows", [](const std::string& path, int64_t n, std::vector<int64_t> rows, int nthreads) {
    std::vector<double> v;
    Status s;
    {
      py::gil_scoped_release rel;
      s = read_matrix_rows(path, n, rows, v, nthreads);
    }
    if (s == Status::CannotOpen) throw std::runtime_error("cannot open " + path);
    if (s == Status::CannotRead) throw std::runtime_error("cannot read " + path);
    return to_array(v, (int64_t)rows.size(), n);
  }, py::arg("path"), py::arg("n"), py::arg("rows"), py::arg("nthreads") = 0,
     "the given rows of an n x n matrix file (one rank's share), same accept set as read_matrix_file");
}
