// AsyncHostDevice — the host executor with REAL asynchronous streams (csrc/runtime/async_host_device.cpp).
//
// HostDevice runs every op before it returns, so a missing event dependency between the engine's
// MAIN / SIDE / COMM streams can never show on the CPU.  Here every stream role is a worker thread
// with an in-order queue (the ops run HostDevice's code), events are fences recorded into those
// queues, and `jitter_us` inserts random delays before queued ops so that the streams interleave
// differently on every run — the same hazards a GPU has, testable without one.
#pragma once

#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "gj/host_device.hpp"

namespace gj {

class AsyncHostDevice : public Device {
 public:
  // nthreads: threads of each op (HostDevice); jitter_us > 0: a random delay in [0, jitter_us)
  // before about one op in four on every stream; wait_timeout_s: a stream waiting longer than this
  // for an event fails (reported at the next synchronisation) instead of hanging.
  explicit AsyncHostDevice(int nthreads = 1, double jitter_us = 0.0, uint64_t seed = 0,
                           double wait_timeout_s = 120.0);
  ~AsyncHostDevice() override;
  bool on_gpu() const override { return false; }
  std::string describe() const override;

  void* alloc(size_t bytes) override { return inner_.alloc(bytes); }
  void release(void* p) override;
  void* alloc_pinned(size_t bytes) override { return inner_.alloc_pinned(bytes); }
  void release_pinned(void* p) override;
  size_t free_memory() const override { return inner_.free_memory(); }
  void memset0(void* p, size_t bytes, int s) override;
  void memset2d(void* p, size_t pitch, size_t width_bytes, size_t height, int s) override;
  void copy(void* dst, const void* src, size_t bytes, int s) override;
  void copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
              size_t height, int s) override;

  int create_event(bool timing = false) override;
  void record(int ev, int s) override;
  void wait(int s, int ev) override;
  void sync_event(int ev) override;
  bool query_event(int ev) override;
  void sync_stream(int s) override;
  void sync_all() override;
  float event_ms(int ev_start, int ev_end) override;
  void* native_stream(int) override { return nullptr; }
  std::shared_ptr<void> mark(int s) override;
  void wait_mark(int s, const std::shared_ptr<void>& h) override;
  void occupy(int s, int nwg, double us, int lds_bytes = 0) override;

  void generate(DType dt, void* X, const Layout& L, GenSpec g, int s) override;
  void widen(DType dt, double* dst, int64_t ldd, const void* X, int64_t ldx, int64_t rows, int64_t cols,
             int s) override;
  void upload_convert(DType dt, void* X, int64_t ldx, const double* src_dev, int64_t src_ld,
                      int64_t rows, int64_t cols, int s) override;
  void extract_neg_t(DType dt, void* Lt, int64_t ldl, const void* X, int64_t ldx, int64_t rows,
                     int64_t col0, int64_t m, int s) override;
  void add_diag(DType dt, void* A, int64_t ld, int64_t nd, double alpha, int s) override;
  void block_inverse(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                     int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                     int s) override;
  bool block_inverse_select(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                            int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                            const PivotSelectArgs& sel, int s) override;
  void candidate_maxabs(DType dt, const void* Lt, int64_t ldl, double* scores, int32_t* valid,
                        const int32_t* used, const Layout& L, double thresh, int s) override;
  void gather_candidate(DType dt, void* sel, const void* Lt, int64_t ldl, const PivotRec* rec, const Layout& L,
                        int s) override;
  void commit_candidate(DType dt, void* inv_t, const void* inv1, const int32_t* valid1, const double* score1, double growth, PivotRec* rec,
                        const Layout& L, int s) override;
  void pivot_local(const double* scores, const int32_t* valid, const int32_t* used,
                   const int32_t* pos, const Layout& L, PivotRec* out, int s) override;
  void pivot_global(const PivotRec* recs, int32_t p, int32_t t, int32_t* pos, int32_t* phys_at,
                    int32_t* used, int32_t* seq, PivotResult* out, PivotResult* host_out,
                    int s) override;
  void owner_edits(DType dt, void* At, int64_t ldl, const int32_t* phys, int64_t p, int64_t k, int64_t j,
                   int64_t m, void* lrow, void* ht, const void* inv, const PieceMove& mv, int s) override;
  void take_rows(DType dt, void* dst, int64_t ldd, void* X, int64_t ldx, const int32_t* phys, int64_t p, int64_t k,
                 int64_t col0, int64_t w, int64_t m, int s) override;
  void sum_slices(DType dt, void* dst, const void* src, int64_t count, int64_t nslices, int s) override;
  void zero_unless_owner(DType dt, void* buf, int64_t count, const int32_t* phys, int64_t p, int64_t k,
                         int s) override;
  void h_block(DType dt, void* R, int64_t ldr, const void* Ht, int64_t m, int s) override;
  void gemm(DType dt, GemmOp op, ALayout al, int64_t M, int64_t N, int64_t K, const void* A,
            int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int s,
            const GemmExtra& ex = GemmExtra()) override;
  void permute_blocks(DType dt, void* dst, int64_t ldd, const void* X, int64_t ldx, int64_t nblk,
                      int64_t m, int64_t Nr, const int32_t* dst_blk, const int32_t* colsrc,
                      int s) override;
  void row_abs_max_minus_i(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                           int s) override;
  void hash_rows(const void* base, int64_t ld_bytes, int64_t width_bytes, int64_t rows, uint64_t* parts,
                 int s) override;
  void row_abs_max(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                   int s) override;
  void residual(DType dt, const void* A, const void* Full, const Layout& L, double* out,
                int s) override;
  void panel_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                 const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign, const int32_t* active,
                 double* colmax, int s) override;
  void panel_rhs_dd(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                    const double* C_in, int64_t ldc, double* Y, int64_t ldy, const int32_t* active, double* colmax,
                    int s) override;
  void gather_rows_natural(double* dst, int64_t ldd, const double* src, int64_t lds, const Layout& L, int64_t k,
                           int s) override;
  void copy_cols_masked(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t k,
                        const int32_t* mask, int s) override;
  void panel_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                   double* S, int64_t lds, const int32_t* active, int s) override;
  void axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S, int64_t lds,
                        double sign, int64_t rows, int64_t k, const int32_t* active, double* colmax, int s) override;
  void col_abs_sum(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, int s) override;
  void panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                     const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax, int s) override;
  void panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                       double* S, int64_t lds, int s) override;
  void bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg, int64_t rows,
                   int64_t k, double nz_eps, double safe1, double safe2, double* berr, int s) override;
  void rank_update(DType dt, void* X, int64_t ldx, const Layout& L, const double* W, int64_t ldw, bool w_natural,
                   const double* Z, int64_t ldz, int64_t k, double sign, int s) override;
  void grad_matrix(DType dt, const void* P, int64_t ldp, int64_t n, double alpha, const double* W, int64_t ldw,
                   const double* Z, int64_t ldz, int64_t k, double sign, bool accumulate, double* G, int64_t ldg,
                   int s) override;
  void slogdet_batch(DType dt, const void* blocks, int64_t stride, int64_t m, int64_t nb, const int32_t* which,
                     double* sign, double* logabs, int s) override;
  void abs_max_rows(DType dt, const void* X, int64_t ldx, const Layout& L, double* out_nat, int s) override;
  void abs_max_cols(DType dt, const void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, double* out,
                    int s) override;
  void scale_pow2(DType dt, void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, const int32_t* cexp,
                  int s) override;
  void batch_pack(DType dt, const double* A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m, int64_t nb,
                  void* Lt, int64_t ldl, double* norm, int32_t* exp, int s) override;
  void batch_unpack(DType dt, const void* inv_t, int64_t n, int64_t m, int64_t nb, const int32_t* exp,
                    const int32_t* valid, void* X, int64_t stride_x, int64_t ldx, int s) override;
  void batch_rhs(DType dt, const void* M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb, const double* V,
                 int64_t stride_v, int64_t ldv, int64_t k, const double* C_in, int64_t stride_c, int64_t ldc,
                 double* Y, int64_t stride_y, int64_t ldy, double sign, const int32_t* active, double* colmax,
                 int s) override;

  // A fence between queues: signalled by the stream that records it, waited on by any stream
  // (of any AsyncHostDevice of this process) or by the host.
  struct Fence {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    double t_ms = 0.0;
    void signal();
    bool wait_for(double seconds);
  };

 private:
  struct Op {
    std::function<void()> f;
    bool signal = false;
  };
  struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Op> q;
    bool stop = false;
    std::mt19937_64 rng;
  };
  // signal = a fence / marker signal: still runs after a failure
  void enqueue(int s, std::function<void()> f, bool signal = false);
  void run(int s);
  void fail(std::exception_ptr e);
  void rethrow();
  void check_stream(int s) const;
  // pivot_global's work on the worker thread (the pinned host record's step field written last)
  void pivot_global_now(const PivotRec* recs, int32_t p, int32_t t, int32_t* pos, int32_t* phys_at, int32_t* used,
                        int32_t* seq, PivotResult* out, PivotResult* host_out, int s);

  HostDevice inner_;
  double jitter_us_, wait_timeout_s_;
  Worker w_[kNumStreams];
  std::mutex ev_mu_;
  std::vector<std::shared_ptr<Fence>> ev_last_;  // per event: the fence of its latest record
  std::mutex err_mu_;
  std::exception_ptr err_;
};

}  // namespace gj
