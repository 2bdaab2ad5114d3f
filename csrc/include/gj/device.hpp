// Device abstraction used by the solver engine.
//
// Two implementations exist:
//   * HipDevice  (csrc/runtime/hip_device.hip)  — the product path: hand-written gfx950 kernels,
//     three HIP streams (MAIN/SIDE/COMM) with priorities, event-based ordering.
//   * HostDevice (csrc/runtime/host_device.cpp) — a plain C++ reference executor with identical
//     semantics.  It is only ever selected explicitly (`--device cpu`, CPU tests, the reference's
//     "512x512 single rank on CPU" plumbing config); a GPU run never falls back to it.
//
// Every op takes a stream role (S_MAIN/S_SIDE/S_COMM); the host device executes synchronously.
#pragma once

#include <atomic>
#include <cmath>
#include <limits>
#include <map>
#include <memory>
#include <string>

#include "gj/common.hpp"
#include "gj/layout.hpp"
#include "gj/pivot.hpp"

namespace gj {

// Matrix generators (reference f / f_i, main.cpp:47-64, plus a seeded random dense generator for
// the synthetic benchmark system).
// RandomShifted: Random + sqrt(n) on the diagonal (well conditioned at any n: where fp32 solves
// and their refinement are meaningful, BASELINE.md "fp32").
enum class GenKind : int { AbsDiff = 0, Hilbert = 1, Identity = 2, Random = 3, Zero = 4, RandomShifted = 5 };

struct GenSpec {
  GenKind kind = GenKind::AbsDiff;
  uint64_t seed = 0;
};

// C (+)= A * B.  A is M x K and is stored either row-major (A[i*lda + k]) or "K-major"
// (At[k*lda + i], the layout the solver keeps its multiplier panel in).
enum class GemmOp : int { Acc = 0, Store = 1 };
enum class ALayout : int { RowMajor = 0, KMajor = 1 };

// Elimination extras of GemmOp::Acc: C enters as 0 in the columns [zc0, zc1) (the pivot block
// columns of the current panel) and in the row blocks [zr[i], zr[i] + zh) (its pivot rows).
struct GemmExtra {
  static constexpr int kMaxZeroRows = 8;  // = the deepest panel (SolveOptions::depth <= 8)
  int64_t zc0 = 0, zc1 = 0;
  int nzr = 0;
  int64_t zr[kMaxZeroRows] = {};
  int64_t zh = 0;
  // Few-tile GEMM on the panel-factorisation critical path: prefer small tiles (more workgroups,
  // shorter K loop per workgroup) over the throughput tiles of the trailing update.
  bool latency = false;
  // latency launch of >= 1024 rows: the LDS-DMA kernel (128 x 64 tiles, 4 per CU) instead of the
  // small tile -- the pivot chain's column updates when they run on reserved CUs (Engine::lat_wide_)
  bool lat_wide = false;
  // latency launch on CUs reserved for the chain: the register-fed small fp64 kernel (every operand
  // fragment loaded straight into registers, two 32-deep K chunks in flight; Engine::lat_reg_)
  bool lat_reg = false;
  // Also write the result transposed and negated, tneg[c*ldtneg + r] = -C[r][c], for the output
  // columns c < tneg_cols (0 = all): the K-major multiplier panel of the next pivot search, fused
  // into the column update that produces it (one launch fewer on the pivot chain).
  void* tneg = nullptr;
  int64_t ldtneg = 0;
  int64_t tneg_cols = 0;
  // Output columns [skip_c0, skip_c1) are neither read nor written (nor are those columns of B):
  // one launch for a chunk whose middle columns another stream updates (the trailing update around
  // the look-ahead columns).  GPU: whole tiles, so both bounds multiples of Device::skip_align().
  int64_t skip_c0 = 0, skip_c1 = 0;
  // Owner-predicated launch (the host-free pivot chain at p > 1): the GEMM does nothing unless this
  // rank owns the pivot g = *owner_phys (g % owner_p == owner_k) -- read on the device.
  const int32_t* owner_phys = nullptr;
  int64_t owner_p = 1, owner_k = 0;
  // Trailing-update residency: 5 LDS-DMA workgroups per CU instead of 4 (a 96-VGPR build).  Faster
  // when the pivot chain has CUs of its own (a CU reservation), slower when it must share them
  // (profiles/gemm_stall_r4.md).
  bool dense = false;
  // This launch's LDS-DMA build (stages * 10 + waves-per-SIMD bound: 23 | 25 | 33), 0 = by `dense`:
  // the owner's chunk-pass normalisations under a CU reservation (Engine::chunk_build_)
  int glds_build = 0;
  // This launch's LDS-DMA tile width (64 | 128), 0 = the device's hint (Device::set_gemm_tile_hint)
  int glds_tile = 0;
  // fp64 LDS-DMA kernel: C read (bit 0) / written (bit 1) with the non-temporal cache policy, for C
  // that nothing reads again soon (MAIN's trailing update: Engine::main_cnt_); -1 = GJ_GLDS_CNT / 0
  int c_nt = -1;
  // Row-block selection (the pivot-chain / deferred split of a panel's column updates, Engine):
  // only the row blocks b (height rsel_m, b < 64 kRselWords) whose bit b of rsel is set take part;
  // M counts the selected rows ((set bits) * rsel_m) and the i-th block of M is the i-th set bit.
  // Rows of A (K-major), C and tneg are addressed through the map; zero rows stay physical.
  // rsel_m = 0: off.  The GPU path needs the tile height to divide rsel_m (64 | rsel_m).
  // GemmOp::Acc reading its input from another array: C = C_in (+ masks) + A B, C_in with its own
  // leading dimension (the owner's pivot-row normalisation, X row -> temp, without a separate copy)
  const void* c_in = nullptr;
  int64_t ldc_in = 0;
  static constexpr int kRselWords = 8;
  uint64_t rsel[kRselWords] = {};
  int64_t rsel_m = 0;
  int64_t rsel_count() const {
    int64_t c = 0;
    for (int w = 0; w < kRselWords; ++w) c += __builtin_popcountll(rsel[w]);
    return c;
  }
  // physical row of selected row i (i < rsel_count() * rsel_m)
  int64_t rsel_row(int64_t i) const {
    int64_t bl = i / rsel_m;
    const int64_t off = i - bl * rsel_m;
    for (int w = 0; w < kRselWords; ++w) {
      uint64_t x = rsel[w];
      const int c = __builtin_popcountll(x);
      if (bl < c) {
        for (; bl > 0; --bl) x &= x - 1;
        return (64 * w + __builtin_ctzll(x)) * rsel_m + off;
      }
      bl -= c;
    }
    return -1;
  }
};

// Owner-side piece work fused into Device::owner_edits (all optional; w = 0 / eye = null: none):
// the pivot row's later panel columns moved out of X, dst[r*ldd + c] = X[(row0+r)*ldx + col0 + c],
// then zeroed in X (r < m, c < w; the next column updates need them as 0), and the m x m identity
// written at eye (ld ld_eye) -- the pivot's own block of the piece GEMM's B, so H_t lands in the
// piece without a separate copy (H I = H exactly).
struct PieceMove {
  void* dst = nullptr;
  int64_t ldd = 0;
  void* X = nullptr;
  int64_t ldx = 0;
  int64_t col0 = 0;
  int64_t w = 0;
  void* eye = nullptr;
  int64_t ld_eye = 0;
};

// Test probe: a short stable name of the kernel family (and build) that the calling thread's last
// Device::gemm / gemm_batch ran ("host" on the host executor, the HIP names in kernels/gemm.hip).
// Written at every launch site, read by nothing but tests: no effect on dispatch, no device work.
inline thread_local const char* g_last_gemm_kernel = "";
// Test probe: a census of those names over every thread of the process (name -> launches), for what a
// whole solve ran on each of its streams and ranks.  Off by default: a launch site then pays one
// relaxed load.  gemm_census_enable(true) clears the counts and starts counting, (false) stops and
// keeps them for gemm_census_counts().  (runtime/host_device.cpp)
extern std::atomic<bool> g_gemm_census_on;
void gemm_census_enable(bool on);
void gemm_census_add(const char* name);
std::map<std::string, int64_t> gemm_census_counts();
// every launch site names its kernel through this
inline void note_gemm_kernel(const char* name) {
  g_last_gemm_kernel = name;
  if (g_gemm_census_on.load(std::memory_order_relaxed)) gemm_census_add(name);
}

// One product of a batched small-GEMM launch (Device::gemm_batch): C (+)= A B, A K-major.
struct GemmDesc {
  GemmOp op = GemmOp::Acc;
  int64_t M = 0, N = 0, K = 0;
  const void* A = nullptr;
  int64_t lda = 0;
  const void* B = nullptr;
  int64_t ldb = 0;
  void* C = nullptr;
  int64_t ldc = 0;
  GemmExtra ex;
};

class Device {
 public:
  virtual ~Device() = default;
  virtual bool on_gpu() const = 0;
  virtual std::string describe() const = 0;
  virtual int device_index() const { return -1; }

  // ---- memory ----
  // release and release_pinned return only after everything enqueued on the device has completed
  // (hipFree and hipHostFree synchronise the device; the host executor is synchronous; the
  // asynchronous one drains its queues; the schedule checker models a host sync), so memory may be
  // released while work that uses it is still enqueued.  Owned through DevBuf (gj/buffer.hpp).
  virtual void* alloc(size_t bytes) = 0;
  virtual void release(void* p) = 0;
  virtual void* alloc_pinned(size_t bytes) = 0;
  // Fine-grained (coherent) pinned host memory: kernels store into it and the host polls it.
  virtual void* alloc_pinned_coherent(size_t bytes) { return alloc_pinned(bytes); }
  virtual void release_pinned(void* p) = 0;
  virtual size_t free_memory() const = 0;
  virtual void memset0(void* p, size_t bytes, int s) = 0;
  virtual void memset2d(void* p, size_t pitch, size_t width_bytes, size_t height, int s) = 0;
  virtual void copy(void* dst, const void* src, size_t bytes, int s) = 0;
  virtual void copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                      size_t height, int s) = 0;

  // ---- ordering ----
  virtual int create_event(bool timing = false) = 0;
  virtual void record(int ev, int s) = 0;
  virtual void wait(int s, int ev) = 0;
  virtual void sync_event(int ev) = 0;
  virtual bool query_event(int ev) = 0;  // true once all work before the record has completed
  virtual void sync_stream(int s) = 0;
  virtual void sync_all() = 0;
  // Non-blocking: true once everything enqueued on stream s has completed (Comm::drain polls it so
  // that a host wait behind a collective can notice a dead peer).  Synchronous devices: always true.
  virtual bool stream_idle(int s) { sync_stream(s); return true; }
  virtual float event_ms(int ev_start, int ev_end) = 0;
  virtual void* native_stream(int s) = 0;  // hipStream_t (nullptr on host)
  // Cross-device ordering points (the asynchronous virtual-rank transport, AsyncLoopbackComm):
  // mark(s) enqueues a marker on stream s and returns a handle that completes when everything
  // enqueued on s before it has; wait_mark(s, h) makes stream s wait for a handle from ANY device
  // of the same kind in this process (HIP: an event, so the same GPU or peer GPUs; host: a fence).
  // A null handle means "already complete".  Devices that execute synchronously return null.
  virtual std::shared_ptr<void> mark(int s) { (void)s; return nullptr; }
  virtual void wait_mark(int s, const std::shared_ptr<void>& h) { (void)s; (void)h; }
  // Timing / scheduling probes: keep stream s busy for `us` microseconds on `nwg` workgroups
  // (nwg = 1: a pure delay, e.g. per-rank start jitter; more: the CU footprint of a transfer in the
  // single-GPU communication-cost model of ShadowComm).  No-op where it has no meaning.
  virtual void occupy(int s, int nwg, double us, int lds_bytes = 0) {
    (void)s; (void)nwg; (void)us; (void)lds_bytes;
  }
  // Zero `bytes` at p on stream s with `nwg` workgroups of an RCCL channel's footprint (the data a
  // synthetic peer "sends" in ShadowComm's cost model, written with the CU footprint of the
  // receiving channel kernels rather than a full-chip fill kernel).  Default: memset0.
  virtual void zero_channels(void* p, size_t bytes, int s, int nwg, int lds_bytes) {
    (void)nwg; (void)lds_bytes;
    memset0(p, bytes, s);
  }
  // Keep the MAIN (trailing-update) stream off `n` CUs so the latency-critical SIDE/COMM kernels
  // always find idle CUs (the first n bits of the CU mask; n = 32 is one CU per shader engine).
  // Returns the number of CUs actually reserved.  Call while the device is idle.
  virtual int reserve_cus(int n) { (void)n; return 0; }
  // alignment (columns) of GemmExtra::skip_c0 / skip_c1 this device honours
  virtual int64_t skip_align() const { return 1; }

  // ---- schedule-checking hooks (RaceCheckDevice, gj/race_check.hpp; no-ops elsewhere) ----
  // Where the caller is (read at every op for reports): its step counter and phase name.
  virtual void trace_context(const int64_t* step, const char* const* phase) { (void)step; (void)phase; }
  // Name of an allocation in reports.
  virtual void label(const void* p, const char* name) { (void)p; (void)name; }
  // The host thread reads / writes host-visible memory directly (pinned staging, polled records).
  virtual void host_access(const void* p, size_t bytes, bool write) { (void)p; (void)bytes; (void)write; }
  // The host observed the record at p that a device op published (pivot_global's host_out): it
  // now knows everything that op was ordered after.
  virtual void host_acquire(const void* p, size_t bytes) { (void)p; (void)bytes; }
  // Host-thread ordering across devices (LoopbackComm's rendezvous): a handle of everything this
  // device's host has observed, and joining a peer's handle into it.
  virtual std::shared_ptr<void> host_mark() { return nullptr; }
  virtual void host_wait_mark(const std::shared_ptr<void>& h) { (void)h; }

  // ---- kernels ----
  // X (layout.rows x npad, ld npad) := A' restricted to this rank's block rows.
  virtual void generate(DType dt, void* X, const Layout& L, GenSpec g, int s) = 0;
  // generate() and out[0] = row_abs_max() of the result (a device may fuse the two passes; the
  // HIP device does, one read of the matrix less)
  virtual void generate_norm(DType dt, void* X, const Layout& L, GenSpec g, double* out, int s) {
    generate(dt, X, L, g, s);
    row_abs_max(dt, X, L.npad, L, out, s);
  }
  // X[r][c] := src[r][c] (doubles, ld src_ld) for r < rows, c < cols (dtype conversion).
  virtual void upload_convert(DType dt, void* X, int64_t ldx, const double* src_dev, int64_t src_ld,
                              int64_t rows, int64_t cols, int s) = 0;
  // dst[r*ldd + c] := (double)X[r*ldx + c] for r < rows, c < cols (X of dtype dt, device memory).
  virtual void widen(DType dt, double* dst, int64_t ldd, const void* X, int64_t ldx, int64_t rows,
                     int64_t cols, int s) = 0;
  // Lt[c*ldl + r] = -X[r*ldx + col0 + c]  for r < rows, c < m   (multiplier panel, K-major).
  virtual void extract_neg_t(DType dt, void* Lt, int64_t ldl, const void* X, int64_t ldx,
                             int64_t rows, int64_t col0, int64_t m, int s) = 0;
  // A[i*ld + i] += alpha, i < nd.
  virtual void add_diag(DType dt, void* A, int64_t ld, int64_t nd, double alpha, int s) = 0;
  // For every local block row b with used[global(b)] == 0: W = -(Lt block b)^T = X[b, col-block],
  // compute inv(W) by Gauss-Jordan with partial pivoting (reference inverse_block, main.cpp:746-820),
  // write it transposed to inv_t[b*m*m + j*m + i] = inv(W)[i][j], its inf-norm to scores[b]
  // (block_norm, main.cpp:669-683), and valid[b] (0 when singular: |pivot| < thresh).
  // A candidate that holds a NaN or an Inf entry, or whose sweep (in the block's own precision)
  // produces one, is invalid: valid[b] = 0, scores[b] = 0, inv_t of that block unspecified.  An Inf
  // or NaN pivot counts as singular, and the score's maximum keeps NaN, so that a NaN row sum cannot
  // hide behind the finite rows; the other candidates of the launch are unaffected.
  // nlive = the number of local blocks with used == 0 (the caller knows every earlier pivot):
  // devices launch one workgroup per LIVE candidate only, so no used block is dispatched (its
  // workgroup would hold a whole CU's LDS / wave slots for nothing); scores / valid of used blocks
  // are then left as they were (every consumer skips used blocks).  nlive < 0: all nblk.
  virtual void block_inverse(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                             int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                             int s) = 0;
  // block_inverse with the pivot selection run by the launch's last workgroup (PivotSelectArgs:
  // p > 1 the local argmin -> *sel.rec, like pivot_local; p == 1 the whole pivot_select_single).
  // Returns false, having enqueued nothing, where the device or the kernel family it would use
  // cannot fuse them; the caller then runs block_inverse and the selection as separate launches.
  virtual bool block_inverse_select(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                                    int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                                    const PivotSelectArgs& sel, int s) {
    (void)dt; (void)Lt; (void)ldl; (void)inv_t; (void)scores; (void)valid; (void)used; (void)L;
    (void)thresh; (void)sel; (void)s;
    return false;
  }
  // Kernel family for the following block_inverse calls (-1 = the process default; 5 = the
  // co-resident form, which the engine picks where its pivot chain waits for whole CUs).  Devices
  // with a single implementation ignore it.
  virtual void set_block_inverse_hint(int variant) { (void)variant; }
  // Tile width of the fp64 LDS-DMA trailing-update kernel for launches that do not name one
  // (GemmExtra::glds_tile): 128 by default, 64 where CUs are reserved for the pivot chain (Engine)
  virtual void set_gemm_tile_hint(int bn) { (void)bn; }
  // Device scratch the candidate-inverse kernel family `variant` needs for layout L (bytes), and
  // its allocation ahead of the first block_inverse call.
  virtual size_t block_inverse_scratch_bytes(DType dt, const Layout& L, int variant) const {
    (void)dt; (void)L; (void)variant;
    return 0;
  }
  virtual void prepare_block_inverse(DType dt, const Layout& L, int variant) { (void)dt; (void)L; (void)variant; }
  // Partial pivoting (SolveOptions::pivot = Partial, `--pivot partial`).  Every local candidate
  // W_b (as in block_inverse) gets scores[b] = -max|W_b| and valid[b] = (max|W_b| >= thresh), so the
  // common argmin (pivot_local) picks this rank's largest-magnitude candidate (a used block: valid
  // 0, score 0; a block with an Inf or a NaN entry is invalid -- the maximum keeps NaN, so one NaN
  // entry cannot hide behind the finite ones); its block alone is
  // then copied out (gather_candidate: sel = K-major m x m, ld m; -I for an invalid record),
  // inverted by block_inverse on a one-block layout, and commit_candidate stores that inverse in
  // the candidate's slot of inv_t and clears rec->valid when the block is singular or, growth > 0,
  // when its growth estimate ||inv||_inf * max|W| (score1[0] * -rec->score) exceeds growth.
  virtual void candidate_maxabs(DType dt, const void* Lt, int64_t ldl, double* scores, int32_t* valid,
                                const int32_t* used, const Layout& L, double thresh, int s) = 0;
  virtual void gather_candidate(DType dt, void* sel, const void* Lt, int64_t ldl, const PivotRec* rec,
                                const Layout& L, int s) = 0;
  virtual void commit_candidate(DType dt, void* inv_t, const void* inv1, const int32_t* valid1, const double* score1, double growth, PivotRec* rec,
                                const Layout& L, int s) = 0;
  // Local argmin over this rank's candidates -> *out.
  virtual void pivot_local(const double* scores, const int32_t* valid, const int32_t* used,
                           const int32_t* pos, const Layout& L, PivotRec* out, int s) = 0;
  // Global selection over p records + book-keeping (pivot_commit) -> *out, and the same record to
  // host_out (pinned host memory the host polls: its `step` field is written last, after a
  // system-scope fence) when host_out != nullptr.
  virtual void pivot_global(const PivotRec* recs, int32_t p, int32_t t, int32_t* pos,
                            int32_t* phys_at, int32_t* used, int32_t* seq, PivotResult* out,
                            PivotResult* host_out, int s) = 0;
  // One rank (p == 1): pivot_local + pivot_global as one launch (the record all-gather is skipped
  // there, so the two were back to back on the pivot chain).  Default: the two calls.
  virtual void pivot_select_single(const double* scores, const int32_t* valid, const Layout& L,
                                   int32_t t, int32_t* pos, int32_t* phys_at, int32_t* used,
                                   int32_t* seq, PivotRec* rec, PivotResult* out,
                                   PivotResult* host_out, int s) {
    pivot_local(scores, valid, used, pos, L, rec, s);
    pivot_global(rec, 1, t, pos, phys_at, used, seq, out, host_out, s);
  }
  // Owner-side edits of a pivot step, fused (one launch).  The pivot is read on the device: g =
  // *phys (the step's entry of the pivot sequence, written by the selection), and the launch does
  // nothing unless g % p == k (this rank owns it), so the host can enqueue it before it has seen
  // the pivot.  For the pivot's local block row b = g / p (rows row0 = b m .. of the K-major
  // multiplier panel At, ld ldl): save the multipliers of the panel's earlier steps,
  // lrow[kk*m + c] = At[kk*ldl + row0 + c] for kk < j*m, set those rows of At to [0 .. 0 | I] over
  // the first (j+1)*m K-rows (identity in segment j), and copy the block's inverse:
  // ht[e] = inv[b*m*m + e], e < m*m.
  // mv: the PieceMove work of the same pivot, in the same launch.
  virtual void owner_edits(DType dt, void* At, int64_t ldl, const int32_t* phys, int64_t p, int64_t k,
                           int64_t j, int64_t m, void* lrow, void* ht, const void* inv, const PieceMove& mv,
                           int s) = 0;
  // Take the pivot row's piece (device-addressed like owner_edits): for g = *phys owned here (else
  // nothing), local rows row0 = (g / p) m .. + m:  dst[r*ldd + c] = X[(row0 + r)*ldx + col0 + c],
  // then X[row0 + r][col0 + c] = 0, for r < m, c < w.  The panel's later columns of a pivot row
  // enter the next column updates as 0 (the sweep's zero-row rule) without a zero-row mask.
  virtual void take_rows(DType dt, void* dst, int64_t ldd, void* X, int64_t ldx, const int32_t* phys, int64_t p,
                         int64_t k, int64_t col0, int64_t w, int64_t m, int s) = 0;
  // dst[i] = sum over q < nslices of src[q*count + i], in q order (identical on every rank).
  virtual void sum_slices(DType dt, void* dst, const void* src, int64_t count, int64_t nslices, int s) = 0;
  // buf[0 .. count) = 0 unless this rank owns the pivot g = *phys (g % p == k): the non-owners'
  // share of a root-agnostic exchange (an all-reduce sum carries the owner's values).
  virtual void zero_unless_owner(DType dt, void* buf, int64_t count, const int32_t* phys, int64_t p, int64_t k,
                                 int s) = 0;
  // R[i*ldr + j] = Ht[j*m + i] for i, j < m: the pivot block's inverse (kept transposed, ld m)
  // written row-major into a panel of leading dimension ldr.
  virtual void h_block(DType dt, void* R, int64_t ldr, const void* Ht, int64_t m, int s) = 0;
  // C (+)= A B with the GemmExtra contract above.  Non-finite operands, the same on every executor:
  // a NaN or an Inf of A or B inside the product's range (rows of the product, k < K, columns that
  // are not skipped) reaches every element of C whose sum it is a term of, also where its factor is
  // 0 (0 * NaN = 0 * Inf = NaN: no executor skips zero multipliers).  What a mask hides is not read
  // at all: C in its zero columns / zero row blocks, C_in likewise, the skipped columns of C and B,
  // rows k >= K and everything outside the M x N x K range, so a NaN there never shows.
  // A leading dimension whose rows one tile of the chosen kernel cannot address with 32-bit byte
  // offsets is refused with Status::BadArgs (GPU), never computed wrongly.
  virtual void gemm(DType dt, GemmOp op, ALayout al, int64_t M, int64_t N, int64_t K, const void* A,
                    int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int s,
                    const GemmExtra& ex = GemmExtra()) = 0;
  // Independent small K-major GEMMs (the panel-piece products of one pivot step) as one launch
  // where the device can; the default issues them one by one.
  virtual void gemm_batch(DType dt, const GemmDesc* d, int n, int s) {
    for (int i = 0; i < n; ++i) {
      GemmExtra ex = d[i].ex;
      ex.latency = true;
      gemm(dt, d[i].op, ALayout::KMajor, d[i].M, d[i].N, d[i].K, d[i].A, d[i].lda, d[i].B, d[i].ldb,
           d[i].C, d[i].ldc, s, ex);
    }
  }
  // Finalisation gather: dst[(dst_blk[b]*m + r)*ldd + c*m + j] = X[(b*m + r)*ldx + colsrc[c]*m + j]
  // for local block b < nblk, destination column block c < Nr.
  virtual void permute_blocks(DType dt, void* dst, int64_t ldd, const void* X, int64_t ldx,
                              int64_t nblk, int64_t m, int64_t Nr, const int32_t* dst_blk,
                              const int32_t* colsrc, int s) = 0;
  // Consumption-point verification (GJ_VERIFY, Engine): a position-dependent 64-bit hash of the
  // bytes [r*ld_bytes, r*ld_bytes + width_bytes) of rows r < rows at `base` (width a multiple of 4),
  // as kHashParts partial sums that add (mod 2^64) to the hash of those bytes (gen.hpp hash_term) --
  // enqueued on the stream that consumes the buffer, right before its consumer, so it sees what the
  // consumer saw.
  static constexpr int kHashParts = 64;
  virtual void hash_rows(const void* base, int64_t ld_bytes, int64_t width_bytes, int64_t rows,
                         uint64_t* parts, int s) = 0;
  // Non-finite values propagate through the three norms below: the maximum keeps NaN (a NaN row sum
  // gives out[0] = NaN whatever the other rows hold, where fmax / std::max would drop it) and an Inf
  // row sum gives +Inf, so that every gate that tests isfinite(residual) sees a broken inverse.
  // Padding (global rows >= n, columns >= n, the pitch gap) is never read into a sum.
  //
  // out[0] = max over local real rows of sum_{j<n} |X[r][j]|  (reference norm(), main.cpp:643-667).
  virtual void row_abs_max(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                           int s) = 0;
  // out[0] = max over local real rows r of sum_{j<n} |X[r][j] - delta(global(r), j)|
  virtual void row_abs_max_minus_i(DType dt, const void* X, int64_t ldx, const Layout& L, double* out,
                                   int s) = 0;
  // out[0] = max over local real rows r of sum_{j<n} |(A_loc * Full)[r][j] - delta(global(r), j)|
  // (matrix_mult_matrix + minus_i + norm, main.cpp:534-667, fused).  A_loc row-major ld npad,
  // Full = the whole inverse in natural row order (npad x npad).
  // The product's inner sum runs over k < n on the host and over k < npad on the GPU: the two agree
  // for the padded system the engine keeps, diag(A, I) and its inverse, i.e. whenever Full's rows
  // >= n are 0 in the columns < n (or A's real rows are 0 in the columns >= n).  A's padding rows
  // and Full's columns >= n never count.  NaN / Inf propagate as above, with one exception on the
  // host, which skips the zero entries of A: a non-finite Full entry whose whole column of A_loc
  // is 0 need not show there.
  virtual void residual(DType dt, const void* A, const void* Full, const Layout& L, double* out,
                        int s) = 0;

  // ---- a block of right-hand sides (Engine::solve_rhs_block) ----
  // Y = C_in + sign * P V for 1 <= k <= kMaxRhs columns (else Status::BadArgs).
  //   P     this rank's rows of a panel, L.rows x L.npad of dtype dt, leading dimension ldp
  //   V     the whole block in natural row order, fp64, k columns, leading dimension ldv
  //   C_in  fp64, L.rows x k, leading dimension ldc; null = 0; may alias Y
  //   Y     fp64, L.rows x k, leading dimension ldy
  //   sign  +1 or -1
  //   active  int32[k] (device) or null: a column with active[j] == 0 is neither computed nor written
  //   colmax  double[k] (device) or null: colmax[j] = max |Y[r][j]| over this rank's real rows
  //           (global row < n), NaN kept as in row_abs_max; left untouched for an inactive column
  // F64: fp64 throughout.  F32: V rounded to fp32 on load, the product accumulated in fp32, widened,
  // then added to C_in in fp64.  The inner sum runs over the columns c < L.n.  Padding columns of P,
  // the rows >= n of V and the pitch gap of every operand are never read (the norms' rule above);
  // the padded local rows of Y are written as C_in (or 0).
  static constexpr int kMaxRhs = 64;
  virtual void panel_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                         int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign,
                         const int32_t* active, double* colmax, int s) = 0;
  // The residual in twice the working precision (Engine::solve_rhs_block with precise):
  // Y = round_fp64(C_in - P V), the whole sum, C_in included, carried as an unevaluated (hi, lo) pair
  // of doubles and rounded once.  Operands, active and colmax as in panel_rhs, with these differences:
  // P is fp64 (any other dt is Status::BadArgs) and there is no sign.  Dot2 (Ogita, Rump, Oishi): per
  // term p = a v, e = fma(a, v, -p), (s, sigma) = TwoSum(s, p), lo += e + sigma; C_in enters the pair
  // exactly; partial sums (the GPU's K lanes and K-slices) are pairs added in a fixed order by
  // double-double additions.  With S = |C_in| + |P| |V| the result obeys, componentwise,
  //   |Y - (C_in - P V)| <= u |C_in - P V| + 4 ((n + 2) u)^2 S,   u = 2^-53.
  // Never read: what panel_rhs never reads; the padded local rows of Y are written as C_in (or 0); an
  // inactive column is neither computed nor written and its colmax is untouched.  A NaN of V reaches Y
  // also through a zero of P.  No floating-point atomics: two launches on the same inputs give the
  // same bits.  The executors need not agree to the bit with each other.
  virtual void panel_rhs_dd(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                            int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy,
                            const int32_t* active, double* colmax, int s) = 0;
  // dst[g*ldd + j] = src[(q*max_nblk*m + b*m + e)*lds + j] for the global rows g = (b*p + q)*m + e < n
  // and j < k: the rank-major rows Comm::allgather delivers (max_nblk*m rows per rank) into natural
  // row order.  Rows >= n of dst are not written.
  virtual void gather_rows_natural(double* dst, int64_t ldd, const double* src, int64_t lds, const Layout& L,
                                   int64_t k, int s) = 0;
  // dst[r*ldd + j] = src[r*lds + j] for r < rows and the columns j < k with mask[j] != 0 (int32[k], device)
  virtual void copy_cols_masked(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows,
                                int64_t k, const int32_t* mask, int s) = 0;

  // ---- the transposed block solve (Engine::solve_rhs_block with trans) ----
  // S[c][j] = sum_r P[r][c] * V[grow(r)][j] for c < L.n and j < k, 1 <= k <= kMaxRhs columns (else
  // Status::BadArgs): this rank's term of P_full^T V.  The sum runs over this rank's local rows r
  // whose global row grow(r) = ((r / m) * p + rank) * m + r % m is below n.
  //   P     this rank's rows of a panel, L.rows x L.npad of dtype dt, leading dimension ldp
  //   V     the whole block in natural row order, fp64, k columns, leading dimension ldv; only the
  //         rows this rank owns are read
  //   S     fp64 in natural order, L.n x k, leading dimension lds; rows >= n are not written
  //   active  int32[k] (device) or null: a column with active[j] == 0 is not computed, S gets +0.0
  //           there (so the sum over the ranks stays defined)
  // F64: fp64 throughout.  F32: V rounded to fp32 on load, the product accumulated in fp32, partial
  // sums widened and added in fp64 (the arithmetic of panel_rhs).  Never read: P's padding rows, P's
  // columns >= n, V's rows >= n, V's rows owned by other ranks and the pitch gap of every operand.
  virtual void panel_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                           int64_t k, double* S, int64_t lds, const int32_t* active, int s) = 0;
  // Y[r][j] = C_in[r][j] + sign * S[r][j] for r < rows and the columns j < k (1 <= k <= kMaxRhs) with
  // active[j] != 0 (int32[k], device; null = all), fp64, sign = +1 or -1.  C_in may be null (0) or
  // alias Y.  colmax (double[k], device, or null): colmax[j] = max |Y[r][j]| over r < rows, NaN kept
  // as in panel_rhs.  Y and colmax[j] of an inactive column stay untouched.
  virtual void axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S,
                                int64_t lds, double sign, int64_t rows, int64_t k, const int32_t* active,
                                double* colmax, int s) = 0;
  // out[c] = sum over this rank's real local rows (global row < n) of |X[r][c]| for c < L.n: this
  // rank's term of the column sums (||A||_1 after a sum over the ranks).  X is L.rows x L.npad of
  // dtype dt, leading dimension ldx; accumulated in fp64, NaN kept; padding never read.
  virtual void col_abs_sum(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, int s) = 0;

  // ---- error bounds of a refined solve (Engine::solve_rhs_block with bounds) ----
  // The two products of panel_rhs / panel_rhs_t on absolute values, 1 <= k <= kMaxRhs columns (else
  // Status::BadArgs), with their operands laid out as there.
  // Both dtypes: fp64 throughout -- an fp32 element of P is widened exactly, V is not rounded, the
  // products and their sum are fp64.  (The bounds' right-hand side is about u (|A| |x| + |b|), which
  // leaves fp32's range for a small b.)  Every term is non-negative, so the result carries a relative
  // error of at most gamma(terms + 2) in fp64 units.  A NaN or an Inf of P or V reaches every element
  // it is a term of, also through a zero factor.  No floating-point atomics: the K / row split is
  // summed in a fixed order, two launches on the same inputs give the same bits.
  // GPU: a leading dimension ldp whose rows one tile cannot address with 32-bit byte offsets is
  // refused with Status::BadArgs.
  //
  // Y[r][j] = |C_in[r][j]| + sum_{c<n} |P[r][c]| * |V[c][j]| for this rank's real local rows; the padded
  // local rows of Y are written as |C_in| (or 0).  C_in: null = 0; may alias Y.  colmax (double[k],
  // device, or null): colmax[j] = max |Y[r][j]| over the real rows, NaN kept.  Never read: what
  // panel_rhs never reads (P's padding rows, its columns >= n, V's rows >= n, every pitch gap).
  virtual void panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                             int64_t k, const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax,
                             int s) = 0;
  // S[c][j] = sum_r |P[r][c]| * |V[grow(r)][j]| for c < L.n over this rank's real local rows: its term
  // of |P_full|^T |V|, in natural order.  Rows >= n of S are not written.  Never read: what panel_rhs_t
  // never reads (P's padding rows, its columns >= n, V's rows >= n and those of other ranks, every
  // pitch gap).
  virtual void panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv,
                               int64_t k, double* S, int64_t lds, int s) = 0;
  // The elementwise step of LAPACK's xGERFS over rows x k fp64 elements, 1 <= k <= kMaxRhs (else
  // Status::BadArgs): with R a residual and D = |A| |x| + |b| >= 0,
  //   G[r][j]  = |R[r][j]| + nz_eps * D[r][j] (one fused multiply-add), plus safe1 where D[r][j] <= safe2
  //   berr[j]  = max_r |R[r][j]| / D[r][j], with (|R| + safe1) / (D + safe1) where D[r][j] <= safe2
  // the maximum with NaN kept as in row_abs_max.  berr (double[k], device) is written, not
  // accumulated: +0.0 for rows == 0.  G may alias R.
  virtual void bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg,
                           int64_t rows, int64_t k, double nz_eps, double safe1, double safe2, double* berr,
                           int s) = 0;

  // ---- the low-rank update of a resident panel (Engine::update_inverse) ----
  // X[r][c] = round_dt(X[r][c] + sign * sum_{j<k} W[wrow(r)][j] * Z[c][j]) for this rank's local rows r
  // whose global row grow(r) = ((r / m) * p + rank) * m + r % m is below L.n, and the columns c < L.n;
  // 1 <= k <= kMaxRhs (else Status::BadArgs).
  //   X     this rank's rows of a panel, L.rows x L.npad of dtype dt, leading dimension ldx, in place
  //   W     fp64, k columns, leading dimension ldw.  w_natural = false: local row order, wrow(r) = r
  //         (what panel_rhs writes); w_natural = true: n x k in natural order, wrow(r) = grow(r) (a
  //         kept copy of A's rows takes A_loc += U_loc V^T without a gather)
  //   Z     fp64, n x k in natural row order, leading dimension ldz
  //   sign  +1 or -1
  // Both dtypes: the k products and their sum in fp64, the panel element widened, the sum added, the
  // result rounded once to dt.  Never read or written: X's rows with global row >= n, X's columns
  // >= n and every pitch gap, so the padding identity of diag(A, I) survives bit for bit.  Never
  // read: W's rows of padded local rows (and, w_natural, of other ranks), Z's rows >= n.  A NaN or an
  // Inf of W or Z reaches every element it is a term of, also through a zero factor (the rule of
  // gemm).  No atomics and no split of the k sum: two launches on the same inputs give the same bits.
  // GPU: a leading dimension ldx whose rows one tile cannot address with 32-bit byte offsets is
  // refused with Status::BadArgs.
  virtual void rank_update(DType dt, void* X, int64_t ldx, const Layout& L, const double* W, int64_t ldw,
                           bool w_natural, const double* Z, int64_t ldz, int64_t k, double sign, int s) = 0;

  // ---- the gradient matrix of a resident inverse (Engine::grad_matrix, Engine::vjp_inverse) ----
  // G[i][j] = (accumulate ? G[i][j] : 0) + alpha * (double)P[j][i] + sign * sum_{c<k} W[i][c] * Z[j][c]
  // for i < n and j < n; 0 <= k <= kMaxRhs, and k > kMaxRhs, k < 0 or n < 0 is Status::BadArgs.
  //   P     n x n of dtype dt, leading dimension ldp, rows in natural order: the resident result panel
  //         at p = 1, or a work buffer of the same dtype.  It enters transposed.
  //   G     fp64, n x n, leading dimension ldg
  //   W, Z  fp64, n x k in natural row order, leading dimensions ldw, ldz
  //   sign  +1 or -1; alpha any double
  // alpha == 0: P is never read and may be null, so a NaN in P does not reach G.  k == 0: W and Z are
  // never read and may be null.  alpha == 0 && k == 0 && !accumulate writes +0.0.
  // Both dtypes work in fp64: an fp32 element of P is widened exactly, the k products and their sum
  // are fp64, the sum is added to alpha * P (one rounding for the product, one for the addition) and
  // that to G when accumulating (one more); nothing is rounded to dt.
  // Never read: P's rows and columns >= n, W's and Z's rows >= n and columns >= k, every pitch gap,
  // and G unless accumulating.  Never written: anything of G outside n x n.  A NaN or an Inf of W or
  // Z reaches every element it is a term of, also through a zero factor (the rule of gemm and
  // rank_update).  No atomics and no split of the k sum: two launches on the same inputs give the same
  // bits.  The executors need not agree to the bit with each other.
  // GPU: a leading dimension ldg or ldp whose rows one tile cannot address with 32-bit byte offsets is
  // refused with Status::BadArgs.
  virtual void grad_matrix(DType dt, const void* P, int64_t ldp, int64_t n, double alpha, const double* W,
                           int64_t ldw, const double* Z, int64_t ldz, int64_t k, double sign, bool accumulate,
                           double* G, int64_t ldg, int s) = 0;

  // ---- determinants of small blocks (Engine::slogdet over the stashed pivot-block inverses) ----
  // For b < nb: (sign[b], logabs[b]) = slogdet of the m x m block at blocks + b*stride (dtype dt, ld m).
  // Worked in fp64 whatever dt is (an fp32 block is widened exactly).  LU with partial pivoting:
  // sign = (-1)^swaps * prod sgn(pivot), logabs = sum log|pivot|, both as double.
  // A NaN or Inf in the block gives sign = logabs = NaN, wherever it stands (every entry is looked at
  // before the first column); so does a pivot that overflows on the way.
  // Otherwise an exactly zero pivot gives sign 0, logabs -inf (numpy's convention).
  // The input is not written.
  // which (int32[nb], device, or null): blocks with which[b] == 0 are skipped and their outputs are left
  // untouched.
  // No atomics: two launches on the same input give the same bits.
  // GPU: m <= 128 runs in LDS; a larger m in an fp64 copy in device scratch that the device keeps and
  // grows on demand, which waits for the device: a caller that must not allocate mid-stream asks for it
  // ahead with prepare_slogdet.  slogdet_scratch_bytes(m, nb) is the size of that scratch for such a
  // launch (0: none needed), for the caller's memory estimate.
  virtual void slogdet_batch(DType dt, const void* blocks, int64_t stride, int64_t m, int64_t nb,
                             const int32_t* which, double* sign, double* logabs, int s) = 0;
  virtual size_t slogdet_scratch_bytes(int64_t m, int64_t nb) const { (void)m; (void)nb; return 0; }
  virtual void prepare_slogdet(int64_t m, int64_t nb) { (void)m; (void)nb; }

  // ---- power-of-two equilibration of a panel (SolveOptions::equilibrate) ----
  // X is this rank's rows of a panel, L.rows x L.npad of dtype dt, leading dimension ldx.  The three
  // ops work on its real rows (global row grow(r) = ((r / m) * p + rank) * m + r % m below L.n) and
  // its columns c < L.n.  Never read: X's padding rows, its columns >= n and every pitch gap, and the
  // entries of a natural-order exponent vector that belong to other ranks' rows.
  // Both maxima are taken in fp64 (an fp32 element is widened exactly) and a NaN or an Inf entry counts
  // as +Inf, never NaN, so that Comm::allreduce_max over the ranks cannot lose it.  No floating-point
  // atomics; the result does not depend on the grid (a maximum is exact in any order).
  // GPU: rows are addressed with 64-bit offsets, so every leading dimension is accepted; the byte
  // offsets inside a row are 32-bit, and an n whose row does not fit them is Status::BadArgs.
  //
  // out_nat[grow(r)] = max_{c<n} |X[r][c]| for this rank's real rows; other entries of out_nat
  // (n doubles, natural row order) are left untouched.
  virtual void abs_max_rows(DType dt, const void* X, int64_t ldx, const Layout& L, double* out_nat, int s) = 0;
  // out[c] = max over this rank's real rows of ldexp(|X[r][c]|, rexp_nat[grow(r)]) for c < n: the
  // column maxima of the row-scaled panel (LAPACK geequ's second pass).  rexp_nat: int32[n] in natural
  // row order (device), null = all 0.  out is written, not accumulated: a rank without real rows
  // writes +0.0.  A scaled value that overflows is +Inf.
  virtual void abs_max_cols(DType dt, const void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat,
                            double* out, int s) = 0;
  // X[r][c] = round_dt(ldexp((double)X[r][c], rexp_nat[grow(r)] + cexp[c])) over the real rows and the
  // columns c < n, in place.  rexp_nat as above, cexp: int32[n] (device), null = all 0.  Exact unless
  // the result leaves dt's normal range: NaN, +-Inf and +-0 (with its sign) are kept, an underflow is
  // rounded once (gradually, to a subnormal or a signed zero), an overflow gives +-Inf.  Nothing is
  // written outside the real rows x n columns, so the padding identity of diag(A, I) survives bit for
  // bit.
  virtual void scale_pow2(DType dt, void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat,
                          const int32_t* cexp, int s) = 0;

  // ---- a stack of small matrices (BatchSolver, gj/batch.hpp) ----
  // The stack's side of block_inverse's calling convention.  Matrix b of a stack is n x n, its rows ld
  // elements apart and the matrices stride elements apart; the block size of the inverter is m >= n
  // and the matrix enters it as diag(As_b, I) of order m.
  //
  // batch_pack: norm[b] = ||A_b||_inf from fp64 row sums (a NaN row sum gives NaN, as in row_abs_max),
  // exp[b] = equil_exponent(norm[b]), and the negated K-major panel of the scaled stack,
  //   Lt[c*ldl + b*m + r] = (dt)(-ldexp(A_b[r][c], exp[b]))  for r, c < n,
  //   -1 on the diagonal and 0 elsewhere                      for n <= r, c < m,
  // extract_neg_t's convention: block_inverse's W_b is ldexp(A_b, exp[b]).  A64 is fp64.  The scaling is
  // exact unless the result leaves dt's range (scale_pow2's rule); NaN, +-Inf and +-0 are kept.
  // Never read: A's pitch gaps and anything outside n x n of a matrix.  Never written: anything outside
  // the m x nb*m panel.  Refused (Status::BadArgs): n < 1, m < n, nb < 0, lda < n, ldl < nb * m.
  virtual void batch_pack(DType dt, const double* A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m,
                          int64_t nb, void* Lt, int64_t ldl, double* norm, int32_t* exp, int s) = 0;
  // batch_unpack: X_b[i][j] = (dt)ldexp(inv_t[b*m*m + j*m + i], exp[b]) for i, j < n -- block_inverse's
  // transposed output as row-major inverses of the unscaled matrices; a block with valid[b] == 0 writes
  // NaN.  inv_t and X are of dtype dt.  Nothing outside n x n of each X_b is written; of inv_t only the
  // leading n x n of a valid block is read.
  virtual void batch_unpack(DType dt, const void* inv_t, int64_t n, int64_t m, int64_t nb, const int32_t* exp,
                            const int32_t* valid, void* X, int64_t stride_x, int64_t ldx, int s) = 0;
  // batch_rhs: Y_b = C_in_b + sign * M_b V_b for b < nb: M_b n x n of dtype dt, V_b, C_in_b and Y_b fp64
  // n x k with 1 <= k <= kMaxRhs (else Status::BadArgs), sign +1 or -1.  Both dtypes work in fp64: an fp32
  // element of M is widened exactly, V is not rounded, the products and their sum are fp64.
  //   active  int32[nb*k] (device) or null: column j of matrix b with active[b*k + j] == 0 is neither
  //           read (C_in, Y) nor written, and its colmax entry is left alone
  //   colmax  double[nb*k] (device) or null: colmax[b*k + j] = max_r |Y_b[r][j]|, NaN kept
  //   C_in    null = 0; may be Y itself (then with Y's strides)
  // Never read: every pitch gap.  A NaN or an Inf of V reaches every element it is a term of, also
  // through a zero of M.  Each sum has one fixed order and there are no floating-point atomics: two
  // launches on the same inputs give the same bits.  The executors need not agree to the bit.
  virtual void batch_rhs(DType dt, const void* M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb,
                         const double* V, int64_t stride_v, int64_t ldv, int64_t k, const double* C_in,
                         int64_t stride_c, int64_t ldc, double* Y, int64_t stride_y, int64_t ldy, double sign,
                         const int32_t* active, double* colmax, int s) = 0;
};

// The exponent rule of the equilibration, one place for the engine and every executor's tests: the e
// with ldexp(amax, e) in [1, 2), i.e. 1 - frexp(amax).exponent; 0 for a maximum that is 0 or not finite.
inline int32_t equil_exponent(double amax) {
  if (!(amax > 0.0) || !(amax < std::numeric_limits<double>::infinity())) return 0;
  int e = 0;
  (void)std::frexp(amax, &e);
  return (int32_t)(1 - e);
}

// Test probe of Device::panel_rhs, like g_last_gemm_kernel: "host" on the host executor,
// "rhs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>" on the GPU.
inline thread_local const char* g_last_rhs_kernel = "";
// The same of Device::panel_rhs_dd: "host", or "rhsdd<16|32|64>:f64:<vec|scalar>:s<split>".
inline thread_local const char* g_last_rhs_dd_kernel = "";
// The same of Device::panel_rhs_t: "host", or "rhst<16|32|64>:<f64|f32>:<vec|scalar>:s<split>".
inline thread_local const char* g_last_rhs_t_kernel = "";
// The same of Device::panel_abs_rhs / panel_abs_rhs_t: "host", or
// "abs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>" / "abst..." for the transposed op.
inline thread_local const char* g_last_abs_kernel = "";
// The same of Device::rank_update: "host", or "rku<k padded to 4>:<f64|f32>:<vec|scalar>".
inline thread_local const char* g_last_rank_update_kernel = "";
// The same of Device::grad_matrix: "host", or "gm<k padded to 4>:<f64|f32|nop>:<vec|scalar>" (nop:
// alpha == 0, P not read).
inline thread_local const char* g_last_grad_matrix_kernel = "";
// The same of Device::slogdet_batch: "host", or "sld:<lds|glob>:<f64|f32>".
inline thread_local const char* g_last_slogdet_kernel = "";
// The same of the three equilibration ops: "host", or "eq:<rmax|cmax|scale>:<f64|f32>:<vec|scalar>".
inline thread_local const char* g_last_equil_kernel = "";
// The same of the three stack ops: "host", or "bpack:<f64|f32>" / "bunpack:<f64|f32>" /
// "brhs<16|32|64>:<f64|f32>:<vec|scalar>".
inline thread_local const char* g_last_batch_kernel = "";

}  // namespace gj
