// Launch wrappers of the hand-written gfx950 kernels (implemented in csrc/kernels/*.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "gj/common.hpp"
#include "gj/device.hpp"
#include "gj/layout.hpp"
#include "gj/pivot.hpp"

namespace gj {
namespace kern {

// gemm.hip
void gemm(DType dt, int op /*0 acc, 1 store*/, int a_kmajor, int64_t M, int64_t N, int64_t K,
          const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
          hipStream_t s, const GemmExtra* ex = nullptr);
// n independent small K-major GEMMs, one launch per 4 (small tiles; Store = C never read)
void gemm_batch(DType dt, const GemmDesc* d, int n, hipStream_t s);
// Test probe: the kernel family and build that this thread's last gemm / gemm_batch launched (or
// "host" after HostDevice::gemm): small | narrow | big | bigpf | squarepf | lat64 |
// glds64:t<64|128>:b<build>[:peel] | glds32:t<128|256> | batch:small | batch:lat.  "" before any.
const char* last_gemm_kernel();
int residual_nparts(int64_t N);
int gemm_variant_id(const char* name);  // big | narrow | squarepf | bigpf | glds | auto; else throws
void set_gemm_variant(int v);
void set_glds_peel(int on);  // fp64 LDS-DMA trailing update: peeled stage-unrolled loop (1) or not (0)
void set_glds_covl(int on);   // fp64 LDS-DMA kernel: C loads overlapped with the first slices (GJ_GLDS_COVL)
void set_lat_glds(int on);   // every latency GEMM of >= 1024 rows on the LDS-DMA kernel (tests; GemmExtra::lat_wide per call)
void set_lat_kernel(int mode); // fp64 latency GEMMs on the register-fed kernel: 1 / 0 forced, -1 per launch (GemmExtra::lat_reg)
void set_glds_build(int b);  // 23 | 25 | 33 (stages * 10 + waves-per-SIMD bound), 0 = auto
void set_glds_tile(int bn);  // 64 | 128: the fp64 LDS-DMA kernel's tile width for every launch, 0 = per launch (GJ_GLDS_TILE)
void set_block_inverse_variant(int v);  // 0 = default families, 1 = register sweep, 5 = co-resident, 6 = generic
int block_inverse_variant();
int block_inverse_variant_id(const char* name);  // panel | sweep | co | generic; else throws
const char* block_inverse_kernel_name(DType dt, int64_t m, int variant);
void residual_partial(DType dt, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                      const void* B, int64_t ldb, int64_t n_real, int64_t blk_m, int64_t p,
                      int64_t k, double* partial, hipStream_t s);

// misc.hip: partial pivoting (SolveOptions::pivot = Partial)
void candidate_maxabs(DType dt, const void* Lt, int64_t ldl, double* scores, int32_t* valid,
                      const int32_t* used, const Layout& L, double thresh, hipStream_t s);
void gather_candidate(DType dt, void* sel, const void* Lt, int64_t ldl, const PivotRec* rec, const Layout& L,
                      hipStream_t s);
void commit_candidate(DType dt, void* inv_t, const void* inv1, const int32_t* valid1, const double* score1, double growth, PivotRec* rec,
                      const Layout& L, hipStream_t s);

// blockinv.hip
void block_inverse(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                   int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                   hipStream_t s, void* scratch, int* iscratch, int variant = -1);
// blockinv_mfma.hip: 16 < m <= 128 (false = not handled)
bool block_inverse_mfma(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                        int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                        hipStream_t s, const PivotSelectArgs* sel = nullptr);
// block_inverse with the pivot selection fused into the launch (PivotSelectArgs) where the kernel
// family the call resolves to supports it (the matrix-core register kernel); false = nothing was
// launched, the caller runs block_inverse and the selection separately
bool block_inverse_select(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores,
                          int32_t* valid, const int32_t* used, const Layout& L, double thresh, int64_t nlive,
                          hipStream_t s, const PivotSelectArgs& sel, int variant = -1, void* scratch = nullptr);
// test probe: when set, the matrix-core block inverses write the pivot row of every column of
// every candidate to piv_out[b * m + c] (device memory; nullptr = off)
void set_block_inverse_probe(int32_t* piv_out);
int32_t* block_inverse_probe();
// blockinv_big.hip: fp64 128 < m <= 256 (false = not handled); scratch: nblk 256 x 256 images
bool block_inverse_big(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores, int32_t* valid,
                       const int32_t* used, const Layout& L, double thresh, int64_t nlive, hipStream_t s, void* scratch);
size_t block_inverse_big_scratch_bytes(DType dt, const Layout& L);
// blockinv_huge.hip: m > 4096 (or GJ_BI_VARIANT=huge), one candidate at a time with the whole GPU
// (panel factor + MFMA GEMM updates); scratch: nblk m x m slabs (the generic path's)
void block_inverse_huge(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores, int32_t* valid,
                        const int32_t* used, const Layout& L, double thresh, int64_t nlive, hipStream_t s,
                        void* scratch);
// the co-resident form (4 waves, fits the slot one trailing-update workgroup frees): fp64 32 < m <= 128;
// with sel, the batch's last workgroup also runs the selection (as block_inverse_mfma)
bool block_inverse_co(DType dt, const void* Lt, int64_t ldl, void* inv_t, double* scores, int32_t* valid,
                      const int32_t* used, const Layout& L, double thresh, int64_t nlive, hipStream_t s, void* scratch,
                      const PivotSelectArgs* sel = nullptr);
// scratch needed by the fp64 m > 128 paths (big kernel / generic sweep)
// (variant: the kernel family to use for this call, -1 = the process-wide setting)
size_t block_inverse_scratch_bytes(DType dt, const Layout& L, int variant = -1);
size_t block_inverse_iscratch_bytes(const Layout& L);

// misc.hip
void generate(DType dt, void* X, const Layout& L, int kind, uint64_t seed, hipStream_t s);
// generate() fused with row_abs_max() of the result (out zeroed here): one pass over the matrix
void generate_norm(DType dt, void* X, const Layout& L, int kind, uint64_t seed, double* out, hipStream_t s);
void widen(DType dt, double* dst, int64_t ldd, const void* X, int64_t ldx, int64_t rows, int64_t cols,
           hipStream_t s);
void upload_convert(DType dt, void* X, int64_t ldx, const double* src, int64_t src_ld, int64_t rows,
                    int64_t cols, hipStream_t s);
void extract_neg_t(DType dt, void* Lt, int64_t ldl, const void* X, int64_t ldx, int64_t rows,
                   int64_t col0, int64_t m, hipStream_t s);
void add_diag(DType dt, void* A, int64_t ld, int64_t nd, double alpha, hipStream_t s);
// nwg workgroups that each spin for `us` microseconds (lds_bytes > 0: 256 threads + that much LDS)
void spin(int nwg, double us, hipStream_t s, int lds_bytes = 0);
// zero `bytes` at p (16-byte vector stores, scalar tail) on nwg 256-thread workgroups holding
// lds_bytes of LDS each: the receiving RCCL channels' footprint in ShadowComm's cost model
void zero_channels(void* p, size_t bytes, int nwg, int lds_bytes, hipStream_t s);
void pivot_local(const double* scores, const int32_t* valid, const int32_t* used, const int32_t* pos,
                 const Layout& L, PivotRec* out, hipStream_t s);
void pivot_select_single(const double* scores, const int32_t* valid, const Layout& L, int32_t t,
                         int32_t* pos, int32_t* phys_at, int32_t* used, int32_t* seq, PivotRec* rec,
                         PivotResult* out, PivotResult* host_out, hipStream_t s);
int host_fence();  // GJ_HOST_FENCE (misc.hip): 1 = system-scope fences around the host pivot mirror
void pivot_global(const PivotRec* recs, int32_t p, int32_t t, int32_t* pos, int32_t* phys_at,
                  int32_t* used, int32_t* seq, PivotResult* out, PivotResult* host_out, hipStream_t s);
void owner_edits(DType dt, void* At, int64_t ldl, const int32_t* phys, int64_t p, int64_t k, int64_t j,
                 int64_t m, void* lrow, void* ht, const void* inv, const PieceMove& mv, hipStream_t s);
void take_rows(DType dt, void* dst, int64_t ldd, void* X, int64_t ldx, const int32_t* phys, int64_t p, int64_t k,
               int64_t col0, int64_t w, int64_t m, hipStream_t s);
void sum_slices(DType dt, void* dst, const void* src, int64_t count, int64_t nslices, hipStream_t s);
void zero_unless_owner(DType dt, void* buf, int64_t count, const int32_t* phys, int64_t p, int64_t k, hipStream_t s);
void h_block(DType dt, void* R, int64_t ldr, const void* Ht, int64_t m, hipStream_t s);
void permute_blocks(DType dt, void* dst, int64_t ldd, const void* X, int64_t ldx, int64_t nblk,
                    int64_t m, int64_t Nr, const int32_t* dst_blk, const int32_t* colsrc,
                    hipStream_t s);
// Device::hash_rows: nparts workgroups, parts[g] = workgroup g's partial hash
void hash_rows(const void* base, int64_t ld_bytes, int64_t width_bytes, int64_t rows, uint64_t* parts,
               int nparts, hipStream_t s);
// minus_identity: sum_j |X[r][j] - delta(global(r), j)| (the streamed residual's row sums)
void row_abs_max(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, hipStream_t s,
                 bool minus_identity = false);
// reduce residual partials: out = max over real local rows of sum_parts partial[r][*]
void residual_reduce(const double* partial, int nparts, const Layout& L, double* out, hipStream_t s);


// panel_rhs.hip: Device::panel_rhs / gather_rows_natural / copy_cols_masked.  scratch: the K-slice
// partials, panel_rhs_scratch_bytes(L, k) bytes (for the split the launch will use).
size_t panel_rhs_scratch_bytes(const Layout& L, int64_t k);
void panel_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
               const double* C_in, int64_t ldc, double* Y, int64_t ldy, double sign, const int32_t* active,
               double* colmax, void* scratch, hipStream_t s);
void gather_rows_natural(double* dst, int64_t ldd, const double* src, int64_t lds, const Layout& L, int64_t k,
                         hipStream_t s);
void copy_cols_masked(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t k,
                      const int32_t* mask, hipStream_t s);
// Test hooks: K-split of the following panel_rhs launches (0 = auto, s >= 1 forces s; a launch never
// runs an empty slice, so at most ceil(n / 16) take part), and the name of this thread's last
// panel_rhs launch, "rhs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>" ("host" on the host executor).
void set_rhs_splitk(int s);
const char* last_rhs_kernel();

// panel_rhs_dd.hip: Device::panel_rhs_dd, Y = round(C_in - P V) from a double-double sum (Dot2), P
// fp64.  The K-split is panel_rhs's plan and takes its test hook (set_rhs_splitk); scratch: the
// (hi, lo) partials of the slices, panel_rhs_dd_scratch_bytes(L, k) bytes.  Test probe: the name of
// this thread's last launch, "rhsdd<16|32|64>:f64:<vec|scalar>:s<split>" ("host" on the host executors).
size_t panel_rhs_dd_scratch_bytes(const Layout& L, int64_t k);
void panel_rhs_dd(const double* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                  const double* C_in, int64_t ldc, double* Y, int64_t ldy, const int32_t* active, double* colmax,
                  void* scratch, hipStream_t s);
const char* last_rhs_dd_kernel();

// panel_rhs_t.hip: Device::panel_rhs_t / axpy_cols_masked / col_abs_sum.  scratch: the row-slice
// partials, panel_rhs_t_scratch_bytes(...) bytes (for the split and load width the launch will use).
size_t panel_rhs_t_scratch_bytes(DType dt, const void* P, int64_t ldp, const Layout& L, int64_t k);
void panel_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                 double* S, int64_t lds, const int32_t* active, void* scratch, hipStream_t s);
void axpy_cols_masked(double* Y, int64_t ldy, const double* C_in, int64_t ldc, const double* S, int64_t lds,
                      double sign, int64_t rows, int64_t k, const int32_t* active, double* colmax, hipStream_t s);
void col_abs_sum(DType dt, const void* X, int64_t ldx, const Layout& L, double* out, hipStream_t s);
// Test hooks: row split of the following panel_rhs_t launches (0 = auto, s >= 1 forces s; a launch
// never runs an empty slice, so at most ceil(real rows / 4) take part), and the name of this thread's
// last panel_rhs_t launch, "rhst<16|32|64>:<f64|f32>:<vec|scalar>:s<split>" ("host" on the host
// executor).  Separate from set_rhs_splitk / last_rhs_kernel.
void set_rhs_t_split(int s);
const char* last_rhs_t_kernel();

// panel_abs.hip: Device::panel_abs_rhs / panel_abs_rhs_t / bound_terms.  The two products take the
// split plans, the scratch sizes (panel_rhs_scratch_bytes / panel_rhs_t_scratch_bytes) and the test
// hooks (set_rhs_splitk / set_rhs_t_split) of their siblings above.  Test probe: the name of this
// thread's last launch of either, "abs<16|32|64>:<f64|f32>:<vec|scalar>:s<split>" or "abst..." for the
// transposed one ("host" on the host executors).
void panel_abs_rhs(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                   const double* C_in, int64_t ldc, double* Y, int64_t ldy, double* colmax, void* scratch,
                   hipStream_t s);
void panel_abs_rhs_t(DType dt, const void* P, int64_t ldp, const Layout& L, const double* V, int64_t ldv, int64_t k,
                     double* S, int64_t lds, void* scratch, hipStream_t s);
void bound_terms(const double* R, int64_t ldr, const double* D, int64_t ldd, double* G, int64_t ldg, int64_t rows,
                 int64_t k, double nz_eps, double safe1, double safe2, double* berr, hipStream_t s);
const char* last_abs_kernel();

// rank_update.hip: Device::rank_update, one pass over X.  Test probe: the name of this thread's last
// launch, "rku<k padded to 4>:<f64|f32>:<vec|scalar>" ("host" on the host executor).
void rank_update(DType dt, void* X, int64_t ldx, const Layout& L, const double* W, int64_t ldw, bool w_natural,
                 const double* Z, int64_t ldz, int64_t k, double sign, hipStream_t s);
const char* last_rank_update_kernel();

// grad_matrix.hip: Device::grad_matrix, one pass over G with P's tiles transposed through LDS.  Test
// probe: the name of this thread's last launch, "gm<k padded to 4>:<f64|f32|nop>:<vec|scalar>" ("host" on
// the host executor).
void grad_matrix(DType dt, const void* P, int64_t ldp, int64_t n, double alpha, const double* W, int64_t ldw,
                 const double* Z, int64_t ldz, int64_t k, double sign, bool accumulate, double* G, int64_t ldg,
                 hipStream_t s);
const char* last_grad_matrix_kernel();

// slogdet.hip: Device::slogdet_batch.  scratch: slogdet_scratch_bytes(m, nb) bytes (0 for m <= 128, the
// LDS form).  Test probe: the name of this thread's last launch, "sld:<lds|glob>:<f64|f32>" ("host" on
// the host executor).
size_t slogdet_scratch_bytes(int64_t m, int64_t nb);
void slogdet_batch(DType dt, const void* blocks, int64_t stride, int64_t m, int64_t nb, const int32_t* which,
                   double* sign, double* logabs, void* scratch, hipStream_t s);
const char* last_slogdet_kernel();

// equilibrate.hip: Device::abs_max_rows / abs_max_cols / scale_pow2, one pass over X each.
void abs_max_rows(DType dt, const void* X, int64_t ldx, const Layout& L, double* out_nat, hipStream_t s);
void abs_max_cols(DType dt, const void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, double* out,
                  hipStream_t s);
void scale_pow2(DType dt, void* X, int64_t ldx, const Layout& L, const int32_t* rexp_nat, const int32_t* cexp,
                hipStream_t s);
// Test hooks: row split of the following abs_max_cols launches (0 = auto, s >= 1 forces s; a launch never
// runs an empty slice), the cache policy of scale_pow2's panel accesses (1 = non-temporal, the default;
// 0 = plain, for measurements), and the name of this thread's last launch of the three,
// "eq:<rmax|cmax|scale>:<f64|f32>:<vec|scalar>" ("host" on the host executor).
void set_equil_col_split(int s);
void set_equil_nt(int on);
const char* last_equil_kernel();

// batch.hip: Device::batch_pack / batch_unpack / batch_rhs over a stack of small matrices.  Test probe:
// the name of this thread's last launch of the three, "bpack:<f64|f32>", "bunpack:<f64|f32>" or
// "brhs<16|32|64>:<f64|f32>:<vec|scalar>" ("host" on the host executors).
void batch_pack(DType dt, const double* A64, int64_t stride_a, int64_t lda, int64_t n, int64_t m, int64_t nb,
                void* Lt, int64_t ldl, double* norm, int32_t* exp, hipStream_t s);
void batch_unpack(DType dt, const void* inv_t, int64_t n, int64_t m, int64_t nb, const int32_t* exp,
                  const int32_t* valid, void* X, int64_t stride_x, int64_t ldx, hipStream_t s);
void batch_rhs(DType dt, const void* M, int64_t stride_m, int64_t ldm, int64_t n, int64_t nb, const double* V,
               int64_t stride_v, int64_t ldv, int64_t k, const double* C_in, int64_t stride_c, int64_t ldc, double* Y,
               int64_t stride_y, int64_t ldy, double sign, const int32_t* active, double* colmax, hipStream_t s);
const char* last_batch_kernel();

}  // namespace kern
}  // namespace gj
