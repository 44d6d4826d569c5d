/* include/spgemm_hip.h — C ABI of libspgemm_hip.so: the MI355X (gfx950) CSR x CSR SpGEMM hot path.
 *
 * This is the drop-in boundary for the reference's SpGEMM kernel call surface.  Every entry point is
 * extern "C", takes plain pointers and sizes (int32 indices, float32 values — QValue is float,
 * nlibs/tools/macro.h:5; indices are int, nlibs/CSR.h:32-38) and returns an int status (0 = ok);
 * nothing throws across this boundary.  The C++ mirror of the reference's CSR/COO types and wrapper
 * functions (sparse_matrix_with_flops_amd/csrc/nlibs) sits on top of it and keeps the reference's
 * exit-on-error convention (nlibs/gpus/cuda_handle_error.h:7-15).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference tree).
 * The reference's other value type (QValue double, FDOUBLE, nlibs/tools/macro.h:3-6) has the *_f64 twins of the SpGEMM
 * entry points, the row sort and R-MCL (prune, fused step, loop), section (5) below.
 * Thread model: one caller thread per handle; calls return after the device work has completed
 * (the reference's GPU path is blocking too: nlibs/gpus/gpu_csr_kernel.cu:162).
 */
#ifndef SPGEMM_HIP_H_
#define SPGEMM_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------------- */
#define SPGEMM_OK                0
#define SPGEMM_ERR_HIP           1   /* a HIP runtime call failed (see spgemm_hip_last_error)         */
#define SPGEMM_ERR_ARG           2   /* bad argument: null pointer, negative size, shape mismatch     */
#define SPGEMM_ERR_OVERFLOW      3   /* nnz(C) does not fit the int32 CSR the boundary mandates       */
#define SPGEMM_ERR_NOMEM         4   /* host malloc failed                                            */
#define SPGEMM_ERR_INPUT         5   /* host CSR failed validation (rowPtr not monotone, col range)   */
#define SPGEMM_ERR_INTERNAL      6   /* device-side invariant broken (hash table full, count mismatch)*/
#define SPGEMM_ERR_NODEVICE      7   /* no HIP device: the product path has NO CPU fallback           */

/* internal row bins by intermediate-product count ("flops") */
#define SPGEMM_NBINS             9
/* reference-visible bin boundaries: hv[] as returned by gpuFlopsClassify (mindex2-cuda/flops.cu:96-107) */
#define SPGEMM_HV_LEN            9
#define SPGEMM_NKERNELS          21

typedef struct spgemm_handle spgemm_handle;

/* per-call statistics (filled by every SpGEMM entry point that takes a handle) */
typedef struct spgemm_stats {
  long long total_flops;          /* P = sum over A nonzeros of nnz(B row): "intermediate_nnz"           */
  int       nnzC;                 /* nnz of the product; -1 after hip_rmcl_expand_prune (the product is never counted) */
  int       bin_rows[SPGEMM_NBINS];/* rows per internal bin {0 | 1 | 2-4 | 5-16 | 17-64 | 65-512 | 513-2048 | 2049-4096 | >4096} */
  float     ms_classify;          /* HIP-event times on the handle's stream                              */
  float     ms_symbolic;
  float     ms_scan_alloc;
  float     ms_numeric;
  float     ms_total;
  float     ms_kernel[SPGEMM_NKERNELS]; /* HIP-event duration of every launch of the last call (0 = not launched);
                                     index = SPGEMM_K_* below                                          */
} spgemm_stats;

/* kernel ids for spgemm_stats.ms_kernel / spgemm_hip_kernel_name */
enum {
  SPGEMM_K_ROW_FLOPS = 0, SPGEMM_K_BIN_SCAN, SPGEMM_K_SCATTER,
  SPGEMM_K_SYM_SMALL4, SPGEMM_K_SYM_G16, SPGEMM_K_SYM_HASH1, SPGEMM_K_SYM_HASH4, SPGEMM_K_SYM_HASH8, SPGEMM_K_SYM_BIG,
  SPGEMM_K_SCAN,
  SPGEMM_K_NUM_SMALL4, SPGEMM_K_NUM_G16, SPGEMM_K_NUM_HASH1, SPGEMM_K_NUM_HASH4, SPGEMM_K_NUM_HASH8, SPGEMM_K_NUM_BIG,
  SPGEMM_K_NUM_BIGHASH,
  SPGEMM_K_CUT, SPGEMM_K_CHAIN,          /* round 4: rows dealt across rows -- the cut into batches; the one-pass kernel (chained prefix) */
  SPGEMM_K_WB_SYM, SPGEMM_K_WB_NUM       /* ... and its two-pass forms (counts / entries)                                                 */
};
const char* spgemm_hip_kernel_name(int id);

/* ---- library / device ------------------------------------------------------------------------ */
const char* spgemm_hip_last_error(void);          /* thread-local message of the last failure          */
int  spgemm_hip_device_count(int* count);
int  spgemm_hip_create(spgemm_handle** h, int device);   /* hipSetDevice(device), stream, workspace   */
int  spgemm_hip_destroy(spgemm_handle* h);
int  spgemm_hip_get_stats(const spgemm_handle* h, spgemm_stats* out);
void* spgemm_hip_stream(spgemm_handle* h);        /* hipStream_t the kernels run on (for event timing) */
/* Per-kernel HIP-event timing (spgemm_stats.ms_kernel): bit i of `mask` brackets the launches of kernel SPGEMM_K_<i>
 * with two events on the handle's stream.  Off by default (an event record costs stream time); bench.py turns on the
 * dominant kernel inside the timed region and all kernels in a separate, untimed pass. */
int  spgemm_hip_set_kernel_timing(spgemm_handle* h, unsigned mask);

/* ---- device memory: replaces the cudaMalloc/cudaMemcpy/cudaFree inside
 *      CSR::toGpuCSR / toCpuCSR / deviceDispose  (nlibs/CSR.cc:342-379) ------------------------- */
int  spgemm_hip_malloc(void** dptr, size_t bytes);
int  spgemm_hip_free(void* dptr);
/* bytes the caching allocator currently holds idle for `device` (tests; blocks are cached per device and given back
 * to the driver when the last handle of the device is destroyed) */
int  spgemm_hip_pool_cached_bytes(int device, size_t* bytes);
int  spgemm_hip_pool_trim(int device);            /* idle cached blocks of `device` go back to the driver now */
int  spgemm_hip_memcpy_h2d(void* dst, const void* src, size_t bytes);
int  spgemm_hip_memcpy_d2h(void* dst, const void* src, size_t bytes);
int  spgemm_hip_memcpy_d2d(void* dst, const void* src, size_t bytes);   /* device to device, same GPU */
/* waits for all work queued on the current device; a device-to-device copy above may return before it has run, so a
 * caller that times one (tools/reorder_bench.py) or hands its destination to another stream waits here */
int  spgemm_hip_device_synchronize(void);

/* ---- (1) host arrays in, host arrays out ------------------------------------------------------
 * Replaces the *_CSR_SpMM family:  sequential_CSR_SpMM / omp_CSR_SpMM / static_omp_CSR_SpMM /
 * flops_omp_CSR_SpMM / group_CSR_SpMM  (nlibs/cpu_csr_kernel.h:63-102), called from the CSR::*spmm
 * one-liners (nlibs/CSR.cc:59-208); also scudaSpMM(hA,hB) (mindex2-cuda/nGpuSpMM.cc:245-279).
 * A is m x k, B is k x n.  Inputs are borrowed.  *IC (m+1), *JC (nnzC), *C (nnzC) are malloc()ed here
 * so the caller's CSR::dispose() == free() stays valid (nlibs/CSR.h:323-327).
 * Rows of C are not column-sorted (same contract as the reference: nlibs/CSR.cc:73-86 exists for that). */
int hip_CSR_SpMM(const int* IA, const int* JA, const float* A, int nnzA,
                 const int* IB, const int* JB, const float* B, int nnzB,
                 int** IC, int** JC, float** C, int* nnzC,
                 int m, int k, int n);

/* wall-clock phases of the latest hip_CSR_SpMM of this process: upload of the operands, the device SpGEMM (hip_gpuSpMM),
 * download of C into the malloc()ed arrays.  Both copies run on 8 threads x 2 pinned 4 MB slots each (pageable memory at
 * PCIe rate, the page faults of the fresh output arrays spread over the threads). */
typedef struct spgemm_host_api_stats {
  float ms_h2d, ms_device, ms_d2h, ms_total;
  long long bytes_h2d, bytes_d2h;
} spgemm_host_api_stats;
int spgemm_hip_host_api_stats(spgemm_host_api_stats* out);

/* ---- (2) device-resident in, device-resident out ----------------------------------------------
 * Replaces CSR gpuSpMMWrapper(const CSR& dA, const CSR& dB)  (nlibs/gpus/gpu_csr_kernel.h:6,
 * gpu_csr_kernel.cu:128-173).  All d* pointers are device memory.  *dIC (m+1), *dJC, *dC are
 * allocated here (release with spgemm_hip_free == CSR::deviceDispose).  h may be NULL (a private
 * per-process handle on device 0 is used, like the reference's implicit device 0). */
int hip_gpuSpMM(spgemm_handle* h,
                const int* dIA, const int* dJA, const float* dA, int nnzA,
                const int* dIB, const int* dJB, const float* dB, int nnzB,
                int m, int k, int n,
                int** dIC, int** dJC, float** dC, int* nnzC);

/* ---- (2b) the same in two phases, outputs owned by the caller ----------------------------------
 * The reference's complete binned path is two-phase as well: gpu_compute_IC (symbolic, per bin) ->
 * exclusive scan -> cudaMalloc JC,C -> sgpu_SpGEMM (numeric, per bin)  ("mindex2-cuda/\":524-555, :322-483).
 * hip_spgemm_symbolic fills dIC[m+1] (caller-allocated device ints) with C's rowPtr and returns nnzC;
 * the handle keeps the row classification.  hip_spgemm_numeric must follow on the same handle with the
 * same A, B and dIC; it writes dJC[nnzC], dC[nnzC] (caller-allocated, e.g. a slice of a gathered
 * multi-GPU buffer).  h must not be NULL. */
int hip_spgemm_symbolic(spgemm_handle* h,
                        const int* dIA, const int* dJA, int nnzA,
                        const int* dIB, const int* dJB, int nnzB,
                        int m, int k, int n, int* dIC, int* nnzC);
int hip_spgemm_numeric(spgemm_handle* h,
                       const int* dIA, const int* dJA, const float* dA, int nnzA,
                       const int* dIB, const int* dJB, const float* dB, int nnzB,
                       int m, int k, int n, const int* dIC, int* dJC, float* dC);

/* per-row product counts only (gcomputeFlops, mindex2-cuda/flops.cu:66-83; dynamic_omp_CSR_flops,
 * nlibs/flops_csr_kernel.cc:14-31): dRowFlops[m] device ints (saturating at INT_MAX), *total_flops = P.
 * Feeds the flops-balanced row partition (arrayEqualPartition64, nlibs/tools/util.cc:123-135). */
int hip_csr_row_flops(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m,
                      int* dRowFlops, long long* total_flops);

/* ---- (3) per-row flop count + row binning ------------------------------------------------------
 * Replaces std::vector<int> gpuFlopsClassify(const CSR& dA, const CSR& dB, int** drowIdsp,
 * int** dflopId)  (mindex2-cuda/flops.cu:110-185; kernels gcomputeFlops :66-83, gcomputeBinId :87-94).
 *   *drowIds   device int[m]   : row ids grouped by bin, bins ascending; inside a bin rows ascend
 *                                (the reference sorts fully by flops with thrust::stable_sort_by_key;
 *                                 no consumer depends on the order inside a bin)
 *   *dflops    device int[m+1] : dflops[0]=0, dflops[1+q] = inclusive scan of the flops of
 *                                drowIds[0..q] (saturating at INT_MAX)        (flops.cu:119,133)
 *   hv[9]      host            : hv[0]=0, hv[b+1] = number of elements with reference bin id <= b in the
 *                                (m+1)-long array {dummy 0-flop element, rows...}; reference bin ids
 *                                (dqueueId, flops.cu:39-47): 0->1, 1->2, 2..4->3, 5..16->4, 17..64->5,
 *                                65..512->6, >512->7.   Callers index rows of bin b as
 *                                drowIds + hv[b] - 1  (mindex2-cuda/gnnz.cuh:27).
 *   *hv_len                    : number of entries the reference's vector would have (max bin + 2)
 *   *total_flops               : P (64-bit; the reference's int scan overflows at 2^31)
 * drowIds/dflops are released by the caller with spgemm_hip_free (nGpuSpMM.cc:271). */
int hip_gpuFlopsClassify(spgemm_handle* h,
                         const int* dIA, const int* dJA, const int* dIB,
                         int m, int k,
                         int** drowIds, int** dflops, int hv[SPGEMM_HV_LEN], int* hv_len,
                         long long* total_flops);

/* ---- (4) binned SpGEMM on a given classification ----------------------------------------------
 * Replaces CSR sgpuSpMMWrapper(const CSR& dA, const CSR& dB, int* drowIds, const vector<int>& hv,
 * int* dflops)  (mindex2-cuda/kernel.cu:311-427; HEAD returns an empty CSR, the complete older
 * version is the file "mindex2-cuda/\":485-565).  drowIds/hv must come from hip_gpuFlopsClassify for
 * the same A,B.  Outputs as in (2). */
int hip_sgpuSpMM(spgemm_handle* h,
                 const int* dIA, const int* dJA, const float* dA, int nnzA,
                 const int* dIB, const int* dJB, const float* dB, int nnzB,
                 int m, int k, int n,
                 const int* drowIds, const int hv[SPGEMM_HV_LEN], const int* dflops,
                 int** dIC, int** dJC, float** dC, int* nnzC);

/* ---- R-MCL (the caller of the path) --------------------------------------
 * hip_rmcl_prune: the post-step of one iteration on device arrays: inflate / threshold-prune / normalise every row of
 * C (dIC[m+1], dJC, dC; inputs are not modified) and compact into new arrays (*dIN, *dJN, *dCN allocated here, release
 * with spgemm_hip_free).  CPU: nlibs/qrmcl.cc:96-117 + nlibs/tools/util.cc:4-69; reference GPU: nlibs/gpus/dutil.cuh.
 * hip_gpuRmclIter: void gpuRmclIter(const int maxIter, const CSR Mgt, CSR& Mt) (nlibs/gpus/gpu_csr_kernel.cu:281-311):
 * host CSRs in; Mt <- prune(Mgt * Mt) maxIter times; the new Mt comes back in malloc()ed arrays (the caller disposes
 * the old ones). */
int hip_rmcl_prune(spgemm_handle* h, int m, const int* dIC, const int* dJC, float* dC,
                   int** dIN, int** dJN, float** dCN, int* nnzN);
/* the same with nnz(C) supplied by the caller (known on the host after every SpGEMM): saves one device read */
int hip_rmcl_prune_n(spgemm_handle* h, int m, int nnz, const int* dIC, const int* dJC, const float* dC,
                     int** dIN, int** dJN, float** dCN, int* nnzN);
/* hip_rmcl_expand_prune: one R-MCL iteration on device arrays as ONE operator, Mt' = prune(A * B) (A = Mgt, B = Mt):
 * what the reference's loop body does with gpuSpMMWrapper + inflate/threshold kernels + thrust::remove
 * (nlibs/gpus/gpu_csr_kernel.cu:281-311 with :218-270).  The product is never materialised: the numeric kernels apply
 * the row rule to each finished row in LDS and write only the kept entries.  Same results as hip_gpuSpMM followed by
 * hip_rmcl_prune up to the summation order of the row sums (entries within float rounding of the threshold).
 * Outputs allocated here (release with spgemm_hip_free); rows keep the order the product kernels emit (unsorted).
 * Domain (this call, its _f64 twin and the loops built on them): the squares of the product's entries are zero or normal
 * numbers of the value type, i.e. |entry| is 0 or at least 2^-63 (float) / 2^-511 (double).  A kept value is
 * v * (1 / kept sum) with one rounded reciprocal per row; a row that keeps a single entry gets 1.0 as such.  Where
 * several kept squares add up to at most 2^-128 (2^-1024), which takes subnormal squares, the reciprocal overflows and
 * the row's values are inf; hip_rmcl_prune divides and has no such limit.  On the edge of the domain (squares of
 * 2^-126 / 2^-1022) every kernel gives the reference's values (tests/test_gpu_rmcl_rule_branches.py). */
int hip_rmcl_expand_prune(spgemm_handle* h,
                          const int* dIA, const int* dJA, const float* dA, int nnzA,
                          const int* dIB, const int* dJB, const float* dB, int nnzB,
                          int m, int k, int n,
                          int** dIN, int** dJN, float** dCN, int* nnzN);
/* hip_gpuRmclIter_device: the loop of gpuRmclIter (nlibs/gpus/gpu_csr_kernel.cu:281-311) on DEVICE arrays: maxIter
 * iterations Mt <- prune(Mgt * Mt) starting from (dtI, dtJ, dtA), which are not modified; the result is a packed device
 * CSR (release with spgemm_hip_free).  Between iterations Mt is kept in the layout the fused epilogues write (every
 * row's kept entries at the front of its scratch range, {start, kept} per row): only the last iteration packs.  Same
 * results as maxIter calls of hip_rmcl_expand_prune.  hip_gpuRmclIter = upload + this + download.  h may be NULL. */
int hip_gpuRmclIter_device(spgemm_handle* h, int maxIter, int rows, int cols,
                           const int* dgI, const int* dgJ, const float* dgA, int gnnz,
                           const int* dtI, const int* dtJ, const float* dtA, int tnnz,
                           int** oI, int** oJ, float** oA, int* onnz);
int hip_gpuRmclIter(int maxIter, int rows, int cols,
                    const int* gIA, const int* gJA, const float* gA, int gnnz,
                    const int* tIA, const int* tJA, const float* tA, int tnnz,
                    int** oIA, int** oJA, float** oA, int* onnz);

/* ---- multi-GPU (north_star: "partition A by row blocks across up to 8 GPUs with B replicated and a
 * final RCCL allgatherv of C's row segments over xGMI") ----------------------------------------------------------------
 * The reference has no multi-device code; its GPU R-MCL entry is the single call gpuRmclIter(maxIter, Mgt, Mt)
 * (nlibs/gpus/gpu_csr_kernel.cu:281-311, dispatched from nlibs/qrmcl.cc:149-152) and its CPU path cuts rows into
 * contiguous ranges of equal flops for its threads (arrayEqualPartition64, nlibs/tools/util.cc:123-135, used by
 * flops_omp_CSR_SpMM, nlibs/flops_csr_kernel.cc:59-63).  The same cut is made here across GPUs.
 *
 * A group is a set of shards, each with its own device, handle and stream.
 *   spgemm_hip_group_create       all shards in THIS process: shard i on devices[i] (NULL: i modulo the device count).
 *                                 Several shards may share a device (logical shards: how a one-GPU box runs the whole
 *                                 sharded path).  transport: how the row segments of the result travel between shards.
 *   spgemm_hip_unique_id +        one process per GPU (torchrun, MPI, ...): rank 0 makes an id (128 bytes), the caller
 *   spgemm_hip_group_create_rank  hands it to every rank by whatever channel it has, every rank creates its one-shard
 *                                 group; the exchange runs over RCCL inside this library.
 * hip_gpuRmclIter uses a group over all visible devices on its own when there is more than one. */
#define SPGEMM_XCHG_AUTO  0   /* RCCL when every shard has its own device and librccl loads, else PEER            */
#define SPGEMM_XCHG_RCCL  1   /* grouped ncclSend/ncclRecv per peer (full xGMI mesh: every segment on its own link) */
#define SPGEMM_XCHG_PEER  2   /* hipMemcpyPeerAsync between the shards' devices (d2d copies on a shared device)    */
#define SPGEMM_XCHG_HOST  3   /* staged through pinned host memory                                                 */
#define SPGEMM_UNIQUE_ID_BYTES 128
typedef struct spgemm_group spgemm_group;
typedef struct spgemm_sharded spgemm_sharded;
int spgemm_hip_group_create(spgemm_group** g, int nshards, const int* devices, int transport);
int spgemm_hip_rccl_available(void);          /* SPGEMM_OK when librccl loads in this process (ask on every rank first) */
int spgemm_hip_unique_id(void* id128);
int spgemm_hip_group_create_rank(spgemm_group** g, int nranks, int rank, int device, const void* id128);
int spgemm_hip_group_info(const spgemm_group* g, int* nranks, int* nlocal, int* transport);
int spgemm_hip_group_destroy(spgemm_group* g);

/* Row-sharded C = A*B with the operands resident: HOST CSR arrays in (every process of a multi-process group passes the
 * same full A and B; B == NULL means B = A), rows of A cut into nranks contiguous blocks of equal flops
 * (arrayEqualPartition64), block r uploaded to shard r, B replicated.  One step = per-row flops, binning, symbolic,
 * numeric on every shard (the single-GPU pipeline, each shard's numeric phase writing straight into its slice of the
 * gathered arrays) and, with gather != 0, the allgatherv after which EVERY shard holds the whole C.
 * *nnzC = nnz of the gathered C (gather = 0: entries held by this process's shards), *totalP = products of the whole job.
 * hip_sharded_spmm_result copies what local shard `local_shard` holds to malloc()ed host arrays (*rows = its row count:
 * m when gathered, the block's rows otherwise).  hip_sharded_spmm_info: the row cut ends[nranks+1] and the last step's
 * compute (slowest local shard, HIP events) and exchange (wall clock) times. */
int hip_sharded_spmm_create(spgemm_group* g, const int* IA, const int* JA, const float* A, int nnzA,
                            const int* IB, const int* JB, const float* B, int nnzB, int m, int k, int n,
                            spgemm_sharded** job);
int hip_sharded_spmm_step(spgemm_sharded* job, int gather, long long* nnzC, long long* totalP);
int hip_sharded_spmm_result(spgemm_sharded* job, int local_shard, int** IC, int** JC, float** C, int* nnzC, int* rows);
int hip_sharded_spmm_info(spgemm_sharded* job, int* ends, float* ms_compute, float* ms_exchange);
/* the handle a local shard computes with (spgemm_hip_get_stats / spgemm_hip_set_kernel_timing); owned by the group */
spgemm_handle* hip_sharded_spmm_handle(spgemm_sharded* job, int local_shard);
int hip_sharded_spmm_destroy(spgemm_sharded* job);

/* gpuRmclIter over a group: Mgt's row blocks (cut by the flops of the first expansion) stay resident per shard, Mt is
 * replicated; every iteration a shard expands AND prunes its own rows (the fused step), packs the kept entries straight
 * into its slice of the next replicated Mt, and the slices are gathered -- what crosses xGMI is the pruned matrix.
 * Host CSRs in, malloc()ed host CSR out (every process of a multi-process group gets the whole result).
 * Replaces the one call the reference's driver makes (nlibs/gpus/gpu_csr_kernel.cu:281-311, nlibs/qrmcl.cc:149-152). */
int hip_gpuRmclIter_sharded(spgemm_group* g, int maxIter, int rows, int cols,
                            const int* gIA, const int* gJA, const float* gA, int gnnz,
                            const int* tIA, const int* tJA, const float* tA, int tnnz,
                            int** oIA, int** oJA, float** oA, int* onnz);

/* The same loop with the operands RESIDENT (round 4): create uploads Mgt's blocks and the initial Mt once; every run does
 * maxIter iterations from that initial Mt on device arrays only (what a caller times: no upload, no download) and leaves
 * the result on every shard; result copies it to malloc()ed host arrays; iter_nnz returns nnz(Mt) after every iteration of
 * the last run (returns their number; at most `cap` are written).  hip_gpuRmclIter_sharded = create + run + result + destroy.
 * A rank whose iteration fails still enters the size exchange (with a sentinel): every rank of a multi-process group
 * leaves the run with an error instead of waiting in a collective. */
typedef struct spgemm_sharded_rmcl spgemm_sharded_rmcl;
int hip_sharded_rmcl_create(spgemm_group* g, int rows, int cols, const int* gIA, const int* gJA, const float* gA, int gnnz,
                            const int* tIA, const int* tJA, const float* tA, int tnnz, spgemm_sharded_rmcl** job);
int hip_sharded_rmcl_run(spgemm_sharded_rmcl* job, int maxIter, int* nnz);
int hip_sharded_rmcl_continue(spgemm_sharded_rmcl* job, int iters, int* nnz);   /* from the previous run's result */
int hip_sharded_rmcl_result(spgemm_sharded_rmcl* job, int local_shard, int** oIA, int** oJA, float** oA, int* onnz);
int hip_sharded_rmcl_iter_nnz(const spgemm_sharded_rmcl* job, long long* out, int cap);
int hip_sharded_rmcl_info(const spgemm_sharded_rmcl* job, int* ends);
int hip_sharded_rmcl_destroy(spgemm_sharded_rmcl* job);

int spgemm_hip_handle_device(const spgemm_handle* h);   /* the device a handle (a group's shard) computes on; -1 for NULL */

/* devices the latest hip_gpuRmclIter of this process computed on: 1 unless SPGEMM_RMCL_DEVICES=N|all (or
 * SPGEMM_RMCL_SHARDS=K, logical shards) asked for the sharded loop -- implicit sharding is opt-in */
int spgemm_hip_rmcl_devices_used(void);

/* test hook: the next `count` symbolic phases / fused R-MCL steps on this handle fail before they queue anything (how the
 * tests make one rank of a multi-rank group fail) */
int spgemm_hip_debug_fail_next(spgemm_handle* h, int count);

/* test hook: how the latest product on this handle split its rows of more than 4096 products (n > 262144 columns, float)
 * between the direct kernel, which keeps only a row's repeated columns in its table, and the multi-pass hash kernel; the
 * re-hits a row may log and still take the direct kernel; the ints of one block's region of the re-hit log (0: no log yet).
 * SPGEMM_BIGDIRECT=0 (read at handle creation) sends every such row to the hash kernel, and so does a product with fewer such
 * rows than SPGEMM_BD_MINROWS (default: the number of CUs; the tests set 1); SPGEMM_RLREGION=<ints> fixes the region size
 * (tests fill a region with it). */
int spgemm_hip_debug_bigrow_paths(spgemm_handle* h, int* direct_rows, int* fallback_rows, int* rehit_cap, int* region_ints);

/* test hook: the same for the rows of 513-4096 products (any n, float): `rows` of the latest product on this handle, how many
 * took the direct kernel (rows without a repeated column, which are expanded, included) and how many the hash kernel of
 * their bin, and the re-hits a row may log and still go direct.  SPGEMM_MIDDIRECT=0 (read at handle creation) keeps the hash
 * kernels for all of them; so does a handle's first call with such rows, which only measures the log it needs, and each of
 * the two bins (513-2048, 2049-4096) when it has fewer rows than SPGEMM_MD_MINROWS (default: 4 x the number of CUs; the
 * tests set 1).
 * SPGEMM_MD_CFG=0..3 picks waves x table slots of the direct kernel for both bins (4x1024, 8x1024, 4x2048, 8x2048; the cap is
 * 7/8 of the slots; default: 4x1024 for 513-2048 products, 8x1024 above), SPGEMM_MD_CAP=<re-hits> lowers the cap and SPGEMM_MRLOG=<ints> fixes the size of the log (tests run it out of
 * space with the two). */
int spgemm_hip_debug_midrow_paths(spgemm_handle* h, int* rows, int* direct_rows, int* fallback_rows, int* rehit_cap);
/* ... and the log behind it: re-hits logged by the rows that went direct (the sum of products - nnz over those rows), ints
 * of log space the call's symbolic pass reserved or would have reserved, ints the log had. */
int spgemm_hip_debug_midrow_log(spgemm_handle* h, long long* logged, long long* reserved, long long* capacity);
/* ... and the two direct kernels of the rows of 513-2048 products: how many of the latest product's direct rows took the
 * wave-per-row kernel (at most 448 re-hits, one wave and a 512-slot table per row) and how many the four-wave kernel (the
 * rows above that up to the cap).  The kernels count on the device; the call waits for the handle's stream.
 * SPGEMM_MD_WAVE=0 (read at handle creation) keeps the four-wave kernel for all of them; so does a product with fewer such
 * rows than SPGEMM_MW_MINROWS (default: 32 x the number of CUs; the tests set 1).  SPGEMM_MW_PERCU=<1..32> sets the waves
 * of the wave-per-row kernel per CU (default 16). */
int spgemm_hip_debug_midrow_kernels(spgemm_handle* h, long long* wave_rows, long long* multiwave_rows);
/* ... and the symbolic kernel that counted and logged the rows of 513-2048 products of the latest product, when its
 * symbolic pass logged: k_sym_midpair (one statically scheduled launch over the bin, two rows of 513-1024 products at a time
 * in a block) or the four-wave kernel with its row queue.  SPGEMM_SYM_PAIR=1 (read at handle creation; default 0: measured no
 * faster) turns k_sym_midpair on for the one-shot hip_gpuSpMM / hip_CSR_SpMM whose previous product on the handle had the same
 * m, n and nnz(A) and at least SPGEMM_SP_MINROWS such rows (default: 32 x the number of CUs; 0 takes it without asking, which
 * the tests set); every other product keeps the four-wave kernel.  SPGEMM_SP_WAVES=2|4 sets the waves of its blocks (default
 * 4: two per row of 513-1024 products), SPGEMM_SP_PERCU=<1..8> its blocks per CU (default 6). */
int spgemm_hip_debug_midrow_sym_paths(spgemm_handle* h, long long* pair_rows, long long* multiwave_rows);

/* ---- the step in front of the path: COO -> CSR on device arrays -------------
 * Replaces COO::addSelfLoopIfNeeded (nlibs/COO.cc:160-188), COO::makeOrdered / orderedAndDuplicatesRemoving
 * (nlibs/COO.cc:222-266: std::sort on (row,col), duplicates summed), COO::toCSR (nlibs/COO.cc:268-291),
 * CSR::averAndNormRowQValue (nlibs/CSR.cc:88-95) and CSR::toAbs (nlibs/CSR.h:152-158): what rmclInit
 * (nlibs/qrmcl.cc:126-134 = SELF_LOOPS | ROW_NORMALISE) and the Matrix-Market / SNAP loaders (= DEDUPE) do after
 * parsing.  dRow/dCol/dVal: device COO (any order).  Outputs: device CSR from the library pool (release with
 * spgemm_hip_free); rows column-sorted.  Duplicates are summed in input order (bit-exact with the CPU loop).
 * Entries outside rows x cols -> SPGEMM_ERR_INPUT. */
#define SPGEMM_COO_DEDUPE         1   /* sum duplicates of one (row,col)                              */
#define SPGEMM_COO_SELF_LOOPS     2   /* append (i,i,1.0) for every row without a diagonal entry      */
#define SPGEMM_COO_ROW_NORMALISE  4   /* every entry of row i becomes 1/count(i)                      */
#define SPGEMM_COO_ABS            8   /* |value|                                                      */
int hip_coo_to_csr(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol, const float* dVal,
                   int flags, int** dIA, int** dJA, float** dA, int* nnzOut);
/* The same for QValue double (the reference's FDOUBLE build): same flags, errors and outputs.  A run of equal (row,col) is
 * summed by one lane, left to right in input order, in double (bit-exact with the CPU loop); ABS is fabs of that sum;
 * ROW_NORMALISE writes the double 1.0 / count (nlibs/CSR.cc:92), not the float quotient widened; an appended self loop is
 * 1.0.  Nothing on the way narrows to float. */
int hip_coo_to_csr_f64(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol, const double* dVal,
                       int flags, int** dIA, int** dJA, double** dA, int* nnzOut);

/* ---- the text in front of that step: edge lines "from to [value]" -> device COO, a file -> device CSR ---------------------
 * Replaces, for line-oriented files, the text half of COO::readSNAPFile (nlibs/COO.cc:48-158): the lines
 * are cut and converted by kernels, with the conversions sscanf("%d%d%f") performs, bit for bit.  A line holding a number
 * the device scanner does not promise to convert like the C library (csrc/edge_scan.hpp: 19 or more digits in an index;
 * inf / nan / hex; more than 2^53 in the digits or a decimal exponent beyond +-22; a value half-way between two floats) is
 * "slow": the host parses exactly those lines with strtol / strtol / strtof and stores their triplets.
 * The counting rule is the reference's: at most `declared` lines are read (declared < 0 is 0), reading stops at the first
 * line with fewer than two fields, entries = min(declared, lines, first such line); a missing value is 1.0; lines at or
 * beyond `declared` are never parsed.  A line ends at '\n'; a NUL byte inside a line ends that line's string; a last line
 * without '\n' counts.  (fgets cuts lines at 1024 characters in the reference; here, as in COO::readSNAPFile of the
 * mirror, a line ends at its newline.)
 * The _f64 entries do the same for QValue double (sscanf("%d%d%lf"), nlibs/COO.cc:101-105,132-136) with strtod's 64 bits.
 * Their value scanner reads the same tokens and converts, exactly and without a floating-point operation, every value
 * with at most 19 significant digits (leading zeros not counted) and |e10| <= 27, e10 = exponent - fraction digits: zero
 * digits are +-0.0, the rest is w * 5^e10 * 2^e10 rounded once to nearest-even in 128-bit integers.  20 or more digits, a
 * larger |e10|, inf / nan / hex are slow and go through strtod on the host.  A float midpoint or a 17-digit value is fast
 * there.
 * Not covered (they stay on the host loader): symmetric MatrixMarket files (a token stream, not lines), texts above 2 GiB.
 * h == NULL = the default handle; a call returns after the device work has completed; st may be NULL.  Argument checks
 * (a null output, null text with nbytes > 0, an unknown flag bit, a misaligned device text -> SPGEMM_ERR_ARG;
 * nbytes > INT32_MAX -> SPGEMM_ERR_OVERFLOW) run before any device is touched.  On any error the outputs are NULL, the
 * counts 0, nothing stays allocated, the handle stays usable. */
#define SPGEMM_EDGES_ONE_BASED 1   /* MatrixMarket: both indices minus 1 */
#define SPGEMM_EDGES_TRANSPOSE 2   /* isTrans: row = second number, col = first */
typedef struct spgemm_edge_stats {
  long long lines;          /* lines in the text */
  long long first_bad_line; /* -1 if none among the lines looked at */
  int entries, slow_lines;  /* slow_lines: parsed on the host */
  float ms_upload, ms_split, ms_parse, ms_slow, ms_total;   /* wall clock: text to the device; count + scan + line starts;
                               the parse kernel; the slow lines; all of it (hip_read_edge_file: without the file read and
                               without hip_coo_to_csr) */
} spgemm_edge_stats;

/* pure host, no device: banner / comment lines / size line, as readSNAPFile reads them (nlibs/COO.cc:56-128).  The first
 * line, if it starts with '%' and has 5 tokens, is a MatrixMarket banner (*one_based = 1; *symmetric = its 5th token is
 * "symmetric", any case).  Lines starting with '#' or '%' are skipped; the next line holds 2 numbers (rows = cols = a,
 * declared = b) or 3 (rows, cols, declared); *data_offset = the byte behind that line.  No such line -> SPGEMM_ERR_INPUT
 * (the reference exits).  An empty text or only comments: sizes and offset zero, SPGEMM_OK. */
int hip_edge_text_header(const char* text, size_t nbytes, int* rows, int* cols, int* declared,
                         int* one_based, int* symmetric, size_t* data_offset);
/* dText: the edge lines in DEVICE memory, 16-byte aligned (not modified).  *dRow, *dCol, *dVal: library pool arrays with
 * room for *entries triplets in line order (release with spgemm_hip_free; never NULL on success). */
int hip_parse_edge_lines(spgemm_handle* h, const char* dText, size_t nbytes, int declared, int flags,
                         int** dRow, int** dCol, float** dVal, int* entries, spgemm_edge_stats* st);
/* double values: the fast class above (<= 19 significant digits, |e10| <= 27; the rest through strtod on the host), a
 * missing value is 1.0; the triplets stay in line order, nothing is summed here */
int hip_parse_edge_lines_f64(spgemm_handle* h, const char* dText, size_t nbytes, int declared, int flags,
                             int** dRow, int** dCol, double** dVal, int* entries, spgemm_edge_stats* st);
/* the same for HOST text (any alignment): uploaded through the pinned lanes hip_CSR_SpMM uses */
int hip_parse_edge_text (spgemm_handle* h, const char* text,  size_t nbytes, int declared, int flags,
                         int** dRow, int** dCol, float** dVal, int* entries, spgemm_edge_stats* st);
/* double values from HOST text: the same fast class; line order, nothing summed */
int hip_parse_edge_text_f64 (spgemm_handle* h, const char* text,  size_t nbytes, int declared, int flags,
                             int** dRow, int** dCol, double** dVal, int* entries, spgemm_edge_stats* st);
/* readSNAPFile(path, isTrans) + hip_coo_to_csr(cooFlags) with the triplets never on the host: reads the file once, parses
 * its header, hip_parse_edge_text on the rest (ONE_BASED from the banner, TRANSPOSE from isTrans), hip_coo_to_csr.
 * A symmetric MatrixMarket file -> SPGEMM_ERR_INPUT; an unreadable file -> SPGEMM_ERR_ARG. */
int hip_read_edge_file  (spgemm_handle* h, const char* path, int isTrans, int cooFlags, int* rows, int* cols,
                         int** dIA, int** dJA, float** dA, int* nnz, spgemm_edge_stats* st);
/* double values: hip_parse_edge_text_f64 (its fast class: <= 19 significant digits, |e10| <= 27) + hip_coo_to_csr_f64
 * (duplicates summed left to right in input = line order, in double) */
int hip_read_edge_file_f64(spgemm_handle* h, const char* path, int isTrans, int cooFlags, int* rows, int* cols,
                           int** dIA, int** dJA, double** dA, int* nnz, spgemm_edge_stats* st);

/* ---- the way out: a device CSR as edge-list text, written on the device -------------------------------------------------
 * The inverse of the parse above and the replacement of the download plus CSR::output's single-threaded
 * printf("%d\t%d\t%.6lf\n") loop (nlibs/CSR.cc): one line "row SEP col SEP value\n" per entry, in CSR order, sized,
 * placed and written by kernels (csrc/edges_write_device.hpp) through a formatter shared with the host
 * (csrc/edge_print.hpp), byte for byte what snprintf writes.
 *   SPGEMM_EDGE_FMT_FIXED6     "%d\t%d\t%.6lf\n", the line of CSR::output.  On the device: +-0 and every finite |x| < 1e15.
 *   SPGEMM_EDGE_FMT_ROUNDTRIP  "%d %d %.9g\n" (float) / "%d %d %.17g\n" (double): reading the text back gives the same bits.
 *                              On the device: +-0 and every finite 1e-15 <= |x| < 1e17.
 * Every other value (inf, nan, outside the class) is "slow": the host formats exactly those entries with snprintf and the
 * device puts their bytes in place.  flags: SPGEMM_EDGES_ONE_BASED prints both indices plus 1, SPGEMM_EDGES_TRANSPOSE prints
 * "col row value" -- the flags hip_parse_edge_* undoes them with.  The _f64 entries take double values.
 * h == NULL = the default handle; a call returns after its work has completed; st may be NULL.  Argument checks (a null
 * output, a null CSR array with m > 0, an unknown fmt, flags or header, row0 > row1 or outside [0, m] -> SPGEMM_ERR_ARG)
 * run before any device is touched; a rowPtr that is not monotone from 0 -> SPGEMM_ERR_INPUT.  On any error the outputs
 * are NULL / 0, the stats zero, nothing stays allocated, the handle stays usable. */
#define SPGEMM_EDGE_FMT_FIXED6    0
#define SPGEMM_EDGE_FMT_ROUNDTRIP 1
typedef struct spgemm_edge_write_stats {
  long long entries, bytes;      /* lines written; bytes of text (hip_write_edge_file: the header included) */
  long long slow_entries;        /* formatted on the host */
  int slabs;                     /* pieces the text was produced in (1 outside hip_write_edge_file) */
  float ms_length, ms_scan, ms_write;   /* device time of the length pass, the scan (with its read-back), the write pass */
  float ms_slow, ms_download, ms_file, ms_total;   /* wall clock: the slow entries; text to the host; fwrite + fclose (runs
                                    beside the next slab's formatting); all of it */
} spgemm_edge_write_stats;

/* pure host, no device, the counterpart of hip_edge_text_header.  header 0: nothing (*nbytes = 0); 1: the size line
 * "rows cols entries\n" readSNAPFile reads; 2: "%%MatrixMarket matrix coordinate real general\n" and the size line (the
 * lines behind it are then one-based).  buf too small (or NULL with header != 0), an unknown header, a negative size ->
 * SPGEMM_ERR_ARG.  64 + 36 bytes always suffice. */
int hip_edge_text_write_header(char* buf, size_t cap, int header, int rows, int cols, long long entries, size_t* nbytes);
/* rows [row0, row1) of the m x n device CSR as text in DEVICE memory: *dText is a library pool block of *nbytes bytes
 * (never NULL on success; release with spgemm_hip_free).  More than INT32_MAX bytes -> SPGEMM_ERR_OVERFLOW. */
int hip_format_csr_edges    (spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const float* dA, int row0, int row1,
                             int fmt, int flags, char** dText, size_t* nbytes, spgemm_edge_write_stats* st);
int hip_format_csr_edges_f64(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const double* dA, int row0, int row1,
                             int fmt, int flags, char** dText, size_t* nbytes, spgemm_edge_write_stats* st);
/* the same into a caller's HOST buffer of cap bytes, brought down through the pinned lanes hip_CSR_SpMM uses.  buf == NULL:
 * only *nbytes, the size to allocate, is computed.  cap below the text's size -> SPGEMM_ERR_ARG. */
int hip_csr_to_edge_text    (spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const float* dA, int row0, int row1,
                             int fmt, int flags, char* buf, size_t cap, size_t* nbytes, spgemm_edge_write_stats* st);
int hip_csr_to_edge_text_f64(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const double* dA, int row0, int row1,
                             int fmt, int flags, char* buf, size_t cap, size_t* nbytes, spgemm_edge_write_stats* st);
/* the whole matrix into the file `path` (created or truncated): the header (0 / 1 / 2 as above, with "m n nnz" whatever
 * the flags; 2 sets ONE_BASED), then the body in slabs of at most SPGEMM_EDGE_SLAB bytes of text (environment, read per
 * call; default 64 MiB; a slab is a whole number of lines and may end anywhere inside a row).  A slab is formatted on the
 * device, brought down through the pinned lanes and handed to a second thread that fwrites it while the next slab is
 * formatted: device memory is bounded by the slab, and a text above INT32_MAX bytes is more slabs, not an error.
 * A path that cannot be opened for writing, or a failed write -> SPGEMM_ERR_ARG. */
int hip_write_edge_file     (spgemm_handle* h, const char* path, int m, int n, const int* dIA, const int* dJA, const float* dA,
                             int fmt, int flags, int header, spgemm_edge_write_stats* st);
int hip_write_edge_file_f64 (spgemm_handle* h, const char* path, int m, int n, const int* dIA, const int* dJA, const double* dA,
                             int fmt, int flags, int header, spgemm_edge_write_stats* st);

/* ---- workload statistics ----------------------------------------------------
 * std::vector<int> flopsStats(IA, JA, IB, JB, m) (nlibs/tools/stats.cc:29-55, pushToStats :3-12): 13 buckets of the
 * per-row product count of A*B; bucket i counts rows with 2^(i-1) < flops <= 2^i, bucket 0 rows with flops <= 1,
 * the last bucket rows above 2^11.  Device CSR arrays in, host histogram out. */
#define SPGEMM_STATS_LEN 13
int hip_flopsStats(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m, int stats[SPGEMM_STATS_LEN]);

/* vector<int> CSR::nnzStats() (nlibs/CSR.cc:241-248, pushToStats nlibs/tools/stats.cc:3-12): 18 power-of-two buckets of
 * the row lengths of a device CSR (dIA = rowPtr[m+1]). */
#define SPGEMM_NNZ_STATS_LEN 18
int hip_nnzStats(spgemm_handle* h, const int* dIA, int m, int stats[SPGEMM_NNZ_STATS_LEN]);

/* Per-bin correctness report: bool resultsComparison(CSR& hC, CSR& rC, const vector<int>& hv, const int* hqueue) with
 * isPartialRawEqual per bin (mindex2-cuda/nGpuSpMM.cc:85-240).  HOST arrays: hC = result under test, rC = reference
 * result (same shape m x n), hv/hqueue = bin boundaries and row queue as returned by hip_gpuFlopsClassify (queue copied
 * to the host).  report[b] describes reference bin b+1 (0 / 1 / 2-4 / 5-16 / 17-64 / 65-512 / >512 products):
 * rows compared, rows that differ (length, a column, or a value beyond `rel` relative), the first such row, and the
 * largest relative value error seen on common columns. */
typedef struct spgemm_bin_report {
  int rows;
  int rows_differ;
  int first_bad_row;        /* -1 if none */
  double max_rel_err;
} spgemm_bin_report;
int hip_resultsComparison(int m, int n, const int* hIC, const int* hJC, const float* hC,
                          const int* rIC, const int* rJC, const float* rC,
                          const int hv[SPGEMM_HV_LEN], int hv_len, const int* hqueue, double rel,
                          spgemm_bin_report report[SPGEMM_HV_LEN - 1]);

/* ---- helpers the reference's drivers use around the path --------------------------------------- */
/* CSR::makeOrdered on device arrays (nlibs/CSR.cc:73-86): sort every row by column, in place. */
int hip_csr_sort_rows(spgemm_handle* h, int m, const int* dIC, int* dJC, float* dC);

/* ---- reordering a device CSR: row / column permutations and the transpose --------------------------------------------
 * All arrays are device pointers; outputs come from the library pool (release with spgemm_hip_free); h == NULL = the
 * default handle; a call returns after the device work has completed.  Argument checks (null output, negative size,
 * nnz > 0 with null arrays -> SPGEMM_ERR_ARG) run before any device is touched.  Every value that becomes an address
 * (rowSrc, colMap, dP, rowPtr, a column renamed through colMap) is validated by a read-only pass that completes before
 * it is used: bad input -> SPGEMM_ERR_INPUT with a message, outputs NULL, the handle stays usable.
 *
 * hip_csr_permute: B = rows of A taken in the order rowSrc, columns renamed by colMap:
 *   row i of B = row rowSrc[i] of A, entries in A's in-row order; column c of A becomes colMap[c].
 * rowSrc == NULL / colMap == NULL: identity on that side (both NULL: a deep copy).
 * rowSrc must be a permutation of 0..m-1, colMap of 0..n-1.
 *   CSR::PM(P)   = (rowSrc = P,  colMap = NULL)      nlibs/CSR.cc:431-445
 *   CSR::MP(P)   = (rowSrc = NULL, colMap = P)       nlibs/CSR.cc:447-464
 *   CSR::PMPt(P) = (rowSrc = P,  colMap = Pt)        nlibs/CSR.cc:466-473   (square only)
 *   CSR::PtMP(P) = (rowSrc = Pt, colMap = P)         nlibs/CSR.cc:475-482   (square only)
 * One pass over the entries (PMPt builds no PM temporary).  Rows of B are not column-sorted after a column rename (as in
 * the reference); hip_csr_sort_rows does that. */
int hip_csr_permute(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                    const int* dRowSrc, const int* dColMap, int** dIB, int** dJB, float** dB);
int hip_csr_permute_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                        const int* dRowSrc, const int* dColMap, int** dIB, int** dJB, double** dB);

/* permutationTranspose (nlibs/tools/util.cc:162-168): dPt[dP[i]] = i, dPt caller-allocated int[len];
 * dP not a permutation of 0..len-1 -> SPGEMM_ERR_INPUT and dPt is not written */
int hip_permutation_transpose(spgemm_handle* h, int len, const int* dP, int* dPt);

/* CSR::rowDescendingOrderPermutation (nlibs/CSR.cc:484-494): *dP = int[m], rows by descending length.
 * Rows of equal length keep ascending row id (the reference's key_value_qsort is unstable: its tie order is no contract). */
int hip_csr_row_descending_permutation(spgemm_handle* h, int m, const int* dIA, int** dP);

/* T = A^T: dIT[n+1], dJT[nnz], dAT[nnz] (the transposed load readSNAPFile(isTrans), nlibs/COO.h:19, for any device CSR).
 * Stable: row c of T holds the entries of column c of A in A's storage order, so its row ids ascend, and entries with the
 * same row id keep their order.  T is column-sorted whenever no row of A repeats a column, whether or not A's rows were
 * sorted.  A column outside [0,n) -> SPGEMM_ERR_INPUT. */
int hip_csr_transpose(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                      int** dIT, int** dJT, float** dAT);
int hip_csr_transpose_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                          int** dIT, int** dJT, double** dAT);

/* ---- comparing two device CSRs: diff report, differs, differsStats -------------------------------------------------------
 * All CSR arrays are device pointers, reports and counts are host memory; h == NULL = the default handle; a call returns
 * after the device work has completed.  Argument checks (null out / counts, negative size, null rowPtr, nnz > 0 with null
 * arrays, npercents outside [0,64], npercents > 0 with null percents, a negative or NaN tolerance -> SPGEMM_ERR_ARG) run
 * before any device is touched.  A and B are both m x n with every row strictly ascending by column (hip_csr_sort_rows
 * gives that for a row without repeated columns).  Both rowPtr arrays are validated by a read-only pass that completes
 * before a rowPtr value becomes an address; columns are only compared.  A bad rowPtr, or a row that is not strictly
 * ascending -> SPGEMM_ERR_INPUT with a message, the report is left zeroed, the handle stays usable.  m == 0 or two empty
 * matrices are valid: a zeroed report with the first_* fields at -1.
 *
 * One report serves the reference's comparisons (B is the reference side, as in CSR::isRelativeEqual):
 *   CSR::differs          nlibs/CSR.cc:210-240    sum_sq
 *   CSR::isEqual          nlibs/CSR.h:195-245     same shape and nnz, rows_len_differ == 0, max_abs_err <= 1e-7 and
 *                                                 max_abs_only_b <= 1e-7
 *   CSR::isRelativeEqual  nlibs/CSR.h:284-320     rel_tol = maxRelativeError, abs_tol = 1e-8: beyond == 0 and
 *                                                 max_abs_only_b <= 1e-8
 *   the parity rule       (the end-of-run check Mt.makeOrdered(); oMt.makeOrdered(); Mt.isEqual(oMt), nrmcl.cc:26-28, on
 *                         device arrays)          rows_len_differ == only_a == only_b == beyond == 0 with abs_tol = 0
 * Every term is computed in double from the stored values.  sum_sq is reduced in a fixed order without floating-point
 * atomics: two calls on the same input return the same bits. */
typedef struct spgemm_csr_diff {
  int       rows_len_differ;   /* rows whose lengths differ                                  */
  int       first_len_row;     /* lowest such row, -1 if none                                */
  long long only_a, only_b;    /* entries whose column is absent from the same row of the other matrix */
  int       first_only_row;    /* lowest row holding one, -1                                 */
  long long beyond;            /* common columns with !(|a-b| <= abs_tol + rel_tol*|b|): a NaN on either side counts */
  int       first_beyond_row;  /* lowest such row, -1                                        */
  double    max_abs_err;       /* over common columns, |a-b| (NaN terms skipped)             */
  double    max_rel_err;       /* over common columns with b != 0, |a-b|/|b| (NaN skipped)   */
  double    max_abs_only_a, max_abs_only_b;  /* largest |value| among only_a / only_b entries, 0 if none */
  double    sum_sq;            /* CSR::differs: sum (a-b)^2 over common + a^2 over only_a + b^2 over only_b */
} spgemm_csr_diff;
int hip_csr_diff(spgemm_handle* h, int m, int n,
                 const int* dIA, const int* dJA, const float* dA, int nnzA,
                 const int* dIB, const int* dJB, const float* dB, int nnzB,
                 double rel_tol, double abs_tol, spgemm_csr_diff* out);
int hip_csr_diff_f64(spgemm_handle* h, int m, int n,
                     const int* dIA, const int* dJA, const double* dA, int nnzA,
                     const int* dIB, const int* dJB, const double* dB, int nnzB,
                     double rel_tol, double abs_tol, spgemm_csr_diff* out);

/* CSR::differsStats (nlibs/CSR.cc:381-415) from the two device rowPtr arrays alone: counts[npercents + 4] (host).  Row by
 * row with acount / bcount the lengths in A / B: acount == 0 && bcount > 0 -> slot n+1; both zero -> slot n+2; equal ->
 * slot n+3; otherwise percent = (bcount - acount) / (QValue)acount goes to the first k with percent < percents[k], else
 * to slot n (n = npercents <= 64; percents is a host array).  The division and the compare are done in float here and in
 * double in the _f64 twin, as QValue is.  The rowPtr values are only subtracted. */
int hip_csr_differsStats(spgemm_handle* h, int m, const int* dIA, const int* dIB,
                         const float* percents, int npercents, int* counts);
int hip_csr_differsStats_f64(spgemm_handle* h, int m, const int* dIA, const int* dIB,
                             const double* percents, int npercents, int* counts);

/* ---- column-partitioned CSR (PCSR): split into column blocks, blockwise product, join ---------------------------------
 * All CSR arrays are device pointers; blockPtr, the block tables (arrays of c device pointers / c counts) and the result
 * counts are host memory; h == NULL = the default handle; a call returns after the device work has completed; outputs
 * come from the library pool (release with spgemm_hip_free).  Argument checks (c outside [1, SPGEMM_PCSR_MAX_BLOCKS], a
 * null output or table, a negative size, nnz > 0 with null arrays -> SPGEMM_ERR_ARG; c * (m + 1) or a total nnz beyond
 * int32 -> SPGEMM_ERR_OVERFLOW) run before any device is touched.  Every value that becomes an address (rowPtr, the
 * column that selects a block) is validated by a read-only pass whose flag the host reads before it is used: bad input
 * -> SPGEMM_ERR_INPUT with a message.  On any error the outputs are NULL, nothing stays allocated, the handle stays usable.
 *
 * The layout is the reference's PCSR (nlibs/PCSR.h:5-10): stride = (n + c - 1) / c (1 when n == 0); an entry with column
 * col belongs to block b = col / stride, its block-local column is col - b * stride; every block is an m x stride CSR. */
#define SPGEMM_PCSR_MAX_BLOCKS 64

/* PCSR::PCSR(const CSR& csr, const int c) (nlibs/PCSR.cc:3-56), the same packed arrays:
 *   *dIP       device int[c * (m + 1)]: block b's rowPtr at b * (m + 1); it starts at 0 and ends at the block's nnz
 *   *dJP, *dP  device, nnz entries each: block b's at blockPtr[b] (local columns)
 *   blockPtr   host int[c + 1]
 * Inside a block the entries are in row order, inside a row in A's storage order (the split is stable); A's rows need
 * not be sorted and may repeat a column.  Block b is formed by pointer arithmetic (dIP + b * (m + 1), dJP + blockPtr[b],
 * dP + blockPtr[b], nnz = blockPtr[b + 1] - blockPtr[b]); as PCSR::dispose (nlibs/PCSR.h:39-50) frees the base arrays
 * only, a caller releases only the three base pointers.  m == 0 or nnz == 0: every rowPtr zero; c > n: the trailing
 * blocks are empty.  A bad rowPtr or a column outside [0, n) -> SPGEMM_ERR_INPUT. */
int hip_csr_split_columns(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                          int c, int** dIP, int** dJP, float** dP, int* blockPtr);
int hip_csr_split_columns_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                              int c, int** dIP, int** dJP, double** dP, int* blockPtr);

/* The inverse view, the row walk of PCSR::isEqual (nlibs/PCSR.h:69-86) written out as a CSR: c device CSRs of shape
 * m x stride (dIB[b], dJB[b], dB[b], nnzB[b]; separate allocations, as a product loop leaves them, or views into a
 * packed split) become one m x n CSR.  Row i of the result is block 0's row i, then block 1's, and so on; each block's
 * in-row order is kept; block b's columns gain b * stride.  join(split(A)) is therefore A with every row stably
 * partitioned by block: A itself, bit for bit, whenever A's rows are column-sorted.  Every block's rowPtr is validated
 * against its count; a local column outside [0, stride) or a global column >= n -> SPGEMM_ERR_INPUT (the result would
 * not be a valid CSR). */
int hip_pcsr_join(spgemm_handle* h, int m, int n, int c, const int* const* dIB, const int* const* dJB,
                  const float* const* dB, const int* nnzB, int** dIC, int** dJC, float** dC, int* nnzC);
int hip_pcsr_join_f64(spgemm_handle* h, int m, int n, int c, const int* const* dIB, const int* const* dJB,
                      const double* const* dB, const int* nnzB, int** dIC, int** dJC, double** dC, int* nnzC);

/* PCSR spmm(const CSR& A, const PCSR& pB, stride) (correctTests/pcsrTest.cc:7-19): C_b = A * B_b for the c blocks of a
 * k x n matrix B (each k x stride, given as for hip_pcsr_join); A is m x k.  dIC, dJC, dC, nnzC are host arrays of
 * length c; every C_b (m x stride, local columns, rows unsorted) is its own allocation.  It is a host loop of c calls of
 * hip_gpuSpMM / hip_gpuSpMM_f64 on the same handle, no product kernel of its own.  If block b fails, the earlier
 * results are freed, every output slot is NULL and the failing block's status is returned.  spgemm_hip_get_stats
 * afterwards describes the LAST block's product only. */
int hip_pcsr_spmm(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA, int m, int k, int n, int c,
                  const int* const* dIB, const int* const* dJB, const float* const* dB, const int* nnzB,
                  int** dIC, int** dJC, float** dC, int* nnzC);
int hip_pcsr_spmm_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA, int m, int k, int n, int c,
                      const int* const* dIB, const int* const* dJB, const double* const* dB, const int* nnzB,
                      int** dIC, int** dJC, double** dC, int* nnzC);

/* ---- blocked CSR (BCSR): a CSR as r x c dense tiles, and back ------------------------------------------------------------
 * All CSR / BCSR arrays are device pointers, the counts are host memory; h == NULL = the default handle; a call returns
 * after the device work has completed; outputs come from the library pool (release with spgemm_hip_free).  Argument
 * checks (r < 1, c < 1, r * c > SPGEMM_BCSR_MAX_TILE, a null output, a negative size, a count > 0 with null arrays, a
 * negative or NaN drop_tol -> SPGEMM_ERR_ARG) run before any device is touched.  Every value that becomes an address
 * (rowPtr, the columns, the block columns) is validated by a read-only pass whose flag the host reads before it is used:
 * bad input -> SPGEMM_ERR_INPUT with a message.  On any error the outputs are NULL, nothing stays allocated, the handle
 * stays usable.
 *
 * r (tile rows) comes before c (tile columns), as in the reference's definition BCSR::BCSR(csr, r, c) (nlibs/BCSR.cc:3);
 * its header declares the two the other way round (nlibs/BCSR.h:15), the definition is what runs.
 * bm = ceil(m / r) block rows, bn = ceil(n / c) block columns; r > m and c > n are valid (one block row / column). */
#define SPGEMM_BCSR_MAX_TILE 4096      /* r >= 1, c >= 1, r * c <= 4096 */

/* BCSR::BCSR(const CSR&, r, c) (nlibs/BCSR.cc:3-65), the same three arrays:
 *   *dIB   device int[bm + 1]: starts at 0, ends at *nnzb
 *   *dJB   device int[nnzb]: block columns
 *   *dB    device, nnzb * r * c values: tile k at k * r * c, entry (i, col) in cell (i % r) * c + col % c; every cell no
 *          entry lands in is +0.0, the cells of a ragged last block row / block column included
 * The tiles of a block row are in first-occurrence order: the reference walks the block row's rows in ascending order,
 * each in A's storage order, and appends a block column when it first meets it -- ascending only when A's rows are
 * column-sorted and r == 1.  Of a repeated (row, col) the last in storage order stays, as the sequential loop leaves it
 * (deterministic: no two stores aim at one cell).  Values are moved, not computed: NaN payloads, -0.0 and denormals keep
 * their bits.  A's rows need not be sorted.  m == 0 or nnz == 0: rowPtr all zero, *nnzb = 0.  A bad rowPtr or a column
 * outside [0, n) -> SPGEMM_ERR_INPUT.  nnzb * r * c > INT32_MAX -> SPGEMM_ERR_OVERFLOW (known only after the count
 * pass; everything is released). */
int hip_csr_to_bcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                    int r, int c, int** dIB, int** dJB, float** dB, int* nnzb);
int hip_csr_to_bcsr_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                        int r, int c, int** dIB, int** dJB, double** dB, int* nnzb);

/* The row walk of BCSR::isEqual (nlibs/BCSR.cc:67-116) written out as a CSR.  Row i (bi = i / r, ei = i % r) is: the
 * tiles of block row bi in storage order, in each tile ej = 0 .. c-1, every cell whose global column bcol * c + ej is
 * below n and whose value has fabs((double)v) > drop_tol.  NaN, +-0 and anything at or below the tolerance are dropped
 * (isEqual's `> 1e-9`); drop_tol = 0 keeps every nonzero non-NaN cell; kept values keep their bits.  The BCSR rowPtr is
 * validated against nnzb and every block column against [0, bn): a violation -> SPGEMM_ERR_INPUT.  A block column
 * repeated inside a block row is no error: the row then repeats columns.  More than INT32_MAX kept cells ->
 * SPGEMM_ERR_OVERFLOW.  For a column-sorted A without repeated columns and no |value| <= drop_tol,
 * hip_csr_sort_rows(hip_bcsr_to_csr(hip_csr_to_bcsr(A))) is A bit for bit; unsorted it is A with every row stably
 * grouped by tile in first-occurrence order, ascending inside a tile. */
int hip_bcsr_to_csr(spgemm_handle* h, int m, int n, int r, int c, int nnzb, const int* dIB, const int* dJB,
                    const float* dB, double drop_tol, int** dIC, int** dJC, float** dC, int* nnzC);
int hip_bcsr_to_csr_f64(spgemm_handle* h, int m, int n, int r, int c, int nnzb, const int* dIB, const int* dJB,
                        const double* dB, double drop_tol, int** dIC, int** dJC, double** dC, int* nnzC);

/* ---- mixed CSR (MCSR): the top-left corner as r x c dense tiles, the rest as a CSR, and back -----------------------------
 * All arrays are device pointers, the counts are host memory; h == NULL = the default handle; a call returns after the
 * device work has completed; outputs come from the library pool (release with spgemm_hip_free).  Argument checks (the
 * tile rules of hip_csr_to_bcsr; blockRows outside [0, m]; blockCols outside [0, n]; blockRows % r != 0, the reference's
 * assert at nlibs/MCSR.cc:15; a null output, a negative size, a count > 0 with null arrays, a negative or NaN drop_tol
 * -> SPGEMM_ERR_ARG) run before any device is touched.  Every value that becomes an address is validated by a read-only
 * pass whose flag the host reads before it is used: bad input -> SPGEMM_ERR_INPUT with a message.  On any error every
 * output is NULL, the counts are 0, nothing stays allocated, the handle stays usable.
 *
 * r comes before c as in the definition MCSR::MCSR(csr, r, c, blockRows, blockCols) (nlibs/MCSR.cc:3); the header
 * (nlibs/MCSR.h:7) declares the two the other way round.  blockCols need not be a multiple of c.
 * bm = blockRows / r block rows, bn = ceil(blockCols / c) block columns. */

/* The FILL pass of MCSR::MCSR (nlibs/MCSR.cc:58-92).  An entry (i, col) with i < blockRows and col < blockCols goes into
 * tile (i / r, col / c), cell (i % r) * c + col % c; every other entry stays in the remainder.
 *   *dIB, *dJB, *dB, *nnzb   exactly what hip_csr_to_bcsr returns for the blockRows x blockCols CSR made of the corner's
 *                            entries in A's storage order: int[bm + 1], int[nnzb] block columns, nnzb * r * c values; the
 *                            tiles of a block row in first-occurrence order; of a repeated (row, col) the last in storage
 *                            order stays; every other cell +0.0, the cells of a ragged last block column included (their
 *                            columns >= blockCols belong to the remainder); values keep their bits
 *   *dIR, *dJR, *dR, *nnzR   the remainder, an m x n CSR with global columns: row i < blockRows holds A's entries of row i
 *                            with col >= blockCols in storage order, row i >= blockRows is A's row unchanged
 * The number of entries that went to the corner, repeats counted, is nnz - *nnzR (the reference leaves BCSR::nnz at 0).
 * A's rows need not be sorted and may repeat a column.  m == 0, nnz == 0, blockRows == 0 or blockCols == 0 (no tiles, the
 * remainder is A) and a corner that covers the whole matrix (an empty remainder) are valid; the arrays of an empty part
 * follow hip_csr_to_bcsr (rowPtr all zero, the other two non-null placeholders).  A bad rowPtr or a column outside
 * [0, n) -> SPGEMM_ERR_INPUT.  nnzb * r * c > INT32_MAX -> SPGEMM_ERR_OVERFLOW.
 * Not reproduced: the reference's COUNT pass (nlibs/MCSR.cc:16-40) resets `top` per block row instead of per row, so for
 * r > 1 its remainder rowPtr over-counts whenever a row other than the last of its block row has remainder entries, and
 * its assert(nnz == top) fails; for r == 1 (its known-answer vectors, tests/MCSR_test.cc) the two passes agree. */
int hip_csr_to_mcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                    int r, int c, int blockRows, int blockCols,
                    int** dIB, int** dJB, float** dB, int* nnzb,
                    int** dIR, int** dJR, float** dR, int* nnzR);
int hip_csr_to_mcsr_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                        int r, int c, int blockRows, int blockCols,
                        int** dIB, int** dJB, double** dB, int* nnzb,
                        int** dIR, int** dJR, double** dR, int* nnzR);

/* The inverse (the reference has no MCSR::isEqual; this is the definition).  Row i < blockRows of the result is the
 * corner's row i followed by the remainder's row i; row i >= blockRows is the remainder's row.  The corner's row is
 * written out as hip_bcsr_to_csr does for a blockRows x blockCols BCSR: tiles in storage order, ej = 0 .. c-1, a cell kept
 * when its global column is below blockCols and fabs((double)v) > drop_tol; kept values keep their bits.  Validated, each
 * -> SPGEMM_ERR_INPUT: the block rowPtr against nnzb, every block column against [0, bn), the remainder's rowPtr against
 * nnzR, every remainder column against [0, n).  A remainder entry inside the corner's range is no error: the row then may
 * repeat a column.  More than INT32_MAX kept entries -> SPGEMM_ERR_OVERFLOW.  For a column-sorted A without repeated
 * columns and no |value| <= drop_tol the round trip is A bit for bit when r == 1, and A after hip_csr_sort_rows when
 * r > 1 (the tiles of a block row are in first-occurrence order over its r rows). */
int hip_mcsr_to_csr(spgemm_handle* h, int m, int n, int r, int c, int blockRows, int blockCols,
                    int nnzb, const int* dIB, const int* dJB, const float* dB,
                    int nnzR, const int* dIR, const int* dJR, const float* dR, double drop_tol,
                    int** dIC, int** dJC, float** dC, int* nnzC);
int hip_mcsr_to_csr_f64(spgemm_handle* h, int m, int n, int r, int c, int blockRows, int blockCols,
                        int nnzb, const int* dIB, const int* dJB, const double* dB,
                        int nnzR, const int* dIR, const int* dJR, const double* dR, double drop_tol,
                        int** dIC, int** dJC, double** dC, int* nnzC);

/* ---- dense matrix: a CSR written out as a dense array, a dense array as a CSR, and the dense product ----------------------
 * All matrix pointers are device pointers, the counts are host memory; h == NULL = the default handle; a call returns
 * after the device work has completed; CSR outputs come from the library pool (release with spgemm_hip_free).  Argument
 * checks (a null output, a negative size, a count > 0 with null arrays, ld below the columns, a rule outside {0, 1}, a
 * negative or NaN tol, C overlapping A or B -> SPGEMM_ERR_ARG) run before any device is touched.  Every value that
 * becomes an address (rowPtr, the columns) is validated by a read-only pass whose flag the host reads before it is used:
 * bad input -> SPGEMM_ERR_INPUT with a message.  On any error the outputs are NULL or untouched, nothing stays allocated,
 * the handle stays usable.
 *
 * A dense matrix is row-major with a leading dimension in elements: cell (i, j) is at i * ld + j, ld >= columns; the
 * cells [i][columns..ld) are padding that no call reads or writes.  Every dense offset is computed in 64 bits, so
 * rows * ld may exceed 2^31. */
#define SPGEMM_DENSE_KEEP_REFERENCE 0   /* keep unless (double)v < tol; tol = 1e-8 is CSR::initWithDenseMatrix */
#define SPGEMM_DENSE_KEEP_ABS       1   /* keep when fabs((double)v) > tol: the rule of hip_bcsr_to_csr */

/* DenseMatrix::DenseMatrix(const CSR&) (nlibs/DenseMatrix.h:6-21): zero-fill, then values[i * cols + col] = val in storage
 * order.  dD is the CALLER's m x ld buffer -- the one place where the library writes into memory it did not allocate, so
 * that a tensor another framework owns (its data_ptr()) is filled in place, without a copy out of the pool.  Every cell
 * [i][0..n) receives a value: +0.0 where no entry lands.  Values are moved, not computed: NaN payloads, -0.0 and denormals
 * keep their bits.  A's rows need not be sorted; of a repeated (row, col) the last in storage order stays, as the
 * reference's sequential loop leaves it (deterministic: no two stores aim at one cell).  rowPtr and the columns are
 * validated before anything is written: a bad rowPtr or a column outside [0, n) -> SPGEMM_ERR_INPUT, dD untouched.
 * m == 0, n == 0 and nnz == 0 are valid. */
int hip_csr_to_dense(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                     float* dD, long long ld);
int hip_csr_to_dense_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                         double* dD, long long ld);

/* CSR::initWithDenseMatrix (nlibs/CSR.h:54-82; its known-answer vectors: tests/CSR_test.cc:65-87): row i of the result
 * holds the kept cells of dense row i in ascending column order; kept values keep their bits.
 *   SPGEMM_DENSE_KEEP_REFERENCE  a cell is dropped when (double)v < tol.  With tol = 1e-8 this is the reference, exactly:
 *                                negative values are dropped; NaN is kept (NaN < tol is false); float(1e-8) is dropped
 *                                (promoted to double it is 9.99999993922529e-09, below 1e-8), the next float up is kept.
 *   SPGEMM_DENSE_KEEP_ABS        a cell is kept when fabs((double)v) > tol: NaN is dropped, negatives are kept; tol = 0
 *                                keeps every nonzero non-NaN cell.
 * More than INT32_MAX kept cells -> SPGEMM_ERR_OVERFLOW, decided from the 64-bit total of the count pass before any
 * output is allocated.  For a CSR with column-sorted rows, no repeated column and no dropped value,
 * hip_dense_to_csr(hip_csr_to_dense(A)) is A bit for bit.  m == 0 or n == 0: rowPtr all zero, *nnzC = 0. */
int hip_dense_to_csr(spgemm_handle* h, int m, int n, const float* dD, long long ld, int rule, double tol,
                     int** dIC, int** dJC, float** dC, int* nnzC);
int hip_dense_to_csr_f64(spgemm_handle* h, int m, int n, const double* dD, long long ld, int rule, double tol,
                         int** dIC, int** dJC, double** dC, int* nnzC);

/* C[m x n] = A[m x k] * B[k x n]: the cblas_dgemm(RowMajor, NoTrans, NoTrans, alpha 1, beta 0) of
 * correctTests/dense-somp.cc, on the matrix cores.  C is fully overwritten in [i][0..n); its padding is untouched.
 * C overlapping A or B (by address range) -> SPGEMM_ERR_ARG.  k == 0 gives all +0.0.  Zeros are multiplied like any
 * other value: unlike the SpGEMM, which never forms a product with an absent entry, 0 * inf gives NaN here.
 * Every C[i][j] is one accumulator over ascending k, starting from +0.0.
 *   float   c = fmaf(A[i][k], B[k][j], c) for k = 0 .. K-1, then fmaf(+0.0, +0.0, c) up to the next multiple of 32:
 *           bit for bit this host loop (the trailing steps change nothing but a -0.0 sum, which becomes +0.0).
 *   double  no order of rounding is promised; |C[i][j] - exact| <= k * 2^-53 * sum_k |A[i][k]| * |B[k][j]|. */
int hip_dense_gemm(spgemm_handle* h, int m, int n, int k, const float* dA, long long lda, const float* dB, long long ldb,
                   float* dC, long long ldc);
int hip_dense_gemm_f64(spgemm_handle* h, int m, int n, int k, const double* dA, long long lda, const double* dB,
                       long long ldb, double* dC, long long ldc);

/* ---- clusters from a finished R-MCL result: attractors, connected components, labels -> clusters ----------------------------
 * The reference stops at the flow matrix Mt (nlibs/qrmcl.cc:136-164); these calls read the clusters out of it on the
 * device.  Interpretation only: the R-MCL loop is not touched.  All CSR and label arrays are device pointers, the counts
 * are host memory; h == NULL = the default handle; a call returns after the device work has completed; array outputs
 * handed out as int** come from the library pool (release with spgemm_hip_free).  Argument checks (m != n, a null
 * output, a negative size, nnz > 0 with null arrays -> SPGEMM_ERR_ARG) run before any device is touched.  Every value
 * that becomes an address (rowPtr, the columns, the labels) is validated by a read-only pass whose flag the host reads
 * before it is used: bad input -> SPGEMM_ERR_INPUT with a message.  On any error the int** outputs are NULL, nothing
 * stays allocated, the handle stays usable.  Every result is integers and the same on every call. */
#define SPGEMM_CC_MAX_ROUNDS 64   /* hard cap of hip_csr_connected_components; at most ceil(log2 m) + 1 are needed */

/* Row i of Mt holds the flow out of node i; dParent[i] (caller's int[m]) = the column of the largest value of row i.
 * The rule does not depend on the storage order of a row (product rows are not column-sorted): an entry (v, c) beats
 * the best so far (bv, bc) iff v > bv, or v == bv and c < bc, starting from (-inf, INT_MAX).  So: of equal maxima the
 * smallest column wins; a NaN never wins; -0.0 == +0.0 and the smaller column wins between them; a row of only -inf
 * gives its smallest column; an empty row and an all-NaN row give dParent[i] = i.  Values are compared in their own
 * type: the _f64 twin does not pass through float.  m != n -> SPGEMM_ERR_ARG; a bad rowPtr or a column outside [0, n)
 * -> SPGEMM_ERR_INPUT, dParent untouched.  m == 0 is valid.
 * hip_rmcl_attractor_lanes: the lanes per row (4, 16 or 64) the kernels use for an m-row matrix with nnz entries. */
int hip_rmcl_attractors    (spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                            int* dParent);
int hip_rmcl_attractors_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                            int* dParent);
int hip_rmcl_attractor_lanes(int m, int nnz);

/* Weakly connected components of a square CSR pattern: every stored entry (i, j) is an undirected edge, values are not
 * read, self loops and repeated entries are harmless.  dLabel[v] (caller's int[m]) = the smallest vertex id of v's
 * component: canonical, equal bit for bit to any correct host implementation.  *ncomp = the number of v with
 * dLabel[v] == v; *rounds (may be NULL) = hook-and-shortcut rounds taken, >= 1 for m > 0, the last of them changed
 * nothing.  More than SPGEMM_CC_MAX_ROUNDS rounds -> SPGEMM_ERR_INTERNAL (never a spin).  m != n -> SPGEMM_ERR_ARG; a bad
 * rowPtr or a column outside [0, n) -> SPGEMM_ERR_INPUT, dLabel untouched.  m == 0: *ncomp = 0, *rounds = 0. */
int hip_csr_connected_components(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, int* dLabel,
                                 int* ncomp, int* rounds);

/* dLabel must be canonical (label[v] <= v and label[label[v]] == label[v], what hip_csr_connected_components writes):
 * anything else -> SPGEMM_ERR_INPUT.  Clusters are numbered 0 .. *k - 1 in ascending order of their smallest member.
 * (*dCluster)[v] = the number of v's cluster, int[m]; (*dClusterPtr)[c] .. [c + 1] = the range of cluster c in
 * *dMembers, int[*k + 1] with [*k] == m; *dMembers = the vertices cluster by cluster, ascending inside a cluster, int[m].
 * Cluster sizes are the differences of *dClusterPtr.  m == 0: *k = 0, (*dClusterPtr)[0] = 0. */
int hip_labels_to_clusters(spgemm_handle* h, int m, const int* dLabel, int* k, int** dCluster, int** dClusterPtr,
                           int** dMembers);

/* The three chained: attractors of Mt, components of the functional graph i -> dParent[i] (the CSR with rowPtr 0..m),
 * labels to clusters.  A node joins its attractor; attractors that point at each other form one cluster. */
int hip_rmcl_clusters    (spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA, int* k,
                          int** dCluster, int** dClusterPtr, int** dMembers);
int hip_rmcl_clusters_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA, int* k,
                          int** dCluster, int** dClusterPtr, int** dMembers);

/* ---- sparse add and the symmetrisation of a directed graph --------------------------------------------------------------
 * (R-)MCL is defined on undirected graphs; the reference's loader only transposes (readSNAPFile(isTrans), nlibs/COO.h:19).
 * These calls make a directed graph undirected on the device, in front of hip_coo_to_csr's rmclInit flags and
 * hip_gpuRmclIter_device.  Every entry point has a _f64 twin.  All arrays are device pointers; array outputs handed out
 * as int** / float** come from the library pool (release with spgemm_hip_free); h == NULL = the default handle; a call
 * returns after its device work has completed.  Argument checks (a null output pointer, a negative size, nnz > 0 with
 * null arrays, a NaN alpha / beta / exponent, an unknown mode -> SPGEMM_ERR_ARG) run before any device is touched.  Every
 * value that becomes an address (rowPtr, a column that indexes a scale or a count) is validated by a read-only pass that
 * completes before it is used: bad input -> SPGEMM_ERR_INPUT with a message, outputs NULL, the handle stays usable.
 *
 * hip_csr_add: C = alpha*A + beta*B.  A and B are m x n with every row strictly ascending by column (what hip_coo_to_csr
 * with SPGEMM_COO_DEDUPE, hip_csr_transpose and hip_csr_sort_rows produce; the contract of hip_csr_diff), checked in the
 * pass itself: an unsorted row, a repeated column or a column outside [0,n) -> SPGEMM_ERR_INPUT.  C holds the union of
 * the two patterns, rows strictly ascending; an entry whose sum is zero stays (the structure depends on the patterns
 * only).  alpha and beta are converted once to the value type V; values are computed with one rounding per operation
 * (no fused multiply-add): V(alpha)*a + V(beta)*b on a common column, V(alpha)*a / V(beta)*b on a column of one operand.
 * No floating-point atomic: two calls return the same bits.  nnz(C) is totalled in 64 bits; above INT_MAX ->
 * SPGEMM_ERR_OVERFLOW.  m == 0 and two empty operands are valid. */
int hip_csr_add(spgemm_handle* h, int m, int n,
                double alpha, const int* dIA, const int* dJA, const float* dA, int nnzA,
                double beta, const int* dIB, const int* dJB, const float* dB, int nnzB,
                int** dIC, int** dJC, float** dC, int* nnzC);
int hip_csr_add_f64(spgemm_handle* h, int m, int n,
                    double alpha, const int* dIA, const int* dJA, const double* dA, int nnzA,
                    double beta, const int* dIB, const int* dJB, const double* dB, int nnzB,
                    int** dIC, int** dJC, double** dC, int* nnzC);

/* dOut[j] = (dRowScale[r] * dA[j]) * dColScale[dJA[j]] for entry j of row r: the row factor first, then the column
 * factor.  Either scale may be NULL (= 1, that multiplication is not done).  dOut (the caller's V[nnz]) may be dA.  The
 * structure is not touched.  With a dColScale the columns are validated (they index it): outside [0,n) ->
 * SPGEMM_ERR_INPUT, dOut untouched. */
int hip_csr_scale(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                  const float* dRowScale, const float* dColScale, float* dOut);
int hip_csr_scale_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                      const double* dRowScale, const double* dColScale, double* dOut);

/* dCount[c] (the caller's int[n]) = the number of entries with column c: the in-degree (the out-degree is the row
 * length).  Integer atomics: the same on every call.  A column outside [0,n) -> SPGEMM_ERR_INPUT, dCount untouched. */
int hip_csr_col_counts(spgemm_handle* h, int n, int nnz, const int* dJA, int* dCount);

/* dOut[i] = V(pow((double)dCount[i], -exponent)), and 0 where the count is 0 (or negative).  A count of 1 gives 1.  Not
 * promised bit-equal to a host pow. */
int hip_degree_factors(spgemm_handle* h, int len, const int* dCount, double exponent, float* dOut);
int hip_degree_factors_f64(spgemm_handle* h, int len, const int* dCount, double exponent, double* dOut);

/* S = a symmetric matrix built from the square m x m A, whose rows must be strictly ascending by column (checked:
 * SPGEMM_ERR_INPUT otherwise).  S has strictly ascending rows and a symmetric pattern.
 *   SPGEMM_SYM_SUM                A + A^T: hip_csr_transpose, then hip_csr_add(1, A, 1, A^T).  The values are symmetric bit
 *                                 for bit; a diagonal entry is doubled, an edge stored in both directions is summed.
 *   SPGEMM_SYM_BIBLIOMETRIC       A*A^T + A^T*A: the transpose, two hip_gpuSpMM, hip_csr_sort_rows on both products, the add.
 *   SPGEMM_SYM_DEGREE_DISCOUNTED  Do^-alpha A Di^-beta A^T Do^-alpha + Di^-beta A^T Do^-alpha A Di^-beta with Do / Di the
 *                                 diagonal matrices of the out- / in-degree COUNTS (alpha = beta = 0.5 is the published
 *                                 default), computed as Y*Y^T + Z^T*Z with Y = Do^-alpha A Di^(-beta/2) and
 *                                 Z = Do^(-alpha/2) A Di^-beta through hip_csr_col_counts, hip_degree_factors and
 *                                 hip_csr_scale.
 * alpha and beta are read by SPGEMM_SYM_DEGREE_DISCOUNTED only (a NaN there -> SPGEMM_ERR_ARG).  Temporaries go back to the
 * pool when the call ends.  The two product modes densify hub-heavy graphs: a node with d in-links makes d*d entries of
 * A^T*A.  The size of S is the caller's concern; the int32 refusal of the product (SPGEMM_ERR_OVERFLOW) applies. */
#define SPGEMM_SYM_SUM               0
#define SPGEMM_SYM_BIBLIOMETRIC      1
#define SPGEMM_SYM_DEGREE_DISCOUNTED 2
int hip_csr_symmetrize(spgemm_handle* h, int mode, double alpha, double beta, int m,
                       const int* dIA, const int* dJA, const float* dA, int nnz,
                       int** dIS, int** dJS, float** dS, int* nnzS);
int hip_csr_symmetrize_f64(spgemm_handle* h, int mode, double alpha, double beta, int m,
                           const int* dIA, const int* dJA, const double* dA, int nnz,
                           int** dIS, int** dJS, double** dS, int* nnzS);

/* ---- selection: the k largest entries of every row (mcl's -S, HipMCL's select), and the R-MCL loop with that row cap ----
 * The reference has no counterpart (its row rule only thresholds); the semantics are pinned by tests/topk_ref.py.  All
 * arrays are device pointers; array outputs come from the library pool (release with spgemm_hip_free); h == NULL = the
 * default handle; a call returns after its device work has completed.  Argument checks (a null output other than rowsCut,
 * k < 1, a flag bit other than SPGEMM_TOPK_NORMALISE, negative sizes, null arrays) -> SPGEMM_ERR_ARG before any device
 * work, with the outputs null / 0; a rowPtr that is not a monotone row pointer ending at nnz or a column outside [0,n)
 * -> SPGEMM_ERR_INPUT.
 *
 * hip_csr_row_topk: row i of N keeps the min(len_i, k) best entries of row i of A IN THEIR STORAGE ORDER.  Entry a beats
 * entry b iff va > vb, or va == vb and ca < cb, or both are equal and a is stored before b (rows may repeat a column).
 * Values are compared in their own type.  -0.0 == +0.0 (the column decides); a NaN ranks below every number, -inf
 * included, and among NaNs the column decides, then the position.  A row with len_i <= k is copied bit for bit (NaN
 * payloads, -0.0, denormals), so k >= the longest row returns a bit-identical copy.  *rowsCut (optional) = the rows with
 * len_i > k.  SPGEMM_TOPK_NORMALISE divides the kept values of the CUT rows, and of those only, by their sum: the sum is
 * formed in double for both value types in a fixed reduction tree (the same bits on every call), rounded to the value
 * type, and divides each kept value by one IEEE division in the value type.  That is meant for kept values that are
 * finite and non-negative with a positive sum; otherwise the values are whatever the division gives, and no error is
 * raised.  Selection, not a sort; no floating-point atomic.
 * hip_csr_row_topk_limits (pure host): rows of up to *waveCap entries are cut by one wave each with the row in registers,
 * rows of up to *blockCap entries by one block each with the row in LDS, longer rows by a block that re-reads them.
 * spgemm_hip_debug_topk_paths (test hook): the rows hip_csr_row_topk has handled on this handle since it was created:
 * copied uncut, cut by the wave / block / stream path (any pointer may be NULL).
 *
 * hip_gpuRmclIter_device_topk: hip_gpuRmclIter_device with a row cap.  Every iteration is
 * X = hip_rmcl_expand_prune(Mgt, Mt), Mt = hip_csr_row_topk(X, k, SPGEMM_TOPK_NORMALISE): composed from the packed public
 * step, so Mt is packed after every iteration.  iterNnz / iterCut: the caller's arrays of maxIter entries, or NULL: the
 * entries of Mt after the selection of iteration i and the rows it cut.  maxIter == 0 returns a copy of Mt.  k < 1 ->
 * SPGEMM_ERR_ARG; otherwise the argument checks of hip_gpuRmclIter_device. */
#define SPGEMM_TOPK_NORMALISE 1
int hip_csr_row_topk(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                     int k, int flags, int** dIN, int** dJN, float** dAN, int* nnzN, int* rowsCut);
int hip_csr_row_topk_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                         int k, int flags, int** dIN, int** dJN, double** dAN, int* nnzN, int* rowsCut);
int hip_csr_row_topk_limits(int isDouble, int* waveCap, int* blockCap);
int spgemm_hip_debug_topk_paths(spgemm_handle* h, long long* copied, long long* wave, long long* block, long long* stream);
int hip_gpuRmclIter_device_topk(spgemm_handle* h, int maxIter, int k, int rows, int cols,
                                const int* dgI, const int* dgJ, const float* dgA, int gnnz,
                                const int* dtI, const int* dtJ, const float* dtA, int tnnz,
                                int** oI, int** oJ, float** oA, int* onnz, long long* iterNnz, long long* iterCut);
int hip_gpuRmclIter_device_topk_f64(spgemm_handle* h, int maxIter, int k, int rows, int cols,
                                    const int* dgI, const int* dgJ, const double* dgA, int gnnz,
                                    const int* dtI, const int* dtJ, const double* dtA, int tnnz,
                                    int** oI, int** oJ, double** oA, int* onnz, long long* iterNnz, long long* iterCut);

/* ---- (5) double values: the reference built with FDOUBLE (QValue double, nlibs/tools/macro.h:3-6) ----------------------
 * The same semantics as the float twins above (argument checks, status codes, h == NULL = the default handle, outputs
 * from the library pool / malloc(), rows of C column-unsorted); only the value type differs.  The classification,
 * symbolic pass and scan are shared with the float path (they read the structure only), so C's structure is the float
 * call's; the numeric kernels accumulate in double.  spgemm_stats is filled as for a float call: f64 numeric launches are
 * timed into the SPGEMM_K_NUM_* slot of their bin (SPGEMM_NKERNELS and the struct layout are unchanged).
 * R-MCL in double (prune, fused step, loop on one device) is declared at the end of this section.
 * Not available in double: multi-GPU (sharded SpGEMM and sharded R-MCL), hip_sgpuSpMM / hip_gpuFlopsClassify, mixed
 * precision (float in, double accumulate).
 * Measured on one MI355X: a double call takes 2.0x the float call on the 1 M-row power-law A*A,
 * 1.45x on the web-graph surrogate. */
/* CSR gpuSpMMWrapper for QValue double: cusparseDcsrgemm (nlibs/gpus/cusparse_spmm.cc:73).  Never takes the opt-in
 * SPGEMM_PATH kernels. */
int hip_gpuSpMM_f64(spgemm_handle* h,
                    const int* dIA, const int* dJA, const double* dA, int nnzA,
                    const int* dIB, const int* dJB, const double* dB, int nnzB,
                    int m, int k, int n, int** dIC, int** dJC, double** dC, int* nnzC);
/* numeric phase in double after hip_spgemm_symbolic on the same handle (one symbolic phase may be followed by either
 * hip_spgemm_numeric or this); without a matching symbolic phase: SPGEMM_ERR_ARG */
int hip_spgemm_numeric_f64(spgemm_handle* h,
                           const int* dIA, const int* dJA, const double* dA, int nnzA,
                           const int* dIB, const int* dJB, const double* dB, int nnzB,
                           int m, int k, int n, const int* dIC, int* dJC, double* dC);
/* host arrays in, malloc()ed host arrays out: the *_CSR_SpMM family with QValue double, mkl_dcsrmultcsr
 * (nlibs/mkls/mkl_csr_kernel.cc:12,36); fills spgemm_hip_host_api_stats like hip_CSR_SpMM */
int hip_CSR_SpMM_f64(const int* IA, const int* JA, const double* A, int nnzA,
                     const int* IB, const int* JB, const double* B, int nnzB,
                     int** IC, int** JC, double** C, int* nnzC, int m, int k, int n);
/* CSR::makeOrdered with double values (nlibs/CSR.cc:73-86) */
int hip_csr_sort_rows_f64(spgemm_handle* h, int m, const int* dIC, int* dJC, double* dC);

/* R-MCL with QValue double: the contracts of hip_rmcl_prune / _n, hip_rmcl_expand_prune, hip_gpuRmclIter_device and
 * hip_gpuRmclIter above (argument checks and status codes, h == NULL = the default handle, outputs from the pool, inputs
 * not modified, rows column-unsorted, maxIter == 0 returns a copy, a square matrix is required).  The row rule is
 * nlibs/tools/util.cc:4-69 / nlibs/qrmcl.cc:96-117 with every operation in double: v*v, row max and row sum,
 * thresh = 0.90*avg*(1 - 2*(max - avg)) with avg = sum / stored entries, raised to 1e-7, lowered to max; keep v*v >= thresh;
 * kept squares divided by their sum.  hip_rmcl_prune_f64 keeps the kept entries in input order.  The fused step always
 * runs the symbolic pass (its scratch C has nnz(C) entries); the loop packs Mt after every iteration.
 * hip_gpuRmclIter_f64 takes host arrays, returns malloc()ed arrays and runs on one device: SPGEMM_RMCL_DEVICES is ignored. */
int hip_rmcl_prune_f64(spgemm_handle* h, int m, const int* dIC, const int* dJC, const double* dC,
                       int** dIN, int** dJN, double** dCN, int* nnzN);
int hip_rmcl_prune_n_f64(spgemm_handle* h, int m, int nnz, const int* dIC, const int* dJC, const double* dC,
                         int** dIN, int** dJN, double** dCN, int* nnzN);
int hip_rmcl_expand_prune_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA,
                              const int* dIB, const int* dJB, const double* dB, int nnzB, int m, int k, int n,
                              int** dIN, int** dJN, double** dCN, int* nnzN);
int hip_gpuRmclIter_device_f64(spgemm_handle* h, int maxIter, int rows, int cols,
                               const int* dgI, const int* dgJ, const double* dgA, int gnnz,
                               const int* dtI, const int* dtJ, const double* dtA, int tnnz,
                               int** oI, int** oJ, double** oA, int* onnz);
int hip_gpuRmclIter_f64(int maxIter, int rows, int cols, const int* gIA, const int* gJA, const double* gA, int gnnz,
                        const int* tIA, const int* tJA, const double* tA, int tnnz,
                        int** oIA, int** oJA, double** oA, int* onnz);

/* device self-test of the wave/block primitives (scans, ballots); returns SPGEMM_OK or INTERNAL */
int spgemm_hip_selftest(spgemm_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* SPGEMM_HIP_H_ */
