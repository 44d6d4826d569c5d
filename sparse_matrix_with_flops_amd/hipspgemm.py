"""ctypes binding of libspgemm_hip.so (include/spgemm_hip.h) + a thin Python mirror of the
reference's host-side call surface for the SpGEMM path.

Mirrors (reference file:line):
  CSR                         struct CSR                       nlibs/CSR.h:23-50
  CSR.hip_spmm(B)             CSR::spmm / omp_spmm / ...       nlibs/CSR.cc:59-208   (host in, host out)
  CSR.toGpuCSR / toCpuCSR / deviceDispose                      nlibs/CSR.cc:342-379
  gpuSpMMWrapper(dA, dB)      gpuSpMMWrapper                   nlibs/gpus/gpu_csr_kernel.cu:128-173
  gpuFlopsClassify(dA, dB)    gpuFlopsClassify                 mindex2-cuda/flops.cu:110-185
  sgpuSpMMWrapper(...)        sgpuSpMMWrapper                  mindex2-cuda/kernel.cu:311-427
  scudaSpMM(hA, hB)           scudaSpMM                        mindex2-cuda/nGpuSpMM.cc:245-279
  CSR.diff / differs / isEqual / isRelativeEqual / isParityEqual / differsStats
                              CSR::differs, isEqual, ...       nlibs/CSR.cc:210-240, 381-415; nlibs/CSR.h:195-320
  PCSR(dM, c) / join / spmm_left / isEqual
                              struct PCSR, spmm(A, pB)         nlibs/PCSR.h:5-100, nlibs/PCSR.cc:3-56, correctTests/pcsrTest.cc:7-19
  BCSR.from_csr(dM, r, c) / to_csr / nonzero_density / is_equal
                              struct BCSR                      nlibs/BCSR.h:6-64, nlibs/BCSR.cc:3-116
  MCSR.from_csr(dM, r, c, blockRows, blockCols) / to_csr / nonzero_density
                              struct MCSR                      nlibs/MCSR.h:6-9, nlibs/MCSR.cc:58-92
  edge_text_header(data) / parse_edge_text(data, declared) / read_edge_file(path, isTrans, flags)
                              COO::readSNAPFile (the text)     nlibs/COO.cc:48-158   (parsed on the device; dtype= picks the value type)
  format_csr_edges(dM) / csr_to_edge_text(dM) / write_edge_file(dM, path, fmt, flags, header)
                              CSR::output (the text)           nlibs/CSR.h:109-168   (formatted on the device; the matrix's dtype)
  rmcl_attractors(dMt) / connected_components(dM) / rmcl_clusters(dMt) -> Clusters
                              (none: the reference stops at Mt, nlibs/qrmcl.cc:136-164; semantics: tests/clusters_ref.py)
  CSR.add(B, alpha, beta) / CSR.symmetrize(mode, alpha, beta)
                              (none: the reference's loader only transposes, nlibs/COO.h:19; semantics: tests/symmetrize_ref.py)

Values are float32 (QValue float, the reference's default) or float64 (its FDOUBLE build, nlibs/tools/macro.h:3-6): a CSR
carries its dtype (CSR.from_arrays(..., dtype=np.float64)) and gpuSpMMWrapper / CSR.hip_spmm / sort_rows_device call the
*_f64 entry points for float64 operands.  Mixing the two raises SpgemmError before any device work.

There is no CPU fallback: if the library or a HIP device is missing, calls raise SpgemmError.
PyTorch is not needed here; bench.py / dist.py use it only for device memory and torch.distributed.
"""
import contextlib
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPGEMM_LIB: diagnostic builds only (make -C csrc ablate); the product library is the default
LIB_PATH = os.environ.get("SPGEMM_LIB") or os.path.join(_HERE, "libspgemm_hip.so")

NBINS = 9
HV_LEN = 9
NKERNELS = 21
_I = C.POINTER(C.c_int)
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)

EXPORTS = [
    "spgemm_hip_last_error", "spgemm_hip_device_count", "spgemm_hip_create", "spgemm_hip_destroy",
    "spgemm_hip_get_stats", "spgemm_hip_stream", "spgemm_hip_malloc", "spgemm_hip_free",
    "spgemm_hip_memcpy_h2d", "spgemm_hip_memcpy_d2h", "spgemm_hip_memcpy_d2d", "hip_CSR_SpMM", "hip_gpuSpMM",
    "hip_gpuFlopsClassify", "hip_sgpuSpMM", "hip_csr_sort_rows", "spgemm_hip_selftest",
    "hip_spgemm_symbolic", "hip_spgemm_numeric", "hip_csr_row_flops", "spgemm_hip_kernel_name",
    "hip_rmcl_prune", "hip_gpuRmclIter", "hip_coo_to_csr", "hip_flopsStats", "spgemm_hip_set_kernel_timing",
    "hip_rmcl_prune_n", "hip_rmcl_expand_prune", "hip_gpuRmclIter_device", "spgemm_hip_pool_cached_bytes", "hip_nnzStats", "hip_resultsComparison",
    "spgemm_hip_group_create", "spgemm_hip_unique_id", "spgemm_hip_group_create_rank", "spgemm_hip_group_info",
    "spgemm_hip_group_destroy", "hip_sharded_spmm_create", "hip_sharded_spmm_step", "hip_sharded_spmm_result",
    "hip_sharded_spmm_info", "hip_sharded_spmm_destroy", "hip_gpuRmclIter_sharded", "spgemm_hip_host_api_stats",
    "hip_sharded_spmm_handle", "spgemm_hip_rccl_available", "spgemm_hip_pool_trim",
    "hip_sharded_rmcl_create", "hip_sharded_rmcl_run", "hip_sharded_rmcl_continue", "hip_sharded_rmcl_result", "hip_sharded_rmcl_iter_nnz",
    "hip_sharded_rmcl_info", "hip_sharded_rmcl_destroy", "spgemm_hip_debug_fail_next", "spgemm_hip_debug_bigrow_paths", "spgemm_hip_debug_midrow_paths", "spgemm_hip_debug_midrow_log", "spgemm_hip_debug_midrow_kernels", "spgemm_hip_debug_midrow_sym_paths", "spgemm_hip_rmcl_devices_used", "spgemm_hip_handle_device",
    "hip_gpuSpMM_f64", "hip_spgemm_numeric_f64", "hip_CSR_SpMM_f64", "hip_csr_sort_rows_f64",
    "hip_csr_permute", "hip_csr_permute_f64", "hip_permutation_transpose", "hip_csr_row_descending_permutation",
    "hip_csr_transpose", "hip_csr_transpose_f64", "spgemm_hip_device_synchronize",
    "hip_csr_diff", "hip_csr_diff_f64", "hip_csr_differsStats", "hip_csr_differsStats_f64",
    "hip_csr_split_columns", "hip_csr_split_columns_f64", "hip_pcsr_join", "hip_pcsr_join_f64",
    "hip_pcsr_spmm", "hip_pcsr_spmm_f64",
    "hip_csr_to_bcsr", "hip_csr_to_bcsr_f64", "hip_bcsr_to_csr", "hip_bcsr_to_csr_f64",
    "hip_csr_to_mcsr", "hip_csr_to_mcsr_f64", "hip_mcsr_to_csr", "hip_mcsr_to_csr_f64",
    "hip_edge_text_header", "hip_parse_edge_lines", "hip_parse_edge_text", "hip_read_edge_file",
    "hip_coo_to_csr_f64", "hip_parse_edge_lines_f64", "hip_parse_edge_text_f64", "hip_read_edge_file_f64",
    "hip_edge_text_write_header", "hip_format_csr_edges", "hip_format_csr_edges_f64", "hip_csr_to_edge_text",
    "hip_csr_to_edge_text_f64", "hip_write_edge_file", "hip_write_edge_file_f64",
    "hip_csr_to_dense", "hip_csr_to_dense_f64", "hip_dense_to_csr", "hip_dense_to_csr_f64",
    "hip_dense_gemm", "hip_dense_gemm_f64",
    "hip_rmcl_attractors", "hip_rmcl_attractors_f64", "hip_rmcl_attractor_lanes", "hip_csr_connected_components",
    "hip_labels_to_clusters", "hip_rmcl_clusters", "hip_rmcl_clusters_f64",
    "hip_rmcl_prune_f64", "hip_rmcl_prune_n_f64", "hip_rmcl_expand_prune_f64", "hip_gpuRmclIter_device_f64",
    "hip_gpuRmclIter_f64",
    "hip_csr_add", "hip_csr_add_f64", "hip_csr_scale", "hip_csr_scale_f64", "hip_csr_col_counts",
    "hip_degree_factors", "hip_degree_factors_f64", "hip_csr_symmetrize", "hip_csr_symmetrize_f64",
    "hip_csr_row_topk", "hip_csr_row_topk_f64", "hip_csr_row_topk_limits", "spgemm_hip_debug_topk_paths",
    "hip_gpuRmclIter_device_topk", "hip_gpuRmclIter_device_topk_f64",
]
TOPK_NORMALISE = 1
SYM_SUM, SYM_BIBLIOMETRIC, SYM_DEGREE_DISCOUNTED = 0, 1, 2
PCSR_MAX_BLOCKS = 64
BCSR_MAX_TILE = 4096
DENSE_KEEP_REFERENCE, DENSE_KEEP_ABS = 0, 1
VALUE_DTYPES = (np.float32, np.float64)
XCHG_AUTO, XCHG_RCCL, XCHG_PEER, XCHG_HOST = 0, 1, 2, 3
XCHG_NAMES = {0: "auto", 1: "rccl", 2: "peer", 3: "host"}
UNIQUE_ID_BYTES = 128


class SpgemmError(RuntimeError):
    pass


class BinReport(C.Structure):
    _fields_ = [("rows", C.c_int), ("rows_differ", C.c_int), ("first_bad_row", C.c_int), ("max_rel_err", C.c_double)]


class CsrDiff(C.Structure):
    """spgemm_csr_diff: the report of hip_csr_diff (include/spgemm_hip.h)"""
    _fields_ = [("rows_len_differ", C.c_int), ("first_len_row", C.c_int), ("only_a", C.c_longlong), ("only_b", C.c_longlong),
                ("first_only_row", C.c_int), ("beyond", C.c_longlong), ("first_beyond_row", C.c_int),
                ("max_abs_err", C.c_double), ("max_rel_err", C.c_double), ("max_abs_only_a", C.c_double),
                ("max_abs_only_b", C.c_double), ("sum_sq", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class EdgeStats(C.Structure):
    """spgemm_edge_stats: what hip_parse_edge_lines / hip_parse_edge_text / hip_read_edge_file report"""
    _fields_ = [("lines", C.c_longlong), ("first_bad_line", C.c_longlong), ("entries", C.c_int), ("slow_lines", C.c_int),
                ("ms_upload", C.c_float), ("ms_split", C.c_float), ("ms_parse", C.c_float), ("ms_slow", C.c_float),
                ("ms_total", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class EdgeWriteStats(C.Structure):
    """spgemm_edge_write_stats: what hip_format_csr_edges / hip_csr_to_edge_text / hip_write_edge_file report"""
    _fields_ = [("entries", C.c_longlong), ("bytes", C.c_longlong), ("slow_entries", C.c_longlong), ("slabs", C.c_int),
                ("ms_length", C.c_float), ("ms_scan", C.c_float), ("ms_write", C.c_float), ("ms_slow", C.c_float),
                ("ms_download", C.c_float), ("ms_file", C.c_float), ("ms_total", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class HostApiStats(C.Structure):
    _fields_ = [("ms_h2d", C.c_float), ("ms_device", C.c_float), ("ms_d2h", C.c_float), ("ms_total", C.c_float),
                ("bytes_h2d", C.c_longlong), ("bytes_d2h", C.c_longlong)]


class Stats(C.Structure):
    _fields_ = [("total_flops", C.c_longlong), ("nnzC", C.c_int), ("bin_rows", C.c_int * NBINS),
                ("ms_classify", C.c_float), ("ms_symbolic", C.c_float), ("ms_scan_alloc", C.c_float),
                ("ms_numeric", C.c_float), ("ms_total", C.c_float), ("ms_kernel", C.c_float * NKERNELS)]

    def as_dict(self):
        return {"total_flops": int(self.total_flops), "nnzC": int(self.nnzC), "bin_rows": [int(x) for x in self.bin_rows],
                "ms_classify": float(self.ms_classify), "ms_symbolic": float(self.ms_symbolic),
                "ms_scan_alloc": float(self.ms_scan_alloc), "ms_numeric": float(self.ms_numeric),
                "ms_total": float(self.ms_total),
                "ms_kernel": {kernel_name(i): float(self.ms_kernel[i]) for i in range(NKERNELS)
                              if kernel_name(i) and self.ms_kernel[i] > 0.0}}


_lib = None


def lib():
    """Load libspgemm_hip.so (built in tree by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SpgemmError(f"{LIB_PATH} is missing: run `make -C sparse_matrix_with_flops_amd/csrc` "
                              "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        L.spgemm_hip_last_error.restype = C.c_char_p
        L.spgemm_hip_stream.restype = C.c_void_p
        L.spgemm_hip_stream.argtypes = [C.c_void_p]
        L.spgemm_hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.spgemm_hip_destroy.argtypes = [C.c_void_p]
        L.spgemm_hip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.spgemm_hip_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.spgemm_hip_free.argtypes = [C.c_void_p]
        L.spgemm_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.spgemm_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hip_CSR_SpMM.argtypes = [_I, _I, _F, C.c_int, _I, _I, _F, C.c_int, C.POINTER(_I), C.POINTER(_I),
                                   C.POINTER(_F), _I, C.c_int, C.c_int, C.c_int]
        dev_in = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.hip_gpuSpMM.argtypes = [C.c_void_p] + dev_in + dev_in + [C.c_int, C.c_int, C.c_int] + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_gpuFlopsClassify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I, _I,
                                           C.POINTER(C.c_longlong)]
        L.hip_sgpuSpMM.argtypes = [C.c_void_p] + dev_in + dev_in + [C.c_int, C.c_int, C.c_int] + \
            [C.c_void_p, _I, C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_spgemm_symbolic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, _I]
        L.hip_spgemm_numeric.argtypes = [C.c_void_p] + dev_in + dev_in + [C.c_int, C.c_int, C.c_int,
                                                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.hip_csr_row_flops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.POINTER(C.c_longlong)]
        L.spgemm_hip_kernel_name.restype = C.c_char_p
        L.spgemm_hip_kernel_name.argtypes = [C.c_int]
        L.hip_coo_to_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I]
        L.hip_coo_to_csr_f64.argtypes = L.hip_coo_to_csr.argtypes
        L.hip_flopsStats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.spgemm_hip_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hip_rmcl_prune.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_rmcl_expand_prune.argtypes = [C.c_void_p] + dev_in + dev_in + [C.c_int, C.c_int, C.c_int] + \
            [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int)]
        L.hip_gpuRmclIter_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + dev_in + dev_in + \
            [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int)]
        L.hip_rmcl_prune_n.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.spgemm_hip_pool_cached_bytes.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
        L.hip_nnzStats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.hip_resultsComparison.argtypes = [C.c_int, C.c_int, _I, _I, _F, _I, _I, _F, _I, C.c_int, _I, C.c_double,
                                            C.POINTER(BinReport)]
        L.hip_gpuRmclIter.argtypes = [C.c_int, C.c_int, C.c_int, _I, _I, _F, C.c_int, _I, _I, _F, C.c_int,
                                      C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I]
        L.hip_rmcl_prune_f64.argtypes = L.hip_rmcl_prune.argtypes
        L.hip_rmcl_prune_n_f64.argtypes = L.hip_rmcl_prune_n.argtypes
        L.hip_rmcl_expand_prune_f64.argtypes = L.hip_rmcl_expand_prune.argtypes
        L.hip_gpuRmclIter_device_f64.argtypes = L.hip_gpuRmclIter_device.argtypes
        L.hip_gpuRmclIter_f64.argtypes = [C.c_int, C.c_int, C.c_int, _I, _I, _D, C.c_int, _I, _I, _D, C.c_int,
                                          C.POINTER(_I), C.POINTER(_I), C.POINTER(_D), _I]
        L.hip_csr_sort_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hip_CSR_SpMM_f64.argtypes = [_I, _I, _D, C.c_int, _I, _I, _D, C.c_int, C.POINTER(_I), C.POINTER(_I),
                                       C.POINTER(_D), _I, C.c_int, C.c_int, C.c_int]
        L.hip_gpuSpMM_f64.argtypes = L.hip_gpuSpMM.argtypes
        L.hip_spgemm_numeric_f64.argtypes = L.hip_spgemm_numeric.argtypes
        L.hip_csr_sort_rows_f64.argtypes = L.hip_csr_sort_rows.argtypes
        L.hip_csr_permute.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        L.hip_csr_permute_f64.argtypes = L.hip_csr_permute.argtypes
        L.hip_permutation_transpose.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hip_csr_row_descending_permutation.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hip_csr_transpose.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + \
            [C.POINTER(C.c_void_p)] * 3
        L.hip_csr_transpose_f64.argtypes = L.hip_csr_transpose.argtypes
        L.hip_csr_diff.argtypes = [C.c_void_p, C.c_int, C.c_int] + dev_in + dev_in + [C.c_double, C.c_double,
                                                                                          C.POINTER(CsrDiff)]
        L.hip_csr_diff_f64.argtypes = L.hip_csr_diff.argtypes
        L.hip_csr_differsStats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _F, C.c_int, _I]
        L.hip_csr_differsStats_f64.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _D, C.c_int, _I]
        table = [C.POINTER(C.c_void_p)] * 3 + [_I]         # host arrays: c rowPtr / colInd / values pointers, c counts
        L.hip_csr_split_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_csr_split_columns_f64.argtypes = L.hip_csr_split_columns.argtypes
        L.hip_pcsr_join.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + table + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_pcsr_join_f64.argtypes = L.hip_pcsr_join.argtypes
        L.hip_pcsr_spmm.argtypes = [C.c_void_p] + dev_in + [C.c_int, C.c_int, C.c_int, C.c_int] + table + table
        L.hip_pcsr_spmm_f64.argtypes = L.hip_pcsr_spmm.argtypes
        L.hip_csr_to_bcsr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_csr_to_bcsr_f64.argtypes = L.hip_csr_to_bcsr.argtypes
        L.hip_bcsr_to_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_double] + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_bcsr_to_csr_f64.argtypes = L.hip_bcsr_to_csr.argtypes
        L.hip_csr_to_mcsr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_int] + ([C.POINTER(C.c_void_p)] * 3 + [_I]) * 2
        L.hip_csr_to_mcsr_f64.argtypes = L.hip_csr_to_mcsr.argtypes
        L.hip_mcsr_to_csr.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] * 2 + \
            [C.c_double] + [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_mcsr_to_csr_f64.argtypes = L.hip_mcsr_to_csr.argtypes
        L.hip_edge_text_header.argtypes = [C.c_char_p, C.c_size_t, _I, _I, _I, _I, _I, C.POINTER(C.c_size_t)]
        edge_out = [C.POINTER(C.c_void_p)] * 3 + [_I, C.POINTER(EdgeStats)]
        L.hip_parse_edge_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int] + edge_out
        L.hip_parse_edge_text.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int] + edge_out
        L.hip_read_edge_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, _I, _I] + edge_out
        L.hip_parse_edge_lines_f64.argtypes = L.hip_parse_edge_lines.argtypes
        L.hip_parse_edge_text_f64.argtypes = L.hip_parse_edge_text.argtypes
        L.hip_read_edge_file_f64.argtypes = L.hip_read_edge_file.argtypes
        L.hip_edge_text_write_header.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                                 C.POINTER(C.c_size_t)]
        csr_in = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        wst = [C.POINTER(C.c_size_t), C.POINTER(EdgeWriteStats)]
        L.hip_format_csr_edges.argtypes = csr_in + [C.c_int] * 4 + [C.POINTER(C.c_void_p)] + wst
        L.hip_csr_to_edge_text.argtypes = csr_in + [C.c_int] * 4 + [C.c_void_p, C.c_size_t] + wst
        L.hip_write_edge_file.argtypes = [C.c_void_p, C.c_char_p] + csr_in[1:] + [C.c_int] * 3 + [C.POINTER(EdgeWriteStats)]
        L.hip_format_csr_edges_f64.argtypes = L.hip_format_csr_edges.argtypes
        L.hip_csr_to_edge_text_f64.argtypes = L.hip_csr_to_edge_text.argtypes
        L.hip_write_edge_file_f64.argtypes = L.hip_write_edge_file.argtypes
        L.hip_csr_to_dense.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_longlong]
        L.hip_csr_to_dense_f64.argtypes = L.hip_csr_to_dense.argtypes
        L.hip_dense_to_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_double] + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_dense_to_csr_f64.argtypes = L.hip_dense_to_csr.argtypes
        L.hip_dense_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p, C.c_longlong] * 3
        L.hip_dense_gemm_f64.argtypes = L.hip_dense_gemm.argtypes
        L.hip_rmcl_attractors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hip_rmcl_attractors_f64.argtypes = L.hip_rmcl_attractors.argtypes
        L.hip_rmcl_attractor_lanes.argtypes = [C.c_int, C.c_int]
        L.hip_csr_connected_components.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   _I, _I]
        L.hip_labels_to_clusters.argtypes = [C.c_void_p, C.c_int, C.c_void_p, _I] + [C.POINTER(C.c_void_p)] * 3
        L.hip_rmcl_clusters.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _I] + \
            [C.POINTER(C.c_void_p)] * 3
        L.hip_rmcl_clusters_f64.argtypes = L.hip_rmcl_clusters.argtypes
        L.hip_csr_add.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_double] + dev_in + [C.c_double] + dev_in + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_csr_add_f64.argtypes = L.hip_csr_add.argtypes
        L.hip_csr_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.hip_csr_scale_f64.argtypes = L.hip_csr_scale.argtypes
        L.hip_csr_col_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.hip_degree_factors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p]
        L.hip_degree_factors_f64.argtypes = L.hip_degree_factors.argtypes
        L.hip_csr_symmetrize.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int] + dev_in + \
            [C.POINTER(C.c_void_p)] * 3 + [_I]
        L.hip_csr_symmetrize_f64.argtypes = L.hip_csr_symmetrize.argtypes
        L.hip_csr_row_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [_I, _I]
        L.hip_csr_row_topk_f64.argtypes = L.hip_csr_row_topk.argtypes
        L.hip_csr_row_topk_limits.argtypes = [C.c_int, _I, _I]
        L.spgemm_hip_debug_topk_paths.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 4
        L.hip_gpuRmclIter_device_topk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + dev_in + dev_in + \
            [C.POINTER(C.c_void_p)] * 3 + [_I, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.hip_gpuRmclIter_device_topk_f64.argtypes = L.hip_gpuRmclIter_device_topk.argtypes
        L.spgemm_hip_selftest.argtypes = [C.c_void_p]
        L.spgemm_hip_set_kernel_timing.argtypes = [C.c_void_p, C.c_uint]
        host_in = [_I, _I, _F, C.c_int]
        L.spgemm_hip_host_api_stats.argtypes = [C.POINTER(HostApiStats)]
        L.spgemm_hip_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, _I, C.c_int]
        L.spgemm_hip_unique_id.argtypes = [C.c_void_p]
        L.spgemm_hip_group_create_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.spgemm_hip_group_info.argtypes = [C.c_void_p, _I, _I, _I]
        L.spgemm_hip_group_destroy.argtypes = [C.c_void_p]
        L.hip_sharded_spmm_create.argtypes = [C.c_void_p] + host_in + host_in + [C.c_int, C.c_int, C.c_int,
                                                                                   C.POINTER(C.c_void_p)]
        L.hip_sharded_spmm_step.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.hip_sharded_spmm_result.argtypes = [C.c_void_p, C.c_int, C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I, _I]
        L.hip_sharded_spmm_info.argtypes = [C.c_void_p, _I, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.hip_sharded_spmm_destroy.argtypes = [C.c_void_p]
        L.hip_sharded_spmm_handle.argtypes = [C.c_void_p, C.c_int]
        L.hip_sharded_spmm_handle.restype = C.c_void_p
        L.hip_gpuRmclIter_sharded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + host_in + host_in + \
            [C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I]
        L.hip_sharded_rmcl_create.argtypes = [C.c_void_p, C.c_int, C.c_int] + host_in + host_in + [C.POINTER(C.c_void_p)]
        L.hip_sharded_rmcl_run.argtypes = [C.c_void_p, C.c_int, _I]
        L.hip_sharded_rmcl_continue.argtypes = [C.c_void_p, C.c_int, _I]
        L.hip_sharded_rmcl_result.argtypes = [C.c_void_p, C.c_int, C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I]
        L.hip_sharded_rmcl_iter_nnz.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
        L.hip_sharded_rmcl_info.argtypes = [C.c_void_p, _I]
        L.hip_sharded_rmcl_destroy.argtypes = [C.c_void_p]
        L.spgemm_hip_debug_fail_next.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "spgemm_hip_debug_bigrow_paths"):      # (an older library loaded through SPGEMM_LIB for an A/B run has none)
            L.spgemm_hip_debug_bigrow_paths.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        if hasattr(L, "spgemm_hip_debug_midrow_paths"):
            L.spgemm_hip_debug_midrow_paths.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
            L.spgemm_hip_debug_midrow_log.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 3
        if hasattr(L, "spgemm_hip_debug_midrow_kernels"):
            L.spgemm_hip_debug_midrow_kernels.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 2
        if hasattr(L, "spgemm_hip_debug_midrow_sym_paths"):
            L.spgemm_hip_debug_midrow_sym_paths.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 2
        L.spgemm_hip_handle_device.argtypes = [C.c_void_p]
        L.free = C.CDLL(None).free
        L.free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def kernel_name(i):
    return lib().spgemm_hip_kernel_name(int(i)).decode()


def _check(rc, what):
    if rc != 0:
        raise SpgemmError(f"{what} failed with status {rc}: {lib().spgemm_hip_last_error().decode(errors='replace')}")


def device_count():
    n = C.c_int(0)
    rc = lib().spgemm_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ---------------------------------------------------------------------------------------------
# the binding kit: what every wrapper of a device entry point does, once
# ---------------------------------------------------------------------------------------------
def _typed(name, dtype):
    """-> (entry point, its name): `name` for float32 values, `name` + "_f64" for float64"""
    name = name + "_f64" if _value_dtype(dtype) == np.float64 else name
    return getattr(lib(), name), name


def _call(name, dtype, *args):
    fn, name = _typed(name, dtype)
    _check(fn(*args), name)


def _hp(handle):
    """the spgemm_handle argument; no Handle = the library's default handle"""
    return handle.ptr if handle else None


def _ptrs(*device_pointers):
    return [C.c_void_p(p) for p in device_pointers]


class _CsrOut:
    """the outputs of an entry point that makes a CSR: three device pointers and (count=True) an int.  refs() are the
    arguments, values() what the call left in them: (rowPtr, colInd, values[, count])."""

    def __init__(self, count=True):
        self._slots = [C.c_void_p(), C.c_void_p(), C.c_void_p()] + ([C.c_int(0)] if count else [])

    def refs(self):
        return [C.byref(s) for s in self._slots]

    def values(self):
        return tuple(s.value for s in self._slots)


# Objects that own something on the C side, closed in dependency order when the interpreter exits (jobs before the groups
# they were made on, groups before plain handles): left to the garbage collector at shutdown they are finalised in any
# order, after the HIP runtime has started to go away -- seen as a segmentation fault at exit after a failed test.
_LIVE = weakref.WeakSet()


def _close_all():
    live = list(_LIVE)
    for kind in ("ShardedSpMM", "ShardedRmcl", "Group", "Handle"):
        for o in live:
            if type(o).__name__ == kind:
                try:
                    o.close()
                except Exception:
                    pass


import atexit  # noqa: E402
atexit.register(_close_all)


class Handle:
    """spgemm_handle: one HIP stream + workspace on one device."""

    def __init__(self, device=0, _borrowed=None):
        self._own = _borrowed is None
        if _borrowed is not None:                   # a handle owned by someone else (a group's shard): never destroyed here
            self._h = C.c_void_p(_borrowed)
        else:
            self._h = C.c_void_p()
            _check(lib().spgemm_hip_create(C.byref(self._h), int(device)), "spgemm_hip_create")
            _LIVE.add(self)
        self.device = device if _borrowed is None else int(lib().spgemm_hip_handle_device(self._h))

    @property
    def ptr(self):
        return self._h

    def stats(self):
        s = Stats()
        _check(lib().spgemm_hip_get_stats(self._h, C.byref(s)), "spgemm_hip_get_stats")
        return s.as_dict()

    def stream(self):
        return lib().spgemm_hip_stream(self._h)

    def selftest(self):
        _check(lib().spgemm_hip_selftest(self._h), "spgemm_hip_selftest")

    def set_kernel_timing(self, mask):
        """bit i: bracket the launches of kernel i with HIP events (stats()['ms_kernel']); 0 = none (default)."""
        _check(lib().spgemm_hip_set_kernel_timing(self._h, int(mask) & 0xFFFFFFFF), "spgemm_hip_set_kernel_timing")

    def fail_next(self, count=1):
        """test hook: the next `count` symbolic phases / fused R-MCL steps on this handle fail"""
        _check(lib().spgemm_hip_debug_fail_next(self._h, int(count)), "spgemm_hip_debug_fail_next")

    def bigrow_paths(self):
        """test hook: rows of the latest product's last bin that took the direct kernel / the multi-pass hash kernel, the
        re-hit cap of the direct kernel and the ints of one block's log region"""
        v = [C.c_int(0) for _ in range(4)]
        _check(lib().spgemm_hip_debug_bigrow_paths(self._h, *[C.byref(x) for x in v]), "spgemm_hip_debug_bigrow_paths")
        return {"direct": v[0].value, "fallback": v[1].value, "cap": v[2].value, "region": v[3].value}

    def midrow_paths(self):
        """test hook: rows of 513-4096 products of the latest product, how many took the direct kernel / the hash kernel of
        their bin, the re-hit cap of the direct kernel; re-hits the direct rows logged, log ints reserved, log ints there;
        direct rows of 513-2048 products that took the wave-per-row kernel / the four-wave kernel"""
        v = [C.c_int(0) for _ in range(4)]
        w = [C.c_longlong(0) for _ in range(3)]
        k = [C.c_longlong(0) for _ in range(2)]
        _check(lib().spgemm_hip_debug_midrow_paths(self._h, *[C.byref(x) for x in v]), "spgemm_hip_debug_midrow_paths")
        _check(lib().spgemm_hip_debug_midrow_log(self._h, *[C.byref(x) for x in w]), "spgemm_hip_debug_midrow_log")
        if hasattr(lib(), "spgemm_hip_debug_midrow_kernels"):
            _check(lib().spgemm_hip_debug_midrow_kernels(self._h, *[C.byref(x) for x in k]), "spgemm_hip_debug_midrow_kernels")
        return {"rows": v[0].value, "direct": v[1].value, "fallback": v[2].value, "cap": v[3].value,
                "logged": w[0].value, "reserved": w[1].value, "capacity": w[2].value,
                "wave": k[0].value, "multiwave": k[1].value}

    def midrow_sym_paths(self):
        """test hook: rows of 513-2048 products of the latest product whose symbolic pass logged them, by the kernel that
        did: k_sym_midpair (SPGEMM_SYM_PAIR=1) / the four-wave kernel"""
        k = [C.c_longlong(0) for _ in range(2)]
        _check(lib().spgemm_hip_debug_midrow_sym_paths(self._h, *[C.byref(x) for x in k]), "spgemm_hip_debug_midrow_sym_paths")
        return {"pair": k[0].value, "multiwave": k[1].value}

    def topk_paths(self):
        """test hook: the rows hip_csr_row_topk has handled on this handle since it was created: copied uncut / cut by the
        wave, the block and the stream path"""
        return topk_paths(self)

    def close(self):
        if self._h and self._own:
            lib().spgemm_hip_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------
def dev_alloc(nbytes):
    p = C.c_void_p()
    _check(lib().spgemm_hip_malloc(C.byref(p), max(int(nbytes), 1)), "spgemm_hip_malloc")
    return p.value


def dev_free(ptr):
    if ptr:
        _check(lib().spgemm_hip_free(C.c_void_p(ptr)), "spgemm_hip_free")


def h2d(arr):
    arr = np.ascontiguousarray(arr)
    p = dev_alloc(arr.nbytes)
    if arr.nbytes:
        _check(lib().spgemm_hip_memcpy_h2d(C.c_void_p(p), arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
    return p


def d2h(ptr, n, dtype):
    out = np.empty(int(n), dtype=dtype)
    if out.nbytes:
        _check(lib().spgemm_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes), "d2h")
    return out


class CSR:
    """Mirror of the reference's `struct CSR` (nlibs/CSR.h:23-50): three arrays + rows/cols/nnz.
    Host CSRs hold numpy arrays; device CSRs (from toGpuCSR / gpuSpMMWrapper) hold raw device
    pointers in the same fields, exactly as the reference reuses one struct for both."""

    def __init__(self, values=None, colInd=None, rowPtr=None, rows=0, cols=0, nnz=0, on_device=False, dtype=None):
        self.values, self.colInd, self.rowPtr = values, colInd, rowPtr
        self.rows, self.cols, self.nnz = int(rows), int(cols), int(nnz)
        self.on_device = on_device
        # value type: a host CSR's values array says it; a device CSR (raw pointers) carries it here
        if dtype is None:
            dtype = values.dtype if isinstance(values, np.ndarray) else np.float32
        self.dtype = np.dtype(dtype)

    @staticmethod
    def from_arrays(rowPtr, colInd, values, rows, cols, dtype=np.float32):
        """dtype: np.float32 (QValue float, the default) or np.float64 (the reference's FDOUBLE build)."""
        dtype = _value_dtype(dtype)
        rowPtr = np.ascontiguousarray(rowPtr, dtype=np.int32)
        return CSR(np.ascontiguousarray(values, dtype=dtype), np.ascontiguousarray(colInd, dtype=np.int32),
                   rowPtr, rows, cols, int(rowPtr[-1]) if len(rowPtr) else 0, dtype=dtype)

    # -- nlibs/CSR.cc:342-379 ------------------------------------------------------------------
    def toGpuCSR(self):
        assert not self.on_device
        return CSR(h2d(self.values), h2d(self.colInd), h2d(self.rowPtr), self.rows, self.cols, self.nnz, True,
                   dtype=self.dtype)

    def toCpuCSR(self):
        assert self.on_device
        return CSR(d2h(self.values, self.nnz, self.dtype), d2h(self.colInd, self.nnz, np.int32),
                   d2h(self.rowPtr, self.rows + 1, np.int32), self.rows, self.cols, self.nnz, False, dtype=self.dtype)

    def deviceDispose(self):
        assert self.on_device
        for p in (self.values, self.colInd, self.rowPtr):
            dev_free(p)
        self.values = self.colInd = self.rowPtr = None

    # -- nlibs/CSR.cc:73-86 -------------------------------------------------------------------
    def makeOrdered(self):
        assert not self.on_device
        row_of = np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.rowPtr.astype(np.int64)))
        order = np.lexsort((self.colInd, row_of))
        self.colInd = np.ascontiguousarray(self.colInd[order])
        self.values = np.ascontiguousarray(self.values[order])

    # -- the drop-in: same role as CSR::spmm/omp_spmm/... (nlibs/CSR.cc:59-208) ----------------
    def hip_spmm(self, B):
        """C = self * B through hip_CSR_SpMM (host arrays in, malloc'd host arrays out)."""
        assert not self.on_device and not B.on_device
        if self.cols != B.rows:
            raise SpgemmError(f"shape mismatch: A is {self.rows}x{self.cols}, B is {B.rows}x{B.cols}")
        dt = _common_dtype(self, B)
        L = lib()
        P = _D if dt == np.float64 else _F
        ic, jc, cv, nnz = _I(), _I(), P(), C.c_int(0)
        fn, name = _typed("hip_CSR_SpMM", dt)
        rc = fn(self.rowPtr.ctypes.data_as(_I), self.colInd.ctypes.data_as(_I), self.values.ctypes.data_as(P),
                self.nnz, B.rowPtr.ctypes.data_as(_I), B.colInd.ctypes.data_as(_I), B.values.ctypes.data_as(P),
                B.nnz, C.byref(ic), C.byref(jc), C.byref(cv), C.byref(nnz), self.rows, self.cols, B.cols)
        _check(rc, name)
        rp, ci, v = _take_malloced(L, ic, jc, cv, self.rows, nnz.value, self.dtype)
        return CSR(v, ci, rp, self.rows, B.cols, nnz.value, dtype=self.dtype)

    # -- reordering (nlibs/CSR.cc:431-494) through the device entry points; host CSR in -> host CSR out (uploaded and
    #    downloaded around the call), device CSR in -> device CSR out, like the rest of the mirror --------------------
    def _on_device(self, fn):
        """fn(device CSR) -> device CSR; wraps the upload / download for a host-resident self"""
        if self.on_device:
            return fn(self)
        d = self.toGpuCSR()
        try:
            out = fn(d)
        finally:
            d.deviceDispose()
        try:
            return out.toCpuCSR()
        finally:
            out.deviceDispose()

    def _permuted(self, rowP, colP, handle):
        dt = _value_dtype(self.dtype)

        def run(d):
            ups = [h2d(x) if x is not None else None for x in (rowP, colP)]
            try:
                ib, jb, vb = _csr_permute(dt, handle, d.rows, d.cols, d.nnz, d.rowPtr, d.colInd, d.values, ups[0], ups[1])
            finally:
                for p in ups:
                    dev_free(p)
            return CSR(vb, jb, ib, d.rows, d.cols, d.nnz, True, dtype=d.dtype)
        return self._on_device(run)

    def PM(self, P, handle=None):
        """CSR::PM (nlibs/CSR.cc:431-445): row i of the result is row P[i] of self.  P: host int32 permutation."""
        return self._permuted(_host_perm(P, self.rows, "PM"), None, handle)

    def MP(self, P, handle=None):
        """CSR::MP (nlibs/CSR.cc:447-464): column c of self becomes column P[c]; rows are left unsorted."""
        return self._permuted(None, _host_perm(P, self.cols, "MP"), handle)

    def PMPt(self, P, handle=None):
        """CSR::PMPt (nlibs/CSR.cc:466-473), square only: PM(P) then MP(Pt), in one pass over the entries."""
        _need_square(self, "PMPt")
        P = _host_perm(P, self.rows, "PMPt")
        return self._permuted(P, permutation_transpose(P, handle), handle)

    def PtMP(self, P, handle=None):
        """CSR::PtMP (nlibs/CSR.cc:475-482), square only: MP(P) then PM(Pt); undoes PMPt(P)."""
        _need_square(self, "PtMP")
        P = _host_perm(P, self.rows, "PtMP")
        return self._permuted(permutation_transpose(P, handle), P, handle)

    def transpose(self, handle=None):
        """self^T on the device (hip_csr_transpose): stable, so the result is column-sorted when no row repeats a column."""
        dt = _value_dtype(self.dtype)

        def run(d):
            it, jt, vt = _csr_transpose(dt, handle, d.rows, d.cols, d.nnz, d.rowPtr, d.colInd, d.values)
            return CSR(vt, jt, it, d.cols, d.rows, d.nnz, True, dtype=d.dtype)
        return self._on_device(run)

    # -- sparse add and symmetrisation (include/spgemm_hip.h "sparse add and the symmetrisation of a directed graph");
    #    rows of the operands must be strictly ascending by column (makeOrdered / sort_rows_device) -----------------
    def add(self, B, alpha=1.0, beta=1.0, handle=None):
        """alpha * self + beta * B (hip_csr_add): the union of the two patterns, rows ascending, zero sums kept.  A host
        B is uploaded for the call."""
        if (self.rows, self.cols) != (B.rows, B.cols):
            raise SpgemmError(f"shape mismatch: A is {self.rows}x{self.cols}, B is {B.rows}x{B.cols}")
        dt = _common_dtype(self, B)

        def run(d):
            b = B if B.on_device else (d if B is self else B.toGpuCSR())
            try:
                ic, jc, vc, nnz = csr_add_raw(handle, d.rows, d.cols, alpha, d.rowPtr, d.colInd, d.values, d.nnz, beta,
                                              b.rowPtr, b.colInd, b.values, b.nnz, dtype=dt)
            finally:
                if b is not B and b is not d:
                    b.deviceDispose()
            return CSR(vc, jc, ic, d.rows, d.cols, nnz, True, dtype=d.dtype)
        return self._on_device(run)

    def symmetrize(self, mode=SYM_SUM, alpha=0.5, beta=0.5, handle=None):
        """hip_csr_symmetrize of a square matrix: SYM_SUM (A + A^T), SYM_BIBLIOMETRIC (A A^T + A^T A) or
        SYM_DEGREE_DISCOUNTED (alpha / beta: the exponents of the out- / in-degree, read by that mode only)."""
        _need_square(self, "symmetrize")
        dt = _value_dtype(self.dtype)

        def run(d):
            i, j, v, nnz = csr_symmetrize_raw(handle, mode, alpha, beta, d.rows, d.rowPtr, d.colInd, d.values, d.nnz, dtype=dt)
            return CSR(v, j, i, d.rows, d.cols, nnz, True, dtype=d.dtype)
        return self._on_device(run)

    def row_topk(self, k, normalise=False, handle=None):
        """hip_csr_row_topk / _f64 on a device CSR -> device CSR: every row keeps its min(len, k) best entries in storage
        order (larger value, then smaller column, then earlier position; NaN last); rows_cut on the result says how many
        rows lost entries.  normalise: the kept values of the cut rows are divided by their sum."""
        if not self.on_device:
            raise SpgemmError("row_topk: takes a device CSR")
        dt = _value_dtype(self.dtype)
        i, j, v, nnz, cut = csr_row_topk_raw(handle, self.rows, self.cols, self.nnz, self.rowPtr, self.colInd, self.values,
                                             k, TOPK_NORMALISE if normalise else 0, dtype=dt)
        out = CSR(v, j, i, self.rows, self.cols, nnz, True, dtype=self.dtype)
        out.rows_cut = cut
        return out

    def rowDescendingOrderPermutation(self, handle=None):
        """CSR::rowDescendingOrderPermutation (nlibs/CSR.cc:484-494) -> host int32[rows]: rows by descending length, rows
        of equal length by ascending id."""
        rp = self.rowPtr if self.on_device else h2d(self.rowPtr)
        try:
            dp = row_descending_permutation_raw(handle, self.rows, rp)
        finally:
            if not self.on_device:
                dev_free(rp)
        try:
            return d2h(dp, self.rows, np.int32)
        finally:
            dev_free(dp)

    # -- comparison (nlibs/CSR.cc:210-240, 381-415; nlibs/CSR.h:195-245, 284-320) through hip_csr_diff /
    #    hip_csr_differsStats: a host CSR is uploaded for the call and the copy released, a device CSR is used in place.
    #    Rows of both operands must be strictly ascending by column (makeOrdered / sort_rows_device). ------------------
    def _with_device_pair(self, B, fn):
        """fn(device self, device B); shape / dtype mismatch raises before any device work"""
        if (self.rows, self.cols) != (B.rows, B.cols):
            raise SpgemmError(f"shape mismatch: A is {self.rows}x{self.cols}, B is {B.rows}x{B.cols}")
        _common_dtype(self, B)
        made = []
        try:
            pair = []
            for M in (self, B):
                if M.on_device:
                    pair.append(M)
                elif M is self and pair:                    # A.diff(A): one upload
                    pair.append(pair[0])
                else:
                    made.append(M.toGpuCSR())
                    pair.append(made[-1])
            return fn(pair[0], pair[1])
        finally:
            for d in made:
                d.deviceDispose()

    def diff(self, B, rel=1e-6, abs=0.0, handle=None):
        """hip_csr_diff of self against B (B is the reference side) -> CsrDiff"""
        dt = _value_dtype(self.dtype)
        return self._with_device_pair(B, lambda a, b: _csr_diff(dt, handle, a.rows, a.cols, a.rowPtr, a.colInd, a.values,
                                                                a.nnz, b.rowPtr, b.colInd, b.values, b.nnz, rel, abs))

    def differs(self, B, handle=None):
        """CSR::differs (nlibs/CSR.cc:210-240): the squared Frobenius norm of self - B, accumulated in double"""
        return float(self.diff(B, handle=handle).sum_sq)

    def differsStats(self, B, percents, handle=None):
        """CSR::differsStats (nlibs/CSR.cc:381-415) -> list of len(percents) + 4 counts; only the row pointers are read"""
        if self.rows != B.rows:
            raise SpgemmError(f"shape mismatch: A has {self.rows} rows, B has {B.rows}")
        dt = _common_dtype(self, B)
        ups = [None if M.on_device else h2d(M.rowPtr) for M in (self, B)]
        try:
            ia, ib = [M.rowPtr if u is None else u for M, u in zip((self, B), ups)]
            return csr_differs_stats_raw(handle, self.rows, ia, ib, percents, dtype=dt)
        finally:
            for u in ups:
                dev_free(u)

    def isEqual(self, B, handle=None):
        """CSR::isEqual (nlibs/CSR.h:195-245): same rows / cols / nnz and row lengths, values within 1e-7 absolute (an
        entry only B holds is compared with 0, as the reference's dense row does)"""
        if (self.rows, self.cols, self.nnz) != (B.rows, B.cols, B.nnz):
            return False
        d = self.diff(B, handle=handle)
        return d.rows_len_differ == 0 and d.max_abs_err <= 1e-7 and d.max_abs_only_b <= 1e-7

    def isRelativeEqual(self, B, maxRelativeError, handle=None):
        """CSR::isRelativeEqual (nlibs/CSR.h:284-320): every entry of B with |b| > 1e-8 is met within maxRelativeError"""
        if (self.rows, self.cols) != (B.rows, B.cols):
            return False
        d = self.diff(B, rel=float(maxRelativeError), abs=1e-8, handle=handle)
        return d.beyond == 0 and d.max_abs_only_b <= 1e-8

    def isParityEqual(self, B, rel=1e-6, handle=None):
        """the parity rule: identical structure, values within `rel` relative"""
        if (self.rows, self.cols, self.nnz) != (B.rows, B.cols, B.nnz):
            return False
        d = self.diff(B, rel=rel, abs=0.0, handle=handle)
        return d.rows_len_differ == 0 and d.only_a == 0 and d.only_b == 0 and d.beyond == 0


def _need_square(M, what):
    if M.rows != M.cols:
        raise SpgemmError(f"{what} needs a square matrix, this one is {M.rows}x{M.cols}")


def _host_perm(P, length, what):
    P = np.ascontiguousarray(P, dtype=np.int32)
    if P.ndim != 1 or len(P) != length:
        raise SpgemmError(f"{what}: P has {P.size} entries, the matrix side has {length}")
    return P


def _value_dtype(dtype):
    dt = np.dtype(dtype)
    if dt not in VALUE_DTYPES:
        raise SpgemmError(f"unsupported value dtype {dt}: float32 or float64")
    return dt


def _common_dtype(A, B):
    """the value type of A*B; float32 and float64 operands do not mix (there is no mixed-precision path)"""
    a, b = _value_dtype(A.dtype), _value_dtype(B.dtype)
    if a != b:
        raise SpgemmError(f"mixed value types: A is {a}, B is {b} (convert one operand)")
    return a


def host_api_timed(A, B, reps=3):
    """hip_CSR_SpMM (host arrays in, malloc()ed host arrays out -- what a reference caller of CSR::*spmm gets) timed
    around the C call alone, outputs freed unread.  -> list of per-run dicts (ms_total, ms_h2d, ms_device, ms_d2h, bytes)."""
    import time
    L = lib()
    runs = []
    for _ in range(reps):
        ic, jc, cv, nnz = _I(), _I(), _F(), C.c_int(0)
        t0 = time.perf_counter()
        rc = L.hip_CSR_SpMM(*_host_args(A), *_host_args(B), C.byref(ic), C.byref(jc), C.byref(cv), C.byref(nnz),
                            A.rows, A.cols, B.cols)
        wall = (time.perf_counter() - t0) * 1e3
        _check(rc, "hip_CSR_SpMM")
        for p in (ic, jc, cv):
            L.free(C.cast(p, C.c_void_p))
        st = HostApiStats()
        _check(L.spgemm_hip_host_api_stats(C.byref(st)), "spgemm_hip_host_api_stats")
        runs.append({"ms_wall": wall, "ms_total": st.ms_total, "ms_h2d": st.ms_h2d, "ms_device": st.ms_device,
                     "ms_d2h": st.ms_d2h, "bytes_h2d": int(st.bytes_h2d), "bytes_d2h": int(st.bytes_d2h), "nnzC": nnz.value})
    return runs


def _dev_args(M):
    return _ptrs(M.rowPtr, M.colInd, M.values) + [M.nnz]


def gpuSpMMWrapper(dA, dB, handle=None):
    """CSR gpuSpMMWrapper(const CSR& dA, const CSR& dB) — device CSRs in, device CSR out."""
    assert dA.on_device and dB.on_device
    if dA.cols != dB.rows:
        raise SpgemmError("shape mismatch")
    ic, jc, cv, nnz = _gpu_spmm(_common_dtype(dA, dB), handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd,
                                dB.values, dB.nnz, dA.rows, dA.cols, dB.cols)
    return CSR(cv, jc, ic, dA.rows, dB.cols, nnz, True, dtype=dA.dtype)


def _gpu_spmm(dtype, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    out = _CsrOut()
    _call("hip_gpuSpMM", dtype, _hp(handle), *_ptrs(IA, JA, VA), int(nnzA), *_ptrs(IB, JB, VB), int(nnzB), int(m), int(k),
          int(n), *out.refs())
    return out.values()


def gpu_spmm_raw(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    """Raw-pointer form for callers that own device memory elsewhere (e.g. torch tensors' data_ptr())."""
    return _gpu_spmm(np.float32, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n)


def gpu_spmm_raw_f64(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    """gpu_spmm_raw with float64 values (hip_gpuSpMM_f64)."""
    return _gpu_spmm(np.float64, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n)


def spgemm_symbolic_raw(handle, IA, JA, nnzA, IB, JB, nnzB, m, k, n, IC_out):
    """Phase 1 on raw device pointers: fills IC_out[m+1] (C.rowPtr), returns nnzC."""
    nnz = C.c_int(0)
    # the two phases need the handle that carries the plan between them: handle.ptr, not _hp (None is an AttributeError)
    _check(lib().hip_spgemm_symbolic(handle.ptr, *_ptrs(IA, JA), int(nnzA), *_ptrs(IB, JB), int(nnzB), int(m), int(k), int(n),
                                     C.c_void_p(IC_out), C.byref(nnz)), "hip_spgemm_symbolic")
    return nnz.value


def _spgemm_numeric(dtype, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n, IC, JC_out, C_out):
    _call("hip_spgemm_numeric", dtype, handle.ptr, *_ptrs(IA, JA, VA), int(nnzA), *_ptrs(IB, JB, VB), int(nnzB), int(m), int(k),
          int(n), *_ptrs(IC, JC_out, C_out))


def spgemm_numeric_raw(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n, IC, JC_out, C_out):
    """Phase 2 on raw device pointers: writes JC_out/C_out (caller-owned, nnzC entries each)."""
    _spgemm_numeric(np.float32, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n, IC, JC_out, C_out)


def spgemm_numeric_raw_f64(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n, IC, JC_out, C_out):
    """Phase 2 with float64 values (hip_spgemm_numeric_f64) after spgemm_symbolic_raw on the same handle."""
    _spgemm_numeric(np.float64, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n, IC, JC_out, C_out)


def d2d(dst, src, nbytes):
    """Device-to-device copy between raw pointers (library pool <-> memory owned elsewhere)."""
    _check(lib().spgemm_hip_memcpy_d2d(C.c_void_p(dst), C.c_void_p(src), int(nbytes)), "spgemm_hip_memcpy_d2d")


def device_synchronize():
    """Wait for all work queued on the current device (a d2d copy may return before it has run)."""
    _check(lib().spgemm_hip_device_synchronize(), "spgemm_hip_device_synchronize")


def _rmcl_prune(dtype, handle, m, IC, JC, CV, nnz):
    out = _CsrOut()
    if nnz is None:
        _call("hip_rmcl_prune", dtype, _hp(handle), int(m), *_ptrs(IC, JC, CV), *out.refs())
    else:
        _call("hip_rmcl_prune_n", dtype, _hp(handle), int(m), int(nnz), *_ptrs(IC, JC, CV), *out.refs())
    return out.values()


def rmcl_prune_raw(handle, m, IC, JC, CV, nnz=None):
    """hip_rmcl_prune on raw device pointers: inflate/prune/normalise the rows of C, compacted into new pool arrays.
    nnz (optional): nnz(C) when the caller knows it (hip_rmcl_prune_n: no device read for it).
    Returns (IN, JN, CN, nnzN); release the three with dev_free."""
    return _rmcl_prune(np.float32, handle, m, IC, JC, CV, nnz)


def rmcl_prune_raw_f64(handle, m, IC, JC, CV, nnz=None):
    """rmcl_prune_raw with float64 values (hip_rmcl_prune_f64 / hip_rmcl_prune_n_f64)."""
    return _rmcl_prune(np.float64, handle, m, IC, JC, CV, nnz)


def _rmcl_expand_prune(dtype, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    out = _CsrOut()
    _call("hip_rmcl_expand_prune", dtype, _hp(handle), *_ptrs(IA, JA, VA), int(nnzA), *_ptrs(IB, JB, VB), int(nnzB),
          int(m), int(k), int(n), *out.refs())
    return out.values()


def rmcl_expand_prune_raw(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    """hip_rmcl_expand_prune on raw device pointers: prune(A*B) of one R-MCL iteration without materialising the product.
    Returns (IN, JN, CN, nnzN) in pool arrays; release the three with dev_free."""
    return _rmcl_expand_prune(np.float32, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n)


def rmcl_expand_prune_raw_f64(handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n):
    """rmcl_expand_prune_raw with float64 values (hip_rmcl_expand_prune_f64)."""
    return _rmcl_expand_prune(np.float64, handle, IA, JA, VA, nnzA, IB, JB, VB, nnzB, m, k, n)


def pool_trim(device=0):
    """idle cached blocks of the device go back to the driver"""
    _check(lib().spgemm_hip_pool_trim(int(device)), "spgemm_hip_pool_trim")


def pool_cached_bytes(device=0):
    n = C.c_size_t(0)
    _check(lib().spgemm_hip_pool_cached_bytes(int(device), C.byref(n)), "spgemm_hip_pool_cached_bytes")
    return int(n.value)


COO_DEDUPE, COO_SELF_LOOPS, COO_ROW_NORMALISE, COO_ABS = 1, 2, 4, 8


def flopsStats(dA, dB, handle=None):
    """std::vector<int> flopsStats(...) (nlibs/tools/stats.cc:45-55) for device CSRs: 13 power-of-two buckets."""
    assert dA.on_device and dB.on_device
    out = (C.c_int * 13)()
    _check(lib().hip_flopsStats(_hp(handle), *_ptrs(dA.rowPtr, dA.colInd, dB.rowPtr), dA.rows, out), "hip_flopsStats")
    return [int(x) for x in out]


def nnzStats(dA, handle=None):
    """CSR::nnzStats (nlibs/CSR.cc:241-248) of a device CSR: 18 power-of-two buckets of the row lengths."""
    out = (C.c_int * 18)()
    _check(lib().hip_nnzStats(_hp(handle), C.c_void_p(dA.rowPtr), int(dA.rows), out), "hip_nnzStats")
    return [int(x) for x in out]


def resultsComparison(hC, rC, hv, hqueue, rel=1e-6):
    """resultsComparison / isPartialRawEqual (mindex2-cuda/nGpuSpMM.cc:85-240) on host CSRs: per reference bin
    {rows, rows_differ, first_bad_row, max_rel_err}.  hv/hqueue: outputs of gpuFlopsClassify (queue on the host)."""
    rep = (BinReport * (HV_LEN - 1))()
    hvv = (C.c_int * HV_LEN)(*([int(x) for x in hv] + [int(hv[-1])] * (HV_LEN - len(hv))))
    q = np.ascontiguousarray(hqueue, dtype=np.int32)
    a = [np.ascontiguousarray(x, dtype=t) for x, t in ((hC.rowPtr, np.int32), (hC.colInd, np.int32), (hC.values, np.float32),
                                                        (rC.rowPtr, np.int32), (rC.colInd, np.int32), (rC.values, np.float32))]
    p = lambda arr, ty: arr.ctypes.data_as(ty)
    _check(lib().hip_resultsComparison(int(hC.rows), int(hC.cols), p(a[0], _I), p(a[1], _I), p(a[2], _F), p(a[3], _I),
                                       p(a[4], _I), p(a[5], _F), hvv, len(hv), p(q, _I), float(rel), rep),
           "hip_resultsComparison")
    return [{"rows": r.rows, "rows_differ": r.rows_differ, "first_bad_row": r.first_bad_row, "max_rel_err": r.max_rel_err}
            for r in rep]


def _coo_to_csr(dtype, handle, rows, cols, nnz, dRow, dCol, dVal, flags):
    out = _CsrOut()
    _call("hip_coo_to_csr", dtype, _hp(handle), int(rows), int(cols), int(nnz), *_ptrs(dRow, dCol, dVal), int(flags), *out.refs())
    return out.values()


def coo_to_csr_raw(handle, rows, cols, nnz, dRow, dCol, dVal, flags):
    """hip_coo_to_csr on raw device pointers -> (dIA, dJA, dA, nnz) from the library pool (release with dev_free)."""
    return _coo_to_csr(np.float32, handle, rows, cols, nnz, dRow, dCol, dVal, flags)


def coo_to_csr_raw_f64(handle, rows, cols, nnz, dRow, dCol, dVal, flags):
    """coo_to_csr_raw with float64 values in and out (hip_coo_to_csr_f64)."""
    return _coo_to_csr(np.float64, handle, rows, cols, nnz, dRow, dCol, dVal, flags)


def coo_to_csr(rows, cols, ri, ci, v, flags, handle=None, dtype=np.float32):
    """Host COO arrays in, device CSR out (COO::toCSR and friends, on the device): returns a device `CSR`.
    flags: COO_DEDUPE | COO_SELF_LOOPS | COO_ROW_NORMALISE | COO_ABS (rmclInit = SELF_LOOPS | ROW_NORMALISE).
    dtype: np.float32, or np.float64 for a double device CSR (hip_coo_to_csr_f64)."""
    dtype = _value_dtype(dtype)
    ri = np.ascontiguousarray(ri, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    v = np.ascontiguousarray(v, dtype=dtype)
    dr, dc, dv = h2d(ri), h2d(ci), h2d(v)
    try:
        ia, ja, av, n = _coo_to_csr(dtype, handle, rows, cols, len(ri), dr, dc, dv, flags)
    finally:
        for p in (dr, dc, dv):
            dev_free(p)
    return CSR(av, ja, ia, rows, cols, n, True, dtype=dtype)


def _csr_permute(dtype, handle, m, n, nnz, IA, JA, VA, rowSrc=None, colMap=None):
    out = _CsrOut(count=False)
    _call("hip_csr_permute", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA, rowSrc, colMap), *out.refs())
    return out.values()


def csr_permute_raw(handle, m, n, nnz, IA, JA, VA, rowSrc=None, colMap=None):
    """hip_csr_permute on raw device pointers (rowSrc / colMap: device int arrays or None = identity) -> (dIB, dJB, dB)
    from the library pool (release with dev_free)."""
    return _csr_permute(np.float32, handle, m, n, nnz, IA, JA, VA, rowSrc, colMap)


def csr_permute_raw_f64(handle, m, n, nnz, IA, JA, VA, rowSrc=None, colMap=None):
    """csr_permute_raw with float64 values (hip_csr_permute_f64)."""
    return _csr_permute(np.float64, handle, m, n, nnz, IA, JA, VA, rowSrc, colMap)


def _csr_transpose(dtype, handle, m, n, nnz, IA, JA, VA):
    out = _CsrOut(count=False)
    _call("hip_csr_transpose", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA), *out.refs())
    return out.values()


def csr_transpose_raw(handle, m, n, nnz, IA, JA, VA):
    """hip_csr_transpose on raw device pointers -> (dIT[n+1], dJT, dAT) from the library pool (release with dev_free)."""
    return _csr_transpose(np.float32, handle, m, n, nnz, IA, JA, VA)


def csr_transpose_raw_f64(handle, m, n, nnz, IA, JA, VA):
    """csr_transpose_raw with float64 values (hip_csr_transpose_f64)."""
    return _csr_transpose(np.float64, handle, m, n, nnz, IA, JA, VA)


def _csr_diff(dtype, handle, m, n, IA, JA, VA, nnzA, IB, JB, VB, nnzB, rel, abs_tol):
    out = CsrDiff()
    _call("hip_csr_diff", dtype, _hp(handle), int(m), int(n), *_ptrs(IA, JA, VA), int(nnzA), *_ptrs(IB, JB, VB), int(nnzB),
          float(rel), float(abs_tol), C.byref(out))
    return out


def csr_diff_raw(handle, m, n, IA, JA, VA, nnzA, IB, JB, VB, nnzB, rel=1e-6, abs_tol=0.0):
    """hip_csr_diff on raw device pointers (float32 values) -> CsrDiff"""
    return _csr_diff(np.float32, handle, m, n, IA, JA, VA, nnzA, IB, JB, VB, nnzB, rel, abs_tol)


def csr_diff_raw_f64(handle, m, n, IA, JA, VA, nnzA, IB, JB, VB, nnzB, rel=1e-6, abs_tol=0.0):
    """csr_diff_raw with float64 values (hip_csr_diff_f64)"""
    return _csr_diff(np.float64, handle, m, n, IA, JA, VA, nnzA, IB, JB, VB, nnzB, rel, abs_tol)


def csr_differs_stats_raw(handle, m, IA, IB, percents, dtype=np.float32):
    """hip_csr_differsStats (dtype float32) / _f64 (float64) on two raw device rowPtr arrays; percents: host sequence.
    -> list of len(percents) + 4 counts"""
    f64 = _value_dtype(dtype) == np.float64
    pc = np.ascontiguousarray(percents, dtype=np.float64 if f64 else np.float32)
    if pc.ndim != 1:
        raise SpgemmError("differsStats: percents must be one-dimensional")
    counts = (C.c_int * (len(pc) + 4))()
    _call("hip_csr_differsStats", dtype, _hp(handle), int(m), *_ptrs(IA, IB),
          pc.ctypes.data_as(_D if f64 else _F) if len(pc) else None, len(pc), counts)
    return [int(x) for x in counts]


def permutation_transpose_raw(handle, length, dP, dPt):
    """hip_permutation_transpose on raw device pointers: dPt[dP[i]] = i (dPt: caller's device int[length])."""
    _check(lib().hip_permutation_transpose(_hp(handle), int(length), *_ptrs(dP, dPt)), "hip_permutation_transpose")


def row_descending_permutation_raw(handle, m, IA):
    """hip_csr_row_descending_permutation on a raw device rowPtr -> device int[m] from the pool (release with dev_free)."""
    dp = C.c_void_p()
    _check(lib().hip_csr_row_descending_permutation(_hp(handle), int(m), C.c_void_p(IA), C.byref(dp)),
           "hip_csr_row_descending_permutation")
    return dp.value


def permutation_transpose(P, handle=None):
    """permutationTranspose (nlibs/tools/util.cc:162-168) on the device: host int32 P in, host Pt out, Pt[P[i]] = i."""
    P = np.ascontiguousarray(P, dtype=np.int32)
    if P.ndim != 1:
        raise SpgemmError("permutation_transpose: P must be one-dimensional")
    dp, dpt = h2d(P), dev_alloc(P.nbytes)
    try:
        permutation_transpose_raw(handle, len(P), dp, dpt)
        return d2h(dpt, len(P), np.int32)
    finally:
        dev_free(dp)
        dev_free(dpt)


def row_flops_raw(handle, IA, JA, IB, m, out_ptr):
    """Per-row product counts into a device int[m]; returns P."""
    tot = C.c_longlong(0)
    _check(lib().hip_csr_row_flops(_hp(handle), *_ptrs(IA, JA, IB), int(m), C.c_void_p(out_ptr), C.byref(tot)),
           "hip_csr_row_flops")
    return tot.value


def gpuFlopsClassify(dA, dB, handle=None):
    """-> (hv list, drowIds devptr, dflops devptr, total_flops).  hv has the reference's length (max bin + 2)."""
    assert dA.on_device and dB.on_device
    ids, fl = C.c_void_p(), C.c_void_p()
    hv = (C.c_int * HV_LEN)()
    hv_len, tot = C.c_int(0), C.c_longlong(0)
    rc = lib().hip_gpuFlopsClassify(_hp(handle), *_ptrs(dA.rowPtr, dA.colInd, dB.rowPtr), dA.rows, dA.cols, C.byref(ids),
                                    C.byref(fl), hv, C.byref(hv_len), C.byref(tot))
    _check(rc, "hip_gpuFlopsClassify")
    return [int(x) for x in hv], hv_len.value, ids.value, fl.value, tot.value


def sgpuSpMMWrapper(dA, dB, drowIds, hv, dflops, handle=None):
    assert dA.on_device and dB.on_device
    hv_arr = (C.c_int * HV_LEN)(*hv)
    out = _CsrOut()
    rc = lib().hip_sgpuSpMM(_hp(handle), *_dev_args(dA), *_dev_args(dB), dA.rows, dA.cols, dB.cols, C.c_void_p(drowIds), hv_arr,
                            C.c_void_p(dflops), *out.refs())
    _check(rc, "hip_sgpuSpMM")
    ic, jc, cv, nnz = out.values()
    return CSR(cv, jc, ic, dA.rows, dB.cols, nnz, True)


def scudaSpMM(hA, hB, handle=None):
    """Host CSRs in, host CSR out via classify + binned SpGEMM (mindex2-cuda/nGpuSpMM.cc:245-279)."""
    dA = hA.toGpuCSR()
    dB = dA if hB is hA else hB.toGpuCSR()
    try:
        hv, hv_len, ids, fl, _ = gpuFlopsClassify(dA, dB, handle)
        try:
            dC = sgpuSpMMWrapper(dA, dB, ids, hv, fl, handle)
        finally:
            dev_free(ids)
            dev_free(fl)
        hC = dC.toCpuCSR()
        dC.deviceDispose()
        return hC
    finally:
        dA.deviceDispose()
        if dB is not dA:
            dB.deviceDispose()


def _rmcl_iter_device(dtype, handle, maxIter, rows, cols, gI, gJ, gV, gnnz, tI, tJ, tV, tnnz):
    out = _CsrOut()
    _call("hip_gpuRmclIter_device", dtype, _hp(handle), int(maxIter), int(rows), int(cols), *_ptrs(gI, gJ, gV), int(gnnz),
          *_ptrs(tI, tJ, tV), int(tnnz), *out.refs())
    return out.values()


def rmcl_iter_device_raw(handle, maxIter, rows, cols, gI, gJ, gV, gnnz, tI, tJ, tV, tnnz):
    """hip_gpuRmclIter_device on raw device pointers: maxIter iterations Mt <- prune(Mgt * Mt) without packing Mt between
    them.  Returns (I, J, V, nnz) of the final Mt in pool arrays; release the three with dev_free."""
    return _rmcl_iter_device(np.float32, handle, maxIter, rows, cols, gI, gJ, gV, gnnz, tI, tJ, tV, tnnz)


def rmcl_iter_device_raw_f64(handle, maxIter, rows, cols, gI, gJ, gV, gnnz, tI, tJ, tV, tnnz):
    """rmcl_iter_device_raw with float64 values (hip_gpuRmclIter_device_f64: Mt is packed after every iteration)."""
    return _rmcl_iter_device(np.float64, handle, maxIter, rows, cols, gI, gJ, gV, gnnz, tI, tJ, tV, tnnz)


def gpuRmclIter_device(maxIter, Mgt, Mt, handle=None):
    """hip_gpuRmclIter_device (float32) / _f64 (float64) on device CSRs: returns the new Mt as a device CSR of the
    operands' value type (the inputs are left alone); mixed value types raise before any device work."""
    assert Mgt.on_device and Mt.on_device
    dtype = _common_dtype(Mgt, Mt)
    i_, j_, c_, n_ = _rmcl_iter_device(dtype, handle, maxIter, Mgt.rows, Mgt.cols, Mgt.rowPtr, Mgt.colInd, Mgt.values, Mgt.nnz,
                                       Mt.rowPtr, Mt.colInd, Mt.values, Mt.nnz)
    return CSR(c_, j_, i_, Mt.rows, Mt.cols, n_, on_device=True, dtype=dtype)


def gpuRmclIterTopK_device(maxIter, k, Mgt, Mt, handle=None):
    """hip_gpuRmclIter_device_topk / _f64 on device CSRs: gpuRmclIter_device with every row of Mt cut to its k largest
    entries (and renormalised) after every iteration -> (Mt, iter_nnz, iter_cut): the new Mt as a device CSR, per iteration
    the entries after the selection and the rows it cut."""
    assert Mgt.on_device and Mt.on_device
    dtype = _common_dtype(Mgt, Mt)
    n = max(int(maxIter), 0)
    out, inz, icut = _CsrOut(), (C.c_longlong * max(n, 1))(), (C.c_longlong * max(n, 1))()
    _call("hip_gpuRmclIter_device_topk", dtype, _hp(handle), int(maxIter), int(k), Mgt.rows, Mgt.cols,
          *_ptrs(Mgt.rowPtr, Mgt.colInd, Mgt.values), Mgt.nnz, *_ptrs(Mt.rowPtr, Mt.colInd, Mt.values), Mt.nnz, *out.refs(),
          inz, icut)
    i_, j_, c_, n_ = out.values()
    return CSR(c_, j_, i_, Mt.rows, Mt.cols, n_, on_device=True, dtype=dtype), list(inz)[:n], list(icut)[:n]


def gpuRmclIter(maxIter, Mgt, Mt):
    """void gpuRmclIter(const int maxIter, const CSR Mgt, CSR& Mt): returns the new Mt (host CSR).  float64 operands go to
    hip_gpuRmclIter_f64 (one device); mixed value types raise before any device work."""
    assert not Mgt.on_device and not Mt.on_device
    L = lib()
    dtype = _common_dtype(Mgt, Mt)
    _V = _D if dtype == np.float64 else _F
    fn, name = _typed("hip_gpuRmclIter", dtype)
    oi, oj, ov, on = _I(), _I(), _V(), C.c_int(0)
    rc = fn(int(maxIter), Mgt.rows, Mgt.cols, Mgt.rowPtr.ctypes.data_as(_I), Mgt.colInd.ctypes.data_as(_I),
            Mgt.values.ctypes.data_as(_V), Mgt.nnz, Mt.rowPtr.ctypes.data_as(_I),
            Mt.colInd.ctypes.data_as(_I), Mt.values.ctypes.data_as(_V), Mt.nnz,
            C.byref(oi), C.byref(oj), C.byref(ov), C.byref(on))
    _check(rc, name)
    rp, ci, v = _take_malloced(L, oi, oj, ov, Mt.rows, on.value, dtype)
    return CSR(v, ci, rp, Mt.rows, Mt.cols, on.value, dtype=dtype)


# ---------------------------------------------------------------------------------------------
# multi-GPU behind the C ABI (include/spgemm_hip.h "multi-GPU"): groups of shards, sharded SpGEMM, sharded R-MCL
# ---------------------------------------------------------------------------------------------
def rccl_available():
    """True when the library could load librccl into this process"""
    return lib().spgemm_hip_rccl_available() == 0


def unique_id():
    """128-byte RCCL id made by rank 0 of a multi-process job; hand it to every rank (bytes)."""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib().spgemm_hip_unique_id(buf), "spgemm_hip_unique_id")
    return buf.raw


class Group:
    """spgemm_group.  Group(nshards, devices=None, transport=XCHG_AUTO): every shard in this process (several may share
    a device).  Group.of_rank(nranks, rank, device, id): one process per GPU, wired with unique_id()."""

    def __init__(self, nshards, devices=None, transport=XCHG_AUTO, _ptr=None):
        self._g = C.c_void_p()
        if _ptr is not None:
            self._g = _ptr
        else:
            dv = None
            if devices is not None:
                dv = (C.c_int * len(devices))(*[int(d) for d in devices])
                assert len(devices) == nshards
            _check(lib().spgemm_hip_group_create(C.byref(self._g), int(nshards), dv, int(transport)), "spgemm_hip_group_create")
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(lib().spgemm_hip_group_info(self._g, C.byref(a), C.byref(b), C.byref(c)), "spgemm_hip_group_info")
        self.nranks, self.nlocal, self.transport = a.value, b.value, c.value
        # jobs made on this group and handles borrowed from it: the C side of a job dereferences the group when it is
        # destroyed, and a borrowed Handle points at a handle the group owns -- close() takes them down first, in that order
        self._jobs = weakref.WeakSet()
        self._borrowed = weakref.WeakSet()
        _LIVE.add(self)

    @staticmethod
    def of_rank(nranks, rank, device, id128):
        g = C.c_void_p()
        buf = C.create_string_buffer(bytes(id128), UNIQUE_ID_BYTES)
        _check(lib().spgemm_hip_group_create_rank(C.byref(g), int(nranks), int(rank), int(device), buf),
               "spgemm_hip_group_create_rank")
        return Group(nranks, _ptr=g)

    @property
    def ptr(self):
        return self._g

    def close(self):
        if self._g:
            for j in list(self._jobs):
                j.close()
            for h in list(self._borrowed):
                h._h = C.c_void_p()                   # the handle dies with the group: a later call fails with "null argument"
            lib().spgemm_hip_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_args(M):
    return [M.rowPtr.ctypes.data_as(_I), M.colInd.ctypes.data_as(_I), M.values.ctypes.data_as(_F), int(M.nnz)]


def _take_malloced(L, pi, pj, pv, rows, n, dtype=np.float32):
    """copies of the three malloc()ed arrays a host-array entry point returned, which are then freed"""
    rp = np.ctypeslib.as_array(pi, shape=(rows + 1,)).copy()
    ci = np.ctypeslib.as_array(pj, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    v = np.ctypeslib.as_array(pv, shape=(n,)).copy() if n else np.zeros(0, dtype)
    for p in (pi, pj, pv):                          # CSR::dispose() == free() (nlibs/CSR.h:323-327)
        L.free(C.cast(p, C.c_void_p))
    return rp, ci, v


class ShardedSpMM:
    """spgemm_sharded: C = A*B row-sharded over a Group with the operands resident (host CSRs in; B=None means B=A)."""

    def __init__(self, group, A, B=None):
        assert not A.on_device and (B is None or not B.on_device)
        self.group = group
        self._keep = (A, B)
        self._j = C.c_void_p()
        bargs = _host_args(B) if B is not None else [None, None, None, 0]
        _check(lib().hip_sharded_spmm_create(group.ptr, *_host_args(A), *bargs, A.rows, A.cols,
                                             (B.cols if B is not None else A.cols), C.byref(self._j)), "hip_sharded_spmm_create")
        self.m, self.n = A.rows, (B.cols if B is not None else A.cols)
        group._jobs.add(self)
        _LIVE.add(self)

    def step(self, gather=True):
        """-> (nnzC, total products P)"""
        nz, P = C.c_longlong(0), C.c_longlong(0)
        _check(lib().hip_sharded_spmm_step(self._j, int(bool(gather)), C.byref(nz), C.byref(P)), "hip_sharded_spmm_step")
        return nz.value, P.value

    def result(self, local_shard=0):
        L = lib()
        pi, pj, pv, n, rows = _I(), _I(), _F(), C.c_int(0), C.c_int(0)
        _check(L.hip_sharded_spmm_result(self._j, int(local_shard), C.byref(pi), C.byref(pj), C.byref(pv), C.byref(n),
                                         C.byref(rows)), "hip_sharded_spmm_result")
        rp, ci, v = _take_malloced(L, pi, pj, pv, rows.value, n.value)
        return CSR(v, ci, rp, rows.value, self.n, n.value)

    def handle(self, local_shard=0):
        """the spgemm_handle of a local shard as a (non-owning) Handle: stats(), set_kernel_timing()"""
        p = lib().hip_sharded_spmm_handle(self._j, int(local_shard))
        if not p:
            raise SpgemmError("no such local shard")
        h = Handle(_borrowed=p)
        self.group._borrowed.add(h)
        return h

    def info(self):
        ends = (C.c_int * (self.group.nranks + 1))()
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().hip_sharded_spmm_info(self._j, ends, C.byref(a), C.byref(b)), "hip_sharded_spmm_info")
        return {"ends": [int(x) for x in ends], "ms_compute": a.value, "ms_exchange": b.value}

    def close(self):
        if self._j:
            lib().hip_sharded_spmm_destroy(self._j)
            self._j = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedRmcl:
    """spgemm_sharded_rmcl: the R-MCL loop over a Group with the operands resident (host CSRs in once; every run() starts
    from the initial Mt and leaves the result on the shards)."""

    def __init__(self, group, Mgt, Mt):
        assert not Mgt.on_device and not Mt.on_device
        self.group = group
        self._keep = (Mgt, Mt)
        self.rows, self.cols = Mt.rows, Mt.cols
        self._j = C.c_void_p()
        _check(lib().hip_sharded_rmcl_create(group.ptr, Mgt.rows, Mgt.cols, *_host_args(Mgt), *_host_args(Mt), C.byref(self._j)),
               "hip_sharded_rmcl_create")
        group._jobs.add(self)
        _LIVE.add(self)

    def run(self, maxIter, restart=True):
        """maxIter iterations from the initial Mt (restart=False: from the previous run's result) -> nnz of the final Mt"""
        n = C.c_int(0)
        fn = lib().hip_sharded_rmcl_run if restart else lib().hip_sharded_rmcl_continue
        _check(fn(self._j, int(maxIter), C.byref(n)), "hip_sharded_rmcl_run")
        return n.value

    def iter_nnz(self):
        buf = (C.c_longlong * 256)()
        n = lib().hip_sharded_rmcl_iter_nnz(self._j, buf, 256)
        return [int(buf[i]) for i in range(min(n, 256))]

    def result(self, local_shard=0):
        L = lib()
        pi, pj, pv, n = _I(), _I(), _F(), C.c_int(0)
        _check(L.hip_sharded_rmcl_result(self._j, int(local_shard), C.byref(pi), C.byref(pj), C.byref(pv), C.byref(n)),
               "hip_sharded_rmcl_result")
        rp, ci, v = _take_malloced(L, pi, pj, pv, self.rows, n.value)
        return CSR(v, ci, rp, self.rows, self.cols, n.value)

    def ends(self):
        e = (C.c_int * (self.group.nranks + 1))()
        _check(lib().hip_sharded_rmcl_info(self._j, e), "hip_sharded_rmcl_info")
        return [int(x) for x in e]

    def close(self):
        if self._j:
            lib().hip_sharded_rmcl_destroy(self._j)
            self._j = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gpuRmclIter_sharded(group, maxIter, Mgt, Mt):
    """gpuRmclIter over a Group (hip_gpuRmclIter_sharded): returns the new Mt (host CSR)."""
    assert not Mgt.on_device and not Mt.on_device
    L = lib()
    oi, oj, ov, on = _I(), _I(), _F(), C.c_int(0)
    rc = L.hip_gpuRmclIter_sharded(group.ptr, int(maxIter), Mgt.rows, Mgt.cols, *_host_args(Mgt), *_host_args(Mt),
                                   C.byref(oi), C.byref(oj), C.byref(ov), C.byref(on))
    _check(rc, "hip_gpuRmclIter_sharded")
    rp, ci, v = _take_malloced(L, oi, oj, ov, Mt.rows, on.value)
    return CSR(v, ci, rp, Mt.rows, Mt.cols, on.value)


def sort_rows_device(dC, handle=None):
    """CSR::makeOrdered on a device CSR (hip_csr_sort_rows, or hip_csr_sort_rows_f64 for float64 values)."""
    _call("hip_csr_sort_rows", dC.dtype, _hp(handle), dC.rows, *_ptrs(dC.rowPtr, dC.colInd, dC.values))


@contextlib.contextmanager
def _sorted_copy_pair(mine, dB, handle):
    """-> (mine, a deep copy of dB), both row-sorted on the device, for one comparison; dB itself is left alone.  Owns
    `mine` (a device CSR made for the comparison) and the copy: both are released on the way out."""
    try:
        ib, jb, vb = _csr_permute(dB.dtype, handle, dB.rows, dB.cols, dB.nnz, dB.rowPtr, dB.colInd, dB.values)   # identity maps
        theirs = CSR(vb, jb, ib, dB.rows, dB.cols, dB.nnz, True, dtype=dB.dtype)
        try:
            sort_rows_device(mine, handle)
            sort_rows_device(theirs, handle)
            yield mine, theirs
        finally:
            theirs.deviceDispose()
    finally:
        mine.deviceDispose()


# what the two tiled formats (BCSR, MCSR's corner) share: rowPtr / colInd / values of nnzb tiles of r x c, nnz entries in them
def _check_tile(r, c):
    if r < 1 or c < 1 or r * c > BCSR_MAX_TILE:
        raise SpgemmError(f"tile r={r} c={c}: need r >= 1, c >= 1, r * c <= {BCSR_MAX_TILE}")


def _tile_density(t):
    cells = t.nnzb * t.r * t.c
    return float(t.nnz) / cells * 100.0 if cells else 0.0


def _free_tiles(t):
    for p in (t.rowPtr, t.colInd, t.values):
        dev_free(p)
    t.rowPtr = t.colInd = t.values = None
    t.nnzb = 0


# ---------------------------------------------------------------------------------------------
# column-partitioned CSR (include/spgemm_hip.h "column-partitioned CSR"): split, blockwise product, join
# ---------------------------------------------------------------------------------------------
def _block_table(blocks):
    """blocks: sequence of (rowPtr, colInd, values, nnz) device pointers -> the four host arrays the C side takes"""
    c = len(blocks)
    cols = [(C.c_void_p * c)(*[b[i] for b in blocks]) for i in range(3)]
    return cols + [(C.c_int * c)(*[int(b[3]) for b in blocks])]


def csr_split_columns_raw(handle, m, n, nnz, IA, JA, VA, c, dtype=np.float32):
    """hip_csr_split_columns (float32) / _f64 on raw device pointers -> (dIP, dJP, dP, blockPtr): the packed arrays from
    the library pool (release the three with dev_free) and the host list of c + 1 block starts."""
    out = _CsrOut(count=False)
    bp = (C.c_int * (max(int(c), 0) + 1))()
    _call("hip_csr_split_columns", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA), int(c), *out.refs(), bp)
    return out.values() + ([int(x) for x in bp],)


def pcsr_join_raw(handle, m, n, blocks, dtype=np.float32):
    """hip_pcsr_join / _f64: blocks = c tuples (rowPtr, colInd, values, nnz) of device pointers, each an m x stride CSR
    -> (dIC, dJC, dC, nnz) from the library pool (release with dev_free)."""
    out = _CsrOut()
    _call("hip_pcsr_join", dtype, _hp(handle), int(m), int(n), len(blocks), *_block_table(blocks), *out.refs())
    return out.values()


def pcsr_spmm_raw(handle, IA, JA, VA, nnzA, m, k, n, blocks, dtype=np.float32):
    """hip_pcsr_spmm / _f64: A (m x k) times the c blocks of a k x n matrix -> list of c tuples (dIC, dJC, dC, nnz), each
    its own allocation (release with dev_free).  handle.stats() afterwards describes the last block's product."""
    c = len(blocks)
    ic, jc, cv, nnz = (C.c_void_p * c)(), (C.c_void_p * c)(), (C.c_void_p * c)(), (C.c_int * c)()
    _call("hip_pcsr_spmm", dtype, _hp(handle), *_ptrs(IA, JA, VA), int(nnzA), int(m), int(k), int(n), c, *_block_table(blocks),
          ic, jc, cv, nnz)
    return [(ic[b], jc[b], cv[b], int(nnz[b])) for b in range(c)]


class PCSR:
    """Mirror of the reference's `struct PCSR` (nlibs/PCSR.h:5-10) on device arrays: rows, cols, c and c blocks, each a
    device CSR of shape rows x stride with block-local columns.

    PCSR(dM, c) splits a device CSR (hip_csr_split_columns): the blocks are views into three packed arrays, which
    deviceDispose() releases (PCSR::dispose frees the base arrays only).  spmm_left(A) returns a PCSR whose blocks are
    separate allocations (spmm(A, pB), correctTests/pcsrTest.cc:7-19)."""

    def __init__(self, dM, c, handle=None):
        assert dM.on_device
        ip, jp, vp, bp = csr_split_columns_raw(handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, c, dM.dtype)
        self.rows, self.cols, self.c, self.dtype = dM.rows, dM.cols, int(c), dM.dtype
        self.blockPtr = bp
        self._base = (ip, jp, vp)
        isz = self.dtype.itemsize
        self.blocks = [CSR(vp + isz * bp[b], jp + 4 * bp[b], ip + 4 * b * (self.rows + 1), self.rows, self.stride,
                           bp[b + 1] - bp[b], True, dtype=self.dtype) for b in range(self.c)]

    @staticmethod
    def from_csr(dM, c, handle=None):
        return PCSR(dM, c, handle)

    @staticmethod
    def _of_blocks(blocks, rows, cols, dtype):
        p = PCSR.__new__(PCSR)
        p.rows, p.cols, p.c, p.dtype = rows, cols, len(blocks), np.dtype(dtype)
        p.blocks, p._base = blocks, None
        p.blockPtr = [0]
        for b in blocks:
            p.blockPtr.append(p.blockPtr[-1] + b.nnz)
        return p

    @property
    def stride(self):
        return max(1, (self.cols + self.c - 1) // self.c)

    def nnz(self):
        return sum(b.nnz for b in self.blocks)

    def block(self, b):
        """block b as a device CSR; a view: it is released with the PCSR, never on its own"""
        return self.blocks[b]

    def _table(self):
        return [(b.rowPtr, b.colInd, b.values, b.nnz) for b in self.blocks]

    def join(self, handle=None):
        """hip_pcsr_join -> device CSR rows x cols: row i = block 0's row i, block 1's row i, ... with global columns"""
        ic, jc, cv, nnz = pcsr_join_raw(handle, self.rows, self.cols, self._table(), self.dtype)
        return CSR(cv, jc, ic, self.rows, self.cols, nnz, True, dtype=self.dtype)

    def spmm_left(self, dA, handle=None):
        """A * self block by block (hip_pcsr_spmm) -> PCSR of shape A.rows x cols, every block its own allocation"""
        assert dA.on_device
        if dA.cols != self.rows:
            raise SpgemmError(f"shape mismatch: A is {dA.rows}x{dA.cols}, the partitioned matrix is {self.rows}x{self.cols}")
        if _value_dtype(dA.dtype) != self.dtype:
            raise SpgemmError(f"mixed value types: A is {dA.dtype}, the partitioned matrix is {self.dtype}")
        outs = pcsr_spmm_raw(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dA.rows, dA.cols, self.cols, self._table(),
                             self.dtype)
        blocks = [CSR(cv, jc, ic, dA.rows, self.stride, nnz, True, dtype=self.dtype) for ic, jc, cv, nnz in outs]
        return PCSR._of_blocks(blocks, dA.rows, self.cols, self.dtype)

    def isEqual(self, dB, handle=None):
        """PCSR::isEqual (nlibs/PCSR.h:52-100): the joined blocks against the device CSR dB by CSR.isEqual's rule, both
        sides row-sorted on the device first (dB itself is left alone: a copy is sorted).  Another shape or nnz: False
        before any device work."""
        assert dB.on_device
        if (self.rows, self.cols, self.nnz()) != (dB.rows, dB.cols, dB.nnz):
            return False
        if _value_dtype(dB.dtype) != self.dtype:
            raise SpgemmError(f"mixed value types: the partitioned matrix is {self.dtype}, B is {dB.dtype}")
        with _sorted_copy_pair(self.join(handle), dB, handle) as (mine, theirs):
            return mine.isEqual(theirs, handle)

    def deviceDispose(self):
        if self._base is not None:
            for p in self._base:
                dev_free(p)
            self._base = None
        else:
            for b in self.blocks:
                b.deviceDispose()
        self.blocks = []


# ---------------------------------------------------------------------------------------------
# blocked CSR (include/spgemm_hip.h "blocked CSR"): a CSR as r x c dense tiles, and back
# ---------------------------------------------------------------------------------------------
def csr_to_bcsr_raw(handle, m, n, nnz, IA, JA, VA, r, c, dtype=np.float32):
    """hip_csr_to_bcsr (float32) / _f64 on raw device pointers -> (dIB, dJB, dB, nnzb): block rowPtr int[bm + 1], block
    columns int[nnzb], nnzb * r * c values, all from the library pool (release with dev_free)."""
    out = _CsrOut()
    _call("hip_csr_to_bcsr", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA), int(r), int(c), *out.refs())
    return out.values()


def bcsr_to_csr_raw(handle, m, n, r, c, nnzb, IB, JB, VB, drop_tol=1e-9, dtype=np.float32):
    """hip_bcsr_to_csr / _f64: the tiles written out row by row -> (dIC, dJC, dC, nnz) from the library pool; a cell is kept
    when its column is below n and fabs(value) > drop_tol (compared in double)."""
    out = _CsrOut()
    _call("hip_bcsr_to_csr", dtype, _hp(handle), int(m), int(n), int(r), int(c), int(nnzb), *_ptrs(IB, JB, VB), float(drop_tol),
          *out.refs())
    return out.values()


class BCSR:
    """Mirror of the reference's `struct BCSR` (nlibs/BCSR.h:6-64) on device arrays: an m x n matrix as r x c dense tiles.
    Fields m, n, r, c, bm, bn, nnzb, nnz (the source CSR's, as the reference keeps it) and the three device arrays rowPtr
    (int[bm + 1]), colInd (int[nnzb] block columns), values (nnzb * r * c).  r comes before c, as in the reference's
    definition (its header declares them the other way round)."""

    def __init__(self, dM, r, c, handle=None):
        assert dM.on_device
        r, c = int(r), int(c)
        _check_tile(r, c)
        self.dtype = _value_dtype(dM.dtype)
        self.m, self.n, self.r, self.c, self.nnz = dM.rows, dM.cols, r, c, dM.nnz
        self.bm, self.bn = (self.m + r - 1) // r, (self.n + c - 1) // c
        self.rowPtr, self.colInd, self.values, self.nnzb = csr_to_bcsr_raw(
            handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, r, c, self.dtype)

    @staticmethod
    def from_csr(dM, r, c, handle=None):
        return BCSR(dM, r, c, handle)

    def to_csr(self, drop_tol=1e-9, handle=None):
        """hip_bcsr_to_csr -> device CSR m x n: row i = the tiles of its block row in storage order, ascending inside a tile"""
        ic, jc, cv, nnz = bcsr_to_csr_raw(handle, self.m, self.n, self.r, self.c, self.nnzb, self.rowPtr, self.colInd,
                                          self.values, drop_tol, self.dtype)
        return CSR(cv, jc, ic, self.m, self.n, nnz, True, dtype=self.dtype)

    def nonzero_density(self):
        """BCSR::nonzeroDensity (nlibs/BCSR.h:61-63): nnz / (nnzb * r * c) * 100; 0.0 without tiles (the reference
        divides by zero there)"""
        return _tile_density(self)

    def is_equal(self, dB, handle=None):
        """BCSR::isEqual (nlibs/BCSR.cc:67-116) against a device CSR: the tiles written out with drop_tol = 1e-9 and a
        copy of dB, both row-sorted on the device, then one hip_csr_diff report with abs_tol = 1e-9: true iff the row
        lengths agree, no common column is further than 1e-9 apart and no entry only dB holds exceeds 1e-9.  dB itself
        is left alone.  Another shape or value type raises before any device work."""
        assert dB.on_device
        if (self.m, self.n) != (dB.rows, dB.cols):
            raise SpgemmError(f"shape mismatch: the blocked matrix is {self.m}x{self.n}, B is {dB.rows}x{dB.cols}")
        if _value_dtype(dB.dtype) != self.dtype:
            raise SpgemmError(f"mixed value types: the blocked matrix is {self.dtype}, B is {dB.dtype}")
        with _sorted_copy_pair(self.to_csr(1e-9, handle), dB, handle) as (mine, theirs):
            d = _csr_diff(self.dtype, handle, self.m, self.n, mine.rowPtr, mine.colInd, mine.values, mine.nnz, theirs.rowPtr,
                          theirs.colInd, theirs.values, theirs.nnz, 0.0, 1e-9)
            return d.rows_len_differ == 0 and d.beyond == 0 and d.max_abs_only_b <= 1e-9

    def dispose(self):
        _free_tiles(self)


# ---------------------------------------------------------------------------------------------
# mixed CSR (include/spgemm_hip.h "mixed CSR"): the top-left corner as r x c dense tiles, the rest as a CSR, and back
# ---------------------------------------------------------------------------------------------
def _check_corner(m, n, r, c, blockRows, blockCols):
    _check_tile(r, c)
    if not (0 <= blockRows <= m and 0 <= blockCols <= n):
        raise SpgemmError(f"corner {blockRows} x {blockCols} outside the {m} x {n} matrix")
    if blockRows % r:
        raise SpgemmError(f"corner: blockRows={blockRows} is not a multiple of r={r}")


def csr_to_mcsr_raw(handle, m, n, nnz, IA, JA, VA, r, c, blockRows, blockCols, dtype=np.float32):
    """hip_csr_to_mcsr (float32) / _f64 on raw device pointers -> (dIB, dJB, dB, nnzb, dIR, dJR, dR, nnzR): the corner's
    block rowPtr int[blockRows / r + 1], block columns int[nnzb] and nnzb * r * c values, then the m x n remainder CSR; all
    from the library pool (release with dev_free)."""
    corner, rest = _CsrOut(), _CsrOut()
    _call("hip_csr_to_mcsr", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA), int(r), int(c), int(blockRows),
          int(blockCols), *corner.refs(), *rest.refs())
    return corner.values() + rest.values()


def mcsr_to_csr_raw(handle, m, n, r, c, blockRows, blockCols, nnzb, IB, JB, VB, nnzR, IR, JR, VR, drop_tol=1e-9,
                    dtype=np.float32):
    """hip_mcsr_to_csr / _f64: row i = the corner's row (as hip_bcsr_to_csr writes it) followed by the remainder's row
    -> (dIC, dJC, dC, nnz) from the library pool."""
    out = _CsrOut()
    _call("hip_mcsr_to_csr", dtype, _hp(handle), int(m), int(n), int(r), int(c), int(blockRows), int(blockCols), int(nnzb),
          *_ptrs(IB, JB, VB), int(nnzR), *_ptrs(IR, JR, VR), float(drop_tol), *out.refs())
    return out.values()


class MCSR:
    """Mirror of the reference's `struct MCSR : public CSR, BCSR` (nlibs/MCSR.h:6-9, the fill pass nlibs/MCSR.cc:58-92) on
    device arrays.  The BCSR side: rowPtr (int[bm + 1]), colInd (int[nnzb] block columns), values (nnzb * r * c) and
    the fields m, n (the whole matrix), r, c, blockRows, blockCols, bm = blockRows / r, bn = ceil(blockCols / c), nnzb and
    nnz = the entries that went into the corner, repeats counted.  The CSR side: `remainder`, a device CSR m x n with
    global columns.  r comes before c, as in the reference's definition."""

    def __init__(self, dM, r, c, blockRows, blockCols, handle=None):
        assert dM.on_device
        r, c, blockRows, blockCols = int(r), int(c), int(blockRows), int(blockCols)
        _check_corner(dM.rows, dM.cols, r, c, blockRows, blockCols)
        self.dtype = _value_dtype(dM.dtype)
        self.m, self.n, self.r, self.c, self.blockRows, self.blockCols = dM.rows, dM.cols, r, c, blockRows, blockCols
        self.bm, self.bn = blockRows // r, (blockCols + c - 1) // c
        self.rowPtr, self.colInd, self.values, self.nnzb, ir, jr, vr, nnzr = csr_to_mcsr_raw(
            handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, r, c, blockRows, blockCols, self.dtype)
        self.remainder = CSR(vr, jr, ir, dM.rows, dM.cols, nnzr, True, dtype=self.dtype)
        self.nnz = dM.nnz - nnzr

    @staticmethod
    def from_csr(dM, r, c, blockRows, blockCols, handle=None):
        return MCSR(dM, r, c, blockRows, blockCols, handle)

    def to_csr(self, drop_tol=1e-9, handle=None):
        """hip_mcsr_to_csr -> device CSR m x n: the corner's row i, then the remainder's row i"""
        rest = self.remainder
        if (rest.rows, rest.cols) != (self.m, self.n):
            raise SpgemmError(f"shape mismatch: the mixed matrix is {self.m}x{self.n}, its remainder {rest.rows}x{rest.cols}")
        if _value_dtype(rest.dtype) != self.dtype:
            raise SpgemmError(f"mixed value types: the corner is {self.dtype}, the remainder {rest.dtype}")
        _check_corner(self.m, self.n, self.r, self.c, self.blockRows, self.blockCols)
        ic, jc, cv, nnz = mcsr_to_csr_raw(handle, self.m, self.n, self.r, self.c, self.blockRows, self.blockCols, self.nnzb,
                                          self.rowPtr, self.colInd, self.values, rest.nnz, rest.rowPtr, rest.colInd,
                                          rest.values, drop_tol, self.dtype)
        return CSR(cv, jc, ic, self.m, self.n, nnz, True, dtype=self.dtype)

    def nonzero_density(self):
        """BCSR::nonzeroDensity (nlibs/BCSR.h:61-63) of the corner: nnz / (nnzb * r * c) * 100; 0.0 without tiles"""
        return _tile_density(self)

    def dispose(self):
        _free_tiles(self)
        if self.remainder is not None:
            self.remainder.deviceDispose()
            self.remainder = None


# ---------------------------------------------------------------------------------------------
# dense matrix (include/spgemm_hip.h "dense matrix"): CSR -> dense, dense -> CSR, the dense product
# ---------------------------------------------------------------------------------------------
def csr_to_dense_raw(handle, m, n, nnz, IA, JA, VA, D, ld, dtype=np.float32):
    """hip_csr_to_dense (float32) / _f64 on raw device pointers: fills the caller's m x ld row-major buffer D in [i][0..n)
    (+0.0 where no entry lands, the last of a repeated (row, col) stays); the padding [i][n..ld) is not written."""
    _call("hip_csr_to_dense", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA, D), int(ld))


def dense_to_csr_raw(handle, m, n, D, ld, rule=DENSE_KEEP_REFERENCE, tol=1e-8, dtype=np.float32):
    """hip_dense_to_csr / _f64 -> (dIC, dJC, dC, nnz) from the library pool: row i = the kept cells of dense row i in
    ascending column order.  DENSE_KEEP_REFERENCE drops a cell when value < tol (CSR::initWithDenseMatrix at 1e-8: NaN is
    kept, negatives go), DENSE_KEEP_ABS keeps it when fabs(value) > tol; both compare in double."""
    out = _CsrOut()
    _call("hip_dense_to_csr", dtype, _hp(handle), int(m), int(n), C.c_void_p(D), int(ld), int(rule), float(tol), *out.refs())
    return out.values()


def dense_gemm_raw(handle, m, n, k, A, lda, B, ldb, Cd, ldc, dtype=np.float32):
    """hip_dense_gemm / _f64: C[m x n] = A[m x k] * B[k x n] on row-major device arrays (alpha 1, beta 0, no transposes)."""
    _call("hip_dense_gemm", dtype, _hp(handle), int(m), int(n), int(k), C.c_void_p(A), int(lda), C.c_void_p(B), int(ldb),
          C.c_void_p(Cd), int(ldc))


class DenseMatrix:
    """Mirror of the reference's `struct DenseMatrix` (nlibs/DenseMatrix.h) on a device array: rows x cols values,
    row-major with leading dimension ld (= cols for everything made here).  Fields values (device pointer), rows, cols,
    ld, dtype."""

    def __init__(self, dM=None, handle=None):
        """DenseMatrix(const CSR&) on a device CSR: zero-fill, then every entry in storage order (the last of a repeated
        column stays)"""
        self.values, self.rows, self.cols, self.ld, self.dtype = None, 0, 0, 0, np.dtype(np.float32)
        if dM is None:
            return
        assert dM.on_device
        self._alloc(dM.rows, dM.cols, dM.dtype)
        try:
            csr_to_dense_raw(handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, self.values, self.ld, self.dtype)
        except SpgemmError:
            self.dispose()
            raise

    def _alloc(self, rows, cols, dtype):
        rows, cols = int(rows), int(cols)
        if rows < 0 or cols < 0:
            raise SpgemmError(f"negative shape {rows}x{cols}")
        self.dtype = np.dtype(_value_dtype(dtype))
        self.rows, self.cols, self.ld = rows, cols, cols
        self.values = dev_alloc(rows * cols * self.dtype.itemsize)

    @staticmethod
    def zeros(rows, cols, dtype=np.float32):
        return DenseMatrix.from_host(np.zeros((int(rows), int(cols)), _value_dtype(dtype)))

    @staticmethod
    def from_host(array):
        """a 2-D float32 / float64 numpy array, uploaded row-major"""
        array = np.asarray(array)
        if array.ndim != 2:
            raise SpgemmError(f"a dense matrix is 2-D, got {array.ndim} dimensions")
        d = DenseMatrix()
        d._alloc(array.shape[0], array.shape[1], array.dtype)
        flat = np.ascontiguousarray(array)
        if flat.nbytes:
            _check(lib().spgemm_hip_memcpy_h2d(C.c_void_p(d.values), flat.ctypes.data_as(C.c_void_p), flat.nbytes), "h2d")
        return d

    def to_csr(self, rule=DENSE_KEEP_REFERENCE, tol=1e-8, handle=None):
        """CSR::initWithDenseMatrix on the device -> device CSR; the defaults are the reference's rule"""
        ic, jc, cv, nnz = dense_to_csr_raw(handle, self.rows, self.cols, self.values, self.ld, rule, tol, self.dtype)
        return CSR(cv, jc, ic, self.rows, self.cols, nnz, True, dtype=self.dtype)

    def matmul(self, other, handle=None):
        """self * other -> a new DenseMatrix.  Another value type or an inner dimension that does not match raises before
        any device work."""
        if not isinstance(other, DenseMatrix):
            raise SpgemmError("matmul takes a DenseMatrix")
        if other.dtype != self.dtype:
            raise SpgemmError(f"mixed value types: {self.dtype} times {other.dtype}")
        if self.cols != other.rows:
            raise SpgemmError(f"shape mismatch: {self.rows}x{self.cols} times {other.rows}x{other.cols}")
        out = DenseMatrix()
        out._alloc(self.rows, other.cols, self.dtype)
        try:
            dense_gemm_raw(handle, self.rows, other.cols, self.cols, self.values, self.ld, other.values, other.ld,
                           out.values, out.ld, self.dtype)
        except SpgemmError:
            out.dispose()
            raise
        return out

    def download(self):
        """-> rows x cols numpy array (the padding of a wider ld is left behind)"""
        flat = d2h(self.values, self.rows * self.ld, self.dtype)
        return flat.reshape(self.rows, self.ld)[:, :self.cols].copy() if self.rows else flat.reshape(0, self.cols)

    def dispose(self):
        dev_free(self.values)
        self.values = None


# ---------------------------------------------------------------------------------------------
# edge-list text (include/spgemm_hip.h "the text in front of that step"): lines "from to [value]" -> device COO, a file
# -> device CSR; the text half of COO::readSNAPFile (nlibs/COO.cc:48-158) on the device
# ---------------------------------------------------------------------------------------------
EDGES_ONE_BASED, EDGES_TRANSPOSE = 1, 2


def _edge_bytes(data, what):
    """the text as bytes; anything that is not bytes-like is refused before any device work"""
    if isinstance(data, str) or not isinstance(data, (bytes, bytearray, memoryview)):
        raise SpgemmError(f"{what}: the text must be bytes, not {type(data).__name__}")
    return bytes(data)


def _edge_flags(flags):
    flags = int(flags)
    if flags & ~(EDGES_ONE_BASED | EDGES_TRANSPOSE):
        raise SpgemmError(f"unknown edge flags 0x{flags:x}: EDGES_ONE_BASED | EDGES_TRANSPOSE")
    return flags


def edge_text_header(data):
    """hip_edge_text_header (pure host): the banner, comment lines and size line of a SNAP / MatrixMarket text ->
    {rows, cols, declared, one_based, symmetric, data_offset}.  A text without a size line raises."""
    data = _edge_bytes(data, "edge_text_header")
    rows, cols, declared, one, sym, off = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    _check(lib().hip_edge_text_header(data, len(data), C.byref(rows), C.byref(cols), C.byref(declared), C.byref(one),
                                      C.byref(sym), C.byref(off)), "hip_edge_text_header")
    return {"rows": rows.value, "cols": cols.value, "declared": declared.value, "one_based": bool(one.value),
            "symmetric": bool(sym.value), "data_offset": int(off.value)}


def _parse_edge_lines(dtype, handle, dText, nbytes, declared, flags):
    flags = _edge_flags(flags)
    out, st = _CsrOut(), EdgeStats()
    _call("hip_parse_edge_lines", dtype, _hp(handle), C.c_void_p(dText), int(nbytes), int(declared), flags, *out.refs(),
          C.byref(st))
    return out.values() + (st.as_dict(),)


def parse_edge_lines_raw(handle, dText, nbytes, declared, flags=0):
    """hip_parse_edge_lines on a raw device pointer (16-byte aligned text) -> (dRow, dCol, dVal, entries, stats dict);
    the three arrays come from the library pool (release with dev_free)."""
    return _parse_edge_lines(np.float32, handle, dText, nbytes, declared, flags)


def parse_edge_lines_raw_f64(handle, dText, nbytes, declared, flags=0):
    """parse_edge_lines_raw with float64 values (hip_parse_edge_lines_f64)."""
    return _parse_edge_lines(np.float64, handle, dText, nbytes, declared, flags)


class EdgeTriplets:
    """device COO triplets in line order, as hip_parse_edge_text leaves them: row, col (int32) and val (`dtype`: float32
    or float64) device pointers, their count `entries` and the call's `stats`"""

    def __init__(self, row, col, val, entries, stats, dtype=np.float32):
        self.row, self.col, self.val, self.entries, self.stats = row, col, val, int(entries), stats
        self.dtype = _value_dtype(dtype)

    def download(self):
        """-> (row, col, val) numpy arrays of `entries` elements"""
        return (d2h(self.row, self.entries, np.int32), d2h(self.col, self.entries, np.int32),
                d2h(self.val, self.entries, self.dtype))

    def dispose(self):
        for p in (self.row, self.col, self.val):
            dev_free(p)
        self.row = self.col = self.val = None


def parse_edge_text(data, declared, one_based=False, transpose=False, handle=None, dtype=np.float32):
    """hip_parse_edge_text: host bytes holding edge lines -> EdgeTriplets on the device.  At most `declared` lines are
    read; one_based subtracts 1 from both indices (MatrixMarket), transpose swaps them (isTrans).  dtype: np.float32, or
    np.float64 for double values (hip_parse_edge_text_f64)."""
    data = _edge_bytes(data, "parse_edge_text")
    dtype = _value_dtype(dtype)
    flags = (EDGES_ONE_BASED if one_based else 0) | (EDGES_TRANSPOSE if transpose else 0)
    out, st = _CsrOut(), EdgeStats()
    _call("hip_parse_edge_text", dtype, _hp(handle), data, len(data), int(declared), flags, *out.refs(), C.byref(st))
    r, c, v, n = out.values()
    return EdgeTriplets(r, c, v, n, st.as_dict(), dtype)


def read_edge_file(path, isTrans=True, flags=COO_DEDUPE, handle=None, dtype=np.float32):
    """hip_read_edge_file: COO::readSNAPFile(path, isTrans) + hip_coo_to_csr(flags) without the triplets ever on the host
    -> device `CSR` (its .edge_stats: the parse's stats).  A symmetric MatrixMarket file raises (use the host loader).
    dtype: np.float32, or np.float64 for a double device CSR (hip_read_edge_file_f64)."""
    dtype = _value_dtype(dtype)
    if not isinstance(path, (str, bytes, os.PathLike)):
        raise SpgemmError(f"read_edge_file: path must be a str, bytes or os.PathLike, not {type(path).__name__}")
    flags = int(flags)
    if flags & ~(COO_DEDUPE | COO_SELF_LOOPS | COO_ROW_NORMALISE | COO_ABS):
        raise SpgemmError(f"unknown COO flags 0x{flags:x}")
    out, st, rows, cols = _CsrOut(), EdgeStats(), C.c_int(), C.c_int()
    _call("hip_read_edge_file", dtype, _hp(handle), os.fsencode(path), int(bool(isTrans)), flags, C.byref(rows), C.byref(cols),
          *out.refs(), C.byref(st))
    ia, ja, av, nnz = out.values()
    M = CSR(av, ja, ia, rows.value, cols.value, nnz, True, dtype=dtype)
    M.edge_stats = st.as_dict()
    return M


# ---------------------------------------------------------------------------------------------
# the way out (include/spgemm_hip.h "the way out"): a device CSR -> edge-list text, formatted on the device; what
# toCpuCSR + CSR::output's printf loop (nlibs/CSR.cc) does on the host
# ---------------------------------------------------------------------------------------------
EDGE_FMT_FIXED6, EDGE_FMT_ROUNDTRIP = 0, 1
EDGE_HEADER_NONE, EDGE_HEADER_SIZES, EDGE_HEADER_MATRIX_MARKET = 0, 1, 2


def edge_text_write_header(header, rows, cols, entries):
    """hip_edge_text_write_header (pure host) -> the header bytes: b"" (0), the size line "rows cols entries" (1), or a
    MatrixMarket banner and the size line (2)."""
    buf, n = C.create_string_buffer(128), C.c_size_t()
    _check(lib().hip_edge_text_write_header(buf, len(buf), int(header), int(rows), int(cols), int(entries), C.byref(n)),
           "hip_edge_text_write_header")
    return buf.raw[:n.value]


def _edge_write_args(what, dM, row0, row1, fmt, flags, dtype):
    """what every write call checks before any device work -> (dtype, row0, row1, fmt, flags)"""
    if not isinstance(dM, CSR) or not dM.on_device:
        raise SpgemmError(f"{what}: takes a device CSR")
    dtype = _value_dtype(dM.dtype if dtype is None else dtype)
    if dtype != dM.dtype:
        raise SpgemmError(f"{what}: dtype {dtype} does not match the matrix's {dM.dtype}")
    fmt = int(fmt)
    if fmt not in (EDGE_FMT_FIXED6, EDGE_FMT_ROUNDTRIP):
        raise SpgemmError(f"{what}: unknown fmt {fmt}: EDGE_FMT_FIXED6 or EDGE_FMT_ROUNDTRIP")
    row0, row1 = int(row0), dM.rows if row1 is None else int(row1)
    if not 0 <= row0 <= row1 <= dM.rows:
        raise SpgemmError(f"{what}: rows [{row0}, {row1}) of {dM.rows}")
    return dtype, row0, row1, fmt, _edge_flags(flags)


def format_csr_edges(dM, row0=0, row1=None, fmt=EDGE_FMT_FIXED6, flags=0, handle=None, dtype=None):
    """hip_format_csr_edges: rows [row0, row1) of the device CSR `dM` as text in device memory -> (dText, nbytes, stats
    dict); dText comes from the library pool (release with dev_free).  dtype: None = the matrix's, else it must match."""
    dtype, row0, row1, fmt, flags = _edge_write_args("format_csr_edges", dM, row0, row1, fmt, flags, dtype)
    text, n, st = C.c_void_p(), C.c_size_t(), EdgeWriteStats()
    _call("hip_format_csr_edges", dtype, _hp(handle), dM.rows, dM.cols, *_ptrs(dM.rowPtr, dM.colInd, dM.values), row0, row1,
          fmt, flags, C.byref(text), C.byref(n), C.byref(st))
    return text.value, int(n.value), st.as_dict()


def csr_to_edge_text(dM, row0=0, row1=None, fmt=EDGE_FMT_FIXED6, flags=0, handle=None, dtype=None):
    """hip_csr_to_edge_text: the same text on the host -> (bytes, stats dict): a first call sizes the buffer, a second
    fills it."""
    dtype, row0, row1, fmt, flags = _edge_write_args("csr_to_edge_text", dM, row0, row1, fmt, flags, dtype)
    args = (_hp(handle), dM.rows, dM.cols, *_ptrs(dM.rowPtr, dM.colInd, dM.values), row0, row1, fmt, flags)
    n, st = C.c_size_t(), EdgeWriteStats()
    _call("hip_csr_to_edge_text", dtype, *args, None, 0, C.byref(n), None)
    buf = C.create_string_buffer(max(int(n.value), 1))
    _call("hip_csr_to_edge_text", dtype, *args, buf, int(n.value), C.byref(n), C.byref(st))
    return buf.raw[:n.value], st.as_dict()


def write_edge_file(dM, path, fmt=EDGE_FMT_FIXED6, flags=0, header=EDGE_HEADER_SIZES, handle=None, dtype=None):
    """hip_write_edge_file: the device CSR `dM` as an edge-list file -> stats dict.  header: EDGE_HEADER_NONE, _SIZES (the
    line readSNAPFile reads) or _MATRIX_MARKET (banner, one-based lines).  The body is formatted on the device in slabs
    (SPGEMM_EDGE_SLAB bytes of text, read per call) and written while the next slab is formatted."""
    dtype, _, _, fmt, flags = _edge_write_args("write_edge_file", dM, 0, None, fmt, flags, dtype)
    if not isinstance(path, (str, bytes, os.PathLike)):
        raise SpgemmError(f"write_edge_file: path must be a str, bytes or os.PathLike, not {type(path).__name__}")
    header = int(header)
    if header not in (EDGE_HEADER_NONE, EDGE_HEADER_SIZES, EDGE_HEADER_MATRIX_MARKET):
        raise SpgemmError(f"write_edge_file: unknown header {header}")
    st = EdgeWriteStats()
    _call("hip_write_edge_file", dtype, _hp(handle), os.fsencode(path), dM.rows, dM.cols,
          *_ptrs(dM.rowPtr, dM.colInd, dM.values), fmt, flags, header, C.byref(st))
    return st.as_dict()


# ---------------------------------------------------------------------------------------------
# clusters (include/spgemm_hip.h "clusters from a finished R-MCL result"): attractors of the flow matrix, connected
# components, labels -> clusters.  The reference has no counterpart: it stops at Mt.
# ---------------------------------------------------------------------------------------------
CC_MAX_ROUNDS = 64


def rmcl_attractor_lanes(m, nnz):
    """hip_rmcl_attractor_lanes (pure host): the lanes per row (4, 16 or 64) the attractor and hook kernels use"""
    return int(lib().hip_rmcl_attractor_lanes(int(m), int(nnz)))


def rmcl_attractors_raw(handle, m, n, nnz, IA, JA, VA, parent, dtype=np.float32):
    """hip_rmcl_attractors / _f64 on raw device pointers: parent (the caller's int32[m]) = per row the column of the
    largest value, the smallest such column on a tie, the row itself where nothing wins"""
    _call("hip_rmcl_attractors", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA, parent))


def connected_components_raw(handle, m, n, nnz, IA, JA, label):
    """hip_csr_connected_components: label (the caller's int32[m]) = the smallest vertex id of each vertex's weakly
    connected component -> (ncomp, rounds)"""
    ncomp, rounds = C.c_int(0), C.c_int(0)
    _check(lib().hip_csr_connected_components(_hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, label), C.byref(ncomp),
                                              C.byref(rounds)), "hip_csr_connected_components")
    return ncomp.value, rounds.value


def labels_to_clusters_raw(handle, m, label):
    """hip_labels_to_clusters on canonical device labels -> (k, dCluster, dClusterPtr, dMembers) from the library pool"""
    k, out = C.c_int(0), _CsrOut(count=False)
    _check(lib().hip_labels_to_clusters(_hp(handle), int(m), C.c_void_p(label), C.byref(k), *out.refs()),
           "hip_labels_to_clusters")
    return (k.value,) + out.values()


class Clusters:
    """what rmcl_clusters / labels_to_clusters leave on the device: `k` clusters numbered by ascending smallest member;
    cluster (int32[m]: a vertex's cluster), ptr (int32[k + 1]) and members (int32[m]: cluster c's vertices, ascending, are
    members[ptr[c]:ptr[c + 1]]) are device pointers."""

    def __init__(self, m, k, cluster, ptr, members):
        self.m, self.k, self.cluster, self.ptr, self.members = int(m), int(k), cluster, ptr, members

    def to_host(self):
        """-> (cluster, ptr, members) numpy int32 arrays"""
        return (d2h(self.cluster, self.m, np.int32), d2h(self.ptr, self.k + 1, np.int32), d2h(self.members, self.m, np.int32))

    def dispose(self):
        for p in (self.cluster, self.ptr, self.members):
            dev_free(p)
        self.cluster = self.ptr = self.members = None


def _square_device(what, dM):
    if not isinstance(dM, CSR) or not dM.on_device:
        raise SpgemmError(f"{what}: takes a device CSR")
    _need_square(dM, what)
    return _value_dtype(dM.dtype)


def rmcl_attractors(dMt, handle=None):
    """per node the column its largest flow goes to (hip_rmcl_attractors, the matrix's dtype) -> int32 device pointer of
    dMt.rows entries (release with dev_free)"""
    dt = _square_device("rmcl_attractors", dMt)
    parent = dev_alloc(4 * dMt.rows)
    try:
        rmcl_attractors_raw(handle, dMt.rows, dMt.cols, dMt.nnz, dMt.rowPtr, dMt.colInd, dMt.values, parent, dt)
    except SpgemmError:
        dev_free(parent)
        raise
    return parent


def connected_components(dM, handle=None):
    """weakly connected components of the pattern of a square device CSR -> (labels, ncomp, rounds); labels: int32
    device pointer of dM.rows entries, the smallest vertex id of each vertex's component (release with dev_free)"""
    _square_device("connected_components", dM)
    label = dev_alloc(4 * dM.rows)
    try:
        ncomp, rounds = connected_components_raw(handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, label)
    except SpgemmError:
        dev_free(label)
        raise
    return label, ncomp, rounds


def labels_to_clusters(label, m, handle=None):
    """canonical device labels (connected_components) -> Clusters"""
    k, cluster, ptr, members = labels_to_clusters_raw(handle, m, label)
    return Clusters(m, k, cluster, ptr, members)


def rmcl_clusters(dMt, handle=None):
    """hip_rmcl_clusters / _f64: the clusters of a finished R-MCL flow matrix (every node joins the column of its largest
    flow; attractors that point at each other are one cluster) -> Clusters"""
    dt = _square_device("rmcl_clusters", dMt)
    k, out = C.c_int(0), _CsrOut(count=False)
    _call("hip_rmcl_clusters", dt, _hp(handle), dMt.rows, dMt.cols, dMt.nnz, *_ptrs(dMt.rowPtr, dMt.colInd, dMt.values),
          C.byref(k), *out.refs())
    return Clusters(dMt.rows, k.value, *out.values())


# ---------------------------------------------------------------------------------------------
# sparse add and symmetrisation (include/spgemm_hip.h "sparse add and the symmetrisation of a directed graph"); the
# CSR methods add / symmetrize are the object form.  The reference has no counterpart: its loader only transposes.
# ---------------------------------------------------------------------------------------------
def csr_add_raw(handle, m, n, alpha, IA, JA, VA, nnzA, beta, IB, JB, VB, nnzB, dtype=np.float32):
    """hip_csr_add / _f64 on raw device pointers: alpha * A + beta * B -> (dIC, dJC, dC, nnzC) from the library pool"""
    out = _CsrOut()
    _call("hip_csr_add", dtype, _hp(handle), int(m), int(n), float(alpha), *_ptrs(IA, JA, VA), int(nnzA), float(beta),
          *_ptrs(IB, JB, VB), int(nnzB), *out.refs())
    return out.values()


def csr_scale_raw(handle, m, n, nnz, IA, JA, VA, rowScale, colScale, VOut, dtype=np.float32):
    """hip_csr_scale / _f64: VOut[j] = (rowScale[row] * VA[j]) * colScale[JA[j]]; a scale of None is 1; VOut may be VA"""
    _call("hip_csr_scale", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA, rowScale, colScale, VOut))


def csr_col_counts_raw(handle, n, nnz, JA, count, dtype=np.float32):
    """hip_csr_col_counts: count (the caller's device int32[n]) = entries per column.  dtype is accepted like the
    neighbours' and not used: the call reads no value."""
    _value_dtype(dtype)
    _check(lib().hip_csr_col_counts(_hp(handle), int(n), int(nnz), *_ptrs(JA, count)), "hip_csr_col_counts")


def degree_factors_raw(handle, length, count, exponent, out, dtype=np.float32):
    """hip_degree_factors / _f64: out[i] = count[i] ** -exponent in the value type, 0 where the count is 0"""
    _call("hip_degree_factors", dtype, _hp(handle), int(length), C.c_void_p(count), float(exponent), C.c_void_p(out))


def csr_symmetrize_raw(handle, mode, alpha, beta, m, IA, JA, VA, nnz, dtype=np.float32):
    """hip_csr_symmetrize / _f64 on raw device pointers -> (dIS, dJS, dS, nnzS) from the library pool"""
    out = _CsrOut()
    _call("hip_csr_symmetrize", dtype, _hp(handle), int(mode), float(alpha), float(beta), int(m), *_ptrs(IA, JA, VA),
          int(nnz), *out.refs())
    return out.values()


# ---------------------------------------------------------------------------------------------
# selection (include/spgemm_hip.h "selection: the k largest entries of every row"); CSR.row_topk is the object form and
# gpuRmclIterTopK_device the loop with the row cap.  The reference has no counterpart: its row rule only thresholds.
# ---------------------------------------------------------------------------------------------
def csr_row_topk_raw(handle, m, n, nnz, IA, JA, VA, k, flags=0, dtype=np.float32):
    """hip_csr_row_topk / _f64 on raw device pointers -> (dIN, dJN, dAN, nnzN, rowsCut); the arrays are the library pool's"""
    out, cut = _CsrOut(), C.c_int(0)
    _call("hip_csr_row_topk", dtype, _hp(handle), int(m), int(n), int(nnz), *_ptrs(IA, JA, VA), int(k), int(flags),
          *out.refs(), C.byref(cut))
    return out.values() + (cut.value,)


def row_topk_limits(dtype=np.float32):
    """hip_csr_row_topk_limits (pure host) -> (waveCap, blockCap): the longest row the wave path / the block path cuts"""
    w, b = C.c_int(0), C.c_int(0)
    _check(lib().hip_csr_row_topk_limits(int(_value_dtype(dtype) == np.float64), C.byref(w), C.byref(b)),
           "hip_csr_row_topk_limits")
    return w.value, b.value


def topk_paths(handle=None):
    """spgemm_hip_debug_topk_paths of a Handle (None: the default handle) -> {"copied", "wave", "block", "stream"}"""
    v = [C.c_longlong(0) for _ in range(4)]
    _check(lib().spgemm_hip_debug_topk_paths(_hp(handle), *[C.byref(x) for x in v]), "spgemm_hip_debug_topk_paths")
    return dict(zip(("copied", "wave", "block", "stream"), (x.value for x in v)))
