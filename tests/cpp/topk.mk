# the selection's C++ check (make -f topk.mk); tests/cpp/Makefile builds the older drivers
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
NL   := $(ROOT)/sparse_matrix_with_flops_amd/csrc/nlibs
LINK_HIP := -L$(ROOT)/sparse_matrix_with_flops_amd -lspgemm_hip -Wl,-rpath,$(ROOT)/sparse_matrix_with_flops_amd \
	    -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -fopenmp
all: topk_check.x
# one product of own_graph.snap's start matrix, CSR::gpuRowTopK against a host std::stable_sort (tests/test_gpu_rmcl_topk.py)
topk_check.x: topk_check.cc $(NL)/CSR.cc $(NL)/CSR.h $(NL)/COO.cc $(NL)/COO.h $(NL)/qrmcl.cc $(NL)/qrmcl.h \
	      $(NL)/process_args.cc $(NL)/gpus/gpu_csr_kernel.h
	g++ -std=c++17 -O2 -ffp-contract=off -I$(NL) -o $@ $(filter %.cc,$^) $(LINK_HIP)
.PHONY: all
