# the symmetrisation's C++ check (make -f symmetrize.mk); tests/cpp/Makefile builds the older drivers
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
NL   := $(ROOT)/sparse_matrix_with_flops_amd/csrc/nlibs
LINK_HIP := -L$(ROOT)/sparse_matrix_with_flops_amd -lspgemm_hip -Wl,-rpath,$(ROOT)/sparse_matrix_with_flops_amd \
	    -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -fopenmp
all: symmetrize_check.x
# own_graph.snap made undirected on the device against a host A + A^T, then R-MCL and clusters (tests/test_gpu_symmetrize.py)
symmetrize_check.x: symmetrize_check.cc $(NL)/CSR.cc $(NL)/CSR.h $(NL)/COO.cc $(NL)/COO.h $(NL)/qrmcl.cc $(NL)/qrmcl.h \
		    $(NL)/process_args.cc $(NL)/gpus/gpu_csr_kernel.h
	g++ -std=c++17 -O2 -ffp-contract=off -I$(NL) -o $@ $(filter %.cc,$^) $(LINK_HIP)
.PHONY: all
