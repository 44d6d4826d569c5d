# the dense matrix's C++ check (make -f dense.mk); tests/cpp/Makefile builds the older drivers
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
NL   := $(ROOT)/sparse_matrix_with_flops_amd/csrc/nlibs
LINK_HIP := -L$(ROOT)/sparse_matrix_with_flops_amd -lspgemm_hip -Wl,-rpath,$(ROOT)/sparse_matrix_with_flops_amd \
	    -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -fopenmp
all: dense_check.x
# the 5 x 6 known answer, the dense-somp scenario and the fmaf chain (tests/test_gpu_dense.py)
dense_check.x: dense_check.cc $(NL)/DenseMatrix.h $(NL)/CSR.cc $(NL)/CSR.h $(NL)/COO.cc $(NL)/COO.h $(NL)/qrmcl.cc $(NL)/qrmcl.h \
	       $(NL)/process_args.cc
	g++ -std=c++17 -O2 -ffp-contract=off -I$(NL) -o $@ $(filter %.cc,$^) $(LINK_HIP)
.PHONY: all
