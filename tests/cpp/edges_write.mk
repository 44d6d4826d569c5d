# the device text writer's C++ checks (make -f edges_write.mk <target>); edges.mk / edges_f64.mk build the parser's
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/sparse_matrix_with_flops_amd/csrc
NL   := $(CSRC)/nlibs
LINK_HIP := -L$(ROOT)/sparse_matrix_with_flops_amd -lspgemm_hip -Wl,-rpath,$(ROOT)/sparse_matrix_with_flops_amd \
	    -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -fopenmp
all: edge_print_check.x edge_print_check_san.x edges_write_check.x
# the shared formatter against snprintf: plain g++, no device, no library
edge_print_check.x: edge_print_check.cc $(CSRC)/edge_print.hpp
	g++ -std=c++17 -O2 -Wall -o $@ $<
# the same program under the address and undefined-behaviour sanitizers (stand-alone: its own main, run outside Python)
edge_print_check_san.x: edge_print_check.cc $(CSRC)/edge_print.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<
# gpuWriteCSRWrapper against the host loader (tests/test_gpu_edges_write.py), and the host fprintf arm of
# tools/edges_write_bench.py
edges_write_check.x: edges_write_check.cc $(NL)/COO.cc $(NL)/COO.h $(NL)/CSR.cc $(NL)/CSR.h $(NL)/qrmcl.cc $(NL)/process_args.cc
	g++ -std=c++17 -O2 -I$(NL) -o $@ $(filter %.cc,$^) $(LINK_HIP)
.PHONY: all
