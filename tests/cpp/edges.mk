# the device text parser's C++ checks (make -f edges.mk <target>); tests/cpp/Makefile builds the older drivers
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/sparse_matrix_with_flops_amd/csrc
NL   := $(CSRC)/nlibs
LINK_HIP := -L$(ROOT)/sparse_matrix_with_flops_amd -lspgemm_hip -Wl,-rpath,$(ROOT)/sparse_matrix_with_flops_amd \
	    -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -fopenmp
all: edge_scan_check.x edge_scan_check_san.x edges_check.x
# the shared scanner against strtol / strtof: plain g++, no device, no library
edge_scan_check.x: edge_scan_check.cc $(CSRC)/edge_scan.hpp
	g++ -std=c++17 -O2 -Wall -o $@ $<
# the same program under the address and undefined-behaviour sanitizers (stand-alone: its own main, run outside Python)
edge_scan_check_san.x: edge_scan_check.cc $(CSRC)/edge_scan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<
# what COO::readSNAPFileToGpuCSR loads (tests/test_gpu_edges_parse.py), and the host loader arm of tools/edges_bench.py
edges_check.x: edges_check.cc $(NL)/COO.cc $(NL)/COO.h $(NL)/CSR.cc $(NL)/CSR.h
	g++ -std=c++17 -O2 -I$(NL) -o $@ $(filter %.cc,$^) $(LINK_HIP)
.PHONY: all
