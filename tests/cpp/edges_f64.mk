# the double scanner's C++ checks (make -f edges_f64.mk <target>); edges.mk builds the float ones
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/sparse_matrix_with_flops_amd/csrc
all: edge_scan_f64_check.x edge_scan_f64_check_san.x
# scan_double / edge_scan_line_f64 against strtol / strtod: plain g++, no device, no library
edge_scan_f64_check.x: edge_scan_f64_check.cc $(CSRC)/edge_scan.hpp
	g++ -std=c++17 -O2 -Wall -o $@ $<
# the same program under the address and undefined-behaviour sanitizers (stand-alone: its own main, run outside Python)
edge_scan_f64_check_san.x: edge_scan_f64_check.cc $(CSRC)/edge_scan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<
.PHONY: all
