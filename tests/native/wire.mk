# Host-only sanitizer build of the in-place scanners' harness (tests/test_wire_sanitizers.py):
# make -f wire.mk -C tests/native OUT=<dir>.  Same flags as the Makefile beside it: compiled as HIP host
# code by hipcc, the sanitizers apply to the host side only (-Xarch_host), nothing runs on a GPU.
HIPCC ?= /opt/rocm/bin/hipcc
SAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=all
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/wire_scan_check
$(OUT)/wire_scan_check: wire_scan_check.cpp $(CSRC)/bincode.cpp $(CSRC)/wire.hpp $(CSRC)/kernels.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	$(HIPCC) -std=c++17 -O1 -g -fno-omit-frame-pointer --offload-arch=gfx950 $(SAN) wire_scan_check.cpp $(CSRC)/bincode.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
