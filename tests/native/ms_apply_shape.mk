# Host-only sanitizer build of nhip_ms_apply_batch's shape validator and staged order (tests/test_ms_apply_ref.py):
# make -f ms_apply_shape.mk -C tests/native OUT=<dir>.  csrc/ms_shape.cpp is a host-only translation unit, so
# the stand-alone check links without HIP; same sanitizer flags as ms_shape.mk beside it.
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/ms_apply_shape_check
$(OUT)/ms_apply_shape_check: ms_apply_shape_check.cpp $(CSRC)/ms_shape.cpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all ms_apply_shape_check.cpp $(CSRC)/ms_shape.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
