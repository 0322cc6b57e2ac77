# Host-only sanitizer build of the workspace layout check (tests/test_stage_layout.py):
# make -f stage_layout.mk -C tests/native OUT=<dir>.  csrc/stage_layout.hpp includes no HIP, so the stand-alone
# check links without it; same sanitizer flags as ms_shape.mk beside it.
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/stage_layout_check
$(OUT)/stage_layout_check: stage_layout_check.cpp $(CSRC)/stage_layout.hpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all stage_layout_check.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
