# Host-only sanitizer build of the witness-update plan check (tests/test_ms_update_plan.py):
# make -f ms_update_plan.mk -C tests/native OUT=<dir>.  csrc/ms_update_plan.cpp and csrc/ms_shape.cpp include no
# HIP, so the stand-alone check links without it; same sanitizer flags as ms_unpack_plan.mk beside it.
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/ms_update_plan_check
$(OUT)/ms_update_plan_check: ms_update_plan_check.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_update_plan.hpp $(CSRC)/ms_shape.cpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -pthread ms_update_plan_check.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_shape.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
