# Host-only builds of the revert plan's check (tests/test_ms_revert_plan.py):
# make -f ms_revert.mk -C tests/native OUT=<dir>.  csrc/ms_revert_plan.cpp, csrc/ms_store.cpp, csrc/ms_update_plan.cpp
# and csrc/ms_shape.cpp include no HIP, so the stand-alone check links without it: once plainly, once under
# ASan + UBSan (the flags of ms_store.mk beside it).
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
SRCS := ms_revert_check.cpp $(CSRC)/ms_revert_plan.cpp $(CSRC)/ms_store.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_shape.cpp
DEPS := $(SRCS) $(CSRC)/ms_revert_plan.hpp $(CSRC)/ms_store.hpp $(CSRC)/ms_update_plan.hpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
all: $(OUT)/ms_revert_check $(OUT)/ms_revert_check_san
$(OUT)/ms_revert_check: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O2 -Wall -Wextra -Werror -pthread $(SRCS) -o $@
$(OUT)/ms_revert_check_san: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -pthread $(SRCS) -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
