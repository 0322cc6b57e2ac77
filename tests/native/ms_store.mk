# Host-only builds of the witness store's mirror check (tests/test_ms_store_host.py):
# make -f ms_store.mk -C tests/native OUT=<dir>.  csrc/ms_store.cpp, csrc/ms_update_plan.cpp and csrc/ms_shape.cpp
# include no HIP, so the stand-alone check links without it: once plainly, once under ASan + UBSan (the flags of
# ms_update_plan.mk beside it).
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
SRCS := ms_store_check.cpp $(CSRC)/ms_store.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_shape.cpp
DEPS := $(SRCS) $(CSRC)/ms_store.hpp $(CSRC)/ms_update_plan.hpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
all: $(OUT)/ms_store_check $(OUT)/ms_store_check_san
$(OUT)/ms_store_check: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O2 -Wall -Wextra -Werror -pthread $(SRCS) -o $@
$(OUT)/ms_store_check_san: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -pthread $(SRCS) -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
