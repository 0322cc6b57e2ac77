# Host-only builds of the hand-over's host check (tests/test_ms_restore_store_host.py):
# make -f ms_restore.mk -C tests/native OUT=<dir>.  csrc/ms_restore_shape.hpp compiles for the host, and
# csrc/ms_archive.cpp, csrc/ms_store.cpp, csrc/ms_update_plan.cpp and csrc/ms_shape.cpp include no HIP, so the
# stand-alone check links without it: once plainly, once under ASan + UBSan (the flags of ms_store.mk beside it).
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
SRCS := ms_restore_check.cpp $(CSRC)/ms_archive.cpp $(CSRC)/ms_store.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_shape.cpp
DEPS := $(SRCS) $(CSRC)/ms_restore_shape.hpp $(CSRC)/ms_archive.hpp $(CSRC)/ms_store.hpp $(CSRC)/ms_update_plan.hpp \
        $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
all: $(OUT)/ms_restore_check $(OUT)/ms_restore_check_san
$(OUT)/ms_restore_check: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O2 -Wall -Wextra -Werror -pthread $(SRCS) -o $@
$(OUT)/ms_restore_check_san: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -pthread $(SRCS) -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
