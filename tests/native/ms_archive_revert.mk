# Host-only builds of the archival mutator set's revert-plan check (tests/test_ms_archive_revert_host.py):
# make -f ms_archive_revert.mk -C tests/native OUT=<dir>.  csrc/ms_archive.cpp, csrc/ms_update_plan.cpp and
# csrc/ms_shape.cpp include no HIP, so the stand-alone check links without it: once plainly, once under ASan + UBSan
# (the flags of ms_archive.mk beside it).
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
SRCS := ms_archive_revert_check.cpp $(CSRC)/ms_archive.cpp $(CSRC)/ms_update_plan.cpp $(CSRC)/ms_shape.cpp
DEPS := $(SRCS) $(CSRC)/ms_archive.hpp $(CSRC)/ms_update_plan.hpp $(CSRC)/ms_shape.hpp ../../include/neptune_hip.h
all: $(OUT)/ms_archive_revert_check $(OUT)/ms_archive_revert_check_san
$(OUT)/ms_archive_revert_check: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O2 -Wall -Wextra -Werror -pthread $(SRCS) -o $@
$(OUT)/ms_archive_revert_check_san: $(DEPS)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -pthread $(SRCS) -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
