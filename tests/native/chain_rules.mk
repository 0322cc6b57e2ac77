# Host-only sanitizer build of the chain-rule check (tests/test_chain_rules.py):
# make -f chain_rules.mk -C tests/native OUT=<dir>.  csrc/chain_rules.hpp and csrc/chain_shape.cpp include no HIP, so
# the stand-alone check links without it; same sanitizer flags as stage_layout.mk beside it.
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/chain_rules_check
$(OUT)/chain_rules_check: chain_rules_check.cpp $(CSRC)/chain_shape.cpp $(CSRC)/chain_shape.hpp $(CSRC)/chain_rules.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all chain_rules_check.cpp $(CSRC)/chain_shape.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
