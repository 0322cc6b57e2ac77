# Host-only sanitizer build of the transaction-rule and host-walk check (tests/test_tx_rules.py):
# make -f tx_rules.mk -C tests/native OUT=<dir>.  csrc/tx_rules.hpp, csrc/bincode.cpp and csrc/blk_ms_parts.cpp include
# no HIP, so the stand-alone check links without it; same sanitizer flags as chain_rules.mk beside it.
CSRC := ../../neptune-core_amd/csrc
OUT ?= build
all: $(OUT)/tx_rules_check
$(OUT)/tx_rules_check: tx_rules_check.cpp $(CSRC)/bincode.cpp $(CSRC)/blk_ms_parts.cpp $(CSRC)/blk_ms_parts.hpp $(CSRC)/tx_rules.hpp $(CSRC)/chain_rules.hpp ../../include/neptune_hip.h
	@mkdir -p $(OUT)
	g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all tx_rules_check.cpp $(CSRC)/bincode.cpp $(CSRC)/blk_ms_parts.cpp -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
