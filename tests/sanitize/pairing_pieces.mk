# AddressSanitizer + UndefinedBehaviorSanitizer build of the pieces of csrc/pairing.hpp on the host (tests/test_pairing_pieces_host.py): the device
# header compiled as plain C++ (hip_host_prelude.hpp) into a stand-alone program, nothing else linked.  One translation unit per curve
# (PIECES_CURVE in pairing_pieces_main.cpp), so that `make -j2` builds them side by side.
#   make -j2 -f pairing_pieces.mk && _build/pairing_pieces_main <case file> <result file>
CXX ?= g++
ROOT := ../..
PKG := $(ROOT)/collaborative-circom_amd
ROCM_PATH ?= $(shell hipconfig --rocmpath 2>/dev/null || echo /opt/rocm)
OUT := _build/pairing_pieces_main
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g
HOSTFLAGS := -O1 -std=c++17 $(SAN) -x c++ -D__HIP_PLATFORM_AMD__ -include hip_host_prelude.hpp -I$(ROCM_PATH)/include -I$(ROOT)/include -I$(PKG)/csrc
HOSTDEPS := pairing_pieces_main.cpp hip_host_prelude.hpp $(wildcard $(PKG)/csrc/*.hpp)
$(OUT): _build/pairing_pieces_bn254.o _build/pairing_pieces_bls381.o
	$(CXX) $(SAN) $^ -o $@
_build/pairing_pieces_bn254.o: $(HOSTDEPS)
	@mkdir -p _build
	$(CXX) $(HOSTFLAGS) -DPIECES_CURVE=0 -c pairing_pieces_main.cpp -o $@
_build/pairing_pieces_bls381.o: $(HOSTDEPS)
	@mkdir -p _build
	$(CXX) $(HOSTFLAGS) -DPIECES_CURVE=1 -c pairing_pieces_main.cpp -o $@
