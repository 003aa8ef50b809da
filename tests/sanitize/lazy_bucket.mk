# AddressSanitizer + UndefinedBehaviorSanitizer build of the host model of the MSM's lazy limb arithmetic (tests/test_lazy_bucket_host.py): the device
# headers csrc/lazy29.hpp and csrc/msm_kernels.hpp compiled as plain C++ (hip_host_prelude.hpp), linked with the CPU oracle and nothing else.
# -fno-sanitize-recover stays: UBSan's signed-overflow check is what detects an overflowing int64 column sum or int32 limb sum.
# The program is compiled -O0 (the column-engine templates take five times as long at -O1; the run is seconds either way) and in two halves
# (LAZY_PART in lazy_bucket_main.cpp), so that `make -j3` builds them and the oracle side by side.
#   make -j3 -f lazy_bucket.mk && _build/lazy_bucket_main [edge point file]
CXX ?= g++
ROOT := ../..
PKG := $(ROOT)/collaborative-circom_amd
ROCM_PATH ?= $(shell hipconfig --rocmpath 2>/dev/null || echo /opt/rocm)
OUT := _build/lazy_bucket_main
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g
HOSTFLAGS := -O0 -std=c++17 $(SAN) -x c++ -D__HIP_PLATFORM_AMD__ -include hip_host_prelude.hpp -I$(ROCM_PATH)/include -I$(ROOT)/include -I$(PKG)/csrc
HOSTDEPS := lazy_bucket_main.cpp hip_host_prelude.hpp $(wildcard $(PKG)/csrc/*.hpp) $(ROOT)/include/cogroth16_hip.h
$(OUT): _build/lazy_bucket_products.o _build/lazy_bucket_rest.o _build/lazy_oracle_capi.o
	$(CXX) -pthread $(SAN) $^ -o $@
_build/lazy_oracle_capi.o: $(ROOT)/oracle/oracle_capi.cpp $(wildcard $(ROOT)/oracle/*.hpp)
	@mkdir -p _build
	$(CXX) -O1 -std=c++17 -mbmi2 -madx -pthread $(SAN) -I$(ROOT)/include -c $(ROOT)/oracle/oracle_capi.cpp -o $@
_build/lazy_bucket_products.o: $(HOSTDEPS)
	@mkdir -p _build
	$(CXX) $(HOSTFLAGS) -DLAZY_PART=1 -c lazy_bucket_main.cpp -o $@
_build/lazy_bucket_rest.o: $(HOSTDEPS)
	@mkdir -p _build
	$(CXX) $(HOSTFLAGS) -DLAZY_PART=2 -c lazy_bucket_main.cpp -o $@
