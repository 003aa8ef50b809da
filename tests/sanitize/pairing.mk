# AddressSanitizer + UndefinedBehaviorSanitizer build of the host pairing (the host side of csrc/capi_pairing.hip) and the host verifier
# (host/capi_verify.cpp, host/capi_tools.cpp for the codecs) in one stand-alone program; everything else comes from the release library.
#   make -f pairing.mk && _build/pairing_main ../golden
HIPCC ?= hipcc
ROOT := ../..
PKG := $(ROOT)/collaborative-circom_amd
OUT := _build/pairing_main
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g
$(OUT): pairing_main.cpp $(wildcard $(PKG)/csrc/*.hpp) $(PKG)/csrc/capi_pairing.hip $(wildcard $(PKG)/host/*.hpp) $(PKG)/host/capi_verify.cpp $(PKG)/host/capi_tools.cpp $(ROOT)/include/cogroth16_host.h $(ROOT)/include/cogroth16_hip.h
	@mkdir -p _build
	$(HIPCC) -O1 -std=c++17 --offload-host-only -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -DCG_WITH_BLS=1 -I$(ROOT)/include -Wno-unused-result -Wno-unused-value -c $(PKG)/csrc/capi_pairing.hip -o _build/pairing_host.o
	for t in verify tools; do $(HIPCC) -x c++ -O1 -std=c++17 -pthread $(SAN) -Wno-unused-function -I$(ROOT)/include -c $(PKG)/host/capi_$$t.cpp -o _build/pairing_host_$$t.o || exit 1; done
	$(HIPCC) -O1 -std=c++17 -pthread $(SAN) -I$(ROOT)/include -x c++ pairing_main.cpp -x none _build/pairing_host.o _build/pairing_host_verify.o _build/pairing_host_tools.o -o $@ \
	    -L$(PKG) -lcogroth16_hip -Wl,-rpath,$(abspath $(PKG))
