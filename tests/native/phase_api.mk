# TEST-ONLY: the phase object and the batcher's phase staging (ajx_phase_api.cpp,
# ajx_batcher_api.cpp, ajx_render_api.cpp over ajx_api.cpp) sequentially and from threads
# under ASan + UBSan, on the host stand-in of the HIP runtime (hipstub/, hip_stub.cpp), as a
# stand-alone program. Run as `make -C tests/native -f phase_api.mk`.
CXX ?= g++
CSRC = ../../authorino_amd/csrc
SRC = $(CSRC)/ajx_api.cpp $(CSRC)/ajx_batcher_api.cpp $(CSRC)/ajx_phase_api.cpp $(CSRC)/ajx_render_api.cpp $(CSRC)/ajx_compiler.cpp $(CSRC)/ajx_regex.cpp $(CSRC)/ajx_index.cpp
HDRS = $(wildcard $(CSRC)/*.h) ../../include/authjx.h hipstub/hip/hip_runtime.h
SANFLAGS = -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
all: phase_api_host
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one runs it)
phase_api_host: phase_api_host.cpp hip_stub.cpp $(SRC) $(HDRS)
	$(CXX) $(SANFLAGS) -std=c++17 -Ihipstub -Wall -Wno-unknown-pragmas -Wno-unused-function -o $@.tmp$$$$ phase_api_host.cpp hip_stub.cpp $(SRC) -lpthread && mv -f $@.tmp$$$$ $@
clean:
	rm -f phase_api_host
