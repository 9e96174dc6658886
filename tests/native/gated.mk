# TEST-ONLY: host build of the verdict fold (authorino_amd/csrc/ajx_verdict.h) and of the gated
# render body (render_request_gated of ajx_render_gated.h) for tests/test_gated_host.py, and
# the same code with its own main under ASan + UBSan. Run as `make -C tests/native -f gated.mk`.
CXX ?= g++
CSRC = ../../authorino_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
HDRS = $(CSRC)/ajx_render.h $(CSRC)/ajx_render_gated.h $(CSRC)/ajx_verdict.h $(CSRC)/ajx_render_prog.h $(CSRC)/ajx_device.h $(CSRC)/ajx_float.h $(CSRC)/ajx_blob.h ../../include/authjx.h
SRCS = gated_host.cpp render_multi_host.cpp render_host.cpp
all: libajx_gatedtest.so san_gated
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one loads or runs it)
libajx_gatedtest.so: $(SRCS) $(HDRS)
	$(CXX) $(CXXFLAGS) -std=c++17 -shared -o $@.tmp$$$$ gated_host.cpp && mv -f $@.tmp$$$$ $@
SANFLAGS = -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
san_gated: san_gated.cpp $(SRCS) $(HDRS)
	$(CXX) $(SANFLAGS) -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -o $@.tmp$$$$ san_gated.cpp gated_host.cpp && mv -f $@.tmp$$$$ $@
clean:
	rm -f libajx_gatedtest.so san_gated
