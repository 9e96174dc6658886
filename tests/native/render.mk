# TEST-ONLY: host builds of the render logic (authorino_amd/csrc/ajx_render.h) for the CPU
# suite (tests/test_render_host.py). Run as `make -C tests/native -f render.mk`.
CXX ?= g++
CSRC = ../../authorino_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
HDRS = $(CSRC)/ajx_render.h $(CSRC)/ajx_render_prog.h $(CSRC)/ajx_device.h $(CSRC)/ajx_float.h $(CSRC)/ajx_blob.h ../../include/authjx.h
all: libajx_rendertest.so san_render
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one loads or runs it)
libajx_rendertest.so: render_host.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -std=c++17 -shared -o $@.tmp$$$$ render_host.cpp && mv -f $@.tmp$$$$ $@
# the same code with its own main under ASan + UBSan
SANFLAGS = -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
san_render: san_render.cpp render_host.cpp $(HDRS)
	$(CXX) $(SANFLAGS) -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -o $@.tmp$$$$ san_render.cpp render_host.cpp && mv -f $@.tmp$$$$ $@
clean:
	rm -f libajx_rendertest.so san_render
