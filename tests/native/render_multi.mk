# TEST-ONLY: host build of the multi-program render body (render_request_multi of
# authorino_amd/csrc/ajx_render.h) for tests/test_render_multi_host.py, and the same code
# with its own main under ASan + UBSan. Run as `make -C tests/native -f render_multi.mk`.
CXX ?= g++
CSRC = ../../authorino_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
HDRS = $(CSRC)/ajx_render.h $(CSRC)/ajx_render_prog.h $(CSRC)/ajx_device.h $(CSRC)/ajx_float.h $(CSRC)/ajx_blob.h ../../include/authjx.h
all: libajx_rendermulti.so san_render_multi
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one loads or runs it)
libajx_rendermulti.so: render_multi_host.cpp render_host.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -std=c++17 -shared -o $@.tmp$$$$ render_multi_host.cpp && mv -f $@.tmp$$$$ $@
SANFLAGS = -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
san_render_multi: san_render_multi.cpp render_multi_host.cpp render_host.cpp $(HDRS)
	$(CXX) $(SANFLAGS) -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -o $@.tmp$$$$ san_render_multi.cpp render_multi_host.cpp && mv -f $@.tmp$$$$ $@
clean:
	rm -f libajx_rendermulti.so san_render_multi
