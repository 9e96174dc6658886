# TEST-ONLY: the host harness with the lean walk's spare-budget setters
# (lean_borrow_host.cpp) for tests/test_lean_borrow.py, and the same code with its own main
# under ASan + UBSan. Run as `make -C tests/native -f lean_borrow.mk`.
# libajx_leanborrow_all.so: every walk() call has an unlimited spare budget by default (the
# existing lean suites run on it with AJX_HOSTTEST_LIB).
CXX ?= g++
CSRC = ../../authorino_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
HDRS = $(CSRC)/ajx_device.h $(CSRC)/ajx_float.h $(CSRC)/ajx_modifiers.h $(CSRC)/ajx_unicode.h $(CSRC)/ajx_fast.h $(CSRC)/ajx_stageb.h $(CSRC)/ajx_lean.h $(CSRC)/ajx_lean_cls.h $(CSRC)/ajx_blob.h $(CSRC)/ajx_compiler.h $(CSRC)/ajx_regex.h $(CSRC)/ajx_stream.h $(CSRC)/ajx_wave.h $(CSRC)/ajx_plan.h $(CSRC)/ajx_request.h $(CSRC)/ajx_stream_body.h
SRCS = lean_borrow_host.cpp $(CSRC)/ajx_compiler.cpp $(CSRC)/ajx_regex.cpp
all: libajx_leanborrow.so
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one loads or runs it)
libajx_leanborrow.so: $(SRCS) host_eval.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -std=c++17 -shared -o $@.tmp$$$$ $(SRCS) && mv -f $@.tmp$$$$ $@
libajx_leanborrow_all.so: $(SRCS) host_eval.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -DAJX_LEAN_SPARE_DEFAULT=2 -std=c++17 -shared -o $@.tmp$$$$ $(SRCS) && mv -f $@.tmp$$$$ $@
SANFLAGS = -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
san_borrow: san_borrow.cpp $(SRCS) host_eval.cpp $(HDRS)
	$(CXX) $(SANFLAGS) -std=c++17 -Wall -Wno-unused-function -Wno-unknown-pragmas -o $@.tmp$$$$ san_borrow.cpp $(SRCS) && mv -f $@.tmp$$$$ $@
clean:
	rm -f libajx_leanborrow.so libajx_leanborrow_all.so san_borrow
