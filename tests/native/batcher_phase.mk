# TEST-ONLY: the micro-batcher's queue with phase requests and the phase plan of
# authorino_amd/csrc/ajx_phase.h on a stand-in evaluator (batcher_phase_host.cpp) for
# tests/test_batcher_phase_host.py, and the same code with its own main under
# ThreadSanitizer. Run as `make -C tests/native -f batcher_phase.mk`.
CXX ?= g++
CSRC = ../../authorino_amd/csrc
CXXFLAGS ?= -O1 -g -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
HDRS = $(CSRC)/ajx_batcher.h $(CSRC)/ajx_phase.h
all: libajx_batchphase.so tsan_phase
# (linked to a temporary name and renamed into place: parallel test workers may rebuild a
# stale target while another one loads or runs it)
libajx_batchphase.so: batcher_phase_host.cpp $(HDRS)
	$(CXX) $(CXXFLAGS) -std=c++17 -shared -o $@.tmp$$$$ batcher_phase_host.cpp -lpthread && mv -f $@.tmp$$$$ $@
# (tsan_prelude.h: gcc 11's TSan does not intercept the clock wait of condition_variable::wait_for)
tsan_phase: tsan_phase.cpp batcher_phase_host.cpp tsan_prelude.h $(HDRS)
	$(CXX) -O1 -g -fsanitize=thread -std=c++17 -include tsan_prelude.h -Wall -Wno-unknown-pragmas -o $@.tmp$$$$ tsan_phase.cpp batcher_phase_host.cpp -lpthread && mv -f $@.tmp$$$$ $@
clean:
	rm -f libajx_batchphase.so tsan_phase
