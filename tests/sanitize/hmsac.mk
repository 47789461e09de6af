# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the host-only code of MSAC scoring for
# homographies (hmsac_harness.cpp: csrc/rsac_host.hip's hom_cost_host / scan_step_msac and
# rsac_math.h's msac_* under AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU, run by hand:
#     make -C tests/sanitize -f hmsac.mk run
# The host code is compiled as plain C++ (clang, HIP headers for the host only); -Xarch_host pins
# the sanitizers to the host compilation, so no device code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/hmsac_asan

$(OUT)/hmsac_asan: hmsac_harness.cpp $(SRC)/rsac_host.hip $(SRC)/rsac_host.h $(SRC)/rsac_math.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=undefined,float-cast-overflow hmsac_harness.cpp $(SRC)/rsac_host.hip -o $@ -pthread

run: $(OUT)/hmsac_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/hmsac_asan

clean:
	rm -rf $(OUT)
