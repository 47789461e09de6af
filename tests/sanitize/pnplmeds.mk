# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the host-only LMedS PnP code
# (pnplmeds_harness.cpp: csrc/rsac_host.hip's pnp_median_host / scan_step_lmeds / lmeds_num_iters and
# rsac_math.h's pnp_err and lmeds_* under AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU,
# run by hand:
#     make -C tests/sanitize -f pnplmeds.mk run
# The host code is compiled as plain C++ (clang, HIP headers for the host only); -Xarch_host pins
# the sanitizers to the host compilation, so no device code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/pnplmeds_asan

$(OUT)/pnplmeds_asan: pnplmeds_harness.cpp $(SRC)/rsac_host.hip $(SRC)/rsac_host.h $(SRC)/rsac_math.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined pnplmeds_harness.cpp $(SRC)/rsac_host.hip -o $@ -pthread

run: $(OUT)/pnplmeds_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/pnplmeds_asan

clean:
	rm -rf $(OUT)
