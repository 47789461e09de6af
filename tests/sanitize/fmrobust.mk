# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the host-only code of MSAC and LMedS for
# the fundamental matrix (fmrobust_harness.cpp: csrc/rsac_host.hip's fm_err_host / fm_cost_host /
# fm_median_host / scan_step_msac / scan_step_lmeds and rsac_math.h's fm_err / fm_msac_term under
# AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU, run by hand:
#     make -C tests/sanitize -f fmrobust.mk run
# The host code is compiled as plain C++ (clang, HIP headers for the host only); -Xarch_host pins
# the sanitizers to the host compilation, so no device code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/fmrobust_asan

$(OUT)/fmrobust_asan: fmrobust_harness.cpp $(SRC)/rsac_host.hip $(SRC)/rsac_host.h $(SRC)/rsac_math.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=undefined,float-cast-overflow fmrobust_harness.cpp $(SRC)/rsac_host.hip -o $@ -pthread

run: $(OUT)/fmrobust_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/fmrobust_asan

clean:
	rm -rf $(OUT)
