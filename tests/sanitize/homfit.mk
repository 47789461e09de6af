# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the host side of the homography refit
# (homfit_harness.cpp: csrc/rsac_host.hip's hom_refine and the rsac_math.h pieces it shares with
# k_hom_fit under AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU, run by hand:
#     make -C tests/sanitize -f homfit.mk run
# The host code is compiled as plain C++ (clang, HIP headers for the host only); -Xarch_host pins
# the sanitizers to the host compilation, so no device code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/homfit_asan

$(OUT)/homfit_asan: homfit_harness.cpp $(SRC)/rsac_host.hip $(SRC)/rsac_host.h $(SRC)/rsac_math.h $(SRC)/rsac_cvepnp.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined homfit_harness.cpp $(SRC)/rsac_host.hip -o $@ -pthread

run: $(OUT)/homfit_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/homfit_asan

clean:
	rm -rf $(OUT)
