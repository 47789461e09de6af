# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the host side of the least-squares
# fundamental matrix (fmfit_harness.cpp: rsac_math.h's fm_fit_host and the pieces it is made of under
# AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU, run by hand:
#     make -C tests/sanitize -f fmfit.mk run
# The host code is compiled as plain C++ (clang, HIP headers for the host only); -Xarch_host pins
# the sanitizers to the host compilation, so no device code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/fmfit_asan

$(OUT)/fmfit_asan: fmfit_harness.cpp $(SRC)/rsac_math.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=undefined,float-cast-overflow fmfit_harness.cpp -o $@ -pthread

run: $(OUT)/fmfit_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/fmfit_asan

clean:
	rm -rf $(OUT)
