# TEST INFRASTRUCTURE: the stand-alone sanitizer program of the pixel -> ground path's host+device
# pieces (geo_harness.cpp: rsac_geo.h's stride_closed_form, dem_interp, utm_inverse_fast, dem_march
# under AddressSanitizer + UndefinedBehaviorSanitizer), on the CPU, run by hand:
#     make -C tests/sanitize -f geo.mk run
# or by tests/test_dem_edges.py::test_geo_harness.  The header is compiled as plain C++ (clang, HIP
# headers for the host only); -Xarch_host pins the sanitizers to the host compilation, so no device
# code object is ever instrumented.
CXX = /opt/rocm/lib/llvm/bin/clang++
SRC = ../../code-reproduction-ransac_amd/csrc
COMMON = -O1 -g -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(SRC) -ffp-contract=off -fno-omit-frame-pointer
OUT ?= build

all: $(OUT)/geo_asan

$(OUT)/geo_asan: geo_harness.cpp $(SRC)/rsac_geo.h $(SRC)/rsac_math.h
	@mkdir -p $(OUT)
	$(CXX) $(COMMON) -Xarch_host -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=undefined,float-cast-overflow geo_harness.cpp -o $@ -pthread

run: $(OUT)/geo_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 $(OUT)/geo_asan

clean:
	rm -rf $(OUT)
