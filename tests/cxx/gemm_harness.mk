# test-only GPU library: csrc/kernels_gemm.hip behind one launcher per contraction kernel (gemm_harness.hip) and csrc/kernels_stream.hip
# behind launchers of its two plane sums (gemm_harness_stream.hip), for tests/test_gpu_gemm_fold.py and tests/test_gpu_gemm_kernels.py.
# Each translation unit takes the product's compile line for the file it includes (csrc/Makefile: the SLP vectoriser stays on for
# kernels_gemm.hip and is off for kernels_stream.hip), and nothing of the product links the library.
# A makefile of its own beside tests/cxx/Makefile (make -C tests/cxx -f gemm_harness.mk; build() runs both).
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../mcarray_amd/csrc
FLAGS := -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function
all: libgemm_harness.so libscan_harness.so
gemm_harness.o: gemm_harness.hip gemm_harness.h $(CSRC)/kernels_gemm.hip $(CSRC)/mca_internal.h
	$(HIPCC) $(FLAGS) -c $< -o $@
gemm_harness_stream.o: gemm_harness_stream.hip gemm_harness.h $(CSRC)/kernels_stream.hip $(wildcard $(CSRC)/*.h)
	$(HIPCC) $(FLAGS) -fno-slp-vectorize -c $< -o $@
libgemm_harness.so: gemm_harness.o gemm_harness_stream.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $^
# the scan / peak-pick / repair-plan kernels of csrc/kernels_stream.hip behind one launcher each (tests/test_gpu_scan_kernels.py): a library
# of its own, because a second translation unit with the same kernels cannot link into libgemm_harness.so
scan_harness.o: scan_harness.hip gemm_harness.h $(CSRC)/kernels_stream.hip $(wildcard $(CSRC)/*.h)
	$(HIPCC) $(FLAGS) -fno-slp-vectorize -c $< -o $@
libscan_harness.so: scan_harness.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $^
clean:
	rm -f libgemm_harness.so gemm_harness.o gemm_harness_stream.o libscan_harness.so scan_harness.o
