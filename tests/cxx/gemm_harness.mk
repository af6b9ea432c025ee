# test-only GPU library: csrc/kernels_gemm.hip behind one launcher of k_srp_gemm_f16_fold, for tests/test_gpu_gemm_fold.py; the product's
# compile line for that file (csrc/Makefile: the SLP vectoriser stays on for it), and nothing of the product links it.
# A makefile of its own beside tests/cxx/Makefile (make -C tests/cxx -f gemm_harness.mk; build() runs both).
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../mcarray_amd/csrc
all: libgemm_harness.so
libgemm_harness.so: gemm_harness.hip $(CSRC)/kernels_gemm.hip $(CSRC)/mca_internal.h
	$(HIPCC) -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -shared $< -o $@
clean:
	rm -f libgemm_harness.so
