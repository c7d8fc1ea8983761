# Builds libsublist_dev_shim.so for gfx950, with the flags of hekaton_system_amd/csrc/Makefile: MsmSort::sublist (the
# sub-list kernels of msm.cuh and scan_u32) on a caller-supplied sorted list, for tests/test_msm_sublist_gpu.py.  Integer
# kernels only, so there is no -DHK_NO_ASM_MUL twin.  Like the libraries of the Makefile next to it, it must pass the
# code-object bounds libhekaton passes (tools/kernel_meta.py --check) before it exists.
# make -f sublist.mk
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
EXTRA ?=
CXXFLAGS = -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wno-unused-result $(EXTRA)
CSRC   = ../../hekaton_system_amd/csrc
OUTDIR ?= ../../hekaton_system_amd/lib
HDRS   = $(wildcard $(CSRC)/*.cuh) $(wildcard $(CSRC)/*.h) ../../include/hekaton.h
META   = ../../tools/kernel_meta.py

all: $(OUTDIR)/libsublist_dev_shim.so

# k_msm_sub_*<0> and k_scan_u32_*<0> are libhekaton's symbols too: -Bsymbolic, so that the library's launches reach its own
# code objects whatever else the process has loaded
$(OUTDIR)/libsublist_dev_shim.so: sublist_dev_shim.hip $(HDRS) $(META)
	@mkdir -p $(OUTDIR)
	$(HIPCC) $(CXXFLAGS) -shared -Wl,-Bsymbolic -o $@.tmp $<
	python3 $(META) --check $@.tmp > $(OUTDIR)/kernel_meta_sublist_dev_shim.txt || { rm -f $@.tmp; tail -5 $(OUTDIR)/kernel_meta_sublist_dev_shim.txt; exit 1; }
	mv $@.tmp $@

clean:
	rm -f $(OUTDIR)/libsublist_dev_shim.so
