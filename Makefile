# Build of the MI355X UHSDR RX hot path (gfx950) and its CPU oracle.
#
#   make            -> uhsdr_amd/lib/libuhsdr_amd.so   (product: C-ABI, HIP kernels + host setup)
#                      oracle/build/libuhsdr_oracle.so (test infrastructure: CPU restatement)
#                      tests/build/libuhsdr_libm_probe{,_host}.so, libuhsdr_expf_probe{,_host}.so (test-only libm probes)
#   make ref        -> oracle/_ref/uhsdr_ref          (reference firmware chain, needs /root/reference)
#   make fixtures-check -> every module fixture under tests/golden re-recorded from the reference and compared (needs it too)
#   make sanitize   -> tests/build/sanitize/: the modules' host code under ASan / UBSan (tools/sanitize.mk; CPU only)
#
# Host C is compiled without FP contraction and without -march, like the reference build,
# so every binary32 rounding of the setup math and of the oracle matches the reference.

HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950
HOSTCFLAGS := -O2 -fPIC -ffp-contract=off -std=gnu11 -Wall -Wno-unused-function
HIPFLAGS   := --offload-arch=$(ARCH) -Iuhsdr_amd/csrc -O3 -fPIC -ffp-contract=off -fno-slp-vectorize -std=c++17 -Wno-unused-result

LIB     := uhsdr_amd/lib/libuhsdr_amd.so
CMSISLIB := uhsdr_amd/lib/libuhsdr_cmsis.so
ORACLE  := oracle/build/libuhsdr_oracle.so
OBJDIR  := uhsdr_amd/build

HOST_SRCS := uhsdr_amd/csrc/uhsdr_setup.c uhsdr_amd/csrc/uhsdr_filter_tables.c
HIP_SRCS  := uhsdr_amd/csrc/uhsdr_rx.hip uhsdr_amd/csrc/uhsdr_tx.hip uhsdr_amd/csrc/uhsdr_spectrum.hip uhsdr_amd/csrc/uhsdr_i2s.hip uhsdr_amd/csrc/uhsdr_fir.hip uhsdr_amd/csrc/uhsdr_cwdec.hip uhsdr_amd/csrc/uhsdr_rtty.hip uhsdr_amd/csrc/uhsdr_psk.hip uhsdr_amd/csrc/uhsdr_digimod.hip uhsdr_amd/csrc/uhsdr_cwgen.hip uhsdr_amd/csrc/uhsdr_nr.hip uhsdr_amd/csrc/uhsdr_nb.hip uhsdr_amd/csrc/uhsdr_meter.hip uhsdr_amd/csrc/uhsdr_display.hip uhsdr_amd/csrc/uhsdr_wfall.hip
HOST_OBJS := $(patsubst uhsdr_amd/csrc/%.c,$(OBJDIR)/%.o,$(HOST_SRCS))
HIP_OBJS  := $(patsubst uhsdr_amd/csrc/%.hip,$(OBJDIR)/%.o,$(HIP_SRCS))
HDRS := uhsdr_amd/csrc/uhsdr_rx_variants.inc include/uhsdr.h uhsdr_amd/csrc/uhsdr_internal.h uhsdr_amd/csrc/uhsdr_dsp.h uhsdr_amd/csrc/uhsdr_libm.h uhsdr_amd/csrc/uhsdr_cfft.h uhsdr_amd/csrc/uhsdr_cwdec.h uhsdr_amd/csrc/uhsdr_rtty.h uhsdr_amd/csrc/uhsdr_psk.h uhsdr_amd/csrc/uhsdr_digiq.h uhsdr_amd/csrc/uhsdr_rttymod.h uhsdr_amd/csrc/uhsdr_pskmod.h uhsdr_amd/csrc/uhsdr_arena.h uhsdr_amd/csrc/uhsdr_digimod_host.h uhsdr_amd/csrc/uhsdr_cwgen.h uhsdr_amd/csrc/uhsdr_cwgen_host.h uhsdr_amd/csrc/uhsdr_cwgen_tables.h uhsdr_amd/csrc/uhsdr_nr.h uhsdr_amd/csrc/uhsdr_nr_tables.h uhsdr_amd/csrc/uhsdr_libm_expf.h uhsdr_amd/csrc/uhsdr_nb.h uhsdr_amd/csrc/uhsdr_meter.h uhsdr_amd/csrc/uhsdr_meter_host.h uhsdr_amd/csrc/uhsdr_meter_tables.h uhsdr_amd/csrc/uhsdr_log10f_fast.h uhsdr_amd/csrc/uhsdr_display.h uhsdr_amd/csrc/uhsdr_display_host.h uhsdr_amd/csrc/uhsdr_display_tables.h uhsdr_amd/csrc/uhsdr_wfall.h uhsdr_amd/csrc/uhsdr_wfall_tables.h

EXAMPLE := examples/build/rx_batch

# test-only probes of uhsdr_libm.h and the IEEE primitives (tests/test_gpu_libm.py): the device
# build under exactly the product's HIPFLAGS, the host build under exactly HOSTCFLAGS
PROBE      := tests/build/libuhsdr_libm_probe.so
PROBE_HOST := tests/build/libuhsdr_libm_probe_host.so
# the same pair for ul_expf (tests/test_expf.py, tests/test_gpu_expf.py)
EXPF_PROBE      := tests/build/libuhsdr_expf_probe.so
EXPF_PROBE_HOST := tests/build/libuhsdr_expf_probe_host.so

all: $(LIB) $(CMSISLIB) $(ORACLE) $(EXAMPLE) $(PROBE) $(PROBE_HOST) $(EXPF_PROBE) $(EXPF_PROBE_HOST)

$(OBJDIR) uhsdr_amd/lib oracle/build tests/build:
	mkdir -p $@

$(PROBE): tests/device/libm_probe.hip uhsdr_amd/csrc/uhsdr_libm.h | tests/build
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

$(PROBE_HOST): tests/device/libm_probe_host.c uhsdr_amd/csrc/uhsdr_libm.h | tests/build
	$(CC) $(HOSTCFLAGS) -shared -o $@ $< -lm

$(EXPF_PROBE): tests/device/expf_probe.hip uhsdr_amd/csrc/uhsdr_libm.h uhsdr_amd/csrc/uhsdr_libm_expf.h | tests/build
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

$(EXPF_PROBE_HOST): tests/device/expf_probe_host.c uhsdr_amd/csrc/uhsdr_libm.h uhsdr_amd/csrc/uhsdr_libm_expf.h | tests/build
	$(CC) $(HOSTCFLAGS) -shared -o $@ $< -lm

$(OBJDIR)/%.o: uhsdr_amd/csrc/%.c $(HDRS) | $(OBJDIR)
	$(CC) $(HOSTCFLAGS) -c $< -o $@

$(OBJDIR)/%.o: uhsdr_amd/csrc/%.hip $(HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(HOST_OBJS) $(HIP_OBJS) | uhsdr_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -lm

# CMSIS-DSP signature shims (include/uhsdr_cmsis.h): a library of their own, so the arm_* names
# never collide with a CMSIS build linked elsewhere; uses libuhsdr_amd.so's setup layer
$(OBJDIR)/uhsdr_cmsis.o: uhsdr_amd/csrc/uhsdr_cmsis.hip include/uhsdr_cmsis.h $(HDRS) | $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CMSISLIB): $(OBJDIR)/uhsdr_cmsis.o $(LIB) | uhsdr_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJDIR)/uhsdr_cmsis.o -Luhsdr_amd/lib -luhsdr_amd -Wl,-rpath,'$$ORIGIN' -lm

$(ORACLE): oracle/uhsdr_oracle.c oracle/uhsdr_oracle.h include/uhsdr.h | oracle/build
	$(CC) $(HOSTCFLAGS) -shared -o $@ $< -lm -lpthread

examples/build:
	mkdir -p $@

# plain C host against the C ABI: gcc only, no HIP headers
$(EXAMPLE): examples/rx_batch.c include/uhsdr.h $(LIB) | examples/build
	$(CC) -O2 -std=gnu11 -Wall -Iinclude -o $@ $< -Luhsdr_amd/lib -luhsdr_amd -Wl,-rpath,'$$ORIGIN/../../uhsdr_amd/lib'

ref:
	$(MAKE) -C oracle/ref

# re-record every module fixture from the reference (tools/recording.py) and the five generated
# table headers, and fail where a committed file would change; nothing is written
MAKERS := cwtext rtty psk digimod cwgen nr nb meter display wfall
fixtures-check:
	set -e; for m in $(MAKERS); do python3 tools/$$m/make_$${m}_golden.py --check; done
	python3 tools/nr/make_nr_chain_golden.py --check
	python3 tools/cwgen/gen_cwgen_tables.py --check
	python3 tools/nr/gen_nr_tables.py --check
	python3 tools/meter/gen_meter_tables.py --check
	python3 tools/display/gen_display_tables.py --check
	python3 tools/wfall/gen_wfall_tables.py --check

include tools/sanitize.mk

clean:
	rm -rf $(OBJDIR) uhsdr_amd/lib oracle/build examples/build tests/build

.PHONY: all ref fixtures-check clean

# compile-time variants of libuhsdr_amd.so for A/B measurement (bench.py with UHSDR_LIB=<path>):
#   make variant VTAG=trace VFLAGS=-DUHSDR_TRACE
# every HIP source is rebuilt with VFLAGS into its own object directory, so a flag read by any
# source takes effect (VFLAGS=-Itools/isa builds only the P48 receive kernels: quick A/B builds;
# VFLAGS comes first on the line, so its -I wins over csrc for uhsdr_rx_variants.inc)
VARIANT_DIR := uhsdr_amd/lib/variants
VOBJDIR = $(OBJDIR)/v_$(VTAG)
VHIP_OBJS = $(patsubst uhsdr_amd/csrc/%.hip,$(VOBJDIR)/%.o,$(HIP_SRCS))
$(OBJDIR)/v_%/.dir:
	mkdir -p $(dir $@) && touch $@
.PRECIOUS: $(OBJDIR)/v_%/.dir
$(VOBJDIR)/%.o: uhsdr_amd/csrc/%.hip $(HDRS) | $(VOBJDIR)/.dir
	$(HIPCC) $(VFLAGS) $(HIPFLAGS) -c $< -o $@
variant: $(HOST_OBJS) $(VHIP_OBJS)
	mkdir -p $(VARIANT_DIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $(VARIANT_DIR)/libuhsdr_amd_$(VTAG).so $(HOST_OBJS) $(VHIP_OBJS) -lm

.PHONY: variant
