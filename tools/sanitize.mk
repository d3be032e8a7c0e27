# Host ASan / UBSan build and run of the ten module drivers (tools/*/*_sanitize.c), included by the
# top-level Makefile:
#
#   make sanitize          (objects, programs, their input files and logs under tests/build/sanitize/)
#
# Stand-alone programs with their own main, on the CPU: the host side of each module's .hip (the
# step functions the kernels run, the arena, the text rings) under the sanitizers, no device call.
# Each module source and the two host C files are compiled once; each program runs on the file its
# dump script writes from tests/golden (cwdec's and nr's dump scripts call the host decoder through
# libuhsdr_amd.so, hence $(LIB)); its output is <program>.log beside it, and the first program
# that exits non-zero stops the target.

SAN          := tests/build/sanitize
SANFLAGS     := -fsanitize=address,undefined -fno-sanitize-recover=undefined
SAN_HIPFLAGS := --offload-arch=$(ARCH) -Iuhsdr_amd/csrc -O1 -g -ffp-contract=off -std=c++17 $(addprefix -Xarch_host ,$(SANFLAGS))
SAN_CFLAGS   := -O1 -g $(SANFLAGS) -ffp-contract=off -Iinclude -Iuhsdr_amd/csrc
PYTHON       ?= python3

# program: its directory under tools/, its dump script, the module sources it links (uhsdr_<m>.hip).
# cwgen takes the text queue's put from digimod, nr's stream can hold a noise blanker; nb_sanitize,
# meter_sanitize, display_sanitize and wfall_sanitize are plain C over uhsdr_nb.h, uhsdr_meter.h,
# uhsdr_display.h and uhsdr_wfall.h and link nothing else (the meter's, the display's and the
# waterfall's dump scripts write each case's plan, built through libuhsdr_amd.so).
SAN_cwdec   := cwtext  dump_states.py  cwdec
SAN_rtty    := rtty    dump_streams.py rtty
SAN_psk     := psk     dump_streams.py psk
SAN_digimod := digimod dump_cases.py   digimod
SAN_cwgen   := cwgen   dump_cases.py   cwgen digimod
SAN_nr      := nr      dump_cases.py   nr nb
SAN_nb      := nb      dump_cases.py
SAN_meter   := meter   dump_cases.py
SAN_display := display dump_cases.py
SAN_wfall   := wfall   dump_cases.py
SAN_PROGS   := cwdec rtty psk digimod cwgen nr nb meter display wfall
SAN_HOST    := $(SAN)/uhsdr_setup.o $(SAN)/uhsdr_filter_tables.o

sanitize: $(LIB) $(SAN_PROGS:%=$(SAN)/%.log)

$(SAN):
	mkdir -p $@

$(SAN)/uhsdr_%.o: uhsdr_amd/csrc/uhsdr_%.hip $(HDRS) | $(SAN)
	$(HIPCC) $(SAN_HIPFLAGS) -c -x hip $< -o $@

$(SAN)/uhsdr_%.o: uhsdr_amd/csrc/uhsdr_%.c $(HDRS) | $(SAN)
	$(CC) $(SAN_CFLAGS) -c $< -o $@

# $(1) program, $(2) directory, $(3) dump script, $(4) module sources
define SAN_PROGRAM
$(SAN)/$(1)_sanitize.o: tools/$(2)/$(1)_sanitize.c $(HDRS) | $(SAN)
	$(CC) $(SAN_CFLAGS) -c $$< -o $$@

$(SAN)/$(1)_sanitize: $(SAN)/$(1)_sanitize.o $(4:%=$(SAN)/uhsdr_%.o) $(if $(4),$(SAN_HOST))
	$(if $(4),$(HIPCC),$(CC)) $(SANFLAGS) $$^ -lm -o $$@

$(SAN)/$(1).bin: tools/$(2)/$(3) $(LIB) FORCE | $(SAN)
	$(PYTHON) $$< $$@

$(SAN)/$(1).log: $(SAN)/$(1)_sanitize $(SAN)/$(1).bin
	$$< $(SAN)/$(1).bin > $$@ 2>&1 || { tail -n 40 $$@; exit 1; }
	@tail -n 1 $$@
endef
$(foreach p,$(SAN_PROGS),$(eval $(call SAN_PROGRAM,$(p),$(word 1,$(SAN_$(p))),$(word 2,$(SAN_$(p))),$(wordlist 3,9,$(SAN_$(p))))))

FORCE:
.PHONY: sanitize FORCE
