# Fragment for oracle/ref/Makefile: the fixture recorder of the RTTY and BPSK modulators.
#
#   make -C oracle/ref -f Makefile -f ../../tools/digimod/digimod.mk OUT=<dir> modgen_driver
#
# compiles the reference where it lies with that Makefile's flags and links its objects, its psk.c,
# the harness without its main, and tools/digimod/modgen_driver.c into $(OUT)/modgen_driver (the two
# modulators alone).  OUT is oracle/_ref (git-ignored) or any directory outside the repository.
#
# The harness defines an empty Psk_Modem_Init / Psk_Demodulator_ProcessSample /
# Psk_Modulator_GenSample, so psk.c and the recorder are compiled with these three renamed, as
# tools/psk/psk.mk does.  Its empty text-ring and TX-off hooks are re-routed to the recorder's at link
# time with --wrap: the reference's calls land in __wrap_<name> of modgen_driver.c.

DIGIMOD_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
DIGIMOD_RENAME := -DPsk_Modem_Init=RefPsk_Modem_Init -DPsk_Demodulator_ProcessSample=RefPsk_Demodulator_ProcessSample \
                  -DPsk_Modulator_GenSample=RefPsk_Modulator_GenSample
DIGIMOD_WRAP := -Wl,--wrap=DigiModes_TxBufferHasData -Wl,--wrap=DigiModes_TxBufferHasDataFor \
                -Wl,--wrap=DigiModes_TxBufferRemove -Wl,--wrap=RadioManagement_Request_TxOff

modgen_driver: $(OUT)/modgen_driver

$(OBJ)/digimod_psk.o: $(REF)/drivers/audio/psk.c | $(OBJ)
	$(CC) $(CFLAGS) $(DIGIMOD_RENAME) -c $< -o $@

$(OBJ)/modgen_driver.o: $(DIGIMOD_DIR)/modgen_driver.c | $(OBJ)
	$(CC) $(CFLAGS) $(DIGIMOD_RENAME) -c $< -o $@

$(OUT)/modgen_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/digimod_psk.o $(OBJ)/modgen_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections $(DIGIMOD_WRAP) -lm

# modtx_driver: the whole transmit chain in DIGI mode, TxProcessor_Run through the harness' own
# main; the harness' Psk_Modulator_GenSample and RadioManagement_IsTxAtZeroIF are wrapped as well
modtx_driver: $(OUT)/modtx_driver

$(OBJ)/modtx_driver.o: $(DIGIMOD_DIR)/modtx_driver.c | $(OBJ)
	$(CC) $(CFLAGS) $(DIGIMOD_RENAME) -c $< -o $@

$(OUT)/modtx_driver: $(REF_OBJS) $(HAR_OBJS) $(OBJ)/hann_tables.o $(OBJ)/digimod_psk.o $(OBJ)/modtx_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections $(DIGIMOD_WRAP) -Wl,--wrap=Psk_Modulator_GenSample \
	      -Wl,--wrap=RadioManagement_IsTxAtZeroIF -lm

.PHONY: modgen_driver modtx_driver
