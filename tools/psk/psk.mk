# Fragment for oracle/ref/Makefile: the fixture recorders of the BPSK decoder.
#
#   make -C oracle/ref -f Makefile -f ../../tools/psk/psk.mk OUT=<dir> psk_driver psk_chain
#
# compiles the reference where it lies with that Makefile's flags.  psk_driver links its objects,
# the reference's psk.c, the harness without its main, and tools/psk/psk_driver.c into
# $(OUT)/psk_driver (the decoder alone); psk_chain links them with the harness' own main and
# tools/psk/psk_capture.c into $(OUT)/psk_chain (the whole receive chain, the samples it hands the
# decoder logged).  OUT is oracle/_ref (git-ignored) or any directory outside the repository.
#
# The harness defines empty Psk_Modem_Init / Psk_Demodulator_ProcessSample / Psk_Modulator_GenSample,
# so psk.c and the two recorders are compiled with these three renamed.  The targets carry the
# binaries' names: a target called psk would meet make's built-in rule psk: psk.c through vpath.

PSK_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
PSK_RENAME := -DPsk_Modem_Init=RefPsk_Modem_Init -DPsk_Demodulator_ProcessSample=RefPsk_Demodulator_ProcessSample \
              -DPsk_Modulator_GenSample=RefPsk_Modulator_GenSample

psk_driver: $(OUT)/psk_driver
psk_chain: $(OUT)/psk_chain

$(OBJ)/psk_decoder.o: $(REF)/drivers/audio/psk.c | $(OBJ)
	$(CC) $(CFLAGS) $(PSK_RENAME) -c $< -o $@

$(OBJ)/psk_capture.o: $(PSK_DIR)/psk_capture.c | $(OBJ)
	$(CC) $(CFLAGS) $(PSK_RENAME) -c $< -o $@

$(OBJ)/psk_driver.o: $(PSK_DIR)/psk_driver.c | $(OBJ)
	$(CC) $(CFLAGS) $(PSK_RENAME) -c $< -o $@

$(OUT)/psk_chain: $(REF_OBJS) $(HAR_OBJS) $(OBJ)/hann_tables.o $(OBJ)/psk_decoder.o $(OBJ)/psk_capture.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=Psk_Demodulator_ProcessSample -Wl,--wrap=UiDriver_TextMsgPutChar -lm

$(OUT)/psk_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/psk_decoder.o $(OBJ)/psk_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=UiDriver_TextMsgPutChar -lm

.PHONY: psk_driver psk_chain
