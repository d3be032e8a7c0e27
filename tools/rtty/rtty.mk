# Fragment for oracle/ref/Makefile: the fixture recorders of the RTTY decoder.
#
#   make -C oracle/ref -f Makefile -f ../../tools/rtty/rtty.mk OUT=<dir> rtty rtty_chain
#
# compiles the reference where it lies with that Makefile's flags.  rtty links its objects, the
# harness without its main, and tools/rtty/rtty_driver.c into $(OUT)/rtty_driver (the decoder
# alone); rtty_chain links them with the harness' own main and tools/rtty/rtty_capture.c into
# $(OUT)/rtty_chain (the whole receive chain, the samples it hands the decoder logged).  OUT is
# oracle/_ref (git-ignored) or any directory outside the repository.

RTTY_SRC := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))rtty_driver.c)

RTTY_CAP_SRC := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))rtty_capture.c)

rtty: $(OUT)/rtty_driver
rtty_chain: $(OUT)/rtty_chain

$(OBJ)/rtty_capture.o: $(RTTY_CAP_SRC) | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/rtty_chain: $(REF_OBJS) $(HAR_OBJS) $(OBJ)/hann_tables.o $(OBJ)/rtty_capture.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=Rtty_Demodulator_ProcessSample -Wl,--wrap=UiDriver_TextMsgPutChar -lm

$(OBJ)/rtty_driver.o: $(RTTY_SRC) | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/rtty_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/rtty_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=UiDriver_TextMsgPutChar -lm

.PHONY: rtty rtty_chain
