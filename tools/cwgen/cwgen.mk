# Fragment for oracle/ref/Makefile: the fixture recorder of the CW generator.
#
#   make -C oracle/ref -f Makefile -f ../../tools/cwgen/cwgen.mk OUT=<dir> cwgen_driver
#
# compiles the reference where it lies with that Makefile's flags and links its objects, the harness
# without its main, and tools/cwgen/cwgen_driver.c into $(OUT)/cwgen_driver.  OUT is oracle/_ref
# (git-ignored) or any directory outside the repository.
#
# The harness' empty key-line, text-ring, TX-request and text-output hooks, and the reference's
# softdds_runIQ, are re-routed to the recorder's at link time with --wrap: the reference's calls land
# in __wrap_<name> of cwgen_driver.c.

CWGEN_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
CWGEN_WRAP := -Wl,--wrap=Board_DitLinePressed -Wl,--wrap=Board_PttDahLinePressed \
              -Wl,--wrap=DigiModes_TxBufferRemove -Wl,--wrap=DigiModes_TxBufferPutChar -Wl,--wrap=DigiModes_TxBufferPutSign \
              -Wl,--wrap=RadioManagement_Request_TxOn -Wl,--wrap=RadioManagement_Request_TxOff \
              -Wl,--wrap=UiDriver_TextMsgPutChar -Wl,--wrap=softdds_runIQ

cwgen_driver: $(OUT)/cwgen_driver

$(OBJ)/cwgen_driver.o: $(CWGEN_DIR)/cwgen_driver.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/cwgen_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/cwgen_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections $(CWGEN_WRAP) -lm

# cwtx_driver: the whole transmit chain in CW mode, TxProcessor_Run through the harness' own main;
# CwGen_Process is wrapped as well, so that every call sets the key lines first
cwtx_driver: $(OUT)/cwtx_driver

$(OBJ)/cwtx_driver.o: $(CWGEN_DIR)/cwtx_driver.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/cwtx_driver: $(REF_OBJS) $(HAR_OBJS) $(OBJ)/hann_tables.o $(OBJ)/cwtx_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections $(CWGEN_WRAP) -Wl,--wrap=CwGen_Process -lm

.PHONY: cwgen_driver cwtx_driver
