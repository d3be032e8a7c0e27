# Fragment for oracle/ref/Makefile: the fixture recorder of the waterfall image.
#
#   make -C oracle/ref -f Makefile -f ../../tools/wfall/wfall.mk OUT=<dir> wfall_driver
#
# compiles the reference where it lies with that Makefile's flags.  wfall_driver links the reference
# objects, the harness, and the two translation units of tools/wfall: wfall_spectrum_tu.c includes
# the reference's ui_spectrum.c (UiSpectrum_DrawWaterfall is static), wfall_driver.c has the program
# and the LCD calls, of which UiLcdHy28_BulkPixel_PutBuffer records the rows.  The harness'
# ref_main.c is compiled once more for this program alone, with its main renamed to
# WfallRec_ref_main and its call of ref_spec_frame to WfallRec_spec_frame, as display.mk does for
# its recorder.  psk_speeds and psk_ctrl_config, which the BPSK markers read, are the reference's
# psk.c, compiled as psk.mk compiles it (the harness defines three of its functions empty, so they
# are renamed).  OUT as for nr.mk.

WFALL_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))

wfall_driver: $(OUT)/wfall_driver

$(OBJ)/wfall_spectrum_tu.o: $(WFALL_DIR)/wfall_spectrum_tu.c $(REF)/drivers/ui/lcd/ui_spectrum.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJ)/wfall_driver.o: $(WFALL_DIR)/wfall_driver.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJ)/wfall_ref_main.o: $(CURDIR)/ref_main.c | $(OBJ)
	$(CC) $(CFLAGS) -Dmain=WfallRec_ref_main -Dref_spec_frame=WfallRec_spec_frame -c $< -o $@

$(OBJ)/wfall_psk.o: $(REF)/drivers/audio/psk.c | $(OBJ)
	$(CC) $(CFLAGS) -DPsk_Modem_Init=RefPsk_Modem_Init -DPsk_Demodulator_ProcessSample=RefPsk_Demodulator_ProcessSample \
	      -DPsk_Modulator_GenSample=RefPsk_Modulator_GenSample -c $< -o $@

$(OUT)/wfall_driver: $(OBJ)/wfall_psk.o $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/wfall_ref_main.o $(OBJ)/wfall_spectrum_tu.o $(OBJ)/wfall_driver.o
	$(CC) -no-pie -o $@ $^ -Wl,--gc-sections -Wl,--unresolved-symbols=ignore-all -Wl,--allow-multiple-definition -lm

.PHONY: wfall_driver
