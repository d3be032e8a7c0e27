# Fragment for oracle/ref/Makefile: the fixture recorder of the display stage.
#
#   make -C oracle/ref -f Makefile -f ../../tools/display/display.mk OUT=<dir> display_driver
#
# compiles the reference where it lies with that Makefile's flags.  display_driver links the
# reference objects, the harness, and the two translation units of tools/display:
# display_spectrum_tu.c includes the reference's ui_spectrum.c (the display's functions are static),
# display_driver.c has the program and the LCD calls those functions reach, defined empty.  The
# harness' ref_main.c is compiled once more for this program alone, with its main renamed to
# DisplayRec_ref_main and its call of ref_spec_frame to DisplayRec_spec_frame (display_driver.c), so
# that the recorder sees every display frame of a harness run, ring snapshot included, without a
# line of the harness changed.  ui_spectrum.c refers to far more of the firmware than the display's
# functions reach; the link leaves that unresolved, as for meter.mk.  OUT as for nr.mk.

DISPLAY_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))

display_driver: $(OUT)/display_driver

$(OBJ)/display_spectrum_tu.o: $(DISPLAY_DIR)/display_spectrum_tu.c $(REF)/drivers/ui/lcd/ui_spectrum.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJ)/display_driver.o: $(DISPLAY_DIR)/display_driver.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJ)/display_ref_main.o: $(CURDIR)/ref_main.c | $(OBJ)
	$(CC) $(CFLAGS) -Dmain=DisplayRec_ref_main -Dref_spec_frame=DisplayRec_spec_frame -c $< -o $@

$(OUT)/display_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/display_ref_main.o $(OBJ)/display_spectrum_tu.o $(OBJ)/display_driver.o
	$(CC) -no-pie -o $@ $^ -Wl,--gc-sections -Wl,--unresolved-symbols=ignore-all -Wl,--allow-multiple-definition -lm

.PHONY: display_driver
