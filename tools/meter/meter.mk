# Fragment for oracle/ref/Makefile: the fixture recorder of the signal meter.
#
#   make -C oracle/ref -f Makefile -f ../../tools/meter/meter.mk OUT=<dir> meter_driver
#
# compiles the reference where it lies with that Makefile's flags.  meter_driver links the
# reference objects, the harness without its main, and the two translation units of tools/meter:
# meter_spectrum_tu.c includes the reference's ui_spectrum.c (UiSpectrum_CalculateDBm is static),
# meter_driver.c its ui_driver.c (UiDriver_HandleSMeter is static) and has the program.  ui_driver.c
# is the firmware's whole front panel: of the several hundred LCD, menu, codec and USB names it
# refers to, the meter's three functions reach a dozen, which meter_driver.c defines empty, so the link
# leaves the rest unresolved; and it defines six small functions the harness also has, where the
# harness' definition, first on the line, is kept (RadioManagement_UsesBothSidebands and
# RadioManagement_LSBActive are the harness' as well, as for every other recorder).  OUT as for nr.mk.

METER_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))

meter_driver: $(OUT)/meter_driver

$(OBJ)/meter_spectrum_tu.o: $(METER_DIR)/meter_spectrum_tu.c $(REF)/drivers/ui/lcd/ui_spectrum.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OBJ)/meter_driver.o: $(METER_DIR)/meter_driver.c $(REF)/drivers/ui/ui_driver.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/meter_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/meter_spectrum_tu.o $(OBJ)/meter_driver.o
	$(CC) -no-pie -o $@ $^ -Wl,--gc-sections -Wl,--unresolved-symbols=ignore-all -Wl,--allow-multiple-definition -lm

.PHONY: meter_driver
