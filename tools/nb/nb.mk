# Fragment for oracle/ref/Makefile, behind tools/nr/nr.mk: the fixture recorders of the noise blanker.
#
#   make -C oracle/ref -f Makefile -f ../../tools/nr/nr.mk -f ../../tools/nb/nb.mk OUT=<dir> nb_driver nb_stream
#
# compiles the reference where it lies with that Makefile's flags.  The harness hard-wires
# is_dsp_nb_active() to false, so audio_nr.c and the recorders are compiled with that name changed to
# NbRec_active, which each recorder defines, on top of nr.mk's renames.  nb_driver links
# tools/nb/nb_driver.c, a translation unit that includes the reference's audio_nr.c (the frame
# function AudioNr_RunNoiseReduction is static), into $(OUT)/nb_driver; nb_stream links the
# reference's audio_nr.c as an object with tools/nb/nb_stream.c, which includes audio_driver.c for
# AudioDriver_RxProcessorNoiseReduction, into $(OUT)/nb_stream.  OUT as for nr.mk.

NB_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
NB_RENAME := $(NR_RENAME) -DFilterInfo=NrFilterInfo -Dis_dsp_nb_active=NbRec_active

nb_driver: $(OUT)/nb_driver
nb_stream: $(OUT)/nb_stream

$(OBJ)/nb_audio_nr.o: $(REF)/drivers/audio/audio_nr.c | $(OBJ)
	$(CC) $(CFLAGS) $(NB_RENAME) -c $< -o $@

$(OBJ)/nb_driver.o: $(NB_DIR)/nb_driver.c $(REF)/drivers/audio/audio_nr.c | $(OBJ)
	$(CC) $(CFLAGS) $(NB_RENAME) -c $< -o $@

$(OBJ)/nb_stream.o: $(NB_DIR)/nb_stream.c | $(OBJ)
	$(CC) $(CFLAGS) $(NB_RENAME) -c $< -o $@

# alt_noise_blanking calls these two (nr.mk has the rule)
NB_STAT := $(OBJ)/nr_arm_var_f32.o $(OBJ)/nr_arm_power_f32.o

$(OUT)/nb_driver: $(NR_BASE) $(NB_STAT) $(OBJ)/nb_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections -lm

$(OUT)/nb_stream: $(filter-out $(OBJ)/har_ref_audio_driver_tu.o,$(NR_BASE)) $(OBJ)/nb_audio_nr.o $(NB_STAT) $(OBJ)/nb_stream.o
	$(CC) -o $@ $^ -Wl,--gc-sections -lm

.PHONY: nb_driver nb_stream
