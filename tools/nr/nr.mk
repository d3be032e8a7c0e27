# Fragment for oracle/ref/Makefile: the fixture recorders of the spectral noise reduction.
#
#   make -C oracle/ref -f Makefile -f ../../tools/nr/nr.mk OUT=<dir> nr_driver nr_stream
#
# compiles the reference where it lies with that Makefile's flags.  nr_driver links its objects,
# the harness without its main, and tools/nr/nr_driver.c, a translation unit that includes the
# reference's audio_nr.c (its frame function is static), into $(OUT)/nr_driver (the frame stage
# alone, the inverse transform, the tables); nr_stream links the reference's audio_nr.c as an
# object with tools/nr/nr_stream.c, a translation unit that includes the reference's audio_driver.c
# for AudioDriver_RxProcessorNoiseReduction, into $(OUT)/nr_stream.  OUT is oracle/_ref
# (git-ignored) or any directory outside the repository.
#
# The harness defines empty NR_Init and NR_*_buffer_* functions, so audio_nr.c and the recorders are
# compiled with those names changed.  FilterInfo is renamed as well: nr_filter.c supplies a table
# of its own, so a case can name any filter width, not only the firmware's.

NR_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
NR_RENAME := -DNR_Init=RefNR_Init -DNR_in_buffer_add=RefNR_in_buffer_add -DNR_in_buffer_peek=RefNR_in_buffer_peek \
             -DNR_in_buffer_remove=RefNR_in_buffer_remove -DNR_in_buffer_reset=RefNR_in_buffer_reset \
             -DNR_in_has_data=RefNR_in_has_data -DNR_in_has_room=RefNR_in_has_room \
             -DNR_out_buffer_add=RefNR_out_buffer_add -DNR_out_buffer_peek=RefNR_out_buffer_peek \
             -DNR_out_buffer_remove=RefNR_out_buffer_remove -DNR_out_buffer_reset=RefNR_out_buffer_reset \
             -DNR_out_has_data=RefNR_out_has_data -DNR_out_has_room=RefNR_out_has_room

nr_driver: $(OUT)/nr_driver
nr_stream: $(OUT)/nr_stream

$(OBJ)/nr_audio_nr.o: $(REF)/drivers/audio/audio_nr.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -DFilterInfo=NrFilterInfo -c $< -o $@

$(OBJ)/nr_driver.o: $(NR_DIR)/nr_driver.c $(REF)/drivers/audio/audio_nr.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -DFilterInfo=NrFilterInfo -c $< -o $@

$(OBJ)/nr_filter.o: $(NR_DIR)/nr_filter.c | $(OBJ)
	$(CC) -O2 -c $< -o $@

$(OBJ)/nr_bitrev.o: $(NR_DIR)/nr_bitrev.c | $(OBJ)
	$(CC) -O2 -c $< -o $@

$(OBJ)/nr_stream.o: $(NR_DIR)/nr_stream.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -DFilterInfo=NrFilterInfo -c $< -o $@

# AudioNr_HandleNoiseReduction reaches the noise blanker (never active here), which calls these two
$(OBJ)/nr_arm_%.o: $(DSP)/StatisticsFunctions/arm_%.c | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

NR_BASE := $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/nr_filter.o $(OBJ)/nr_bitrev.o

$(OUT)/nr_driver: $(NR_BASE) $(OBJ)/nr_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections -lm

$(OUT)/nr_stream: $(filter-out $(OBJ)/har_ref_audio_driver_tu.o,$(NR_BASE)) $(OBJ)/nr_audio_nr.o $(OBJ)/nr_arm_var_f32.o $(OBJ)/nr_arm_power_f32.o $(OBJ)/nr_stream.o
	$(CC) -o $@ $^ -Wl,--gc-sections -lm

.PHONY: nr_driver nr_stream
