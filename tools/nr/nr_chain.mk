# Fragment for oracle/ref/Makefile, behind tools/nr/nr.mk: the recorder of the noise reduction and
# blanker inside the receive chain (tests/golden/nrchain_*.npz).
#
#   make -C oracle/ref -f Makefile -f ../../tools/nr/nr.mk -f ../../tools/nr/nr_chain.mk OUT=<dir> nr_chain
#
# compiles the reference where it lies with that Makefile's flags.  The harness has empty NR_Init and
# NR_*_buffer_* functions and hard-wires is_dsp_nb_active() to false, so its audio-driver translation
# unit (oracle/ref/ref_audio_driver_tu.c) is compiled a second time with nr.mk's renames and with
# is_dsp_nb_active changed to NrChain_enter, and the reference's audio_nr.c with the renames and
# is_dsp_nb_active changed to NrChain_nb_active; tools/nr/nr_chain_capture.c defines both.  They are
# linked with the reference's objects, the rest of the harness, its own main, and the capture object,
# with arm_scale_f32, UiDriver_Callback_AudioISR and Rtty_Demodulator_ProcessSample wrapped, into
# $(OUT)/nr_chain.  FilterInfo is the reference's own here: the filter path decides the width.
# OUT is oracle/_ref (git-ignored) or any directory outside the repository; with
# OUT=<dir>/mchf VARIANT_CFLAGS="-include $(CURDIR)/mchf_board.h" it is the mcHF board's chain.

NRC_DIR := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))

nr_chain: $(OUT)/nr_chain

$(OBJ)/nrc_audio_driver_tu.o: $(CURDIR)/ref_audio_driver_tu.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -Dis_dsp_nb_active=NrChain_enter -c $< -o $@

$(OBJ)/nrc_audio_nr.o: $(REF)/drivers/audio/audio_nr.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -Dis_dsp_nb_active=NrChain_nb_active -c $< -o $@

$(OBJ)/nrc_capture.o: $(NRC_DIR)/nr_chain_capture.c | $(OBJ)
	$(CC) $(CFLAGS) $(NR_RENAME) -c $< -o $@

$(OUT)/nr_chain: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_audio_driver_tu.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o \
                 $(OBJ)/nrc_audio_driver_tu.o $(OBJ)/nrc_audio_nr.o $(OBJ)/nr_bitrev.o $(OBJ)/nr_arm_var_f32.o $(OBJ)/nr_arm_power_f32.o $(OBJ)/nrc_capture.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=arm_scale_f32 -Wl,--wrap=UiDriver_Callback_AudioISR \
	    -Wl,--wrap=Rtty_Demodulator_ProcessSample -lm

.PHONY: nr_chain
