# Fragment for oracle/ref/Makefile: the fixture recorder of the CW decoder back end.
#
#   make -C oracle/ref -f Makefile -f ../../tools/cwtext/cwtext.mk OUT=<dir> cwtext
#
# compiles the reference where it lies with that Makefile's flags and links its objects, the
# harness without its main, and tools/cwtext/cwtext_driver.c into $(OUT)/cwtext_driver.  OUT is
# oracle/_ref (git-ignored) or any directory outside the repository.

CWTEXT_SRC := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))cwtext_driver.c)

cwtext: $(OUT)/cwtext_driver

$(OBJ)/cwtext_driver.o: $(CWTEXT_SRC) | $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

$(OUT)/cwtext_driver: $(REF_OBJS) $(filter-out $(OBJ)/har_ref_main.o,$(HAR_OBJS)) $(OBJ)/hann_tables.o $(OBJ)/cwtext_driver.o
	$(CC) -o $@ $^ -Wl,--gc-sections -Wl,--wrap=UiDriver_TextMsgPutChar -lm

.PHONY: cwtext
