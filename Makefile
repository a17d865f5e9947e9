# Top-level build (no cmake needed): gcc for host C, hipcc for gfx950.
#
#   make            libhiphuff.so + HuffFramework CLI + oracle + test emulator
#   make lib        huffmandecoderongpus_amd/libhiphuff.so only
#
# Outputs stay in-tree (git-ignored) so they travel to the GPU box.

HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
CXX      ?= g++
ARCH     ?= gfx950
PKG      := huffmandecoderongpus_amd
CSRC     := $(PKG)/csrc
BUILD    := build
INC      := -Iinclude -I$(CSRC)
CFLAGS   := -O3 -fPIC -Wall -Wextra -std=gnu11 $(INC)
HIPFLAGS := $(HIPEXTRA) -O3 -fPIC -std=c++17 --offload-arch=$(ARCH) -Wall -Wno-unused-result -Wno-unused-value \
            -Wno-comment $(INC)

LIB      := $(PKG)/libhiphuff.so
CLI      := $(BUILD)/HuffFramework
EMU      := tests/emu/libhh_emu.so
# the decoder's .hip units, listed once for `lib` and `variant`, and the
# objects a variant takes as built
DEC_UNITS  := hh_device hh_r2 hh_exact hh_host hh_fsm hh_one hh_batch hh_batch_plan hh_batch_read hh_batch_gather hh_batch_take
DEC_HDRS   := $(addprefix $(CSRC)/,hh_algo.h hh_batch.h hh_batch_algo.h hh_batch_gather_algo.h hh_batch_plan_algo.h \
              hh_batch_read_algo.h hh_batch_take_algo.h hh_dec.h \
              hh_fsm.h hh_fsm_algo.h hh_fsm_dev.h hh_fsm_kern.h hh_internal.h) include/hiphuff.h
OTHER_OBJS := $(BUILD)/hh_encode.o $(BUILD)/hh_encb.o $(BUILD)/hh_encr.o $(BUILD)/hh_hist.o $(BUILD)/hh_probe.o $(BUILD)/hh_build.o \
              $(BUILD)/hh_plugin.o

all: lib cli oracle emu ubench

lib: $(LIB)
cli: $(CLI)
emu: $(EMU)

$(BUILD):
	mkdir -p $(BUILD)

$(BUILD)/hh_huff.o: $(CSRC)/hh_huff.c $(CSRC)/hh_internal.h $(CSRC)/hh_fsm.h include/hiphuff.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(BUILD)/hh_plugin.o: $(CSRC)/hh_plugin.c include/hiphuff.h include/hiphuff_plugin.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

# the decoder's units: one rule, every private header a prerequisite of each
# (a unit rebuilt once too often rather than once too seldom)
$(DEC_UNITS:%=$(BUILD)/%.o): $(BUILD)/%.o: $(CSRC)/%.hip $(DEC_HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hh_encode.o: $(CSRC)/hh_encode.hip $(CSRC)/hh_enc_kern.h $(CSRC)/hh_internal.h $(CSRC)/hh_enc.h \
                      include/hiphuff.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hh_encb.o: $(CSRC)/hh_encb.hip $(CSRC)/hh_enc_kern.h $(CSRC)/hh_internal.h $(CSRC)/hh_enc.h \
                    include/hiphuff.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hh_encr.o: $(CSRC)/hh_encr.hip $(CSRC)/hh_encr_algo.h $(CSRC)/hh_enc_kern.h $(CSRC)/hh_internal.h \
                    $(CSRC)/hh_enc.h include/hiphuff.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hh_hist.o: $(CSRC)/hh_hist.hip $(CSRC)/hh_hist_kern.h $(CSRC)/hh_enc.h include/hiphuff.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hh_build.o: $(CSRC)/hh_build.c include/hiphuff.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(BUILD)/hh_probe.o: $(CSRC)/hh_probe.hip include/hiphuff.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(DEC_UNITS:%=$(BUILD)/%.o) $(BUILD)/hh_encode.o $(BUILD)/hh_encb.o $(BUILD)/hh_encr.o $(BUILD)/hh_hist.o \
        $(BUILD)/hh_probe.o $(BUILD)/hh_huff.o $(BUILD)/hh_build.o $(BUILD)/hh_plugin.o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^

$(CLI): $(PKG)/host/hh_cli.c $(LIB) include/hiphuff.h include/hiphuff_plugin.h
	$(CC) -O2 -Wall -Wextra -std=gnu11 $(INC) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< -L$(PKG) -lhiphuff \
	    -Wl,-rpath,'$$ORIGIN/../$(PKG)' -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lm

oracle:
	$(MAKE) -C oracle

# microbenchmarks the profiling scripts run (tools/profile.sh: FETCH_SIZE
# calibration on known byte counts)
ubench: $(BUILD)/ub_fetch $(BUILD)/ub_hist
# the histogram kernel's LDS copies x workgroups per CU (DESIGN.md "Compression")
$(BUILD)/ub_hist: tools/ubench/ub_hist.hip $(CSRC)/hh_hist_kern.h | $(BUILD)
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -I$(CSRC) -o $@ $<
$(BUILD)/ub_fetch: tools/ubench/ub_fetch.hip | $(BUILD)
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ $<

$(EMU): tests/emu/hh_emu.cpp tests/emu/hh_fsm_emu.cpp tests/emu/hh_batch_emu.cpp tests/emu/hh_batch_plan_emu.cpp \
        tests/emu/hh_blocks_read_emu.cpp tests/emu/hh_blocks_gather_emu.cpp tests/emu/hh_encr_emu.cpp tests/emu/hh_take_emu.cpp \
        $(CSRC)/hh_batch_take_algo.h $(CSRC)/hh_algo.h $(CSRC)/hh_fsm_algo.h $(CSRC)/hh_encr_algo.h \
        $(CSRC)/hh_batch_algo.h $(CSRC)/hh_batch_gather_algo.h $(CSRC)/hh_batch_plan_algo.h \
        $(CSRC)/hh_batch_read_algo.h $(CSRC)/hh_fsm.h $(CSRC)/hh_internal.h $(BUILD)/hh_huff.o
	$(CXX) -O2 -fPIC -shared $(INC) -Wno-comment -o $@ tests/emu/hh_emu.cpp tests/emu/hh_fsm_emu.cpp \
	    tests/emu/hh_batch_emu.cpp tests/emu/hh_batch_plan_emu.cpp tests/emu/hh_blocks_read_emu.cpp \
	    tests/emu/hh_blocks_gather_emu.cpp tests/emu/hh_encr_emu.cpp tests/emu/hh_take_emu.cpp $(BUILD)/hh_huff.o

clean:
	rm -rf $(BUILD) $(LIB) $(EMU)
	$(MAKE) -C oracle clean

.PHONY: all lib cli emu oracle ubench clean

# A/B variant of the library: make variant V=name HIPEXTRA="-DHH_X=1"
# -> build/libhiphuff_<name>.so (tools/mkvar.sh, tools/gpu_ab.sh): the decoder's
# units and hh_huff.c compiled again with HIPEXTRA, the rest as built
$(BUILD)/%_$(V).o: $(CSRC)/%.hip FORCE | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(BUILD)/hh_huff_$(V).o: $(CSRC)/hh_huff.c FORCE | $(BUILD)
	$(CC) $(CFLAGS) $(HIPEXTRA) -c $< -o $@
variant: $(DEC_UNITS:%=$(BUILD)/%_$(V).o) $(BUILD)/hh_huff_$(V).o $(OTHER_OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $(BUILD)/libhiphuff_$(V).so $^
FORCE:
.PHONY: variant FORCE
