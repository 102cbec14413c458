# Builds the drop-in C-ABI library (HIP kernels for gfx950 + C host planner).
#   make            -> fftw3_amd/lib/libfftw3_amd.so (+ libfftw3.so.3 alias)
#   make oracle     -> oracle/liboracle.so (CPU restatement, test infrastructure)
HIPCC ?= /opt/rocm/bin/hipcc
CC ?= gcc
ARCH ?= gfx950
CSRC := fftw3_amd/csrc
LIBDIR := fftw3_amd/lib
CFLAGS := -O2 -fPIC -std=gnu99 -Wall -Wextra -Iinclude -I$(CSRC)
HIPFLAGS := -O3 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -std=c++17 -Wall

OBJS := $(CSRC)/api.o $(CSRC)/planner.o $(CSRC)/split.o $(CSRC)/exec.o $(CSRC)/sharded.o $(CSRC)/slab.o $(CSRC)/slab1d.o $(CSRC)/hostmath.o $(CSRC)/kernels.o $(CSRC)/kernels_elem.o $(CSRC)/fa_hip.o $(CSRC)/kernels_rr.o $(CSRC)/kernels_rr1.o $(CSRC)/kernels_rr2.o $(CSRC)/kernels_r3.o $(CSRC)/kernels_r3r.o $(CSRC)/kernels_r2cm.o $(CSRC)/kernels_blue.o $(CSRC)/kernels_r1.o $(CSRC)/kernels_sq.o $(CSRC)/kernels_r3w.o $(CSRC)/kernels_r3tw.o $(CSRC)/kernels_bluew.o $(CSRC)/kernels_slab.o $(CSRC)/kernels_tr.o $(CSRC)/kernels_img.o $(CSRC)/kernels_imgl.o $(CSRC)/kernels_imgw.o $(CSRC)/kernels_imgr.o $(CSRC)/kernels_imglr.o $(CSRC)/kernels_vol.o $(CSRC)/kernels_volr.o

all: $(LIBDIR)/libfftw3_amd.so

$(CSRC)/%.o: $(CSRC)/%.c $(CSRC)/fa_plan.h $(CSRC)/fa_hip.h include/fftw3.h include/fftw3_amd.h
	$(CC) $(CFLAGS) -c $< -o $@
# the measured cost tables (tools/perf/fit_split_costs.py writes them) are included by split.c alone
$(CSRC)/split.o: $(CSRC)/split_costs.inc $(CSRC)/split_align.inc $(CSRC)/split2_costs.inc $(CSRC)/split2_align.inc

# every HIP unit depends on exactly the headers it includes (a full rebuild of the two menu units takes minutes)
HIPCOMMON := $(CSRC)/common.hpp $(CSRC)/launch.hpp $(CSRC)/butterflies.h $(CSRC)/fa_hip.h include/fftw3_amd.h $(CSRC)/pass1024.hpp
$(CSRC)/kernels.o: $(CSRC)/kernels.hip $(HIPCOMMON)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_elem.o: $(CSRC)/kernels_elem.hip $(CSRC)/common.hpp $(CSRC)/launch.hpp $(CSRC)/butterflies.h $(CSRC)/fa_hip.h include/fftw3_amd.h $(CSRC)/r2r_epi.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/fa_hip.o: $(CSRC)/fa_hip.hip $(CSRC)/common.hpp $(CSRC)/butterflies.h $(CSRC)/fa_hip.h include/fftw3_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_rr.o: $(CSRC)/kernels_rr.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3w.hpp $(CSRC)/rr_dispatch.hpp $(CSRC)/rr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_rr1.o: $(CSRC)/kernels_rr1.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/rr_dispatch.hpp $(CSRC)/rr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_rr2.o: $(CSRC)/kernels_rr2.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/rr_dispatch.hpp $(CSRC)/rr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_r3.o: $(CSRC)/kernels_r3.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/r2crows.hpp $(CSRC)/r2r_epi.hpp $(CSRC)/r3_menu.inc $(CSRC)/r3t_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_r3r.o: $(CSRC)/kernels_r3r.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/r3r_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_r2cm.o: $(CSRC)/kernels_r2cm.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/r2crows.hpp $(CSRC)/r2r_epi.hpp $(CSRC)/r2cr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_bluew.o: $(CSRC)/kernels_bluew.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/pass3b.hpp $(CSRC)/bluew_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_blue.o: $(CSRC)/kernels_blue.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/pass3b.hpp $(CSRC)/blue_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/kernels_r1.o: $(CSRC)/kernels_r1.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass1r.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_sq.o: $(CSRC)/kernels_sq.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3q.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_r3w.o: $(CSRC)/kernels_r3w.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/r3w_menu.inc $(CSRC)/r3rw_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_r3tw.o: $(CSRC)/kernels_r3tw.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass3s.hpp $(CSRC)/pass3g.hpp $(CSRC)/r3tw_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_slab.o: $(CSRC)/kernels_slab.hip $(CSRC)/common.hpp $(CSRC)/butterflies.h $(CSRC)/fa_hip.h include/fftw3_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_tr.o: $(CSRC)/kernels_tr.hip $(CSRC)/transpose.hpp $(HIPCOMMON)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_img.o: $(CSRC)/kernels_img.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/img2d_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_imgl.o: $(CSRC)/kernels_imgl.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass2dl.hpp $(CSRC)/img2dl_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_imgw.o: $(CSRC)/kernels_imgw.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass2dl.hpp $(CSRC)/pass2dw.hpp $(CSRC)/img2dw_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_imgr.o: $(CSRC)/kernels_imgr.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass2dr.hpp $(CSRC)/img2dr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_imglr.o: $(CSRC)/kernels_imglr.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass2dl.hpp $(CSRC)/pass2dlr.hpp $(CSRC)/img2dlr_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_vol.o: $(CSRC)/kernels_vol.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass3d.hpp $(CSRC)/vol3d_menu.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/kernels_volr.o: $(CSRC)/kernels_volr.hip $(HIPCOMMON) $(CSRC)/passrr.hpp $(CSRC)/pass2d.hpp $(CSRC)/pass2dr.hpp $(CSRC)/pass3dr.hpp $(CSRC)/vol3dr_menu.inc $(CSRC)/vol3dr_pad.inc
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libfftw3_amd.so: $(OBJS)
	mkdir -p $(LIBDIR)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -lm -lpthread -ldl
	ln -sf libfftw3_amd.so $(LIBDIR)/libfftw3.so.3
	ln -sf libfftw3_amd.so $(LIBDIR)/libfftw3.so

oracle:
	$(MAKE) -C oracle

# host-only sanitizer check of the two-trip c2r planner path: the C sources under ASan + UBSan, the HIP units (host-side
# tables only) from the ordinary library.  Planning needs no device.
SANSRC := $(CSRC)/api.c $(CSRC)/planner.c $(CSRC)/split.c $(CSRC)/exec.c $(CSRC)/sharded.c $(CSRC)/slab.c $(CSRC)/slab1d.c $(CSRC)/hostmath.c
san-c2r: $(LIBDIR)/libfftw3_amd.so
	mkdir -p build
	$(CC) -O1 -g -std=gnu99 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -I$(CSRC) tools/san/plan_c2r_decimated.c $(SANSRC) -o build/plan_c2r_decimated_san -L$(LIBDIR) -lfftw3_amd -Wl,-rpath,$(abspath $(LIBDIR)) -lm -lpthread -ldl
	./build/plan_c2r_decimated_san

# the executor on a CPU against a recording fake of the runtime calls (tools/trace/exec_trace.c): every case under
# ASan + UBSan, each in its own process
san-exec: $(LIBDIR)/libfftw3_amd.so
	mkdir -p build
	$(CC) -O1 -g -std=gnu99 -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude -I$(CSRC) tools/trace/exec_trace.c $(SANSRC) -o build/exec_trace_san -L$(LIBDIR) -lfftw3_amd -Wl,-rpath,$(abspath $(LIBDIR)) -lm -lpthread -ldl
	set -e; for c in $$(./build/exec_trace_san --list); do ./build/exec_trace_san $$c > /dev/null; done

clean:
	rm -f $(OBJS) $(LIBDIR)/*.so* build/plan_c2r_decimated_san build/exec_trace_san

.PHONY: all oracle clean san-c2r san-exec
