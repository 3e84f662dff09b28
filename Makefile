# Build of the MI355X (gfx950) hot-path library and the CPU oracle.
#   make            -> sp-slam_amd/libspslam_gpu.so  and  oracle/liboracle.so
# hipcc cross-compiles for gfx950 in the build container (no GPU needed).
# One object per source (parallel with make -j), linked into one shared library.
HIPCC ?= /opt/rocm/bin/hipcc
OFFLOAD_ARCH ?= gfx950
HIPFLAGS ?= --offload-arch=$(OFFLOAD_ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -Wall -Wno-unused-result

PKG := sp-slam_amd
CSRC := $(PKG)/csrc
OBJDIR := build/obj
KERNELS := orb_kernels pose_kernels plane_kernels plane_segment supposed_kernels frame_kernels lba_kernels lba_g2o lba_g2o_wide \
           assoc_kernels match_kernels map_point_kernels track_kernels local_map_kernels grab_kernels bow_kernels triangulate_kernels covis_kernels \
           place_kernels sim3_kernels sim3_opt_kernels pnp_kernels
HOST_SRCS := capi_core capi_orb_frame capi_planes capi_solve capi_match capi_track capi_bow capi_local_mapping capi_place capi_loop_closing capi_reloc spslam_step
GPU_HDRS := $(wildcard $(CSRC)/*.h) include/spslam_gpu.h include/spslam_brief_pattern.inc

all: $(PKG)/libspslam_gpu.so oracle/liboracle.so tests/shim/libreference_shim.so

# One library: $(call lib_rules,<object dir>,<extra compile flags>,<library>,<command after the link>).
# The wide LocalBundleAdjustment instance is lba_g2o.hip compiled again.
define lib_rules
$(1)/%.o: $$(CSRC)/%.hip $$(GPU_HDRS)
	@mkdir -p $(1)
	$$(HIPCC) $$(HIPFLAGS) $(2) -c -o $$@ $$<

$(1)/%.o: $$(CSRC)/%.cpp $$(GPU_HDRS)
	@mkdir -p $(1)
	$$(HIPCC) $$(HIPFLAGS) $(2) -c -x hip -o $$@ $$<

$(1)/lba_g2o_wide.o: $$(CSRC)/lba_g2o.hip

$(3): $$(addprefix $(1)/,$$(addsuffix .o,$$(KERNELS) $$(HOST_SRCS)))
	$$(HIPCC) --offload-arch=$$(OFFLOAD_ARCH) -shared -fPIC -o $$@ $$^
	$(4)
endef

$(eval $(call lib_rules,$(OBJDIR),,$(PKG)/libspslam_gpu.so,@python3 tools/build_info.py $$@ > $(PKG)/build_info.json))

# Diagnostic build: PoseOptimization phase timers (tools/pose_phases.py loads it via SPSLAM_GPU_LIB).
PROFDIR := build/prof
prof: $(PKG)/libspslam_gpu_prof.so
$(eval $(call lib_rules,$(PROFDIR),-DSPSLAM_POSE_PROF,$(PKG)/libspslam_gpu_prof.so))

# Measurement variants: make variant VARIANT=<name> VAR_FLAGS="-D..." -> sp-slam_amd/libspslam_gpu_<name>.so
# (loaded via SPSLAM_GPU_LIB).
VARIANT ?= var
VAR_FLAGS ?=
VARDIR := build/var_$(VARIANT)
variant: $(PKG)/libspslam_gpu_$(VARIANT).so
$(eval $(call lib_rules,$(VARDIR),$(VAR_FLAGS),$(PKG)/libspslam_gpu_$(VARIANT).so))

# Reference-side shim (test infrastructure, INTEGRATION.md 1-7 compiled): plain g++ against the C ABI.
tests/shim/libreference_shim.so: tests/shim/reference_shim.cpp tests/shim/cv_lite.h include/spslam_gpu.h $(PKG)/libspslam_gpu.so
	g++ -O2 -std=c++17 -fPIC -shared -Wall -Wextra -o $@ tests/shim/reference_shim.cpp \
	    -L$(PKG) -l:libspslam_gpu.so -Wl,-rpath,'$$ORIGIN/../../$(PKG)'

oracle/liboracle.so:
	$(MAKE) -C oracle liboracle.so

clean:
	rm -rf $(PKG)/libspslam_gpu*.so build/var_* tests/shim/libreference_shim.so $(OBJDIR) $(PROFDIR)
	$(MAKE) -C oracle clean

.PHONY: all clean prof variant oracle/liboracle.so
