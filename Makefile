# Build of the MI355X render path (no cmake).  `make` builds:
#   miniraytracer_amd/libmrt.so   C-ABI (include/mrt.h): host scene builder + HIP kernels for gfx950
#   bin/mrt                       command-line driver with the reference's flags
#   oracle/liboracle.so           C restatement used by tests / bench cpu_baseline (test infra only)
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950
JOBS    ?= 8
# Numerics contract: no FMA contraction, IEEE division/sqrt, denormals kept.
# No SLP vectorisation: it packed unrelated float ops into v_pk_* pairs whose constant halves
# were kept live in VGPR pairs and spilled (C2 +8%, bunny +7% without it; results identical).
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function
# per-lane traversal stacks stay in scratch instead of being promoted into VGPR vectors; uniform
# regions keep plain scalar branches instead of exec-mask structurisation (C2 +1.7%)
HIPDEV   = -mllvm -disable-promote-alloca-to-vector -mllvm -structurizecfg-skip-uniform-regions
CSRC     = miniraytracer_amd/csrc
OBJDIR   = build/obj

LIB_OBJS = $(OBJDIR)/mrt_render.o $(OBJDIR)/mrt_fold.o $(OBJDIR)/mrt_upload.o $(OBJDIR)/mrt_query.o $(OBJDIR)/mrt_kernels_exact.o $(OBJDIR)/mrt_kernels_fast.o $(OBJDIR)/mrt_kernels_fastz.o \
           $(OBJDIR)/mrt_kernels_pex.o $(OBJDIR)/mrt_aux.o $(OBJDIR)/mrt_cast.o $(OBJDIR)/mrt_probe.o $(OBJDIR)/mrt_probegen.o $(OBJDIR)/mrt_denoise.o $(OBJDIR)/mrt_adaptive.o \
           $(OBJDIR)/mrt_temporal.o $(OBJDIR)/mrt_cpu.o $(OBJDIR)/mrt_tables.o $(OBJDIR)/scene_builder.o $(OBJDIR)/mrt_common.o $(OBJDIR)/mrt_comm.o \
           $(OBJDIR)/mrt_mathfn_api.o
# the path kernels twice: exact contract (no contraction, IEEE division) and tolerance contract
# (FMA contraction, reciprocal division, hardware rcp/sqrt/rsq, f32 transcendentals)
# (-fno-hip-fp32-correctly-rounded-divide-sqrt: f32 division by v_rcp_f32 + multiply instead of
# the 10-instruction IEEE sequence; -freciprocal-math alone does not lower it)
FASTFLAGS = -DMRT_FAST=1 -ffp-contract=fast -freciprocal-math -fno-hip-fp32-correctly-rounded-divide-sqrt
HDRS     = include/mrt.h include/mrt_scene.h include/mrt_mathfn.h $(wildcard $(CSRC)/*.h) Makefile

all: miniraytracer_amd/libmrt.so bin/mrt oracle/liboracle.so

$(OBJDIR)/mrt_kernels_exact.o: $(CSRC)/mrt_kernels.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -DMRT_FAST=0 -c $< -o $@

$(OBJDIR)/mrt_kernels_fast.o: $(CSRC)/mrt_kernels.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) $(FASTFLAGS) -c $< -o $@

# the tolerance contract again with f32 denormals flushed, for the variants mrt_launch.h's
# kFtzVariant selects (the others are not instantiated in it)
FTZFLAGS = -fgpu-flush-denormals-to-zero -DMRT_TABLE_FTZ=1
$(OBJDIR)/mrt_kernels_fastz.o: $(CSRC)/mrt_kernels.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) $(FASTFLAGS) $(FTZFLAGS) -c $< -o $@

# the tolerance contract's path-exact variants (mrt_launch.h kPathExact): the exact build's
# arithmetic with the forward fold; its bvh_node kernels in two 12-wave groups per CU (6 waves per
# SIMD, 80 VGPRs): book2 4.83 against 4.19 Grays/s in one 16-wave group, 2.90 in two 10-wave groups
# (profiles/r04_ab.txt)
PEXFLAGS = -DMRT_FAST=0 -DMRT_FWD_FOLD=1 -DMRT_TABLE_PEX=1 -DMRT_TREE_WG=768 -DMRT_WPE_WIDE=6
$(OBJDIR)/mrt_kernels_pex.o: $(CSRC)/mrt_kernels.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) $(PEXFLAGS) -c $< -o $@

# the CPU backend: the same hot-path headers compiled for the host only (exact contract).
# -mfma: the reference's fused multiply-adds (mrt_device.h ref_fma) as one instruction instead of a
# libm fmaf call (same result; the reference's own build is x86 FMA too, -march=native)
HOSTFMA ?= -mfma
$(OBJDIR)/mrt_cpu.o: $(CSRC)/mrt_cpu.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HOSTFMA) --offload-host-only -c $< -o $@

# the scene compiler (view -> SceneTables, both backends): host code only, and no -mfma -- its float
# arithmetic (dielectric quotients, box.h recognition) is built as it was inside mrt_render.hip
$(OBJDIR)/mrt_tables.o: $(CSRC)/mrt_tables.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) --offload-host-only -c $< -o $@

# the first-hit feature buffers (mrt_aux_kernel<F>): the exact contract's hit code in a translation
# unit of its own, so the path-kernel objects above do not change with it
$(OBJDIR)/mrt_aux.o: $(CSRC)/mrt_aux.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -DMRT_FAST=0 -c $< -o $@

# the ray queries (mrt_cast_kernel<F>): the same, in a translation unit of its own
$(OBJDIR)/mrt_cast.o: $(CSRC)/mrt_cast.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -DMRT_FAST=0 -c $< -o $@

# the radiance queries (mrt_probe_kernel<F>) and mrt_radiance_fold, host and device from
# include/mrt_radiance.h: the same, in a translation unit of its own
$(OBJDIR)/mrt_probe.o: $(CSRC)/mrt_probe.hip include/mrt_radiance.h $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -DMRT_FAST=0 -c $< -o $@

# the probe generators (mrt_gen_*_kernel) and their host forms from mrt_probegen.h: the exact contract
# on both sides (no contraction; the host's explicit fma() as one instruction, as in the CPU backend),
# in a translation unit of its own
$(OBJDIR)/mrt_probegen.o: $(CSRC)/mrt_probegen.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -DMRT_FAST=0 $(if $(HOSTFMA),-Xarch_host $(HOSTFMA)) -c $< -o $@

# the a-trous filter, host and device from include/mrt_denoise.h: no contraction on either side
# (HIPFLAGS), the host's explicit fma() as one instruction (as in the CPU backend)
$(OBJDIR)/mrt_denoise.o: $(CSRC)/mrt_denoise.hip include/mrt_denoise.h $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(if $(HOSTFMA),-Xarch_host $(HOSTFMA)) -c $< -o $@

# the sample moments and the adaptive render's merge, host and device from include/mrt_adaptive.h:
# no contraction on either side (HIPFLAGS); a translation unit of its own, like the two above
$(OBJDIR)/mrt_adaptive.o: $(CSRC)/mrt_adaptive.hip include/mrt_adaptive.h $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# temporal reprojection, host and device from include/mrt_temporal.h, and the camera-record store:
# no contraction on either side (HIPFLAGS, no fast flags); a translation unit of its own
$(OBJDIR)/mrt_temporal.o: $(CSRC)/mrt_temporal.hip include/mrt_temporal.h include/mrt_denoise.h $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the contract's transcendentals as array calls (mrt_mathfn[_d][_device]), host and device from
# include/mrt_mathfn.h under the exact contract's flags (the host's explicit fma() as one instruction,
# as in the CPU backend): a translation unit of its own
$(OBJDIR)/mrt_mathfn_api.o: $(CSRC)/mrt_mathfn_api.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) $(if $(HOSTFMA),-Xarch_host $(HOSTFMA)) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPDEV) -c $< -o $@

miniraytracer_amd/libmrt.so: $(LIB_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(LIB_OBJS) -ldl -o $@

bin/mrt: $(CSRC)/mrt_cli.cpp miniraytracer_amd/libmrt.so include/mrt.h
	@mkdir -p bin
	$(HIPCC) -O2 -std=c++17 -ffp-contract=off $(CSRC)/mrt_cli.cpp -Lminiraytracer_amd -lmrt -Wl,-rpath,'$$ORIGIN/../miniraytracer_amd' -o $@

oracle/liboracle.so: oracle/mrt_oracle.c oracle/mrt_oracle.h include/mrt_scene.h include/mrt_mathfn.h
	$(CC) -O2 -std=c11 -fPIC -shared -ffp-contract=off -fno-fast-math $(HOSTFMA) -Wall -o $@ oracle/mrt_oracle.c -lm -lpthread

# The scene compiler stand-alone on the CPU under AddressSanitizer + UBSan (host code only, nothing
# preloaded; not part of `all`): tools/tables_check.cpp builds the tables of scenes 0-9 under every
# test hook, tools/tables_digest.py --compare checks its digests against tests/golden/tables_parent.json
TABLES_CHECK_SRC = tools/tables_check.cpp $(CSRC)/mrt_tables.hip $(CSRC)/scene_builder.cpp $(CSRC)/mrt_common.cpp
SANFLAGS = -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -g
build/tables_check: $(TABLES_CHECK_SRC) $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) --offload-host-only -x hip $(SANFLAGS) $(TABLES_CHECK_SRC) -ldl -o $@

tables-check: build/tables_check
	python3 tools/pack_assets.py --unpack
	MRT_ASSET_DIR=assets build/tables_check > build/tables_check.out
	python3 tools/tables_digest.py --compare < build/tables_check.out

# The host forms of mrt_make_camera and mrt_reproject stand-alone under the same sanitizers (host
# code only, nothing preloaded; not part of `all`): tools/temporal_check.cpp
TEMPORAL_CHECK_SRC = tools/temporal_check.cpp $(CSRC)/mrt_temporal.hip $(CSRC)/scene_builder.cpp $(CSRC)/mrt_common.cpp
build/temporal_check: $(TEMPORAL_CHECK_SRC) include/mrt_temporal.h include/mrt_denoise.h $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) --offload-host-only -x hip -DMRT_TEMPORAL_HOST_ONLY=1 $(SANFLAGS) $(TEMPORAL_CHECK_SRC) -ldl -o $@

temporal-check: build/temporal_check
	build/temporal_check

# The Cornell walk kernels' 32-bit pool arithmetic (mrt_launch.h pool_claim32 ...) against the 64-bit
# expressions it replaces, stand-alone under the same sanitizers (host code only, nothing preloaded;
# not part of `all`): tools/claim_check.cpp
build/claim_check: tools/claim_check.cpp $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) --offload-host-only -x hip $(SANFLAGS) tools/claim_check.cpp -o $@

claim-check: build/claim_check
	build/claim_check

# The radiance queries' host side -- the CPU backend's trace loop and level rows, the probe helpers,
# mrt_radiance_fold -- stand-alone under the same sanitizers (host code only, nothing preloaded; not
# part of `all`): tools/probe_check.cpp.  Without UBSan's alignment check: mrt_cpu_scene_create copies the
# view's triangle arrays as float4 from the blob's 8-byte-aligned storage, which that check stops at
# before any of the code under test runs.
PROBE_CHECK_SRC = tools/probe_check.cpp $(CSRC)/mrt_cpu.hip $(CSRC)/mrt_probe.hip $(CSRC)/mrt_tables.hip \
                  $(CSRC)/scene_builder.cpp $(CSRC)/mrt_common.cpp
build/probe_check: $(PROBE_CHECK_SRC) include/mrt_radiance.h include/mrt_adaptive.h $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(HOSTFMA) --offload-host-only -x hip -DMRT_FAST=0 -DMRT_PROBE_HOST_ONLY=1 $(SANFLAGS) -Xarch_host -fno-sanitize=alignment $(PROBE_CHECK_SRC) -ldl -o $@

probe-check: build/probe_check
	build/probe_check

# The probe generators' host forms stand-alone under the same sanitizers (host code only, nothing
# preloaded; not part of `all`): tools/probegen_check.cpp runs the range forms at ragged ranges against
# the per-record functions, and the surface probes on hand-made hits (misses, non-finite normals)
PROBEGEN_CHECK_SRC = tools/probegen_check.cpp $(CSRC)/mrt_probegen.hip $(CSRC)/mrt_cpu.hip $(CSRC)/mrt_probe.hip $(CSRC)/mrt_tables.hip \
                     $(CSRC)/scene_builder.cpp $(CSRC)/mrt_common.cpp
build/probegen_check: $(PROBEGEN_CHECK_SRC) include/mrt_radiance.h include/mrt_adaptive.h $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(HOSTFMA) --offload-host-only -x hip -DMRT_FAST=0 -DMRT_PROBE_HOST_ONLY=1 -DMRT_PROBEGEN_HOST_ONLY=1 $(SANFLAGS) -Xarch_host -fno-sanitize=alignment $(PROBEGEN_CHECK_SRC) -ldl -o $@

probegen-check: build/probegen_check
	build/probegen_check

clean:
	rm -rf build miniraytracer_amd/libmrt.so bin oracle/liboracle.so

.PHONY: all clean tables-check temporal-check claim-check probe-check probegen-check
