# Top-level build: the product library (gfx950 HIP + host runtime) and the
# test-only oracle.  `make` is what __graft_entry__.build() runs.
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
ARCH ?= gfx950
JOBS ?= 8

# -ffp-contract=off: no implicit FMA anywhere (bit parity with the oracle);
# no fast-math: IEEE division/sqrt (HIP's default correctly rounded fp32 div/sqrt).
HIPFLAGS = $(EXTRA_HIPFLAGS) -O3 -std=c++17 --offload-arch=$(ARCH) -mcode-object-version=5 -ffp-contract=off -fno-fast-math -fPIC \
           -Wall -Wno-unused-result -Iinclude -Igaussianrenderer_amd/csrc
HOSTFLAGS = -O2 -std=c++17 -I$(ROCM)/include -ffp-contract=off -fno-fast-math -fPIC -Wall -Iinclude -Igaussianrenderer_amd/csrc

LIB = gaussianrenderer_amd/lib/libgsr.so
OBJDIR = build/obj
SRCDIR = gaussianrenderer_amd/csrc
HDRS = include/gsr.h include/gsr_types.h include/gsr_detmath.h $(SRCDIR)/gsr_internal.h
DEVHDRS = $(SRCDIR)/gsr_device.h $(SRCDIR)/gsr_blend_device.h $(SRCDIR)/gsr_preprocess_device.h \
          $(SRCDIR)/gsr_geom_device.h

all: $(LIB) oracle

# the kernel translation units (gfx950 device code + launch wrappers); a stage that gets a
# file of its own is added here
KOBJS = $(addprefix $(OBJDIR)/,gsr_kernels.o gsr_bucket_sort.o gsr_blend.o gsr_blend_derived.o gsr_scene_ops.o gsr_scene_densify.o gsr_scene_init.o gsr_scene_adam.o gsr_scene_pack.o gsr_image_loss.o gsr_project.o gsr_probes.o)

$(OBJDIR)/%.o: $(SRCDIR)/%.hip $(HDRS) $(DEVHDRS)
	mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OBJDIR)/%.o: $(SRCDIR)/%.cpp $(HDRS) $(SRCDIR)/gsr_host.h $(SRCDIR)/gsr_context.h
	mkdir -p $(OBJDIR)
	$(HIPCC) $(HOSTFLAGS) -x c++ -D__HIP_PLATFORM_AMD__ -c $< -o $@

$(OBJDIR)/gsr_gl.o: include/gsr_gl.h

# the host translation units (gsr_context.h is private to the three that work on a context; the
# rule above rebuilds every host file when it changes, which costs a few seconds)
HOBJS = $(addprefix $(OBJDIR)/,gsr_runtime.o gsr_path.o gsr_inspect.o gsr_compat.o gsr_camera.o gsr_scene.o gsr_scene_save.o gsr_ply.o gsr_gl.o)

$(LIB): $(KOBJS) $(HOBJS)
	mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl -Wl,-soname,libgsr.so

oracle: $(LIB)
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

# host-code ASan + UBSan build of libgsr.so and the oracle (tools/asan.mk; CPU tests only)
asan: $(KOBJS)
	$(MAKE) -f tools/asan.mk -j $(JOBS) KOBJS="$(KOBJS)"

.PHONY: asan
