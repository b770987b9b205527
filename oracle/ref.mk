# REFERENCE build recipe — test infrastructure only (make -C oracle -f ref.mk; __graft_entry__.build() runs it wherever
# the reference's sources are present).  Everything lands in oracle/_ref/, which git ignores; the built files travel with
# the working tree to machines that do not hold the reference.  Nothing of the reference is copied: its sources are
# piped to the compiler from host/, so that their quoted includes resolve against the mirror and nowhere else.
#
# _ref/ref_<pass>.o (+ .d): every hot-path pass source of the reference compiled UNCHANGED against the host mirror;
#   the dependency list records every header it read (tests/test_reference_sources_compile.py).
# _ref/libvkr_host_refpasses.so: the SAME mirror (gpu/, rendergraph/, frame.cpp ...) but with the pass classes
#   DownsamplePass, GTAO, AdvancedSSR, TAA and DeferedShadingPass taken from the reference's own
#   {downsample_pass,gtao,advanced_ssr,taa,defered_shading}.cpp instead of passes.cpp's implementations
#   (-DVKR_REFERENCE_PASSES leaves those out).  tests/test_reference_passes_gpu.py runs a frame through it on the GPU and
#   compares with the oracle: the reference's host code driving the HIP kernels through the mirror, which is what
#   "each pass drops into the frame loop unchanged" means.  Not an oracle, not part of the product.
#   rand() is wrapped (host/refpasses_rand.cpp) so that GTAO's per-frame angle jitter (gtao.cpp:111) is exactly 0.
CXX      ?= g++
ROCM     ?= /opt/rocm
REF      ?= /root/reference/src
HOST     := $(abspath ../vk-renderer_amd/host)
CSRC     := $(abspath ../vk-renderer_amd/csrc)
OUT      := $(abspath _ref)
CXXFLAGS ?= -O2 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I.
MIRROR   := gpu/gpu.cpp rendergraph/rendergraph.cpp passes.cpp image_readback.cpp gpu_transfer.cpp frame.cpp refpasses_rand.cpp
PASSES   := taa downsample_pass ssr screen_trace gtao advanced_ssr defered_shading
LINKED   := downsample_pass gtao advanced_ssr taa defered_shading
HDRS     := $(wildcard $(HOST)/*.hpp $(HOST)/gpu/*.hpp $(HOST)/rendergraph/*.hpp) $(abspath ../include/vkr_postfx.h)

all: $(PASSES:%=$(OUT)/ref_%.o) $(OUT)/libvkr_host_refpasses.so

$(OUT)/mirror/%.o: $(HOST)/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	cd $(HOST) && $(CXX) $(CXXFLAGS) -Wno-unused-function -DVKR_REFERENCE_PASSES -c $*.cpp -o $@

$(OUT)/ref_%.o: $(REF)/%.cpp $(HDRS)
	@mkdir -p $(OUT)
	cd $(HOST) && $(CXX) $(CXXFLAGS) -Wno-unused-variable -Wno-sign-compare -Wno-missing-field-initializers -MD -MF $(OUT)/ref_$*.d \
	    -x c++ -c - -o $@ < $<

$(OUT)/libvkr_host_refpasses.so: $(MIRROR:%.cpp=$(OUT)/mirror/%.o) $(LINKED:%=$(OUT)/ref_%.o) $(CSRC)/libvkr_postfx.so
	$(CXX) -shared -o $@ $(filter %.o,$^) -Wl,--wrap=rand -L$(CSRC) -lvkr_postfx -L$(ROCM)/lib -lamdhip64 \
	    -Wl,-rpath,'$$ORIGIN/../../vk-renderer_amd/csrc' -Wl,-rpath,$(ROCM)/lib

clean:
	rm -rf _ref

.PHONY: all clean
