# Builds librvcx.so (HIP, gfx950 only) in-tree.  `python -c "import __graft_entry__ as g; g.build()"`
# drives this; the .so travels to the GPU box with the repo snapshot.
HIPCC ?= hipcc
ARCH  ?= gfx950
CSRC  := polgen-rvc_amd/csrc
OUT   := polgen-rvc_amd/librvcx.so
SRCS  := $(wildcard $(CSRC)/*.hip)
OBJS  := $(patsubst $(CSRC)/%.hip,build/%.o,$(SRCS))
HDRS  := $(wildcard $(CSRC)/*.h) include/rvcx.h
FLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-pass-failed -Wno-unused-result $(EXTRA)

all: $(OUT)

build/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(FLAGS) -c $< -o $@

$(OUT): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -o $@

# ---- host-side sanitizer build (CPU container only; never on the GPU box) ------------------------------------------
# The HOST pass of every .hip file under AddressSanitizer + UBSan, linked against tools/hipstub (HIP runtime on host memory,
# kernel launches are no-ops): build/asan/librvcx_asan.so.  tools/host_asan.sh builds it and runs tools/host_asan_driver.py.
CLANGXX ?= /opt/rocm/lib/llvm/bin/clang++
ASAN_FLAGS := --cuda-host-only -O1 -g -std=c++17 -fPIC -Wno-pass-failed -Wno-unused-result -fsanitize=address,undefined \
              -fno-sanitize-recover=undefined -fno-omit-frame-pointer
ASAN_OBJS := $(patsubst $(CSRC)/%.hip,build/asan/%.o,$(SRCS))

build/asan/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build/asan
	$(HIPCC) $(ASAN_FLAGS) -c $< -o $@

build/asan/hipstub.o: tools/hipstub/hipstub.cpp
	@mkdir -p build/asan
	$(HIPCC) $(ASAN_FLAGS) -x hip -c $< -o $@

# one dummy definition per translation unit's __hip_fatbin_<hash> (the device code objects a host-only pass does not have)
build/asan/fatbins.c: $(ASAN_OBJS)
	nm $(ASAN_OBJS) | awk '/ U __hip_fatbin_/ {print "char " $$2 "[64] = {0};"}' | sort -u > $@

build/asan/librvcx_asan.so: $(ASAN_OBJS) build/asan/hipstub.o build/asan/fatbins.c
	$(CLANGXX) -shared -fPIC -fsanitize=address,undefined -shared-libasan $(ASAN_OBJS) build/asan/hipstub.o build/asan/fatbins.c -o $@

host-asan: build/asan/librvcx_asan.so

# a stand-alone program (its own main, no Python, nothing preloaded) over the host twins of stages 17 and 18, linked against the
# library above and run on the spot
build/asan/formant_main: tools/formant_asan_main.cpp build/asan/librvcx_asan.so
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
	    -shared-libasan -Iinclude $< -Lbuild/asan -lrvcx_asan -Wl,-rpath,'$$ORIGIN' \
	    -Wl,-rpath,$(dir $(shell $(CLANGXX) -print-file-name=libclang_rt.asan-x86_64.so)) -o $@

host-asan-formant: build/asan/formant_main
	ASAN_OPTIONS=abort_on_error=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build/asan/formant_main

# the same for the host twin of stage 19 (the live formant shift)
build/asan/formant_live_main: tools/formant_live_asan_main.cpp build/asan/librvcx_asan.so
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
	    -shared-libasan -Iinclude $< -Lbuild/asan -lrvcx_asan -Wl,-rpath,'$$ORIGIN' \
	    -Wl,-rpath,$(dir $(shell $(CLANGXX) -print-file-name=libclang_rt.asan-x86_64.so)) -o $@

host-asan-formant-live: build/asan/formant_live_main
	ASAN_OPTIONS=abort_on_error=1:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 build/asan/formant_live_main

# ---- the same host pass under ThreadSanitizer (tools/host_tsan.sh runs tools/host_tickets_driver.py on it): conversion
# tickets are the first code of the library where the state of two requests can meet
TSAN_FLAGS := --cuda-host-only -O1 -g -std=c++17 -fPIC -Wno-pass-failed -Wno-unused-result -fsanitize=thread \
              -fno-omit-frame-pointer
TSAN_OBJS := $(patsubst $(CSRC)/%.hip,build/tsan/%.o,$(SRCS))

build/tsan/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build/tsan
	$(HIPCC) $(TSAN_FLAGS) -c $< -o $@

build/tsan/hipstub.o: tools/hipstub/hipstub.cpp
	@mkdir -p build/tsan
	$(HIPCC) $(TSAN_FLAGS) -x hip -c $< -o $@

build/tsan/fatbins.c: $(TSAN_OBJS)
	nm $(TSAN_OBJS) | awk '/ U __hip_fatbin_/ {print "char " $$2 "[64] = {0};"}' | sort -u > $@

build/tsan/librvcx_tsan.so: $(TSAN_OBJS) build/tsan/hipstub.o build/tsan/fatbins.c
	$(CLANGXX) -shared -fPIC -fsanitize=thread -shared-libsan $(TSAN_OBJS) build/tsan/hipstub.o build/tsan/fatbins.c -o $@

host-tsan: build/tsan/librvcx_tsan.so

clean:
	rm -rf build $(OUT)

.PHONY: all clean host-asan host-asan-formant host-asan-formant-live host-tsan
