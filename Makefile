# Build of the MI355X (gfx950) SIFT hot path.
#   libsift_hip.so   -- HIP kernels + C ABI (include/sift_hip.h)
#   libsift_cuda.so  -- C++ drop-in surface sift_cuda::Detector / matchBruteForce
#                       (include/sift_cuda/*.hh), g++ only, links libsift_hip.so
#   tools            -- C++ callers mirroring the reference's tool/ examples
# The CPU oracle (test infrastructure) builds separately: make -C oracle.
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
PKG      := another-cuda-sift_amd
SRC      := $(PKG)/csrc
OUT      := $(PKG)/lib
JOBS     ?= 8
ROCM_LIB ?= /opt/rocm/lib

# -ffp-contract=off + correctly rounded f32 div/sqrt: the float operation order
# written in the kernels is the one executed (bit-exact parity with the oracle).
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fhip-fp32-correctly-rounded-divide-sqrt -Iinclude -I$(SRC) -Wall -Wno-unused-result $(EXTRA_HIPFLAGS) \
            $(if $(strip $(EXTRA_HIPFLAGS)),-DSIFT_AB_FLAGS='"$(strip $(EXTRA_HIPFLAGS))"')
CXXFLAGS := -O2 -std=c++17 -fPIC -Iinclude -Wall -Wextra

HIP_SRCS := $(SRC)/detector.hip $(SRC)/lanes.hip $(SRC)/datagen.hip $(SRC)/matcher_api.hip $(SRC)/keypoints.hip $(SRC)/descriptor.hip \
            $(SRC)/upsample.hip $(SRC)/blur.hip $(SRC)/blur_tail.hip $(SRC)/extrema.hip \
            $(SRC)/match.hip $(SRC)/match_select.hip $(SRC)/match_knn.hip \
            $(SRC)/multi.hip $(SRC)/verify.hip $(SRC)/essential.hip $(SRC)/refit.hip $(SRC)/pose.hip $(SRC)/pose_homography.hip $(SRC)/verify_api.hip $(SRC)/rootsift.hip
HIP_OBJS := $(patsubst $(SRC)/%.hip,$(OUT)/obj/%.o,$(HIP_SRCS)) $(OUT)/obj/synth_frame.o

all: $(OUT)/libsift_hip.so $(OUT)/libsift_cuda.so tools

# Each object's headers come from the dependency file the compiler writes beside it (-MMD -MP), so a unit is rebuilt
# when a header it includes changes and not otherwise.
$(OUT)/obj/%.o: $(SRC)/%.hip include/sift_hip.h
	@mkdir -p $(OUT)/obj
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

-include $(HIP_OBJS:.o=.d)

$(OUT)/obj/synth_frame.o: $(SRC)/synth_frame.cpp include/sift_hip.h
	@mkdir -p $(OUT)/obj
	$(CXX) $(CXXFLAGS) -c $< -o $@

$(OUT)/libsift_hip.so: $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIP_OBJS) -ldl -L$(ROCM_LIB) -lrocprofiler-sdk-roctx \
	    -Wl,-rpath,$(ROCM_LIB) -Wl,-soname,libsift_hip.so

CXX_SRCS := $(SRC)/detector_cxx.cpp $(SRC)/multi_cxx.cpp $(SRC)/verify_cxx.cpp $(SRC)/match_batched_cxx.cpp

$(OUT)/libsift_cuda.so: $(CXX_SRCS) $(wildcard include/sift_cuda/*.hh) include/sift_hip.h $(OUT)/libsift_hip.so
	$(CXX) $(CXXFLAGS) -pthread -shared -o $@ $(CXX_SRCS) -L$(OUT) -lsift_hip -Wl,-rpath,'$$ORIGIN'

tools: $(OUT)/detection_example $(OUT)/extract_and_match_example $(OUT)/multi_gpu_example $(OUT)/host_pipeline_bench

$(OUT)/%: tools/%.cpp $(OUT)/libsift_cuda.so
	$(CXX) $(CXXFLAGS) -pthread -o $@ $< -L$(OUT) -lsift_cuda -lsift_hip -Wl,-rpath,'$$ORIGIN'

# The host pipeline microbenchmark also calls the HIP runtime (pinned frames, a copy stream).
$(OUT)/host_pipeline_bench: tools/host_pipeline_bench.cpp $(OUT)/libsift_cuda.so
	$(CXX) $(CXXFLAGS) -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< -L$(OUT) -lsift_cuda -lsift_hip \
	    -L$(ROCM_LIB) -lamdhip64 -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(ROCM_LIB)

oracle:
	$(MAKE) -C oracle

# Sanitizer builds of the host code (HIP kernels are not
# instrumented, and GPU ASan is not available on the GPU pool): the CPU oracle,
# and the C++ drop-in surface (detector_cxx.cpp, multi_cxx.cpp) linked into the
# CPU orchestration test tests/cpp/test_multi.cpp, all with
# -fsanitize=address,undefined.  tests/test_asan.py runs both.
ASAN_DIR  := $(OUT)/asan
SANFLAGS  := -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined

asan: $(ASAN_DIR)/test_multi $(ASAN_DIR)/test_verify_args $(ASAN_DIR)/test_homography_args $(ASAN_DIR)/test_affine_args $(ASAN_DIR)/test_essential_args $(ASAN_DIR)/test_verify_batched_args $(ASAN_DIR)/test_refit_args $(ASAN_DIR)/test_pose_args $(ASAN_DIR)/test_pose_homography_args $(ASAN_DIR)/test_match_knn_args $(ASAN_DIR)/test_match_knn_gated_args
	$(MAKE) -C oracle asan

$(ASAN_DIR)/test_multi: tests/cpp/test_multi.cpp $(CXX_SRCS) $(wildcard include/sift_cuda/*.hh) include/sift_hip.h $(OUT)/libsift_hip.so
	@mkdir -p $(ASAN_DIR)
	$(CXX) -std=c++17 -Iinclude -Wall -Wextra $(SANFLAGS) -pthread -o $@ tests/cpp/test_multi.cpp $(CXX_SRCS) \
	    -L$(OUT) -lsift_hip -Wl,-rpath,'$$ORIGIN/..'

# Argument validation of the verifier's C++ surface (verify_cxx.cpp), CPU only: test_verify_args (run by
# tests/test_verify_asan.py), test_homography_args for the homography calls and the projection, test_verify_batched_args
# for the batched calls, test_refit_args for the refit calls, test_pose_args for the pose calls,
# test_pose_homography_args for the plane pose calls, test_affine_args for the affine and similarity calls and
# test_essential_args for the essential calls, each with its tests/test_*_asan.py.
$(ASAN_DIR)/test_%_args: tests/cpp/test_%_args.cpp $(SRC)/verify_cxx.cpp $(wildcard include/sift_cuda/*.hh) include/sift_hip.h $(OUT)/libsift_hip.so
	@mkdir -p $(ASAN_DIR)
	$(CXX) -std=c++17 -Iinclude -Wall -Wextra $(SANFLAGS) -pthread -o $@ $< $(SRC)/verify_cxx.cpp \
	    -L$(OUT) -lsift_hip -Wl,-rpath,'$$ORIGIN/..'

# Argument validation of the k-NN C++ surface (match_batched_cxx.cpp) and of the k-NN ABI calls that need no matcher,
# CPU only (run by tests/test_match_knn_asan.py; the gated forms: test_match_knn_gated_args, run by
# tests/test_match_knn_gated_asan.py).  An explicit rule: the pattern above links verify_cxx.cpp.
$(ASAN_DIR)/test_match_knn_args $(ASAN_DIR)/test_match_knn_gated_args: $(ASAN_DIR)/%: tests/cpp/%.cpp $(SRC)/match_batched_cxx.cpp $(wildcard include/sift_cuda/*.hh) include/sift_hip.h $(OUT)/libsift_hip.so
	@mkdir -p $(ASAN_DIR)
	$(CXX) -std=c++17 -Iinclude -Wall -Wextra $(SANFLAGS) -pthread -o $@ $< $(SRC)/match_batched_cxx.cpp \
	    -L$(OUT) -lsift_hip -Wl,-rpath,'$$ORIGIN/..'

clean:
	rm -rf $(OUT)

.PHONY: all tools oracle asan clean

# Isolated kernel timing (tools/kernel_bench.hip), not part of `all`.
KBENCH_OBJS := $(OUT)/obj/blur.o $(OUT)/obj/extrema.o $(OUT)/obj/synth_frame.o
tools/kernel_bench: tools/kernel_bench.hip $(KBENCH_OBJS)
	$(HIPCC) $(HIPFLAGS) -c $< -o tools/kernel_bench.o
	$(HIPCC) --offload-arch=$(ARCH) -o $@ tools/kernel_bench.o $(KBENCH_OBJS)
