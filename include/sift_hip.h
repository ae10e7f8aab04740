/*
 * sift_hip.h -- C ABI of the MI355X SIFT hot path (libsift_hip.so).
 *
 * Plain C types only: no HIP, torch or C++ types cross this boundary.  Device
 * memory is owned by the handle; device pointers handed out are valid until the
 * next sift_hip_detect* call on the same handle (the reference's contract for
 * Detector::device_* members, /root/reference/sift_cuda/interface/Detector.hh:54-57).
 * Streams are passed as `void*` (a hipStream_t; NULL = the handle's own stream).
 * Every function returns 0 (SIFT_HIP_OK) or a negative error; the message of the
 * last error on the calling thread is in sift_hip_last_error().
 *
 * Each entry point names the reference interface it replaces.  The C++ surface
 * sift_cuda::Detector / CudaSiftConfig / matchBruteForce in include/sift_cuda/ is
 * a thin wrapper over this ABI.
 */
#ifndef SIFT_HIP_H
#define SIFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT_HIP_OK 0
#define SIFT_HIP_ERR_INVALID (-1)   /* bad argument / size mismatch        */
#define SIFT_HIP_ERR_RUNTIME (-2)   /* HIP runtime error                   */
#define SIFT_HIP_ERR_STATE   (-3)   /* call out of order (e.g. no warmup)  */
#define SIFT_HIP_ERR_NOMEM   (-4)   /* device allocation failed            */

#define SIFT_HIP_ABI_VERSION 1

typedef struct sift_hip_detector* sift_hip_t;
typedef struct sift_hip_matcher* sift_hip_matcher_t;

/* Mirrors CudaSiftConfig (/root/reference/sift_cuda/types/CudaSiftConfig.hh:3-14),
 * field for field including the reference's spellings, plus defaulted extras.
 *
 * Limit: every Gaussian blur of the pyramid has at most 63 taps (radius 31),
 * taps = cvRound(8 s + 1) | 1 as in OpenCV.  The blurs are the initial one, s =
 * sqrt(sigma^2 - 0.25) (sqrt(sigma^2 - 1) with upscale), and per layer i =
 * 1 .. numOctaveLayers + 2, s = sigma 2^((i-1)/L) sqrt(2^(2/L) - 1), L =
 * numOctaveLayers.  sift_hip_create refuses a configuration beyond the limit
 * with SIFT_HIP_ERR_INVALID (OpenCV does not truncate its kernels): e.g. sigma
 * 1.6 needs numOctaveLayers >= 2, and numOctaveLayers 3 allows sigma <= 4.0.
 * A layer blur of one tap (s < 0.0625) is refused in the same way. */
typedef struct {
    int    col_width;           /* image width  (CudaSiftConfig.hh:4)            */
    int    row_width;           /* image height (CudaSiftConfig.hh:5)            */
    int    numFeatures;         /* retainBest count, 0 = keep all (.hh:6)        */
    int    numOctaveLayers;     /* (.hh:7)                                      */
    double contrastThreshould;  /* (.hh:8)                                      */
    double edgeThreshould;      /* (.hh:9)                                      */
    double sigma;               /* (.hh:10)                                     */
    int    upscale;             /* 1 = double the base image = OpenCV default   */
                                /* firstOctave -1 (.hh:12, broken there)        */
    int    numOctaves;          /* extra: 0 = auto (OpenCV formula)             */
    int    maxKeypoints;        /* extra: result capacity; 0 = numFeatures + 25 % (or pyramid pixels / 32 when numFeatures = 0), at most 65536 */
} sift_hip_config;

/* Fills the reference defaults (CudaSiftConfig.hh:6-12) for a w x h image. */
void sift_hip_default_config(sift_hip_config* cfg, int w, int h);

/* Library / build info: "abi=<n> arch=gfx950 hip=<ver>". */
const char* sift_hip_version(void);
const char* sift_hip_last_error(void);

/* --- Detector (replaces sift_cuda::Detector, Detector.hh:24-96) ------------ */

/* Detector::Detector(const CudaSiftConfig&) (Detector.hh:26-29).  device < 0
 * binds to the calling thread's current HIP device like the reference. */
int sift_hip_create(const sift_hip_config* cfg, int device, sift_hip_t* out);
int sift_hip_destroy(sift_hip_t h);

/* Detector::gpuWarmUpAndAllocate() (Detector.cu:17-39): allocate every buffer,
 * build the hipGraph of the whole pipeline and run it once on a blank frame. */
int sift_hip_warmup(sift_hip_t h);

/* Octave count and per-octave geometry chosen for this configuration. */
int sift_hip_num_octaves(sift_hip_t h, int* n);
int sift_hip_octave_dims(sift_hip_t h, int octave, int* w, int* hgt, int* pitch_floats);

/* Detector::detectAndCompute(const Imagef&) (Detector.cu:133-233): uploads the
 * fp32 host image (row stride in bytes, 0 = packed) and runs the pipeline;
 * returns when results are ready.  Keypoint count via sift_hip_num_keypoints. */
int sift_hip_detect(sift_hip_t h, const float* host_img, size_t row_stride_bytes);

/* Pixel formats of a caller's frame.  OpenCV converts CV_8U input to float
 * exactly (createInitialImage), so an 8-bit frame gives the results of the
 * float frame holding the same values; it crosses PCIe in a quarter of the
 * bytes and is converted inside the first GPU kernel. */
#define SIFT_HIP_F32 0  /* float, 0..255 (Imagef, HostImage.hh:188)        */
#define SIFT_HIP_U8  1  /* uint8 (Image8U, HostImage.hh:187; cv::Mat CV_8U) */

/* Detector::detectAndCompute for an 8-bit host frame (the reference converts
 * cv::Mat to Imagef first, cvUtils/ConversionImpl.hpp:8-31).  Synchronous. */
int sift_hip_detect_u8(sift_hip_t h, const uint8_t* host_img, size_t row_stride_bytes);

/* Same, for an image already in device memory (HBM-resident input); enqueued on
 * `stream` (NULL = internal) and NOT synchronised: call sift_hip_sync.  The
 * result accessors address this frame at once (device-ordered use); counts
 * are valid after sift_hip_sync. */
int sift_hip_detect_device(sift_hip_t h, const float* dev_img, size_t row_stride_bytes, void* stream);
int sift_hip_detect_device_fmt(sift_hip_t h, const void* dev_img, size_t row_stride_bytes, int format,
                               void* stream);
int sift_hip_sync(sift_hip_t h);

/* Descriptors for caller-supplied keypoints: cv::Feature2D::compute, i.e.
 * cv::SIFT::detectAndCompute(img, mask, kpts, desc, useProvidedKeypoints =
 * true) -- tracked points of the previous frame, re-projected map points,
 * another detector's corners.  The call builds the Gaussian pyramid of the
 * frame and describes the n keypoints on it (OpenCV's calcDescriptors: each
 * keypoint's packed octave picks its plane, no orientation is assigned);
 * extrema, refinement, orientation and ordering do not run.
 *
 * sift_hip_keypoint is cv::KeyPoint minus class_id (24 bytes).  `octave` is
 * OpenCV's packed form: octave & 255 | layer << 8 | xi << 16 (the value
 * feats4[0] holds as a float); x, y, size in input-image pixels, angle in
 * degrees.
 *
 * The call counts as a frame like a single-frame detect: it takes the next
 * frame number and results slot, and every result accessor works unchanged --
 * sift_hip_num_keypoints gives n, rows are in the caller's order, kpts3 =
 * {x, y, layer} and feats4 = {(float)octave, size, response, angle} are
 * written from the input, prev_desc is the previous frame's rows and the
 * matcher sidecar is that of the new rows.  On a batch handle it uses frame
 * 0's arena.  Not available as submit / micro-batch / batch variants.
 *
 * A keypoint is valid when: its octave lies in [firstOctave, firstOctave +
 * nOctaves - 1] of this handle (firstOctave = -1 with upscale, else 0) and
 * its layer in [0, numOctaveLayers + 2] (every Gaussian plane, as in OpenCV);
 * x, y and size are finite and size > 0; 0 <= angle <= 360; and -W <= x <= 2W,
 * -H <= y <= 2H (points a little outside the frame are legitimate and give
 * partial or all-zero rows; further out the integer window arithmetic is not
 * defended).
 *
 * In the default descriptor mode the +-1 contract against OpenCV is stated for
 * keypoints in the detector's scale range (size * scale / 2 <= sigma *
 * 2^((L + 0.5) / L), scale = 2^-octave).  Larger windows (12 to 200 px on
 * every plane of a 96 x 80 frame) also measured +-1, with a lower share of
 * exact bytes (0.9905 against 0.998).
 * SIFT_HIP_DESC_EXACT is bit-identical to OpenCV for every valid keypoint. */
typedef struct { float x, y, size, angle, response; int octave; } sift_hip_keypoint;

/* Host-only (valid right after sift_hip_create, no device call): *first_bad =
 * index of the first invalid keypoint, or -1 when all n are valid; returns
 * SIFT_HIP_OK either way.  n < 0 or n above the result capacity
 * (sift_hip_capacities) is SIFT_HIP_ERR_INVALID. */
int sift_hip_check_keypoints(sift_hip_t h, const sift_hip_keypoint* kpts, int n, int* first_bad);

/* Host image and host keypoints; synchronous, as sift_hip_detect.  Keypoints
 * are validated first: an invalid one, n < 0 or n above the result capacity
 * returns SIFT_HIP_ERR_INVALID (the index in sift_hip_last_error) and nothing
 * is launched -- the previous results stay current.  n = 0 is legal (count 0). */
int sift_hip_compute   (sift_hip_t h, const float*   host_img, size_t row_stride_bytes,
                        const sift_hip_keypoint* kpts, int n);
int sift_hip_compute_u8(sift_hip_t h, const uint8_t* host_img, size_t row_stride_bytes,
                        const sift_hip_keypoint* kpts, int n);

/* Device image (SIFT_HIP_F32 / SIFT_HIP_U8) and device keypoints, enqueued
 * after `stream` and NOT synchronised, as sift_hip_detect_device_fmt; both
 * buffers must stay unchanged until sift_hip_sync.  The keypoints cannot be
 * checked on the host: the job kernel validates them, an invalid keypoint gets
 * an all-zero descriptor row (and the sidecar codes of a zero row) and sets
 * SIFT_HIP_FLAG_BAD_KEYPOINT in the frame's sift_hip_overflow_flags.  n is
 * checked on the host as above. */
#define SIFT_HIP_FLAG_BAD_KEYPOINT 16
int sift_hip_compute_device(sift_hip_t h, const void* dev_img, size_t row_stride_bytes, int format,
                            const sift_hip_keypoint* dev_kpts, int n, void* stream);

/* Detection mask: cv::SIFT::detectAndCompute(img, mask, kpts, desc) with a
 * non-empty mask.  The mask is an 8-bit image of the frame's size (col_width x
 * row_width bytes, row stride in bytes, 0 = packed).  OpenCV applies it to the
 * detector's final keypoint list (KeyPointsFilter::runByPixelsMask) -- after
 * the duplicate filter, after retainBest(numFeatures) and after the upscale
 * rescale of pt -- and so does this build: a keypoint is REMOVED when
 *     mask[(int)(pt.y + 0.5f)][(int)(pt.x + 0.5f)] == 0
 * (float32 add, truncating cast, on the coordinates kpts3 holds; any non-zero
 * byte keeps it; the index is clamped to the mask, which detector keypoints
 * never need).  The kept keypoints keep their order, and everything downstream
 * sees the kept rows only: sift_hip_num_keypoints, kpts3 / feats4 / desc, the
 * matcher sidecar, prev_desc of the next frame, the host results.  The result
 * capacity (overflow flag 8) is judged on the kept count.
 *
 * The mask acts AFTER retainBest: with numFeatures = N a masked frame returns
 * the kept subset of the unmasked frame's N best -- usually fewer than N, not
 * the N best of the masked region.  With numFeatures = 0 (keep all) masked-out
 * keypoints are dropped before their orientation histogram is built, so their
 * orientation and descriptor work is saved.
 *
 * A masked call is a frame like any other single-frame (or batch) detect: next
 * frame number and results slot, prev_desc = the previous frame's rows, fresh
 * sidecars; on a batch handle the single-frame calls use frame 0's arena; on a
 * micro-batching / auto-group handle queued frames are launched first.  It
 * launches the detect chain's kernels eagerly with the mask as an argument;
 * frames without a mask launch the captured graphs as before.  mask == NULL
 * makes each call identical to its unmasked counterpart.  A mask stride below
 * the width (or an unknown format) is SIFT_HIP_ERR_INVALID, and a masked call
 * while sift_hip_set_datagen is active is SIFT_HIP_ERR_STATE (the dump format
 * holds no mask, so a replay could not reproduce the frame); in both cases
 * nothing is launched and the previous results stay current.  Timing mode works.
 * There are no pipelined (sift_hip_submit / sift_hip_submit_device /
 * micro-batch) variants.  sift_hip_compute* take no mask: OpenCV ignores the
 * mask when useProvidedKeypoints is set.
 *
 * Host image (SIFT_HIP_F32 / SIFT_HIP_U8) and host mask; synchronous.  The mask
 * goes through handle-owned staging allocated at the first such call; both
 * buffers are free on return. */
int sift_hip_detect_masked(sift_hip_t h, const void* host_img, size_t row_stride_bytes, int format,
                           const uint8_t* host_mask, size_t mask_stride_bytes);
/* Device image and device mask, enqueued after `stream`, not synchronised (as
 * sift_hip_detect_device_fmt).  The mask is read in place: like the image it
 * must stay unchanged until sift_hip_sync. */
int sift_hip_detect_device_masked(sift_hip_t h, const void* dev_img, size_t row_stride_bytes, int format,
                                  const uint8_t* dev_mask, size_t mask_stride_bytes, void* stream);
/* n device frames and n device masks (mask i at dev_masks + i *
 * mask_frame_stride_bytes, 0 = mask stride * height), as
 * sift_hip_detect_batch_device.  Each frame's results are those of the
 * single-frame masked call on it, bit for bit. */
int sift_hip_detect_batch_device_masked(sift_hip_t h, const void* dev_frames, int n, size_t row_stride_bytes,
                                        size_t frame_stride_bytes, int format, const uint8_t* dev_masks,
                                        size_t mask_stride_bytes, size_t mask_frame_stride_bytes, void* stream);

/* Frame batches (C4: many frames per GPU).  sift_hip_set_batch(h, B), called
 * before sift_hip_warmup, gives the handle B frame arenas (pyramid, keypoint
 * lists, counters and result slots per frame) and a pipeline graph whose every
 * launch processes all B frames: B x the workgroups per launch and 1/B of the
 * dispatches per frame.  Results per frame are those of the single-frame call
 * on the same frame, bit for bit.  B = 1 (default) is the single-frame handle;
 * every single-frame entry point keeps working on a batch handle (frame 0's
 * arena, a one-frame graph).  Replaces the per-frame loop of
 * /root/reference/tool/extract_and_match_example.cc:69-101 over
 * Detector::detectAndCompute (Detector.cu:133-233). */
int sift_hip_set_batch(sift_hip_t h, int frames);
int sift_hip_batch_capacity(sift_hip_t h, int* frames);

/* Descriptor histogram summation, called before sift_hip_warmup (the mode is
 * part of the captured graphs).  The reference sums each bin with float
 * shared-memory atomics in scheduling order (SiftOps.cu:587-600); OpenCV sums
 * it sequentially in raster order (sift.simd.hpp calcSIFTDescriptor).
 *   SIFT_HIP_DESC_FAST  (default) fixed-point integer histogram: deterministic,
 *                       the exact sum of the rounded contributions; a byte can
 *                       differ from OpenCV's by +-1 (float summation order).
 *   SIFT_HIP_DESC_EXACT OpenCV's sequential float sum and correctly rounded
 *                       sample math: descriptors bit-identical to the oracle,
 *                       at a higher descriptor cost.
 * Keypoints are identical in both modes. */
#define SIFT_HIP_DESC_FAST  0
#define SIFT_HIP_DESC_EXACT 1
int sift_hip_set_descriptor_mode(sift_hip_t h, int mode);
int sift_hip_descriptor_mode(sift_hip_t h, int* mode);

/* Descriptor normalisation ("RootSIFT", Arandjelovic & Zisserman 2012: the
 * square root of the L1-normalised row, so that the Euclidean distance of the
 * matcher is the Hellinger distance of the histograms; COLMAP's L1_ROOT with
 * its round(512 x) conversion to 8 bits, applied to OpenCV's bytes).  The rule,
 * in float32, total, for a row of 128 values v[i]:
 *   1. b[i] = clamp(cvRound(v[i]), 0, 255): round half even, NaN -> 0.  The
 *      identity on the bytes the detector would have written without the norm.
 *   2. s = sum b[i], an integer (<= 32,640: exact in any order).
 *   3. s == 0: the row is all zero.
 *   4. Otherwise r[i] = sqrtf((float)b[i] / (float)s): one IEEE correctly
 *      rounded division and one correctly rounded square root, nothing fused.
 *   5. out[i] = min(255, cvRound(512.f * r[i])), stored as the fp16 of that
 *      integer like every descriptor row.
 *   6. Sidecar code out[i] - 128 and key bias -(256 * sum code^2 + (row & 255)),
 *      from the new bytes: matches of two ROOT buffers keep the direct path.
 * sum r^2 = 1, so rows keep the scale of OpenCV's rows (norm ~512; 509.9 to
 * 513.5 on SIFT-like rows, largest byte ~115).  The clamp of step 5 acts only
 * where one entry holds more than 24.7 % of the row's L1 mass.
 * sift_amd.cv.rootsift is the numpy mirror; the device equals it byte for byte.
 *
 * Detector norm, called before sift_hip_warmup (part of the captured graphs;
 * later SIFT_HIP_ERR_STATE; an unknown norm SIFT_HIP_ERR_INVALID):
 *   SIFT_HIP_NORM_L2   (default) OpenCV's rows.
 *   SIFT_HIP_NORM_ROOT every descriptor row this handle writes -- single
 *                      frames, batches, lanes, micro-batches, masked calls,
 *                      sift_hip_compute*, the pinned host rows, the replay of
 *                      the descriptor stage -- is the rule applied to the row
 *                      the call would have written, in the kernel that
 *                      computes it (no extra pass or launch).  An invalid
 *                      keypoint of sift_hip_compute* keeps its zero row.
 * Independent of sift_hip_set_descriptor_mode (four combinations); keypoints
 * are identical in both norms.  Stage dumps are compared with the oracle's L2
 * rows: sift_hip_set_datagen on a ROOT handle, and ROOT while dumps are on,
 * are SIFT_HIP_ERR_STATE.
 * Rows of different norms must not be matched against each other, and
 * max_distance caps of the match lists are on the new rows' scale. */
#define SIFT_HIP_NORM_L2   0
#define SIFT_HIP_NORM_ROOT 1
int sift_hip_set_descriptor_norm(sift_hip_t h, int norm);
int sift_hip_descriptor_norm(sift_hip_t h, int* norm);

/* The same rule for rows the detector did not write in ROOT (a database's
 * descriptors, a frame the caller kept, another extractor's rows): n rows of
 * 128 fp16 values in device memory, desc_in -> desc_out.  Handle-free, one
 * launch on `stream` (NULL = the default stream), not synchronised, no
 * allocation: capturable.  desc_out == desc_in transforms in place; any other
 * overlap of the two n * 256-byte ranges, n < 0, a null pointer with n > 0 or
 * an odd pointer is SIFT_HIP_ERR_INVALID; n == 0 is a no-op.
 * A caller transforming a detector's own buffer declares the write first
 * (sift_hip_descriptors_written; C++ / Python: mutable_data()), so that the
 * matcher converts the written rows instead of reading the stale sidecar.
 * sift_hip_rootsift_host takes host rows through the device, synchronously
 * (allocates and frees its staging buffer on the current device). */
int sift_hip_rootsift_device(const uint16_t* desc_in, int n, uint16_t* desc_out, void* stream);
int sift_hip_rootsift_host(const uint16_t* desc_in, int n, uint16_t* desc_out);

/* n (1..B) device frames, frame i at dev_frames + i * frame_stride_bytes (0 =
 * row_stride * height), enqueued on `stream` (NULL = internal), NOT
 * synchronised (sift_hip_sync).  The batch becomes the current launch group. */
int sift_hip_detect_batch_device(sift_hip_t h, const void* dev_frames, int n, size_t row_stride_bytes,
                                 size_t frame_stride_bytes, int format, void* stream);
/* Frames in the current launch group (1 after a single-frame call). */
int sift_hip_batch_frames(sift_hip_t h, int* n);
/* Frame i of the current group: count / overflow flags (valid after
 * sift_hip_sync) and its device result arrays (layouts as
 * sift_hip_results_device). */
int sift_hip_batch_results_device(sift_hip_t h, int i, int* count, int* overflow, const float** kpts3,
                                  const float** feats4, const uint16_t** desc);
/* Copies min(count, cap) results of frame i to host memory (desc nullable). */
int sift_hip_batch_copy_to_host(sift_hip_t h, int i, float* kpts3, float* feats4, uint16_t* desc, int cap,
                                int* count);

/* Pipelined host input (replaces the synchronous upload of CudaImage.cu:97-105
 * and the per-frame loop of extract_and_match_example.cc:69-101).
 * sift_hip_submit copies the frame into one of its lane's two mapped pinned
 * staging buffers (the caller's buffer is free again on return), enqueues a
 * small copy kernel (staging -> device, over PCIe) and the pipeline on the
 * lane's stream and returns a ticket without waiting.
 * sift_hip_wait(ticket) blocks until that frame is complete and makes it the
 * frame the result accessors address (prev_desc = frame ticket-1).  At most
 * 2 x lanes frames may be in flight past the last waited one
 * (SIFT_HIP_ERR_STATE otherwise); sift_hip_detect / sift_hip_detect_u8 =
 * submit + wait.
 *
 * Frames in flight compute concurrently: a handle has up to `lanes` compute
 * lanes (a HIP stream with its own frame arenas, graphs and results ring
 * each).  A frame goes to the first idle lane; when every lane is busy and
 * fewer than `lanes` exist, a new one is created (its arenas and graphs, once:
 * a synchronous caller never pays for a second lane).  Results are identical
 * on every lane.  sift_hip_set_lanes(h, n), n = 1..4 (default 2), before
 * sift_hip_warmup; n = 1 runs every frame of the handle in submission order
 * on one stream.  sift_hip_lanes reports the limit and the lanes created. */
int sift_hip_submit(sift_hip_t h, const void* host_img, size_t row_stride_bytes, int format,
                    long long* ticket);
int sift_hip_wait(sift_hip_t h, long long ticket);
int sift_hip_set_lanes(sift_hip_t h, int lanes);
int sift_hip_lanes(sift_hip_t h, int* max_lanes, int* created);

/* Pipelined device input: like sift_hip_submit for a frame already in device
 * memory (f32 or u8, row stride in bytes), read on the frame's lane after
 * `stream` (NULL: no ordering) reaches this call; the buffer must stay
 * unchanged until sift_hip_wait(ticket) returns.  The results follow at
 * sift_hip_wait, as for host frames. */
int sift_hip_submit_device(sift_hip_t h, const void* dev_img, size_t row_stride_bytes, int format, void* stream,
                           long long* ticket);

/* Micro-batching of pipelined frames: with frames = M > 1 (before
 * sift_hip_warmup; the handle's batch size becomes M), frames submitted by
 * sift_hip_submit_device or sift_hip_submit queue until M of them run as ONE
 * launch group on a lane (each frame's rows copied into the lane's group
 * input -- device frames after their `stream` event, host frames from the
 * pinned staging block they were copied into at submit; one launch per
 * pipeline stage for the group, as sift_hip_detect_batch_device).  Tickets, results and prev_descriptor are per
 * frame and identical to unbatched submission.  A frame still queued is
 * launched (with the frames before it, as a partial group) by sift_hip_wait
 * on it, sift_hip_sync, or any other detect / submit call; its `dev_img` must
 * stay unchanged until then.  At most 2 x lanes x M frames may be in flight
 * past the last waited one.  Default 1 (every frame launched at submit). */
int sift_hip_set_micro_batch(sift_hip_t h, int frames);
int sift_hip_micro_batch(sift_hip_t h, int* frames);

/* Automatic launch groups (the default, frames = 8; before sift_hip_warmup;
 * 0 or 1 turns them off) on a handle without a batch or micro-batch and with
 * more than one lane.  Frames of sift_hip_submit / sift_hip_submit_device run
 * as single frames while at most 2 per lane are in flight past the last
 * waited one (exactly as without groups); past that they queue, and the queue
 * runs as ONE launch group (as with a micro-batch) when it holds `frames`
 * frames, or -- checked at each submit -- when a lane that can take it is
 * free and it holds frames / 2, or at a wait on a queued frame /
 * sift_hip_sync / any other detect.  So a caller keeping many frames in
 * flight gets micro-batched launches with no extra call, and a synchronous or
 * shallow caller runs unchanged.  Lane 0 keeps one frame arena; lanes created
 * later hold `frames` arenas and 8 results slots.  Each results slot of a
 * group lane then holds at least frames / 2 frames, which bounds the frames in flight past the last
 * waited one at max(2 x lanes, (lanes - 1) x 3 x frames / 2) (24 for 3 lanes
 * and the default 8).  A group of 8-bit and f32 frames runs as f32 (8-bit
 * frames converted exactly).  Queued host frames go through a pinned staging
 * block of (2 x lanes + 1) x frames frame slots, allocated at the first one
 * (1920x1200 8-bit frames, 2 lanes: 92 MB; f32: 369 MB) -- a caller that
 * never keeps more than 2 frames per lane in flight never allocates it.
 * Results, tickets and prev_descriptor are per frame and identical to
 * unbatched submission. */
int sift_hip_set_auto_micro_batch(sift_hip_t h, int frames);
int sift_hip_auto_micro_batch(sift_hip_t h, int* frames);

/* Detector::total_size (Detector.hh:62, Detector.cu:584-604). */
int sift_hip_num_keypoints(sift_hip_t h, int* n);
/* Capacities of the handle's per-frame buffers (host-only, valid right after
 * sift_hip_create): 3x3x3 candidates, refined keypoints, oriented slots and
 * results.  Sized from the octave geometry and numFeatures (maxKeypoints
 * overrides the result capacity); NULL arguments are skipped. */
int sift_hip_capacities(sift_hip_t h, int* candidates, int* refined, int* oriented, int* results);

/* Non-zero when a capacity overflowed (1 candidates, 2 refined, 4 oriented,
 * 8 results) or sift_hip_compute_device met an invalid keypoint
 * (SIFT_HIP_FLAG_BAD_KEYPOINT, 16).  With bit 1 (value 1) set the frame's
 * candidate list was full: an arbitrary subset of the candidates (atomic
 * order) went on, so the results are a subset of the full result and can
 * differ between runs; every keypoint returned is still a correct one. */
int sift_hip_overflow_flags(sift_hip_t h, int* flags);

/* Device result arrays (Detector.hh:54-57): kpts = float3 {x, y, layer}
 * per keypoint, features = float4 {octave packed as float, size, response,
 * angle}, descriptors = 128 x IEEE half (values 0..255) per keypoint.
 * prev_desc = the previous frame's descriptors (Detector.cu:136-141).  Blocks
 * the host until the current frame's counts are final (they come from the
 * device), as the reference's own count read-back does (Detector.cu:542-548). */
int sift_hip_results_device(sift_hip_t h, const float** kpts3, const float** feats4,
                            const uint16_t** desc, const uint16_t** prev_desc,
                            int* prev_count, int* capacity);

/* Detector::copyToHost(bool descriptor) (Detector.cu:606-634).  Copies
 * min(count, cap) results; desc may be NULL. */
int sift_hip_copy_to_host(sift_hip_t h, float* kpts3, float* feats4, uint16_t* desc, int cap);

/* The same results without a copy into caller memory: the reference's
 * detector-owned host vectors final_kpts / final_features / descriptors
 * (Detector.hh:58-60, filled by copyToHost).  Returns pointers into the
 * handle's pinned results region of the current frame (*count rows; desc may
 * be NULL).  A frame submitted from host memory already had its results
 * written there by its last kernel; any other frame's are copied there by
 * this call.  The rows stay valid while the frame is the current or the
 * previous one (the lifetime of prev_descriptor): until a second later frame
 * has been made current by wait / detect.  Read-only for the caller. */
int sift_hip_results_host(sift_hip_t h, const float** kpts3, const float** feats4, const uint16_t** desc,
                          int* count);

/* Device-to-device copy of this frame's descriptors (e.g. into a torch tensor
 * for an RCCL all-gather).  Copies min(count, cap) rows, pads nothing.  The
 * row count is needed on the host, so this call (like sift_hip_results_device
 * and sift_hip_num_keypoints after an unsynchronised detect) first blocks the
 * host until the frame's counts are final; the copy itself is then enqueued on
 * `stream`. */
int sift_hip_copy_descriptors_device(sift_hip_t h, uint16_t* dst, int cap, void* stream);

/* The current frame's matcher sidecar (device pointers, valid as its
 * descriptor rows): int8 codes v - 128 (128 B per keypoint row) and per row
 * the key bias -(256 |c|^2 + (row & 255)), written by the descriptor kernel
 * beside the fp16 rows.  The C5 exchange all-gathers these (132 B per row
 * instead of 256) and matches them with sift_hip_match_codes_batched.  No
 * reference counterpart (the reference gathers nothing, Match.cu:8-33). */
int sift_hip_results_sidecar(sift_hip_t h, const int8_t** codes, const int** keys);

/* Detector::setDataGen(path) (Detector.hh:48-51; the reference dumps each
 * stage's octave-0 inputs/outputs as msgpack+zlib, Detector.cu:145-229,
 * PerfData.cuh:12-155).  With a non-empty dir every following single-frame
 * detect completes synchronously and writes this build's stage dumps of the
 * frame into dir (overwritten per frame; dir is created): meta.json (config,
 * octave geometry, counts, file layouts), input.f32, gauss_o<o>_l<l>.f32 (every
 * Gaussian plane), candidates.i32, kpts3.f32, feats4.f32, desc.f16, and the
 * keypoint stages' device records refined.rec, oriented.rec, jobs.rec,
 * range.u32, counters.u32 -- raw little-endian arrays.  tests/stage_check.py replays a dump against
 * the CPU oracle and this library.  NULL or "" switches the dumps off. */
int sift_hip_set_datagen(sift_hip_t h, const char* dir);

/* Per-stage replay (the reference's tool/perf.cu:43-100, which runs each
 * HostInterface.hh:11-69 stage -- runFilter ... runDescriptor -- alone on a
 * setDataGen snapshot): runs ONE stage of the pipeline on the inputs recorded
 * in a sift_hip_set_datagen dump directory and writes that stage's outputs,
 * with the dump's file names and formats, into out_dir.  Stages and files:
 *   "pyramid"     input.f32                          -> gauss_o<o>_l<l>.f32
 *   "extrema"     gauss planes                       -> candidates.i32
 *   "refine"      planes, candidates.i32             -> refined.rec
 *   "orientation" planes, refined.rec                -> oriented.rec
 *   "order"       planes, oriented.rec, counters.u32 -> kpts3.f32, feats4.f32, jobs.rec
 *   "descriptor"  planes, jobs.rec, range.u32        -> desc.f16
 * The dump must come from a handle of the same configuration.  Synchronous;
 * the handle's current results are discarded (it is left as after warm-up). */
int sift_hip_replay_stage(sift_hip_t h, const char* dump_dir, const char* stage, const char* out_dir);

/* Stage timing for roofline reporting: when enabled, the next detect calls run
 * un-graphed with HIP events around every kernel; names are stable strings.
 * enable >= 2 also repeats each (pure) blur launch `enable` times back to back
 * inside its event pair, so the per-launch figure carries one event pair per
 * `enable` launches instead of one per launch. */
int sift_hip_set_timing(sift_hip_t h, int enable);
int sift_hip_timing_count(sift_hip_t h, int* n);
int sift_hip_timing_entry(sift_hip_t h, int i, const char** name, double* total_ms,
                          int* launches, double* algo_bytes);
int sift_hip_timing_reset(sift_hip_t h);

/* Debug/parity accessors (tests): Gaussian plane (octave, layer) as w*h floats;
 * pre-refinement candidates as (octave, layer, r, c) int quadruples: OpenCV's
 * 3x3x3 extrema (|v| > thr, thr = floor(0.5 * contrastThreshould /
 * numOctaveLayers * 255)), at thr = 0 minus those whose 3x3 block in their own
 * DoG layer is constant (rounding residue of flat regions), which
 * adjustLocalExtrema can never keep.  *count is the number
 * of hits, stored or not: above the candidate capacity min(*count, capacity)
 * rows exist (overflow flag 1). */
int sift_hip_debug_gaussian(sift_hip_t h, int octave, int layer, float* out);
int sift_hip_debug_candidates(sift_hip_t h, int* quads, int cap, int* count);

/* --- Brute-force matcher (replaces sift_cuda::matchBruteForce, Match.cuh:9-25) */

/* Scratch for up to max_query x max_train per pair and max_pairs pairs.  One
 * launch per match call: the split workgroups merge their top-2 through
 * device-scope atomics in this scratch, so calls on ONE matcher must be
 * ordered (same stream, or synchronised); use one matcher per stream for
 * concurrent matching. */
int sift_hip_matcher_create(int device, int max_query, int max_train, int max_pairs,
                            sift_hip_matcher_t* out);
int sift_hip_matcher_destroy(sift_hip_matcher_t m);

/* Top-2 L2 neighbours of each query row in train, 128-D half descriptors in
 * device memory.  Outputs (device, may be NULL): idx2[2*i+{0,1}] (-1 if none),
 * d2[2*i+{0,1}] squared L2 distance (exact for integer descriptors).
 * match[i] = idx2[2i] if d2[2i] < ratio^2 * d2[2i+1] (ratio on distances,
 * ratio_on_squared = 0) or d2[2i] < ratio * d2[2i+1] (ratio_on_squared = 1, the
 * reference's Match.cu:172 convention), else -1; a query with one train row
 * matches it.  Enqueued on `stream`.
 *
 * The general path.  A set holding a value that is not an integer 0..255
 * (unrounded x512 SIFT, RootSIFT, learned descriptors; -0.0, NaN and infinities
 * count) is matched in fp16/fp32 instead of int8/int32: exact fp16 products,
 * fp32 sums, d2 = |t|^2 - 2 q.t + |q|^2.  This holds for every match call of
 * this header (single, batched, guided, epipolar, lists), for finite inputs:
 *   1. Sign.  Every returned d2 is >= 0 and never NaN (three fp32 sums round
 *      apart, so the raw value of a duplicate row can be below 0: it is clamped
 *      to 0); its sqrt, and so every sift_hip_dmatch.distance, is finite.
 *   2. Accuracy.  With D = sum_k (q_k - t_k)^2 in float64 on the fp16 values,
 *      |d2 - D| <= B = 136 * 2^-23 * (|q|^2 + |t|^2 + 2 sum_k |q_k| |t_k|):
 *      three sums of 128 exact products in any order ((n - 1) u sum |terms|),
 *      9 combining operations, u = 2^-23 allowing for a truncating MFMA.
 *   3. Indices.  With D1 <= D2 <= D3 the query's three smallest D among its
 *      candidates and Bq its largest B: D[i1] <= D1 + 2 Bq, D[i2] <= D2 + 2 Bq,
 *      i1 != i2; where D2 - D1 > 2 Bq and D3 - D2 > 2 Bq the indices are the
 *      float64 order's exactly.
 *   4. Duplicates.  Train rows of identical bytes get bit-identical d2 for any
 *      query, and their tie goes to the lower index in every merge, across
 *      splits too.
 *   5. Routes.  idx2 and d2 of one pair are the same bytes through
 *      sift_hip_match_device, sift_hip_match_batched (one pair or several),
 *      sift_hip_match_guided_device with radius = inf and
 *      sift_hip_match_epipolar_device with every row a candidate.
 *   6. match, and every list, are the rules of this header applied to the
 *      returned idx2 / d2 themselves (float32).
 *   7. Special values.  A train row holding NaN or +-Inf is nobody's neighbour;
 *      a query row holding one gets (-1, -1, FLT_MAX, FLT_MAX) and match -1;
 *      every other query gets the bytes it would get with those train rows
 *      deleted.  -0.0 selects the path but is the value 0.
 * On integer sets 0..255 the general path returns the integer path's bytes
 * (every sum is an integer below 2^24). */
int sift_hip_match_device(sift_hip_matcher_t m, const uint16_t* query, int nq,
                          const uint16_t* train, int nt, float ratio, int ratio_on_squared,
                          int* idx2, float* d2, int* match, void* stream);

/* P independent (query_p, train_p) pairs in ONE launch (8-way cross-GPU match).
 * Arrays of P device pointers / counts live in host memory; outputs are packed
 * per pair at offset sum_{q<p} nq[q]. */
int sift_hip_match_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query,
                           const int* nq, const uint16_t* const* train, const int* nt,
                           float ratio, int ratio_on_squared, int* idx2, float* d2,
                           int* match, void* stream);

/* Descriptor buffers handed out by a detector handle (sift_hip_results_device
 * and the batch accessors: the base of a results slot) carry a matcher
 * sidecar written by the same kernel -- int8 codes v - 128 and a per-row key
 * bias.  A single-pair call whose query and train pointers are both such
 * bases (e.g. matchBruteForce(prev_descriptor, n0, device_descriptor, n1))
 * matches those codes directly: no fp16 conversion, no prep launch (results
 * identical).  Treat detector buffers as read-only.  enable = 0 turns the
 * lookup off for matcher m (every call converts the fp16 rows). */
int sift_hip_matcher_set_sidecars(sift_hip_matcher_t m, int enable);

/* The caller wrote into a detector descriptor buffer (a results-slot base as
 * handed out above; C++: DeviceBuffer::mutable_data, Python:
 * DeviceBuffer.mutable_data): its sidecar no longer describes the rows, so
 * matches on that buffer convert the fp16 rows, as for a foreign buffer, until
 * the detector launches a frame into it again.  Unknown pointers: no-op. */
int sift_hip_descriptors_written(const uint16_t* desc);

/* Pairs of code sets already in device memory (e.g. every rank's sidecar
 * all-gathered, C5): int8 codes (128 B rows) and int32 key biases as
 * sift_hip_results_sidecar lays them out (biases computed with set-local row
 * indices).  Pair p matches the nq[p] query rows starting at code row qrow0[p]
 * (their biases from key index qkey0[p]) against the nt[p] train rows starting
 * at code row trow0[p] (biases from tkey0[p]), all pairs in ONE batched launch
 * with no conversion (no k_match_prep).  Outputs and the ratio test as
 * sift_hip_match_batched (packed per pair).  Host arrays of P ints. */
int sift_hip_match_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                 const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                 const int* tkey0, const int* nt, float ratio, int ratio_on_squared, int* idx2,
                                 float* d2, int* match, void* stream);

/* matchBruteForce(des, num_des, src, num_src) (Match.cu:8-33): synchronous,
 * result to host memory out[nq]. */
int sift_hip_match_host(sift_hip_matcher_t m, const uint16_t* query, int nq,
                        const uint16_t* train, int nt, float ratio, int ratio_on_squared,
                        int* out);

/* --- Match lists: match -> filter -> ordered compaction on the device -------
 *
 * What a caller of sift_hip_match_* does next (cv::BFMatcher(NORM_L2,
 * crossCheck = true), COLMAP / SiftGPU's cross_check, "mutual nearest
 * neighbour") in one enqueued operation: the top-2 search in both directions,
 * the filter below, and the surviving matches as cv::DMatch-layout records in
 * query order with their count -- nothing returns to the host in between.
 *
 * The rule.  For a pair (query set Q of nq rows, train set T of nt rows):
 *   forward top-2  (i1, e1, i2, e2)[i] is what sift_hip_match_device(Q, T)
 *                  writes to idx2 / d2 for query i (squared distances, ties to
 *                  the lower train index, -1: none);
 *   reverse top-2  (j1, f1, j2, f2)[t] is what sift_hip_match_device(T, Q)
 *                  writes for train row t (ties to the lower query index);
 *   ratio_pass(a1, d1, a2, d2): the ratio test of sift_hip_match_device's
 *                  `match` output -- a1 >= 0 is required; it passes if a2 < 0;
 *                  with ratio_on_squared the test is d1 < ratio * d2, else
 *                  sqrtf(d1) < ratio * sqrtf(d2) in float32; ratio <= 0
 *                  switches the test off (only a1 >= 0 remains).
 * Query i is kept when all of these hold:
 *   1. i1 >= 0;
 *   2. ratio_pass(forward[i]);
 *   3. max_distance <= 0, or sqrtf(e1) <= max_distance (float32);
 *   4. if cross_check: j1[i1] == i;
 *   5. if ratio_both_ways: ratio_pass(reverse[i1]).
 * The output is the kept queries in ascending queryIdx, one record each:
 * {queryIdx = i, trainIdx = i1, imgIdx = the pair's index p in the call,
 * distance = sqrtf(e1)}, and the number of records.  The bytes are the same in
 * every run (slots are assigned by prefix sums, not by atomics).  With neither
 * cross_check nor ratio_both_ways the reverse direction is not computed: the
 * call is a compacting form of sift_hip_match_device's ratio test.  The rule
 * consumes whatever top-2 the match kernels produce, so it holds unchanged for
 * sets with non-integer fp16 values (the general path, float d2).
 *
 * A mutual list (cross_check) is symmetric: the list of (b, a) is the list of
 * (a, b) with queryIdx and trainIdx swapped (in trainIdx order).  An all-pairs
 * exchange over 8 sets therefore needs the 28 unordered pairs, not the 56
 * ordered ones.
 *
 * Scratch: the top-2 arrays of both directions live in matcher-owned scratch
 * that is allocated at the first sift_hip_match_list_* call on the matcher, so
 * a matcher that never makes one keeps its footprint.  That FIRST call
 * allocates device memory and must not run under stream capture; later calls
 * only launch kernels.  Calls on one matcher must be ordered, as for
 * sift_hip_match_*. */
typedef struct {
    int queryIdx, trainIdx, imgIdx;
    float distance;
} sift_hip_dmatch; /* 16 bytes, cv::DMatch's fields in its order */

typedef struct {
    float ratio;          /* Lowe's ratio; <= 0: no ratio test */
    int ratio_on_squared; /* the ratio applies to squared distances (matchBruteForce's convention) */
    int ratio_both_ways;  /* the reverse top-2 of the matched train row passes the ratio test too */
    float max_distance;   /* cap on the L2 distance (not squared); <= 0: none */
    int cross_check;      /* keep mutual nearest neighbours only */
} sift_hip_match_filter;

/* ratio 0.8 on distances, one way, no distance cap, cross_check on. */
void sift_hip_default_match_filter(sift_hip_match_filter* filter);

/* One pair.  out: device, room for nq records; count: device int.  When the
 * filter needs the reverse direction (cross_check or ratio_both_ways) the pair
 * is also matched with the roles swapped, so nt <= max_query and
 * nq <= max_train must hold besides sift_hip_match_device's limits.  A pair of
 * detector buffers with fresh sidecars matches their codes directly in both
 * directions.  A null matcher, filter, out or count, or a size over a limit:
 * SIFT_HIP_ERR_INVALID, nothing is launched.  nq == 0 or nt == 0: count 0. */
int sift_hip_match_list_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* count, void* stream);

/* P pairs (host arrays as sift_hip_match_batched; P <= max_pairs).  Pair p's
 * records start at row sum_{r<p} nq[r] of out (device, sum nq rows) and carry
 * imgIdx = p; counts: device, P ints.  With the reverse direction needed and
 * 2 P <= max_pairs the forward and reverse pairs run in one 2P-pair launch
 * (each distinct set is converted once), otherwise in two P-pair launches on
 * the stream; the results are the same bytes. */
int sift_hip_match_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                const uint16_t* const* train, const int* nt, const sift_hip_match_filter* filter,
                                sift_hip_dmatch* out, int* counts, void* stream);

/* The same for pairs of ready code sets (sift_hip_match_codes_batched's
 * arguments). */
int sift_hip_match_list_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                      const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                      const int* tkey0, const int* nt, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* counts, void* stream);

/* Synchronous, one pair, records to host memory: copies min(count, cap)
 * records to out_host and sets *count to the full count. */
int sift_hip_match_list_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                             const sift_hip_match_filter* filter, sift_hip_dmatch* out_host, int cap, int* count);

/* --- k nearest neighbours (k <= 8) and capped radius lists -------------------
 *
 * cv::BFMatcher::knnMatch(query, train, k) and radiusMatch capped at k per
 * query, without a distance matrix in memory: the few best candidates of each
 * query for a verifier to choose from (repetitive structure, where the ratio
 * test discards the right match because its twin is second), voting and
 * retrieval.  sift_hip_verify_* accept the lists as they are (repeated
 * queryIdx).
 *
 * The rule.  For a pair (Q: nq rows, T: nt rows) and 1 <= k <= SIFT_HIP_KNN_MAX:
 *   row i of idx[nq][k] / d2[nq][k] holds the min(k, candidates) train rows of
 *   smallest squared L2 distance to query i, in ascending (d2, train index)
 *   order -- a tie at any rank, the k-th included, goes to the lower train
 *   index -- and -1 / FLT_MAX in the remaining entries.  On integer sets d2 is
 *   the float32 of the exact integer.  On the general path (a set holding a
 *   value that is not an integer 0..255) d2 and the special values follow items
 *   1, 2, 4 and 7 of the general-path contract above, a query row holding NaN
 *   or an infinity getting -1 / FLT_MAX throughout; the arithmetic is that of
 *   sift_hip_match_device: the same MFMA sequence, (|t|^2 - 2 q.t) + |q|^2,
 *   the clamp at 0, candidates ordered on |t|^2 - 2 q.t.
 *   Routes.  k = 2 gives, byte for byte, what sift_hip_match_device writes to
 *   idx2 / d2, on both paths.  Column j of a call with k equals column j of a
 *   call with any k' > j.  The bytes do not depend on the launch plan, on the
 *   kernel instantiation that served the call, on max_pairs, or on whether the
 *   sets came as detector buffers, fp16 rows or codes.
 * The list of a pair is its table as records: neighbour j of query i is kept
 * when idx[i][j] >= 0 and (max_distance <= 0 or sqrtf(d2[i][j]) <= max_distance,
 * float32); the kept neighbours come out in (queryIdx, rank) order as
 * {queryIdx = i, trainIdx = idx[i][j], imgIdx = the pair's index p,
 * distance = sqrtf(d2[i][j])}, their number in a device int.  Slots come from
 * prefix sums: the bytes are the same in every run.  max_distance <= 0 gives
 * the whole table.
 *
 * Refusals (SIFT_HIP_ERR_INVALID, nothing launched, nothing written, judged
 * before any device call): k outside 1..SIFT_HIP_KNN_MAX; a null matcher; a
 * size over the matcher's limits; P outside 1..max_pairs; a null descriptor
 * pointer of a non-empty set; for the list calls a null out or count, or a NaN
 * max_distance.  nq == 0: nothing is written (a list's count is 0).  nt == 0:
 * every entry is -1 / FLT_MAX and the count is 0.
 *
 * Scratch.  Train rows are split over workgroups by whole groups of 256 rows,
 * at most 8 splits; each split writes a sorted list of 8-byte keys per query,
 * which the last split of a query block merges.  The matcher allocates, at its
 * first k-NN call (not under stream capture; later calls only launch),
 *   64 B * max_query * max(8, 2 * max_pairs)        the split lists,
 *   2 * 4 B * 8 * max_pairs * max_query             the table of the list and host calls,
 *   16 B * 8 * max_query + 4 B * max_pairs          the records and counts of the host calls,
 * and a call of P pairs with the largest nq = Q uses S splits with
 * P * S * Q <= max_query * max(8, 2 * max_pairs): the plan's S, lowered if need
 * be.  A matcher that never makes a k-NN call keeps its footprint.  Calls on
 * one matcher must be ordered, as for sift_hip_match_*.
 *
 * k-NN inside the window and the epipolar gate: the section "Gated k nearest
 * neighbours" after the batched gated calls below.  Gated k-NN forms on ready
 * code sets (a _codes_batched family over all-gathered codes) are not
 * provided. */
#define SIFT_HIP_KNN_MAX 8

/* One pair.  idx / d2: device, nq * k entries; either may be NULL.  Two
 * detector buffers with fresh sidecars match their codes directly (no prep
 * launch), subject to sift_hip_matcher_set_sidecars and
 * sift_hip_descriptors_written as sift_hip_match_device is. */
int sift_hip_match_knn_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt, int k,
                              int* idx, float* d2, void* stream);

/* P pairs (host arrays as sift_hip_match_batched); pair p's rows start at row
 * sum_{r<p} nq[r] of idx / d2. */
int sift_hip_match_knn_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                               const uint16_t* const* train, const int* nt, int k, int* idx, float* d2, void* stream);

/* The same for pairs of ready code sets (sift_hip_match_codes_batched's
 * arguments). */
int sift_hip_match_knn_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                     const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                     const int* tkey0, const int* nt, int k, int* idx, float* d2, void* stream);

/* Synchronous, one pair, the table to host memory (nq * k entries each; either
 * may be NULL). */
int sift_hip_match_knn_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt, int k,
                            int* idx_host, float* d2_host);

/* The list of one pair.  out: device, room for nq * k records; count: device
 * int. */
int sift_hip_match_knn_list_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                   int k, float max_distance, sift_hip_dmatch* out, int* count, void* stream);

/* P pairs: pair p's records start at row k * sum_{r<p} nq[r] of out (device,
 * k * sum nq rows) and carry imgIdx = p; counts: device, P ints. */
int sift_hip_match_knn_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                    const uint16_t* const* train, const int* nt, int k, float max_distance,
                                    sift_hip_dmatch* out, int* counts, void* stream);

/* Synchronous, one pair: copies min(count, cap) records to out_host and sets
 * *count to the full count. */
int sift_hip_match_knn_list_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                 int k, float max_distance, sift_hip_dmatch* out_host, int cap, int* count);

/* Train splits a k-NN call of this shape launches with on a matcher whose
 * scratch holds them (host-only, for tests and tools).  The gated k-NN calls
 * take the same launch shape and splits: this describes them too. */
int sift_hip_match_knn_plan(int nq, int nt, int pairs, int k, int* splits);

/* --- Guided matching: top-2 and match lists inside a search window ----------
 *
 * A tracker matches a point near its previous position, an SfM front end a
 * re-projected map point near where it should land (ORB-SLAM's search by
 * projection, SiftGPU's and COLMAP's guided match, the mask argument of
 * cv::DescriptorMatcher::knnMatch).  The best and second-best rows inside the
 * window are in general not the global top-2, so this cannot be derived from
 * sift_hip_match_device's output; here the window is a predicate inside the
 * matcher's top-2 fold and no nq x nt matrix ever exists.
 *
 * The rule.  A gate gives every row of both sets a position:
 *   query i at (qx, qy) = query_xy[i * query_stride + {0, 1}],
 *   train t at (tx, ty) = train_xy[t * train_stride + {0, 1}].
 * Train row t is a candidate of query i when
 *   fabsf(tx - qx) <= radius && fabsf(ty - qy) <= radius
 * evaluated in float32: one subtraction per axis and an inclusive compare (no
 * product, so no contraction can change it).  A NaN coordinate makes its row a
 * candidate of nothing; radius = +inf is no gate.  The predicate is symmetric
 * in the two rows, so the reverse direction of a cross check is the same gate
 * with the roles swapped.
 * The guided top-2 of query i is sift_hip_match_device's top-2 restricted to
 * i's candidates: the same squared distances, ties to the lower train index, an
 * absent neighbour -1 / FLT_MAX.  The `match` output's ratio test is unchanged:
 * a query with one candidate matches it, a query with none gets -1.
 * The guided match list is the match-list rule above with both top-2 arrays
 * replaced by the guided ones.
 *
 * Positions are device arrays of float rows; a stride of 3 passes a detector's
 * keypoint buffer ({x, y, layer} rows, sift_hip_results_device's kpts3) as it
 * is.  Exactly nq and nt rows are read.
 *
 * One pair per call.  Two detector descriptor buffers with fresh sidecars are
 * matched on their codes in one launch; any other pair is converted first (two
 * launches); a set with non-integer fp16 values takes the general path, as in
 * sift_hip_match_device.  P pairs in one call, on fp16 sets or on ready code
 * sets (the all-gathered buffers of a multi-GPU run), are the batched gated
 * calls below (sift_hip_match_guided_batched and its kin). */
typedef struct {
    const float* query_xy; /* device; query i's predicted position is query_xy[i*query_stride + {0,1}] */
    int query_stride;      /* floats per row, >= 2 (3 passes a detector's kpts3 buffer as it is) */
    const float* train_xy; /* device; the same for train rows */
    int train_stride;
    float radius;          /* pixels, > 0; +inf = no gate */
} sift_hip_match_gate;

/* sift_hip_match_device under a gate.  SIFT_HIP_ERR_INVALID, with nothing
 * launched, for: a null matcher or gate, a stride < 2, a radius that is not
 * > 0 (NaN included), a size over the matcher's limits, a null descriptor or
 * position pointer of a non-empty set.  nq == 0: nothing is written.  nt == 0:
 * every query gets -1 / FLT_MAX. */
int sift_hip_match_guided_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                 const sift_hip_match_gate* gate, float ratio, int ratio_on_squared, int* idx2,
                                 float* d2, int* match, void* stream);

/* The train splits S a guided call of this shape launches with (host-only, as
 * sift_hip_match_plan). */
int sift_hip_match_guided_plan(int nq, int nt, int* splits);

/* sift_hip_match_list_device under a gate: the forward guided top-2, with
 * cross_check or ratio_both_ways the reverse guided top-2 (the gate's roles
 * swapped), then the filter and the compaction.  Outputs, size limits and the
 * first call's scratch allocation as sift_hip_match_list_device. */
int sift_hip_match_list_guided_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                      int nt, const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* count, void* stream);

/* Synchronous, records to host memory, as sift_hip_match_list_host. */
int sift_hip_match_list_guided_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                    const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                    sift_hip_dmatch* out_host, int cap, int* count);

/* --- Guided matching under a fundamental matrix (the epipolar gate) -----------
 *
 * The gate of two-view geometry: COLMAP's and SiftGPU's guided match, ORB-SLAM's
 * SearchForTriangulation.  The caller knows F -- from the relative pose of two
 * keyframes, a calibrated stereo rig, or a first RANSAC pass over a match list
 * (sift_hip_verify_fundamental_device below) -- but not where on its epipolar line a point lands, so no predicted position
 * and no radius expresses it.  As with the window, the two nearest rows inside
 * the band are not the global top-2.  (Under a homography the gate is the
 * window above on projected query positions: sift_hip_verify_homography_device
 * finds H and sift_hip_project_homography_device projects, both below.)
 *
 * The rule.  F is 9 floats, row-major, with x_train^T F x_query = 0: the matrix
 * cv::findFundamentalMat(query_points, train_points) returns.  Positions are
 * read as for sift_hip_match_gate.  All arithmetic is float32, round to
 * nearest, in exactly this order, and no multiply-add is fused:
 *   per query (qx, qy):   a = (F[0]*qx + F[1]*qy) + F[2]
 *                         b = (F[3]*qx + F[4]*qy) + F[5]
 *                         c = (F[6]*qx + F[7]*qy) + F[8]
 *                         nq = a*a + b*b
 *   per train (tx, ty):   u = (F[0]*tx + F[3]*ty) + F[6]
 *                         v = (F[1]*tx + F[4]*ty) + F[7]
 *                         nr = u*u + v*v
 *   per pair:             r = (a*tx + b*ty) + c
 *                         e2 = max_error*max_error
 * Train row t is a candidate of query i when
 *   r*r <= e2 * (nq + nr)
 *   && fabsf(tx - qx) <= radius && fabsf(ty - qy) <= radius
 * -- the Sampson distance <= max_error, inclusive, inside the window (radius =
 * +inf: no window; a stereo or SLAM caller bounds the search along the line
 * with it).  A NaN anywhere makes a compare false, so its row is a candidate of
 * nothing; in the overflow and degenerate cases the formula is the rule.
 * sift_amd.cv.epipolar_mask is the same rule in numpy.
 *
 * The reverse direction of a cross check is the same formula with the roles
 * swapped and F transposed (the library transposes).  In real arithmetic the
 * predicate is symmetric; in float32 a pair within rounding of the threshold
 * may be a candidate in one direction only.  The list rule is unchanged: the
 * match-list filter on the two guided top-2 arrays.
 *
 * Everything else is as under sift_hip_match_gate: the same squared distances,
 * ties to the lower train index, an absent neighbour -1 / FLT_MAX, a query with
 * one candidate matches it, one pair per call, the same routes (sidecar codes,
 * or converted first; non-integer sets on the general path).  The launch shape
 * is the window gate's: sift_hip_match_guided_plan describes it. */
typedef struct {
    const float* query_xy; /* device; as sift_hip_match_gate */
    int query_stride;      /* floats per row, >= 2 */
    const float* train_xy;
    int train_stride;
    float radius;          /* pixels, > 0; +inf = no window */
    float F[9];            /* row-major; x_train^T F x_query = 0 */
    float max_error;       /* Sampson distance in pixels, > 0 and finite */
} sift_hip_match_epipolar_gate;

/* sift_hip_match_guided_device under the epipolar gate.  SIFT_HIP_ERR_INVALID,
 * with nothing launched, for: a null matcher or gate, a stride < 2, a radius
 * that is not > 0, a max_error that is not > 0 or not finite, a non-finite entry
 * of F or F all zero, a size over the matcher's limits, a null descriptor or
 * position pointer of a non-empty set.  Empty sets as in the guided calls. */
int sift_hip_match_epipolar_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                   const sift_hip_match_epipolar_gate* gate, float ratio, int ratio_on_squared,
                                   int* idx2, float* d2, int* match, void* stream);

/* sift_hip_match_list_guided_device / _host under the epipolar gate. */
int sift_hip_match_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                        int nt, const sift_hip_match_epipolar_gate* gate,
                                        const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* count,
                                        void* stream);
int sift_hip_match_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                      int nt, const sift_hip_match_epipolar_gate* gate,
                                      const sift_hip_match_filter* filter, sift_hip_dmatch* out_host, int cap,
                                      int* count);

/* --- Batched guided matching: both gates for all pairs of a batch -------------
 *
 * What sift_hip_match_batched / sift_hip_match_list_batched are to the
 * single-pair calls: P pairs under a gate in one pass on one stream, so that
 * match_list_batched -> verify_*_batched_device -> (project_homography_batched_
 * device ->) the guided rematch never returns to the host.  Per pair: its sets
 * and a position record; per call: both strides, the radius, and under the
 * epipolar gate max_error and the geometry -- P records of nine floats in
 * DEVICE memory, pair p's at geometry + p * geometry_stride_bytes (>= 36, a
 * multiple of 4).  geometry = the results of
 * sift_hip_verify_fundamental_batched_device with stride 52 takes those records
 * as they lie; the host never reads them.  P = 1 is the single-pair epipolar
 * call without the read-back of F.
 *
 * The rule.  Pair p of a batched gated call gives, byte for byte, the idx2 /
 * d2 / match rows, or the list records and count, of the single-pair call on
 * that pair under the gate {pair p's positions, the call's strides and radius,
 * F = pair p's nine floats, the call's max_error}.  Rows and records lie in
 * sift_hip_match_batched's / sift_hip_match_list_batched's layout: pair p's
 * start at sum_{r<p} nq[r], records carry imgIdx = p, counts[p] is a device
 * int, rows of `out` past a pair's count are not written.
 * The single-pair epipolar call refuses an unusable F on the host; a batched
 * call cannot see it, so on the device: a pair whose nine floats hold a value
 * that is not finite, or are all zero (the empty verify result, hypothesis =
 * -1), has no candidates -- every query of it gets -1 / -1, FLT_MAX / FLT_MAX
 * and match = -1, and its list count is 0.  (Without this rule a zero F would
 * make every row a candidate: 0 <= e2 * 0.)  sift_amd.cv.geometry_usable is the
 * same test in numpy.
 *
 * The fp16 forms always convert their sets first (distinct sets once, as
 * sift_hip_match_batched does for P > 1; sidecars are not used); a set with
 * non-integer values sends its pairs down the gated general path.  A launch
 * holds at most 32 pairs (kernel-argument space), so a call is
 * ceil(pairs / 32) match launches per pass: the forward and reverse pairs of a
 * list in one pass of 2P pairs when 2P <= max_pairs, otherwise in two of P.
 * The bytes do not depend on it.  The matcher's scratch is restored when a
 * call ends.
 *
 * SIFT_HIP_ERR_INVALID, with nothing launched, for: a stride < 2, a radius that
 * is not > 0, a max_error that is not > 0 or not finite, a null geometry, a
 * geometry stride below 36 or not a multiple of 4 (these need no matcher and
 * are looked at first); a null matcher; P outside 1..max_pairs or a null pair
 * array; a size over the matcher's limits (with a filter that needs the reverse
 * direction also nt <= max_query and nq <= max_train); a null descriptor or
 * position pointer of a non-empty set; the list calls' rules for filter, out
 * and counts. */
typedef struct {
    const float* query_xy; /* device; pair p's query positions, rows of query_stride floats */
    const float* train_xy; /* device; its train positions, rows of train_stride floats */
} sift_hip_match_positions;

/* sift_hip_match_batched under the window gate / the epipolar gate. */
int sift_hip_match_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                  const uint16_t* const* train, const int* nt,
                                  const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                  float radius, float ratio, int ratio_on_squared, int* idx2, float* d2, int* match,
                                  void* stream);
int sift_hip_match_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                    const uint16_t* const* train, const int* nt,
                                    const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                    float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                    float ratio, int ratio_on_squared, int* idx2, float* d2, int* match, void* stream);

/* sift_hip_match_list_batched under the two gates. */
int sift_hip_match_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                       const uint16_t* const* train, const int* nt,
                                       const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                       float radius, const sift_hip_match_filter* filter, sift_hip_dmatch* out,
                                       int* counts, void* stream);
int sift_hip_match_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                         const uint16_t* const* train, const int* nt,
                                         const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                         float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                         const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                         void* stream);

/* sift_hip_match_list_codes_batched under the two gates: pairs of ready code
 * sets (e.g. every rank's sidecars all-gathered), no conversion. */
int sift_hip_match_list_guided_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                             const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                             const int* tkey0, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const sift_hip_match_filter* filter,
                                             sift_hip_dmatch* out, int* counts, void* stream);
int sift_hip_match_list_epipolar_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                               const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                               const int* tkey0, const int* nt,
                                               const sift_hip_match_positions* positions, int query_stride,
                                               int train_stride, float radius, const void* geometry,
                                               int geometry_stride_bytes, float max_error,
                                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                               void* stream);

/* --- Gated k nearest neighbours: k-NN inside the window and the epipolar gate ---
 *
 * cv::DescriptorMatcher::knnMatch(query, train, k, mask).  On repetitive
 * structure the band around an epipolar line, or a window on a facade, still
 * holds several twins of the right match: the rematch under a verified F or H
 * keeps the k best candidates inside the gate for a second verify pass, for
 * voting or for a multi-view consistency test.  As with the top-2 gates, the k
 * nearest rows inside a gate are not the global k nearest, so this cannot be
 * filtered out of sift_hip_match_knn_device's output; here the gate is a
 * per-key predicate in the matcher's K-entry fold.
 *
 * The rule.  For a pair (Q: nq rows, T: nt rows), 1 <= k <= SIFT_HIP_KNN_MAX
 * and a gate, cand(i) is the set of train rows the gate admits for query i: the
 * window predicate of sift_hip_match_gate, or the epipolar predicate of
 * sift_hip_match_epipolar_gate, both unchanged (float32, the stated order of
 * operations, nothing fused, inclusive compares, a NaN is a candidate of
 * nothing).
 *   The table.  Row i of idx[nq][k] / d2[nq][k] holds the min(k, |cand(i)|)
 *   rows of cand(i) of smallest squared L2 distance to query i, in ascending
 *   (d2, train index) order -- a tie at any rank goes to the lower train index
 *   -- and -1 / FLT_MAX in the remaining entries.  Distances follow the ungated
 *   k-NN rule: exact integers as float32 on integer sets, the general-path
 *   contract otherwise.
 *   Consequences.  radius = +inf under the window gate gives
 *   sift_hip_match_knn_device's bytes, and so does the epipolar gate with
 *   max_error = 1e30 and no window.  k = 2 gives the idx2 / d2 bytes of
 *   sift_hip_match_guided_device / sift_hip_match_epipolar_device.  Column j of
 *   a call with k equals column j of a call with any k' > j.  The bytes do not
 *   depend on the launch plan, on the kernel instantiation that served the
 *   call, on max_pairs, or on whether the sets came as detector buffers
 *   (sidecar codes) or fp16 rows.
 *   The list is the k-NN list rule above (max_distance, (queryIdx, rank) order,
 *   slots from prefix sums) applied to the gated table.
 *   Batched.  Pair p gives, byte for byte, the single-pair call's table or list
 *   under {pair p's positions, the call's strides, radius and max_error, F =
 *   its nine floats read from device memory at geometry + p *
 *   geometry_stride_bytes}; the geometry follows sift_hip_match_epipolar_batched
 *   (stride >= 36 and a multiple of 4; 52 takes verifier records as they lie).
 *   An unusable record (a value that is not finite, or nine zeros) gives its
 *   pair no candidates: every entry -1 / FLT_MAX and a list count of 0.  Table
 *   rows lie at sum_{r<p} nq[r], list records at k * sum_{r<p} nq[r] with
 *   imgIdx = p; rows of `out` past a pair's count are not written.
 * k-NN has no reverse direction: there is no cross check and no transposed F.
 * Gated k-NN on ready code sets (_codes_batched) is not provided.
 *
 * Routes.  A single-pair call on two detector buffers with fresh sidecars
 * matches their codes directly (no prep launch), subject to
 * sift_hip_matcher_set_sidecars / sift_hip_descriptors_written as
 * sift_hip_match_knn_device is; any other pair is converted first.  The
 * batched forms always convert (distinct sets once).  A set with non-integer
 * values sends its pairs down the gated general path.  The single-pair epipolar
 * call checks F on the host and passes it as a kernel argument (no copy to the
 * device).  A launch holds at most 32 pairs; a call of more is several launches
 * ordered on the stream.  Scratch, splits and the first call's allocation are
 * those of the k-NN calls above (the first k-NN call of either kind allocates,
 * not under stream capture); every call restores the counters it used.
 *
 * Refusals (SIFT_HIP_ERR_INVALID, nothing launched, nothing written).  First
 * what needs no matcher: k outside 1..SIFT_HIP_KNN_MAX; for the list calls a
 * NaN max_distance; a null gate; a stride < 2; a radius that is not > 0; a
 * max_error that is not > 0 or not finite; an unusable host F; a null geometry;
 * a geometry stride below 36 or not a multiple of 4.  Then: a null matcher, a
 * size over the matcher's limits, P outside 1..max_pairs or a null pair array,
 * a null descriptor or position pointer of a non-empty set, the list calls'
 * null out or count.  nq == 0: nothing is written (a list's count is 0).
 * nt == 0: every entry is -1 / FLT_MAX and the count is 0.
 * sift_amd.cv.guided_knn / epipolar_knn / mask_knn are the rule in numpy. */
int sift_hip_match_knn_guided_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                     const sift_hip_match_gate* gate, int k, int* idx, float* d2, void* stream);
int sift_hip_match_knn_epipolar_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                       int nt, const sift_hip_match_epipolar_gate* gate, int k, int* idx, float* d2,
                                       void* stream);
int sift_hip_match_knn_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                      const uint16_t* const* train, const int* nt,
                                      const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                      float radius, int k, int* idx, float* d2, void* stream);
int sift_hip_match_knn_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                        const uint16_t* const* train, const int* nt,
                                        const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                        float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                        int k, int* idx, float* d2, void* stream);

/* The lists: out / count(s) as sift_hip_match_knn_list_device / _batched. */
int sift_hip_match_knn_list_guided_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                          int nt, const sift_hip_match_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out, int* count, void* stream);
int sift_hip_match_knn_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                            int nt, const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                            sift_hip_dmatch* out, int* count, void* stream);
int sift_hip_match_knn_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                           const uint16_t* const* train, const int* nt,
                                           const sift_hip_match_positions* positions, int query_stride,
                                           int train_stride, float radius, int k, float max_distance,
                                           sift_hip_dmatch* out, int* counts, void* stream);
int sift_hip_match_knn_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* query, const int* nq,
                                             const uint16_t* const* train, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const void* geometry,
                                             int geometry_stride_bytes, float max_error, int k, float max_distance,
                                             sift_hip_dmatch* out, int* counts, void* stream);

/* Synchronous, one pair, to host memory: the table (nq * k entries each; either
 * may be NULL) as sift_hip_match_knn_host, the list as
 * sift_hip_match_knn_list_host (min(count, cap) records, *count the full
 * count). */
int sift_hip_match_knn_guided_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                   const sift_hip_match_gate* gate, int k, int* idx_host, float* d2_host);
int sift_hip_match_knn_epipolar_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train, int nt,
                                     const sift_hip_match_epipolar_gate* gate, int k, int* idx_host, float* d2_host);
int sift_hip_match_knn_list_guided_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                        int nt, const sift_hip_match_gate* gate, int k, float max_distance,
                                        sift_hip_dmatch* out_host, int cap, int* count);
int sift_hip_match_knn_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* query, int nq, const uint16_t* train,
                                          int nt, const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out_host, int cap, int* count);

/* The launch plan a match call of this shape gets: train splits S per query
 * block (S > 1: split workgroups merge their top-2 through the scratch's
 * atomics) and waves per workgroup.  Host-only (no GPU call beyond reading the
 * CU count; 256 without a device), for tests and tools. */
int sift_hip_match_plan(int max_query, int max_train, int pairs, int* splits, int* waves);

/* --- The verifier's refusals ----------------------------------------------------
 *
 * Every verifier call that takes a match list (sift_hip_verify_*, sift_hip_score_*,
 * sift_hip_refine_*, sift_hip_recover_pose_* and sift_hip_recover_pose_homography_*,
 * single-pair and batched, device and host form) judges
 * its arguments in ONE order and reports the first rule broken, with nothing
 * launched and nothing written.  First what needs no look at the verifier:
 *   a null verifier; null pairs; a null params or result (the score calls: a
 *   null F / H or counts); P outside 1..64; a stride < 2; then pair by pair a cap
 *   outside 0..65536, a negative nq or nt, a null position pointer with cap > 0;
 *   null matches with a row to read; max_error not > 0 and finite; out
 *   overlapping matches (device forms); the refine calls' null mask, then rounds
 *   outside 1..8;
 *   the pose calls (from F and from H alike), which have no params or result
 *   among the first rules and no max_error, after the list rules (null
 *   matches): a null camera pointer; pair
 *   by pair, query camera first, fx or fy not > 0 and finite, then cx or cy not
 *   finite; a null params, result or pose; max_depth not > 0 (+inf is allowed, a
 *   NaN is refused); max_cos_parallax outside [-1, 1]; a null mask with a row to
 *   read; out overlapping matches (device forms);
 * then the verifier's limits: hypotheses outside 1..max_hypotheses, P over
 * max_pairs, the caps' sum (the cap) over max_matches.  A single-pair call is
 * judged as the batch of its one pair; a batched call names the pair in the
 * message of a per-pair rule. */

/* --- Two-view verification: RANSAC for the fundamental matrix ------------------
 *
 * The step between a putative match list and guided matching under F (COLMAP's
 * and SiftGPU's two-stage match; cv::findFundamentalMat(FM_RANSAC) plus its
 * inlier mask): a fixed budget of K hypotheses, each the normalised 8-point
 * solution of 8 sampled matches, each scored against every match by the
 * epipolar predicate above; the best one's F, its inlier mask and its inlier
 * records.  Everything runs on the caller's stream, the number of matches is
 * read from device memory (a call can follow sift_hip_match_list_device with no
 * host round trip), and the same bytes come out in every run.
 *
 * The rule.  All arithmetic is float32, every operation rounded to nearest, one
 * at a time, in the written order; nothing is fused; sums run in index order
 * ((x0 + x1) + x2 ...).  sift_amd.cv.ransac_fundamental is the same rule in
 * numpy.
 *
 * Input.  n = min(max(*count, 0), cap), or cap when count is NULL.  Match j is
 * (queryIdx, trainIdx) of record j; its positions (qx, qy), (tx, ty) are read
 * as for sift_hip_match_gate (stride >= 2, x and y first).  nq and nt are the
 * row counts of the position arrays: a record with queryIdx outside [0, nq) or
 * trainIdx outside [0, nt) is never read through -- its four coordinates count
 * as NaN, so it is an inlier of nothing and a hypothesis that samples it is
 * invalid.
 *
 * Sampling.  mix(h), on uint32 (lowbias32):
 *   h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
 * Hypothesis k (0 <= k < K) has base = mix(seed ^ mix(k)).  Draw j = 0..7:
 *   h = mix(base + 0x9e3779b9 * (j + 1))            (uint32, wrapping)
 *   r = (uint64(h) * (n - j)) >> 32
 *   for every earlier pick p, in ascending order of p: if r >= p: r++
 *   sample[j] = r
 * The 8 indices are distinct and the rule is total for every n >= 8; it is a
 * function of (seed, k, n) only.
 *
 * Solver.  For each side of the sample (the 8 query positions; the 8 train
 * positions), with (x_i, y_i) in sample order:
 *   mx = (sum x_i) / 8, my = (sum y_i) / 8
 *   dx_i = x_i - mx, dy_i = y_i - my, d_i = sqrtf(dx_i*dx_i + dy_i*dy_i)
 *   md = (sum d_i) / 8, s = 1.41421354f / md
 *   x'_i = dx_i * s, y'_i = dy_i * s, ox = -(s * mx), oy = -(s * my)
 * (sq, oqx, oqy) for the query side and (st, otx, oty) for the train side.
 * Row i of the 8 x 9 system A is, on the normalised coordinates,
 *   [tx*qx, tx*qy, tx, ty*qx, ty*qy, ty, qx, qy, 1].
 * Gaussian elimination with full pivoting, steps c = 0..7: the pivot is the
 * entry of largest fabsf among rows c..7 and columns c..8, found by a scan that
 * starts with (c, c), visits rows c..7 and inside a row columns c..8, and moves
 * to an entry only when its fabsf is strictly larger (ties go to the first in
 * row-major order; a NaN is never larger).  Rows c and the pivot's are swapped,
 * then columns c and the pivot's (in all rows; perm records the columns).  The
 * pivot p = A[c][c]; a zero or non-finite p makes the hypothesis invalid.  For
 * rows r = c+1..7: m = A[r][c] / p, and for columns j = c+1..8:
 *   A[r][j] = A[r][j] - m * A[c][j].
 * Back-substitution with the free variable y[8] = 1, i = 7..0:
 *   acc = A[i][i+1]*y[i+1]; for j = i+2..8: acc = acc + A[i][j]*y[j]
 *   y[i] = (-acc) / A[i][i]
 * The permutation is undone, g[perm[j]] = y[j] (perm[j]: the original column at
 * position j), G = g as 3 x 3 row-major, and F = Tt^T G Tq written out:
 *   H[r][0] = G[r][0]*sq, H[r][1] = G[r][1]*sq,
 *   H[r][2] = (G[r][0]*oqx + G[r][1]*oqy) + G[r][2]                  (r = 0..2)
 *   F[0][c] = st*H[0][c], F[1][c] = st*H[1][c],
 *   F[2][c] = (otx*H[0][c] + oty*H[1][c]) + H[2][c]                  (c = 0..2)
 * and scaled to unit Frobenius norm: ss = sum F[i]*F[i] over i = 0..8,
 * F[i] = F[i] / sqrtf(ss).  A non-finite entry of the result makes the
 * hypothesis invalid.  No rank-2 constraint is enforced (neither the Sampson
 * formula nor the epipolar gate needs one).  An invalid hypothesis has inlier
 * count 0 and F all zero.
 *
 * Score.  Match j is an inlier of a valid hypothesis when the epipolar
 * predicate above holds for its own pair under the hypothesis' F, with
 * e2 = max_error*max_error and radius = +inf (no window):
 * r*r <= e2 * (nq + nr), inclusive.  A NaN is an inlier of nothing.  An
 * overflow is no NaN: for a finite position so large that both sides of the
 * compare overflow (coordinates of about 1e18 and beyond) the compare reads
 * +inf <= +inf and holds, so such a record is an inlier of every hypothesis
 * that does not turn it into a NaN.  Positions are expected in pixels.
 *
 * Selection.  The valid hypothesis with the most inliers wins, ties to the
 * lowest k.  With n < 8 (no hypothesis is drawn: every sample index is -1) or
 * no valid hypothesis the result is hypothesis = -1, inliers = 0, F zero, an
 * empty list and a zero mask -- a status of success, not an error.
 *
 * Output.  The result record; optionally (each may be NULL) the inlier records
 * at out -- the input records, unchanged, in input order, room for cap --,
 * their number at out_count, and a byte mask of cap entries (mask[j] = 1 for an
 * inlier, 0 otherwise, also for j >= n).  out may not overlap the input. */
typedef struct sift_hip_verifier* sift_hip_verifier_t;

typedef struct {
    int hypotheses;   /* K, 1 .. the verifier's max_hypotheses */
    unsigned seed;
    float max_error;  /* pixels, > 0 and finite: Sampson distance (the homography calls: transfer error) */
} sift_hip_verify_params;

typedef struct {
    float F[9];            /* row-major; x_train^T F x_query = 0; zero when hypothesis = -1 */
    int inliers;           /* inliers of the winning hypothesis */
    int hypothesis;        /* its index k, -1: none */
    int matches;           /* n */
    int valid_hypotheses;  /* hypotheses that were solved */
} sift_hip_verify_result;  /* 52 bytes */

/* 1024 hypotheses, seed 0, max_error 1.5 px. */
void sift_hip_default_verify_params(sift_hip_verify_params* params);

/* A verifier owns all scratch of its calls (nothing is allocated later: every
 * device call below only launches kernels and may run under stream capture).
 * max_matches 1..65536, max_hypotheses 1..4096.  Calls on ONE verifier must be
 * ordered (same stream, or synchronised). */
int sift_hip_verifier_create(int device, int max_matches, int max_hypotheses, sift_hip_verifier_t* out);
int sift_hip_verifier_destroy(sift_hip_verifier_t v);

/* The operation, enqueued on `stream`, not synchronised.  matches, count,
 * positions, result, out, out_count, mask: device memory.  SIFT_HIP_ERR_INVALID,
 * with nothing launched, for: a null verifier, params or result; cap negative
 * or over the verifier's max_matches; hypotheses outside 1..max_hypotheses; a
 * max_error that is not > 0 and finite; a stride < 2; nq or nt negative; null
 * matches or positions with cap > 0; out overlapping matches.  cap == 0
 * succeeds with the empty result. */
int sift_hip_verify_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                       const float* query_xy, int query_stride, int nq, const float* train_xy,
                                       int train_stride, int nt, const sift_hip_verify_params* params,
                                       sift_hip_verify_result* result, sift_hip_dmatch* out, int* out_count,
                                       uint8_t* mask, void* stream);

/* Synchronous; matches, count and the positions still live on the device, the
 * result record, the result->inliers records (out_host: room for cap, may be
 * NULL) and the mask (mask_host: cap bytes, may be NULL) go to host memory. */
int sift_hip_verify_fundamental_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, const sift_hip_verify_params* params,
                                     sift_hip_verify_result* result_host, sift_hip_dmatch* out_host,
                                     uint8_t* mask_host);

/* The score alone, on the caller's own hypotheses (a 5-point solver with known
 * intrinsics, a pose prior): counts[k] (device, K ints) = the matches that are
 * inliers of F[9 k .. 9 k + 8] (device, K x 9) by the Score rule -- the formula
 * is the rule for every F (an all-NaN F counts nothing).  K and the other
 * arguments as above. */
int sift_hip_score_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,
                                      int train_stride, int nt, const float* F, int K, float max_error, int* counts,
                                      void* stream);

/* For tests and tools: what the last verify call on v drew, solved and counted
 * -- samples (K x 8), F (K x 9, zero rows: invalid hypotheses) and counts (K)
 * of its first min(cap, K) hypotheses to host memory (each may be NULL).
 * Synchronises the device.  SIFT_HIP_ERR_STATE before the first verify call. */
int sift_hip_verify_hypotheses_host(sift_hip_verifier_t v, int* samples, float* F, int* counts, int cap);

/* --- Homography verification: 4-point RANSAC and projection --------------------
 *
 * The model of planar targets, pure-rotation frames, panoramas and object
 * instances (cv::findHomography(query_points, train_points, RANSAC) plus its
 * inlier mask) -- the cases in which the fundamental matrix above is
 * degenerate.  The same fixed budget of K hypotheses on the same verifier, each
 * the normalised 4-point solution of 4 sampled matches, each scored against
 * every match by the forward transfer error; the best one's H, its inlier mask
 * and its inlier records.  sift_hip_project_homography_device then carries
 * positions over by an H it reads from device memory -- the result record itself
 * -- so match_list_device -> verify_homography_device ->
 * project_homography_device -> match_list_guided_device runs on one stream with
 * no read-back at all.
 *
 * The rule.  x_train ~ H x_query, H row-major h[0..8].  The conventions are the
 * fundamental rule's: float32, every operation rounded to nearest, one at a
 * time, in the written order; nothing fused; division and square root correctly
 * rounded; sums in index order.  sift_amd.cv.ransac_homography is the same rule
 * in numpy.
 *
 * Input.  As above: n, the positions of match j, and the four NaNs of a record
 * with an index outside [0, nq) / [0, nt).
 *
 * Sampling.  The sampler above with 4 draws in place of 8: j = 0..3, the same
 * base, h and r, the same skip of earlier picks.  Total for every n >= 4; with
 * n < 4 nothing is drawn and every sample index is -1.
 *
 * Orientation test, on the raw sample coordinates (x_i, y_i), before any
 * normalisation.  For the triples (i, j, k) = (0,1,2), (0,1,3), (0,2,3),
 * (1,2,3) and each side:
 *   a = (x_j - x_i) * (y_k - y_i) - (y_j - y_i) * (x_k - x_i)
 * and p = a_query * a_train.  The sample is kept only when all four p > 0 or
 * all four p < 0; a zero (three collinear points on either side) or a NaN fails
 * both and makes the hypothesis invalid (OpenCV's sample check).
 *
 * Solver.  Each side is normalised as above with 8 replaced by 4 (mx, my, d_i,
 * md, s = 1.41421354f / md, x' = dx * s, ox = -(s * mx), oy = -(s * my)):
 * (sq, oqx, oqy) for the query side, (st, mtx, mty) -- the scale and the mean --
 * for the train side.  With the normalised (x, y) / (u, v) of pair i, rows 2i
 * and 2i+1 of the 8 x 9 system A are
 *   [x, y, 1, 0, 0, 0, -(u*x), -(u*y), -u]
 *   [0, 0, 0, x, y, 1, -(v*x), -(v*y), -v]
 * Then word for word as above: Gaussian elimination with full pivoting (the same
 * scan order, tie rule, NaN rule and invalid-pivot rule, on all 8 x 9 stored
 * entries, the structural zeros included), back-substitution with the free
 * variable y[8] = 1, the permutation undone: G.  H = Tt^-1 G Tq written out:
 *   M[r][0] = G[r][0]*sq, M[r][1] = G[r][1]*sq,
 *   M[r][2] = (G[r][0]*oqx + G[r][1]*oqy) + G[r][2]                  (r = 0..2)
 *   H[0][c] = M[0][c] / st + mtx * M[2][c],
 *   H[1][c] = M[1][c] / st + mty * M[2][c],  H[2][c] = M[2][c]       (c = 0..2)
 * scaled to unit Frobenius norm (ss = sum H[i]*H[i] over i = 0..8 in index
 * order, H[i] = H[i] / sqrtf(ss)).  Then w0 = (h6*qx0 + h7*qy0) + h8 for sample
 * 0's raw query position; if w0 < 0 every entry of H is negated.  The hypothesis
 * is invalid when any entry is non-finite or w0 == 0, and -- the own-sample
 * rule -- when one of its own four pairs fails the score's predicate below
 * under H and the call's max_error: where the horizon of H (w = 0) passes next
 * to a sample's query position, the float32 rounding of px and py divided by w
 * is worth pixels and no float32 H reproduces that pair (samples that hold an
 * unrelated pair do this about once in 300).  So every valid hypothesis counts
 * at least its own 4 matches.  An invalid hypothesis has
 * H all zero and inlier count 0.  There is no refit on the inliers and no
 * h8 = 1 scaling: divide by H[8] for OpenCV's convention;
 * sift_amd.cv.homography_lstsq refits on the host.
 *
 * Score.  Match (qx, qy, tx, ty) is an inlier of a valid hypothesis when
 *   px = (h0*qx + h1*qy) + h2;  py = (h3*qx + h4*qy) + h5;  w = (h6*qx + h7*qy) + h8
 *   dx = px - tx*w;  dy = py - ty*w
 *   w > 0  &&  dx*dx + dy*dy <= (max_error*max_error) * (w*w)
 * -- the forward transfer error (OpenCV's reprojection error) <= max_error,
 * inclusive, division-free, with the chirality test the sign rule makes
 * meaningful.  A NaN is an inlier of nothing; an overflow of both sides to
 * +inf is an inlier, as for the fundamental matrix.
 *
 * Selection and output.  As above: most inliers among the valid hypotheses,
 * ties to the lowest k; with n < 4 or no valid hypothesis hypothesis = -1,
 * inliers = 0, H zero, an empty list and a zero mask, status success; the
 * 52-byte record, the records in input order, their count, the cap-byte mask;
 * no atomics, the same bytes in every run.
 *
 * Projection.  Row i of xy (xy[i*stride + {0, 1}]) gives px, py, w as in the
 * score; the output row is (px / w, py / w) when w > 0 and (NaN, NaN) otherwise
 * (w <= 0 or NaN).  The window gate treats a NaN position as a candidate of
 * nothing, so a zero H -- the empty result -- yields an empty guided list.  Only
 * the first two floats of an output row are written. */
typedef struct {
    float H[9];            /* row-major; x_train ~ H x_query, unit norm; zero when hypothesis = -1 */
    int inliers;           /* inliers of the winning hypothesis */
    int hypothesis;        /* its index k, -1: none */
    int matches;           /* n */
    int valid_hypotheses;  /* hypotheses that passed the orientation test and were solved */
} sift_hip_homography_result;  /* 52 bytes */

/* sift_hip_verify_fundamental_device / _host / sift_hip_score_fundamental_device
 * for the homography, argument for argument, on the same verifier (one model at
 * a time: calls on one verifier are ordered); params->max_error is the transfer
 * error in pixels.  The same arguments are refused, with nothing launched, and
 * cap == 0 succeeds with the empty result. */
int sift_hip_verify_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,
                                      int train_stride, int nt, const sift_hip_verify_params* params,
                                      sift_hip_homography_result* result, sift_hip_dmatch* out, int* out_count,
                                      uint8_t* mask, void* stream);
int sift_hip_verify_homography_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                    const float* query_xy, int query_stride, int nq, const float* train_xy,
                                    int train_stride, int nt, const sift_hip_verify_params* params,
                                    sift_hip_homography_result* result_host, sift_hip_dmatch* out_host,
                                    uint8_t* mask_host);
int sift_hip_score_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, const float* H, int K, float max_error, int* counts,
                                     void* stream);

/* sift_hip_verify_hypotheses_host for the homography: samples (K x 4), H
 * (K x 9, zero rows: invalid hypotheses) and counts (K).  A verifier remembers
 * the model of its last verify call: each of the two getters returns
 * SIFT_HIP_ERR_STATE unless that call was of its own model (and before any). */
int sift_hip_verify_homography_hypotheses_host(sift_hip_verifier_t v, int* samples, float* H, int* counts, int cap);

/* The projection, enqueued on `stream` of the current device, not synchronised;
 * needs no handle.  H: 9 floats in device memory, normally the result record of
 * sift_hip_verify_homography_device on the same stream (H is its first field).
 * xy: n device rows of `stride` floats, x and y first; out_xy: n device rows of
 * out_stride floats.  out_xy may be xy itself with equal strides (in place);
 * otherwise the two may not overlap.  SIFT_HIP_ERR_INVALID, with nothing
 * launched, for: a null H, a stride below 2, a negative n, a null xy or out_xy
 * with n > 0, a partial overlap.  n == 0 succeeds. */
int sift_hip_project_homography_device(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride,
                                       void* stream);

/* P projections in one launch: set p goes through the 9 floats at
 * geometry + p * geometry_stride_bytes (device memory; stride 52 takes the
 * records of sift_hip_verify_homography_batched_device as they lie) and gives,
 * byte for byte, what the single call gives on {that H, sets[p]}.  `sets` is a
 * host array of P records; the strides are the call's.  SIFT_HIP_ERR_INVALID,
 * with nothing launched, for: a null geometry or sets, a geometry stride below
 * 36 or not a multiple of 4, P outside 1..64, a stride below 2, and per set
 * the single call's rules (n == 0 is an empty set). */
typedef struct {
    const float* xy; /* device; n rows of `stride` floats */
    int n;
    float* out_xy;   /* device; n rows of `out_stride` floats; may be xy with equal strides */
} sift_hip_project_set;
int sift_hip_project_homography_batched_device(const void* geometry, int geometry_stride_bytes, int P,
                                               const sift_hip_project_set* sets, int stride, int out_stride,
                                               void* stream);

/* --- Batched verification: every pair of a match batch in one pass --------------
 *
 * What sift_hip_match_list_batched is to sift_hip_match_list_device: P lists
 * verified by one gather, one hypotheses, one score and one select launch, on
 * the caller's stream, so the chain match_list_batched -> verify_*_batched_device
 * runs with no read-back for the whole batch.
 *
 * The rule.  Pair p of a batched call gives, byte for byte, the result record,
 * mask, out records and out_count of the single-pair call above on that pair's
 * list and positions with the same hypotheses and max_error and the seed
 * params->seed + p (uint32, wrapping): sift_amd.cv.ransac_fundamental /
 * ransac_homography (matches_p, q_xy_p, t_xy_p, max_error, K, seed + p).
 *
 * Layout.  A host array of P pair records.  query_xy / train_xy: the pair's
 * device position rows, nq / nt their row counts; cap: the pair's number of
 * rows in matches, out and mask.  Pair p's rows start at row0[p] = the sum of
 * cap[r] over r < p in all three arrays -- with cap[p] = nq[p] exactly what
 * sift_hip_match_list_batched wrote.  counts: P device ints, pair p counts
 * n = min(max(counts[p], 0), cap[p]) records (NULL: all cap[p]).  results: P
 * device records of 52 bytes; out_counts: P device ints.  query_stride and
 * train_stride hold for every pair.  A pair with cap = 0, or with fewer than 8
 * (homography: 4) matches, gives the empty result (hypothesis = -1, matches = n,
 * out_count = 0), as the single call does. */
typedef struct {
    const float* query_xy;
    const float* train_xy;
    int nq, nt;
    int cap;
} sift_hip_verify_pair;

/* A verifier for batched calls (and for the single-pair calls above, which it
 * serves as any other): max_pairs 1..64 pairs per call, max_matches
 * 1..64 x 65536 rows over all the pairs of a call (a single-pair call's cap is
 * bounded by it and by 65536), max_hypotheses 1..4096 per pair.  It owns, from
 * creation on, the gathered points of max_matches rows and the samples, models,
 * valid flags and counts of max_pairs x max_hypotheses hypotheses.
 * sift_hip_verifier_create gives max_pairs = 1. */
int sift_hip_verifier_create_batched(int device, int max_matches, int max_hypotheses, int max_pairs,
                                     sift_hip_verifier_t* out);

/* Enqueued on `stream`, not synchronised; matches, counts, positions, results,
 * out, out_counts, mask: device memory; pairs: host memory, read before the
 * call returns.  out, out_counts and mask may each be NULL.  All cap[p] mask
 * bytes of every pair are written; out rows past a pair's inlier count are not
 * touched.  SIFT_HIP_ERR_INVALID, with nothing launched, for: a null verifier,
 * pairs, params or results; P < 1 or over the verifier's max_pairs; a cap[p]
 * outside 0..65536; the caps' sum over the verifier's max_matches; a negative
 * nq or nt; a stride < 2; a null position pointer on a pair with cap > 0; null
 * matches with a caps' sum > 0; hypotheses outside 1..max_hypotheses; a
 * max_error that is not > 0 and finite; out overlapping matches. */
int sift_hip_verify_fundamental_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                               int P, const sift_hip_verify_pair* pairs, int query_stride,
                                               int train_stride, const sift_hip_verify_params* params,
                                               sift_hip_verify_result* results, sift_hip_dmatch* out, int* out_counts,
                                               uint8_t* mask, void* stream);
int sift_hip_verify_homography_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                              int P, const sift_hip_verify_pair* pairs, int query_stride,
                                              int train_stride, const sift_hip_verify_params* params,
                                              sift_hip_homography_result* results, sift_hip_dmatch* out, int* out_counts,
                                              uint8_t* mask, void* stream);

/* Synchronous; matches, counts and the positions still live on the device.  P
 * result records, pair p's results[p].inliers records at row0[p] of out_host
 * (room for the caps' sum, may be NULL; rows past a pair's inliers are not
 * written) and the masks (mask_host: the caps' sum bytes, may be NULL) go to
 * host memory. */
int sift_hip_verify_fundamental_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                             int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                             const sift_hip_verify_params* params, sift_hip_verify_result* results_host,
                                             sift_hip_dmatch* out_host, uint8_t* mask_host);
int sift_hip_verify_homography_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                            int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                            const sift_hip_verify_params* params,
                                            sift_hip_homography_result* results_host, sift_hip_dmatch* out_host,
                                            uint8_t* mask_host);
/* After a batched call sift_hip_verify_hypotheses_host and
 * sift_hip_verify_homography_hypotheses_host return SIFT_HIP_ERR_STATE (the
 * scratch holds P pairs' hypotheses) until a single-pair verify call has run. */

/* --- Refit of the verified model: least-squares F and H on the inliers ----------
 *
 * A verify call returns the winning minimal-sample model (8 points for F, 4 for
 * H).  A refine call refits that model on its inliers, on the device, rescores
 * it with the verifier's own predicate and keeps it when it counts at least as
 * many records: the local-optimisation step of LO-RANSAC, and the algebraic
 * least-squares fit cv::findFundamentalMat / cv::findHomography end with (no
 * Levenberg-Marquardt polish).  Its result records, mask and out lists have the
 * layouts the guided matchers and the projection read.  The numpy mirror
 * sift_amd.cv.refit_fundamental / refit_homography (one fit) and
 * refine_fundamental / refine_homography (the operation) is the specification:
 * the device equals it byte for byte.
 *
 * The rule.  One round, for a list of n records, the current result record and
 * its mask:
 *   1. Fit set: the records j < n with mask[j] != 0 whose four gathered
 *      coordinates (qx, qy, tx, ty; NaN for an index outside its position
 *      array) are finite; m their number, j0 the first.  A masked record with a
 *      NaN coordinate is skipped.  m < 8 (H: 4): the refit is invalid.
 *   2. Arithmetic: IEEE float64 throughout, nothing fused, correctly rounded
 *      division and square root.  Coordinates convert float32 -> float64
 *      exactly; the nine results are rounded to float32 once, at the end.
 *   3. Summation order, for every sum below: record j belongs to slot j mod 256;
 *      a slot adds its fit records to +0 in ascending j (a record with two rows
 *      adds the even row's term, then the odd row's); the 64 slots of each group
 *      [64 g, 64 g + 64), g = 0..3, combine by a halving tree (slot i += slot
 *      i + d for d = 32, 16, .. 1, i mod 64 < d); the total is
 *      (g0 + g1) + (g2 + g3).  It depends on j alone, not on a launch shape.
 *   4. Hartley normalisation of each side: mean = sum / m per coordinate;
 *      md = (sum of sqrt(dx dx + dy dy)) / m with dx = x - mean_x;
 *      s = 1.4142135623730951 / md; x' = dx s.  s not finite on either side
 *      (all points equal): invalid.
 *   5. Normal matrix M = A^T A, its 45 upper-triangle sums of a_r a_c, over the
 *      rows the minimal solvers use, in normalised coordinates (q' = (x, y),
 *      t' = (u, v)).  F, one row per record: (u x, u y, u, v x, v y, v, x, y, 1).
 *      H, two rows: (x, y, 1, 0, 0, 0, -(u x), -(u y), -u) and
 *      (0, 0, 0, x, y, 1, -(v x), -(v y), -v); a product with a structural zero
 *      adds nothing.
 *   6. Smallest eigenvector of M by cyclic Jacobi: V = I; 8 sweeps.  A sweep
 *      of an m x m matrix (m = 9, and 3 in step 7) visits the pivots in
 *      round-robin order: round r = 0 .. m - 1 holds the pivots
 *      ((r + i) mod m, (r - i) mod m), i = 1 .. (m - 1) / 2, each taken as
 *      (p, q) with p < q.  Every index pair occurs once per sweep, and the
 *      pivots of a round are disjoint (index r rests), so a device may apply a
 *      round's rotations side by side: the only entries two of them share are
 *      updated by the earlier pivot first, which is this sequential order.  A
 *      pivot with M[p][q] exactly 0 is skipped.  With a = M[p][q]:
 *        theta = (M[q][q] - M[p][p]) / (2 a);
 *        t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0;
 *        c = 1 / sqrt(t t + 1);  s = t c;
 *        k != p, q: M[k][p] = M[p][k] = c M[k][p] - s M[k][q] and
 *                   M[k][q] = M[q][k] = s M[k][p] + c M[k][q] (old values);
 *        M[p][p] -= t a;  M[q][q] += t a;  M[p][q] = M[q][p] = 0;
 *        every k:   V[k][p] = c V[k][p] - s V[k][q] and
 *                   V[k][q] = s V[k][p] + c V[k][q] (old values).
 *      g = the column of V whose diagonal entry of M is the smallest (ties to
 *      the lowest index), G = g as 3 x 3 row-major.  The sweep count: on every
 *      test case 6 sweeps already give the float32 output of 8, and a 9th
 *      changes none (tests/test_refit_cases.py checks 8 against 9).
 *   7. F only, rank 2, in normalised coordinates: N = G^T G with
 *      N[r][c] = (G[0][r] G[0][c] + G[1][r] G[1][c]) + G[2][r] G[2][c]; v its
 *      eigenvector of the smallest eigenvalue by the same routine (3 x 3, 8
 *      sweeps); w[r] = (G[r][0] v[0] + G[r][1] v[1]) + G[r][2] v[2];
 *      G[r][c] -= w[r] v[c].
 *   8. Denormalise with the minimal solvers' formulas in float64 (ox = -(s mean_x)):
 *      T = G Tq, then F = Tt^T T, or H = Tt^-1 T.  Scale to unit Frobenius norm
 *      (squares summed in index order, each entry divided by the root).  H only:
 *      w0 = (H[6] qx + H[7] qy) + H[8] at record j0's raw coordinates; w0 < 0
 *      negates H; w0 = 0 is invalid.  Round to float32; a non-finite entry is
 *      invalid.  An invalid refit is all zero.
 *   9. Rescore the refit over all n records with the model's predicate (the
 *      Sampson / transfer test of the verify rule, float32, same max_error).
 *      Accept when the refit is valid and passes at least result.inliers
 *      records: the record's model and inliers, and mask[0, n), become the
 *      refit's.  Otherwise everything stays as it was.  hypothesis, matches and
 *      valid_hypotheses never change.
 * `rounds` (1..8) repeats this; each round fits on the mask the one before left.
 * A rejected round leaves the state unchanged, so every later round rejects too.
 * A current record that is empty (hypothesis < 0) or whose nine floats are not
 * all finite and not all zero stays as it is.  After the last round `out` holds
 * the records j < n with mask[j] != 0 in input order and out_count their number
 * (rows past them are not written); `accepted` receives the number of accepted
 * rounds.
 *
 * Consequences.  The inlier count never decreases.  The output is a function of
 * the inputs alone: the same bytes in every run, and in the single and batched
 * forms (pair p of a batched call equals the single call on that pair).
 *
 * Device forms: enqueued on `stream`, not synchronised, no allocation (all
 * scratch is the verifier's), capturable.  The list, count(s), cap(s) and
 * positions are the matching verify call's; result(s) and mask are in-out device
 * memory (mask: cap bytes, the caps' sum for a batch; bytes at and past n are
 * neither read nor written); out, out_count(s) and accepted may each be NULL.
 * SIFT_HIP_ERR_INVALID, with nothing launched, for what the matching verify call
 * refuses on the same arguments (hypotheses aside) and for: a null result; a
 * null mask with cap (a batch: the caps' sum) > 0; rounds outside 1..8.
 * Host forms: synchronous; the list and positions still live on the device,
 * result(s) and mask are in-out host memory, out_host / out_count(s)_host /
 * accepted_host (each nullable) receive host copies. */
int sift_hip_refine_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                       const float* query_xy, int query_stride, int nq, const float* train_xy,
                                       int train_stride, int nt, float max_error, int rounds,
                                       sift_hip_verify_result* result, uint8_t* mask, sift_hip_dmatch* out,
                                       int* out_count, int* accepted, void* stream);
int sift_hip_refine_fundamental_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, float max_error, int rounds,
                                     sift_hip_verify_result* result_host, uint8_t* mask_host, sift_hip_dmatch* out_host,
                                     int* out_count_host, int* accepted_host);
int sift_hip_refine_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,
                                      int train_stride, int nt, float max_error, int rounds,
                                      sift_hip_homography_result* result, uint8_t* mask, sift_hip_dmatch* out,
                                      int* out_count, int* accepted, void* stream);
int sift_hip_refine_homography_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                    const float* query_xy, int query_stride, int nq, const float* train_xy,
                                    int train_stride, int nt, float max_error, int rounds,
                                    sift_hip_homography_result* result_host, uint8_t* mask_host,
                                    sift_hip_dmatch* out_host, int* out_count_host, int* accepted_host);
/* The batched forms: results, out_counts and accepted hold P entries, mask and
 * out the caps' sum rows, laid out as in the batched verify calls. */
int sift_hip_refine_fundamental_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                               int P, const sift_hip_verify_pair* pairs, int query_stride,
                                               int train_stride, float max_error, int rounds,
                                               sift_hip_verify_result* results, uint8_t* mask, sift_hip_dmatch* out,
                                               int* out_counts, int* accepted, void* stream);
int sift_hip_refine_fundamental_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                             int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                             float max_error, int rounds, sift_hip_verify_result* results_host,
                                             uint8_t* mask_host, sift_hip_dmatch* out_host, int* out_counts_host,
                                             int* accepted_host);
int sift_hip_refine_homography_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                              int P, const sift_hip_verify_pair* pairs, int query_stride,
                                              int train_stride, float max_error, int rounds,
                                              sift_hip_homography_result* results, uint8_t* mask, sift_hip_dmatch* out,
                                              int* out_counts, int* accepted, void* stream);
int sift_hip_refine_homography_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                            int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                            float max_error, int rounds, sift_hip_homography_result* results_host,
                                            uint8_t* mask_host, sift_hip_dmatch* out_host, int* out_counts_host,
                                            int* accepted_host);

/* --- Affine and similarity verification: 3- and 2-point RANSAC ------------------
 *
 * The models of motions that are a 2-D affine map (6 degrees of freedom:
 * cv::estimateAffine2D) or a similarity (4: cv::estimateAffinePartial2D) --
 * video stabilisation, aerial and satellite strips, scanned sheets, microscope
 * mosaics, a fronto-parallel object instance, a tracker's frame-to-frame motion.
 * The same fixed budget of K hypotheses on the same verifier, but a sample is 3
 * or 2 matches instead of 4, and the chance that a sample is clean falls with
 * the power of its size: at 20 % planted pairs a 2-point sample is clean once in
 * 25 draws, a 3-point sample once in 125, a 4-point sample once in 625.  One
 * call argument, `model`, selects between the two.
 *
 * The result is stored as the 3 x 3 matrix [a b tx; c d ty; 0 0 1] in the
 * homography's 52-byte record (sift_hip_affine_result is that type), so
 * everything downstream of a homography -- sift_hip_project_homography_device,
 * its batched form, the window-gated matchers on projected positions -- takes it
 * as it lies.
 *
 * The rule.  x_train = A x_query + t.  The conventions are the verifier's:
 * float32, every operation rounded to nearest, one at a time, in the written
 * order; nothing fused; division correctly rounded.  The refit is float64 in one
 * written association.  sift_amd.cv.ransac_affine / refine_affine is the same
 * rule in numpy; the device equals it byte for byte.
 *
 * Input.  As for the other models: n, the positions (qx, qy, tx, ty) of match j,
 * and the four NaNs of a record with an index outside [0, nq) / [0, nt).
 *
 * Sampling.  The sampler of the fundamental rule with m = 3 draws (affine) or
 * m = 2 (similarity): j = 0..m-1, the same base, h and r, the same skip of
 * earlier picks.  With n < m nothing is drawn and every sample index is -1.
 *
 * Affine from 3, on the raw sample coordinates (q_i, t_i the query and train
 * position of sample i).  d1 = q1 - q0, d2 = q2 - q0, e1 = t1 - t0, e2 = t2 - t0.
 *   det = d1x*d2y - d1y*d2x;  dett = e1x*e2y - e1y*e2x;  p = det * dett
 * The sample is degenerate when p is neither > 0 nor < 0: a collinear triple on
 * either side, a repeated position, or a NaN.  A negative p -- a reflection --
 * is allowed, as in OpenCV.
 *   a = (e1x*d2y - e2x*d1y) / det;  b = (e2x*d1x - e1x*d2x) / det
 *   c = (e1y*d2y - e2y*d1y) / det;  d = (e2y*d1x - e1y*d2x) / det
 *   tx = t0x - (a*q0x + b*q0y);     ty = t0y - (c*q0x + d*q0y)
 *
 * Similarity from 2.  dq = q1 - q0, dt = t1 - t0.
 *   den = dqx*dqx + dqy*dqy;  dent = dtx*dtx + dty*dty
 * The sample is degenerate unless den > 0 and dent > 0.
 *   a = (dqx*dtx + dqy*dty) / den;  b = (dqx*dty - dqy*dtx) / den
 * The matrix is [a, -b, tx; b, a, ty] with
 *   tx = t0x - (a*q0x - b*q0y);     ty = t0y - (b*q0x + a*q0y)
 * (the negation is exact, and x - y is x + (-y): one formula serves both models).
 *
 * Model record.  Nine floats {m0, m1, m2, m3, m4, m5, 0, 0, 1}; the last row is
 * exact and there is no unit-norm scaling.  A hypothesis is invalid when its
 * sample is degenerate or one of m0..m5 is not finite; its row is then all zero
 * (the 1 included) and its count 0.  There is no own-sample rule.
 *
 * Score.  Match (qx, qy, tx, ty) is an inlier of a valid hypothesis when
 *   px = (m0*qx + m1*qy) + m2;  py = (m3*qx + m4*qy) + m5
 *   dx = px - tx;  dy = py - ty
 *   dx*dx + dy*dy <= max_error*max_error
 * inclusive; a NaN is an inlier of nothing.  This is the homography's predicate
 * on the same nine floats (its w is exactly 1 for every finite position), so
 * the record is interchangeable with a homography record, and
 * sift_hip_score_affine_device needs no model argument.
 *
 * Selection and output.  Word for word the other models': most inliers among the
 * valid hypotheses, ties to the lowest k; with n < m or no valid hypothesis
 * hypothesis = -1, inliers = 0, a zero model, an empty list and a zero mask,
 * status success; the 52-byte record, the records in input order, their count,
 * the cap-byte mask; no atomics, the same bytes in every run.
 *
 * Refit (sift_hip_refine_affine_*).  One round refits the model on the records
 * the mask marks: the refit rule's fit set (step 1, with m >= 3 for the affine
 * map and m >= 2 for the similarity), arithmetic (step 2) and summation order
 * (step 3), then
 *   pass 1: m and the means mqx, mqy, mtx, mty (each sum / m);
 *   pass 2: with x = qx - mqx, y = qy - mqy, u = tx - mtx, v = ty - mty the seven
 *     sums Sxx = sum x x, Sxy = sum x y, Syy = sum y y, Txx = sum u x,
 *     Txy = sum u y, Tyx = sum v x, Tyy = sum v y;
 *   affine: det = Sxx*Syy - Sxy*Sxy must be finite and > 0;
 *     a = (Txx*Syy - Txy*Sxy) / det;  b = (Txy*Sxx - Txx*Sxy) / det
 *     c = (Tyx*Syy - Tyy*Sxy) / det;  d = (Tyy*Sxx - Tyx*Sxy) / det
 *   similarity: den = Sxx + Syy must be finite and > 0;
 *     a = (Txx + Tyy) / den;  c = (Tyx - Txy) / den;  b = -c;  d = a
 *   translation: tx = mtx - (a*mqx + b*mqy);  ty = mty - (c*mqx + d*mqy)
 * rounded to float32 once, over the row 0 0 1; a non-finite entry is invalid.
 * There is no normalisation and no Jacobi: the problem is linear and centred.
 * The accept step is the refit rule's step 9 with the predicate above, `rounds`
 * is 1..8, and a rejected round changes no byte. */
#define SIFT_HIP_MODEL_AFFINE 0      /* 6 degrees of freedom, 3-point samples */
#define SIFT_HIP_MODEL_SIMILARITY 1  /* 4 degrees of freedom, 2-point samples */

/* The homography's record, reused: H holds {m0 .. m5, 0, 0, 1}, and
 * valid_hypotheses counts the samples that were not degenerate. */
typedef sift_hip_homography_result sift_hip_affine_result;

/* The homography calls, argument for argument, with `model` behind the handle.
 * The same arguments are refused, with nothing launched, and so is a model that
 * is neither constant above; cap == 0 succeeds with the empty result. */
int sift_hip_verify_affine_device(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches, const int* count,
                                  int cap, const float* query_xy, int query_stride, int nq, const float* train_xy,
                                  int train_stride, int nt, const sift_hip_verify_params* params,
                                  sift_hip_affine_result* result, sift_hip_dmatch* out, int* out_count, uint8_t* mask,
                                  void* stream);
int sift_hip_verify_affine_host(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches, const int* count,
                                int cap, const float* query_xy, int query_stride, int nq, const float* train_xy,
                                int train_stride, int nt, const sift_hip_verify_params* params,
                                sift_hip_affine_result* result_host, sift_hip_dmatch* out_host, uint8_t* mask_host);
/* The score alone on the caller's K models (K x 9 floats, rows 0 0 1 last); the
 * predicate is both models' own, so there is no model argument. */
int sift_hip_score_affine_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                 const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride,
                                 int nt, const float* A, int K, float max_error, int* counts, void* stream);
/* samples (K x 3 for the affine map, K x 2 for the similarity), A (K x 9, zero
 * rows: invalid hypotheses) and counts (K).  SIFT_HIP_ERR_STATE unless the
 * verifier's last verify call was a single-pair call of this very model; the
 * two getters above refuse after an affine call in the same way. */
int sift_hip_verify_affine_hypotheses_host(sift_hip_verifier_t v, int model, int* samples, float* A, int* counts,
                                           int cap);
int sift_hip_verify_affine_batched_device(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches,
                                          const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride,
                                          int train_stride, const sift_hip_verify_params* params,
                                          sift_hip_affine_result* results, sift_hip_dmatch* out, int* out_counts,
                                          uint8_t* mask, void* stream);
int sift_hip_verify_affine_batched_host(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches,
                                        const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride,
                                        int train_stride, const sift_hip_verify_params* params,
                                        sift_hip_affine_result* results_host, sift_hip_dmatch* out_host,
                                        uint8_t* mask_host);
int sift_hip_refine_affine_device(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches, const int* count,
                                  int cap, const float* query_xy, int query_stride, int nq, const float* train_xy,
                                  int train_stride, int nt, float max_error, int rounds, sift_hip_affine_result* result,
                                  uint8_t* mask, sift_hip_dmatch* out, int* out_count, int* accepted, void* stream);
int sift_hip_refine_affine_host(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches, const int* count,
                                int cap, const float* query_xy, int query_stride, int nq, const float* train_xy,
                                int train_stride, int nt, float max_error, int rounds,
                                sift_hip_affine_result* result_host, uint8_t* mask_host, sift_hip_dmatch* out_host,
                                int* out_count_host, int* accepted_host);
int sift_hip_refine_affine_batched_device(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches,
                                          const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride,
                                          int train_stride, float max_error, int rounds, sift_hip_affine_result* results,
                                          uint8_t* mask, sift_hip_dmatch* out, int* out_counts, int* accepted,
                                          void* stream);
int sift_hip_refine_affine_batched_host(sift_hip_verifier_t v, int model, const sift_hip_dmatch* matches,
                                        const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride,
                                        int train_stride, float max_error, int rounds,
                                        sift_hip_affine_result* results_host, uint8_t* mask_host,
                                        sift_hip_dmatch* out_host, int* out_counts_host, int* accepted_host);

/* --- Relative pose from a verified fundamental matrix ---------------------------
 *
 * What a calibrated caller does with a verified F (cv::recoverPose, ORB-SLAM's
 * ReconstructF): E = Kt^T F Kq, its four (R, t) candidates, the inliers
 * triangulated under each, and the candidate that puts them in front of both
 * cameras.  A pose call does this on the device from what a verify or refine
 * call left there -- the list, the 52-byte result record, the mask -- on the
 * caller's stream, with no read-back.  The numpy mirror
 * sift_amd.cv.essential_from_fundamental / decompose_essential /
 * triangulate_depths (the steps) and recover_pose (the operation) is the
 * specification: the device equals it byte for byte.
 *
 * Arithmetic.  IEEE float64 throughout, nothing fused, correctly rounded division
 * and square root, every sum and product in the association written below.
 * float32 inputs (F, the cameras, the positions, the two thresholds) convert
 * exactly; the outputs are rounded to float32 once, at the end.  No cos() is
 * evaluated anywhere.
 *
 * Inputs.  The list, count, cap, positions, strides, nq and nt, read exactly as
 * the refine calls read them (n, the gathered coordinates qx, qy, tx, ty, NaN
 * for an index outside its position array).  The current result record in device
 * memory, whose first nine floats are F with x_train^T F x_query = 0.  The mask.
 * Two pinhole cameras (fx, fy, cx, cy), query side and train side, and the
 * thresholds max_depth and max_cos_parallax, from host memory.
 *
 * The rule.
 *   1. Usable record: hypothesis >= 0 and nine floats that are finite and not all
 *      zero (the refit's test).  Otherwise the result is empty.
 *   2. E = Kt^T F Kq for skew-free K, row r and column c from 0:
 *        G[r][0] = F[r][0] fxq;  G[r][1] = F[r][1] fyq;
 *        G[r][2] = (F[r][0] cxq + F[r][1] cyq) + F[r][2];
 *        E[0][c] = fxt G[0][c];  E[1][c] = fyt G[1][c];
 *        E[2][c] = (cxt G[0][c] + cyt G[1][c]) + G[2][c].
 *   3. N = E^T E with N[r][c] = (E[0][r] E[0][c] + E[1][r] E[1][c]) + E[2][r] E[2][c].
 *      Its eigen-decomposition by the refit's Jacobi routine (step 6 there: 3 x 3,
 *      V = I, 8 sweeps, the same pivot order).  i1 = the index of the largest
 *      diagonal entry, i2 of the largest of the other two, ties to the lower index
 *      both times; w1, w2 those entries, v1, v2 those columns of V.
 *      s1 = sqrt(w1), s2 = sqrt(w2); s2 not finite or not > 0 (rank <= 1): the
 *      result is empty.  v3 = v1 x v2;
 *      u1[r] = ((E[r][0] v1[0] + E[r][1] v1[1]) + E[r][2] v1[2]) / s1, u2 likewise
 *      with v2 and s2; u3 = u1 x u2, where (a x b)[0] = a[1] b[2] - a[2] b[1],
 *      [1] = a[2] b[0] - a[0] b[2], [2] = a[0] b[1] - a[1] b[0].  U = (u1 u2 u3)
 *      and V = (v1 v2 v3) are proper by construction.
 *   4. Candidates.  With W = [[0,-1,0],[1,0,0],[0,0,1]], R1 = U W V^T and
 *      R2 = U W^T V^T; W only permutes and negates columns, so
 *        R1[r][c] = (u2[r] v1[c] - u1[r] v2[c]) + u3[r] v3[c],
 *        R2[r][c] = (u1[r] v2[c] - u2[r] v1[c]) + u3[r] v3[c];  t = u3.
 *      In cv::recoverPose's order: 0 = (R1, t), 1 = (R2, t), 2 = (R1, -t),
 *      3 = (R2, -t).  The query camera is [I | 0], the train camera [R | t]:
 *      X_train = R X_query + t, and |t| = 1 up to rounding.
 *   5. Fit set: the records j < n with mask[j] != 0 whose four gathered
 *      coordinates are finite (the refit's set); m their number.
 *   6. Per fit record and candidate (R, t):
 *        xq = ((qx - cxq) / fxq, (qy - cyq) / fyq), xt = ((tx - cxt) / fxt,
 *        (ty - cyt) / fyt), the rays being (xq, 1) and (xt, 1);
 *        p[r] = (R[r][0] xq[0] + R[r][1] xq[1]) + R[r][2];
 *        pp = (p[0] p[0] + p[1] p[1]) + p[2] p[2];
 *        xx = (xt[0] xt[0] + xt[1] xt[1]) + 1;
 *        px = (p[0] xt[0] + p[1] xt[1]) + p[2];
 *        pt = (p[0] t[0] + p[1] t[1]) + p[2] t[2];
 *        xt_t = (xt[0] t[0] + xt[1] t[1]) + t[2];
 *        det = pp xx - px px;
 *        a = (px xt_t - pt xx) / det;  b = (pp xt_t - px pt) / det
 *      -- the depths (a in the query camera, b in the train camera) that minimise
 *      |a p + t - b (xt, 1)|^2, from its 2 x 2 normal equations.  (Negating t
 *      negates pt and xt_t and with them a and b, exactly.)  The record is IN
 *      FRONT when det > 0, a > 0, b > 0, a < max_depth and b < max_depth; a NaN
 *      fails every test.  It has PARALLAX when it is in front and
 *      px / sqrt(pp xx) < max_cos_parallax.
 *   7. Winner: the candidate with the most records in front, ties to the lowest
 *      index.  A winning count of 0 gives the empty result.
 *   8. Outputs.  The pose record: R (row-major) and t of the winner, rounded to
 *      float32; in_front and with_parallax, its two counts; counts[4], the records
 *      in front under each candidate; candidate, its index; fit = m.  mask_out
 *      (cap bytes): 1 for a fit record in front under the winner, else 0, also for
 *      the rows in [n, cap).  points (cap x 3 float32): row j < n is (a xq[0],
 *      a xq[1], a) rounded to float32 -- the point in the query camera's frame, in
 *      units of the baseline -- for a record in front under the winner, and three
 *      times the quiet NaN 0x7FC00000 otherwise; rows >= n are not written.  out:
 *      the records in front in input order, out_count their number (rows past them
 *      are not written).
 * The empty result: R and t zero, in_front, with_parallax and counts[] 0,
 * candidate = -1, fit still m, mask_out all zero, every points row j < n NaN, an
 * empty list.  It is a success, not an error, as a verify call's n < 8 is.
 *
 * Thresholds.  max_depth = 50 is cv::recoverPose's distanceThresh, in baselines
 * (+inf: no far bound); max_cos_parallax = 0.99998 is ORB-SLAM's bar: with_parallax
 * counts the records whose rays meet at more than about 0.36 degrees, which tells
 * a pose with a usable baseline from a near-pure rotation.
 *
 * Consequences.  The output is a function of the inputs alone: the same bytes in
 * every run, and in the single and batched forms (pair p of a batched call equals
 * the single call on that pair with cam_query[p] and cam_train[p]).  -F gives the
 * same pose through the candidate with R1 and R2 swapped. */
typedef struct {
    float fx, fy, cx, cy;
} sift_hip_camera;

typedef struct {
    float max_depth;        /* > 0, +inf allowed; default 50 */
    float max_cos_parallax; /* in [-1, 1]; default 0.99998 */
} sift_hip_pose_params;

void sift_hip_default_pose_params(sift_hip_pose_params* p);

typedef struct {
    float R[9]; /* row-major, X_train = R X_query + t */
    float t[3]; /* |t| = 1 */
    int in_front;
    int with_parallax;
    int counts[4];
    int candidate; /* 0..3, -1: the empty result */
    int fit;
} sift_hip_pose_result;
#ifdef __cplusplus
static_assert(sizeof(sift_hip_pose_result) == 80, "sift_hip_pose_result is 80 bytes");
#else
typedef char sift_hip_pose_result_is_80_bytes[sizeof(sift_hip_pose_result) == 80 ? 1 : -1];
#endif

/* Device form: two launches after the gather, enqueued on `stream`, not
 * synchronised, no allocation (the candidates' scratch is the verifier's),
 * capturable.  The list, count, cap and positions are the verify call's; result
 * and mask (device memory) are what it or a refine call wrote and are only read.
 * cam_query, cam_train and params: host memory, read before the call returns.
 * pose: device memory.  mask_out (cap bytes), points (cap x 3 floats), out (cap
 * records) and out_count may each be NULL; mask_out may be the mask itself (the
 * same address: the mask then becomes the in-front mask; any other overlap of the
 * two is not allowed).  The verifier's hypothesis scratch is not touched: what
 * sift_hip_verify_hypotheses_host answers stays.  SIFT_HIP_ERR_INVALID, with
 * nothing launched and nothing written, by the rules and in the order of "The
 * verifier's refusals".
 * Host form: synchronous; the list, count and positions still live on the device;
 * result_host and mask_host are host memory, pose_host, mask_out_host,
 * points_host, out_host and out_count_host (the last four nullable) receive host
 * copies: mask_out_host all cap bytes, points_host the rows j < n, out_host the
 * out_count records. */
int sift_hip_recover_pose_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                 const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride,
                                 int nt, const sift_hip_verify_result* result, const uint8_t* mask,
                                 const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                 const sift_hip_pose_params* params, sift_hip_pose_result* pose, uint8_t* mask_out,
                                 float* points, sift_hip_dmatch* out, int* out_count, void* stream);
int sift_hip_recover_pose_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                               const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride,
                               int nt, const sift_hip_verify_result* result_host, const uint8_t* mask_host,
                               const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                               const sift_hip_pose_params* params, sift_hip_pose_result* pose_host, uint8_t* mask_out_host,
                               float* points_host, sift_hip_dmatch* out_host, int* out_count_host);
/* The batched forms: results, poses and out_counts hold P entries, cam_query and
 * cam_train P cameras each (host memory); mask, mask_out and out hold the caps'
 * sum rows and points three floats per row, laid out as in the batched verify
 * calls.  A verifier serves up to its max_pairs pairs per call. */
int sift_hip_recover_pose_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts, int P,
                                         const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                         const sift_hip_verify_result* results, const uint8_t* mask,
                                         const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                         const sift_hip_pose_params* params, sift_hip_pose_result* poses, uint8_t* mask_out,
                                         float* points, sift_hip_dmatch* out, int* out_counts, void* stream);
int sift_hip_recover_pose_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts, int P,
                                       const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                       const sift_hip_verify_result* results_host, const uint8_t* mask_host,
                                       const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                       const sift_hip_pose_params* params, sift_hip_pose_result* poses_host,
                                       uint8_t* mask_out_host, float* points_host, sift_hip_dmatch* out_host,
                                       int* out_counts_host);

/* --- Relative pose from a verified homography -----------------------------------
 *
 * What a calibrated caller does with a verified H of a plane
 * (cv::decomposeHomographyMat and cv::filterHomographyDecompByVisibleRefpoints,
 * ORB-SLAM's ReconstructH): A = Kt^-1 H Kq = s (R + t n^T / d), its four
 * (R, t, n, d) candidates, the inliers triangulated under each, and the candidate
 * that puts them in front of both cameras.  These are the cases in which the pose
 * from F is degenerate: planar targets, floors and facades, low parallax.  A plane
 * pose call does it on the device from what a homography verify or refine call
 * left there, on the caller's stream, with no read-back.  The numpy mirror
 * sift_amd.cv.calibrated_homography / decompose_homography / triangulate_depths
 * (the steps) and recover_pose_homography (the operation) is the specification:
 * the device equals it byte for byte.
 *
 * Arithmetic and inputs: as for "Relative pose from a verified fundamental
 * matrix" above, with the record's first nine floats read as H (x_train ~ H
 * x_query).  The decomposition is the one of Ma, Soatto, Kosecka, Sastry, "An
 * Invitation to 3-D Vision", 5.3.3: it needs the eigen-decomposition of a
 * symmetric 3 x 3 matrix and nothing else.
 *
 * The rule.
 *   1. Usable record: hypothesis >= 0 and nine floats that are finite and not all
 *      zero (the refit's test).  Otherwise the result is empty.
 *   2. A = Kt^-1 H Kq for skew-free K, row r and column c from 0:
 *        G[r][0] = H[r][0] fxq;  G[r][1] = H[r][1] fyq;
 *        G[r][2] = (H[r][0] cxq + H[r][1] cyq) + H[r][2];
 *        A[0][c] = (G[0][c] - cxt G[2][c]) / fxt;
 *        A[1][c] = (G[1][c] - cyt G[2][c]) / fyt;  A[2][c] = G[2][c].
 *      H is used with the sign it has.  The verify and refine calls sign H so that
 *      every record they count has w = (H[2][0] qx + H[2][1] qy) + H[2][2] > 0, and
 *      the third row of A applied to the normalised query ray is that same w.
 *   3. S = A^T A with S[r][c] = (A[0][r] A[0][c] + A[1][r] A[1][c]) + A[2][r] A[2][c].
 *      Its eigen-decomposition by the refit's Jacobi routine (3 x 3, V = I, 8
 *      sweeps, the same pivot order).  i1 = the index of the largest diagonal
 *      entry, i2 of the largest of the other two, ties to the lower index both
 *      times, i3 the remaining one; w1 >= w2 >= w3 those entries, v1, v2 the
 *      columns i1, i2 of V, v3 = v1 x v2 (the cross product as written above).
 *      The result is empty when w2 is not finite or not > 0 (rank <= 1), or when
 *      w1 - w3 is not > 0.  No other threshold is set.
 *   4. Hn[r][c] = A[r][c] / sqrt(w2).  With max0(x) = x when x > 0, else 0:
 *        a = sqrt(max0(w2 - w3) / (w1 - w3));  b = sqrt(max0(w1 - w2) / (w1 - w3));
 *        u+[k] = a v1[k] + b v3[k];  u-[k] = a v1[k] - b v3[k].
 *      (The formulas are scale-free in w: nothing is renormalised first.)
 *   5. Per u (u+ gives R+, t+, N+, d+; u- gives R-, t-, N-, d-):
 *        N = v2 x u;
 *        hv[r] = (Hn[r][0] v2[0] + Hn[r][1] v2[1]) + Hn[r][2] v2[2];
 *        hu[r] = (Hn[r][0] u[0] + Hn[r][1] u[1]) + Hn[r][2] u[2];  hc = hv x hu;
 *        R[r][c] = (hv[r] v2[c] + hu[r] u[c]) + hc[r] N[c]
 *      -- R = W U^T with U = (v2, u, N) and W = (Hn v2, Hn u, Hn v2 x Hn u) --;
 *        T[r] = ((Hn[r][0] - R[r][0]) N[0] + (Hn[r][1] - R[r][1]) N[1])
 *               + (Hn[r][2] - R[r][2]) N[2];
 *        |T| = sqrt((T[0] T[0] + T[1] T[1]) + T[2] T[2]);
 *      the result is empty when either |T| is not finite or not > 0;
 *        t = T / |T|;  d = 1 / |T|,
 *      the plane's distance from the query camera in baselines:
 *      Hn = R + (t / d) N^T.
 *   6. Candidates, in this order: 0 = (R+, t+, N+, d+), 1 = (R-, t-, N-, d-),
 *      2 = (R+, -t+, -N+, d+), 3 = (R-, -t-, -N-, d-).  X_train = R X_query + t,
 *      |t| = 1 and |n| = 1 up to rounding, n^T X_query = d on the plane.
 *   7. Fit set: the records j < n with mask[j] != 0 whose four gathered coordinates
 *      are finite (the refit's set) and whose w (step 2, in float64 from the
 *      float32 entries and positions) is > 0; fit their number.  It is counted
 *      from the record's floats as they are, also when the record is not usable.
 *      A wrongly signed H therefore gives fit = 0 and the empty result, visibly.
 *   8. Depths, the IN FRONT test and the PARALLAX test: step 6 of the rule for F,
 *      word for word, per fit record and candidate (R, t).  Negating t negates
 *      both depths exactly, so the four candidates cost two evaluations.
 *   9. Winner: the candidate with the most records in front, ties to the lowest
 *      index.  A winning count of 0 gives the empty result.
 *  10. Outputs.  The plane pose record: the pose record of the rule for F, filled
 *      the same way, then normal and distance of the winner, rounded to float32.
 *      mask_out, points, out and out_count: as for F.  candidates (4 records per
 *      pair, nullable): R, t, normal, distance of the candidates 0..3 rounded to
 *      float32, written whenever steps 1 to 5 gave a decomposition -- also when no
 *      record is in front -- and all zero otherwise.
 * The empty result: the pose record as for F (zero, candidate = -1, fit still
 * counted), normal and distance zero, mask_out all zero, every points row j < n
 * NaN, an empty list.  It is a success, not an error.
 *
 * A TIE IS NOT AN ACCIDENT HERE.  A plane seen from two views has, in general,
 * two physically valid decompositions: both put every point in front of both
 * cameras.  ORB-SLAM gives up in that case and OpenCV returns both.  This call
 * reports and does not hide: counts[4] shows two equal top counts, the winner is
 * the first of them (the rule above, not a judgement), and candidates holds all
 * four.  The caller decides with a prior on the normal, a third view, or
 * ORB-SLAM's bar (the second count below 0.75 of the first).
 *
 * A near-pure rotation (|t| much smaller than d) leaves w1, w2 and w3 equal up to
 * rounding.  When w1 - w3 rounds to 0 the result is empty; otherwise R is still
 * the rotation, distance is very large (of order 1e7) and t and normal are
 * directions of rounding noise.  The call sets no threshold for this: distance
 * and with_parallax tell.
 *
 * Consequences.  The output is a function of the inputs alone: the same bytes in
 * every run, and in the single and batched forms. */
typedef struct {
    float R[9]; /* the first 80 bytes: a sift_hip_pose_result as it lies */
    float t[3];
    int in_front;
    int with_parallax;
    int counts[4];
    int candidate; /* 0..3, -1: the empty result */
    int fit;
    float normal[3]; /* the plane n^T X_query = distance, |n| = 1 */
    float distance;  /* in baselines */
} sift_hip_plane_pose_result;

typedef struct {
    float R[9];
    float t[3];
    float normal[3];
    float distance;
} sift_hip_plane_candidate;
#ifdef __cplusplus
static_assert(sizeof(sift_hip_plane_pose_result) == 96, "sift_hip_plane_pose_result is 96 bytes");
static_assert(sizeof(sift_hip_plane_candidate) == 64, "sift_hip_plane_candidate is 64 bytes");
#else
typedef char sift_hip_plane_pose_result_is_96_bytes[sizeof(sift_hip_plane_pose_result) == 96 ? 1 : -1];
typedef char sift_hip_plane_candidate_is_64_bytes[sizeof(sift_hip_plane_candidate) == 64 ? 1 : -1];
#endif

/* Argument for argument the pose calls above, with the homography's record, the
 * plane pose record and the trailing nullable candidates (device form: device
 * memory, 4 records; host form: host memory; batched: 4 P records, pair p's at
 * 4 p).  Device forms: two launches after the gather, no allocation, not
 * synchronised, capturable, the hypothesis scratch untouched; refusals by the
 * rules and in the order of "The verifier's refusals", with nothing launched and
 * nothing written. */
int sift_hip_recover_pose_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count,
                                            int cap, const float* query_xy, int query_stride, int nq,
                                            const float* train_xy, int train_stride, int nt,
                                            const sift_hip_homography_result* result, const uint8_t* mask,
                                            const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                            const sift_hip_pose_params* params, sift_hip_plane_pose_result* pose,
                                            uint8_t* mask_out, float* points, sift_hip_dmatch* out, int* out_count,
                                            sift_hip_plane_candidate* candidates, void* stream);
int sift_hip_recover_pose_homography_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                          const float* query_xy, int query_stride, int nq, const float* train_xy,
                                          int train_stride, int nt, const sift_hip_homography_result* result_host,
                                          const uint8_t* mask_host, const sift_hip_camera* cam_query,
                                          const sift_hip_camera* cam_train, const sift_hip_pose_params* params,
                                          sift_hip_plane_pose_result* pose_host, uint8_t* mask_out_host,
                                          float* points_host, sift_hip_dmatch* out_host, int* out_count_host,
                                          sift_hip_plane_candidate* candidates_host);
int sift_hip_recover_pose_homography_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches,
                                                    const int* counts, int P, const sift_hip_verify_pair* pairs,
                                                    int query_stride, int train_stride,
                                                    const sift_hip_homography_result* results, const uint8_t* mask,
                                                    const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                                    const sift_hip_pose_params* params,
                                                    sift_hip_plane_pose_result* poses, uint8_t* mask_out, float* points,
                                                    sift_hip_dmatch* out, int* out_counts,
                                                    sift_hip_plane_candidate* candidates, void* stream);
int sift_hip_recover_pose_homography_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                                  int P, const sift_hip_verify_pair* pairs, int query_stride,
                                                  int train_stride, const sift_hip_homography_result* results_host,
                                                  const uint8_t* mask_host, const sift_hip_camera* cam_query,
                                                  const sift_hip_camera* cam_train, const sift_hip_pose_params* params,
                                                  sift_hip_plane_pose_result* poses_host, uint8_t* mask_out_host,
                                                  float* points_host, sift_hip_dmatch* out_host, int* out_counts_host,
                                                  sift_hip_plane_candidate* candidates_host);

/* --- Essential-matrix verification: 5-point RANSAC -------------------------------
 *
 * The model of a calibrated pair (cv::findEssentialMat, the call OpenCV documents
 * in front of cv::recoverPose).  The same fixed budget of K samples, but a sample
 * is 5 matches instead of 8 -- at 30 % true pairs a 5-point sample is clean once
 * in about 400 draws, an 8-point sample once in about 15,000 -- and the solver is
 * not degenerate on a dominant plane with some structure off it.  The cameras
 * are the pose calls' sift_hip_camera, host memory, one per side (one per pair
 * and side in the batched form), under the pose calls' rules.
 *
 * A sample has up to ten solutions, so it owns ten model slots: slot 10 k + r is
 * root r of sample k.  Every slot holds a pixel-space fundamental matrix
 * F = Kt^-T E Kq^-1, so max_error stays in pixels, the score and the selection
 * are the fundamental rule's over the 10 K slots, and the record is a
 * sift_hip_verify_result that sift_hip_recover_pose_*, sift_hip_refine_fundamental_*
 * and the epipolar matchers take as it lies.
 *
 * The rule.  float64 from the rays to the unit-norm F, every operation rounded to
 * nearest, one at a time, in the written association; nothing fused; division and
 * square root correctly rounded and no other function; no iteration whose length
 * depends on the data.  sift_amd.cv.ransac_essential is the same rule in numpy;
 * the device equals it byte for byte.
 *
 * Input and sampling.  As for the other models; the sampler of the fundamental
 * rule with m = 5 draws.  With n < 5 nothing is drawn, every sample index is -1
 * and every slot is invalid.
 *
 * Rays.  With the cameras' float32 values widened to float64, for sample i
 *   qx = (qx - cxq) / fxq;  qy = (qy - cyq) / fyq;  likewise tx, ty under cam_train.
 *
 * Null space.  Row i of the 5 x 9 system is the 8-point system's row
 *   (tx*qx, tx*qy, tx, ty*qx, ty*qy, ty, qx, qy, 1).
 * Gauss-Jordan with full pivoting: at step c = 0..4 the pivot is the largest
 * |entry| of rows >= c and columns >= c, the scan starting at (c, c) in row-major
 * order and moving on a strictly larger value only (solve_8x9's rule); rows c and
 * pr are exchanged, then columns c and pc (and the permutation); a pivot that is
 * zero or not finite: no model from this sample; then for every row r != c
 *   m = A[r][c] / p;  A[r][j] = A[r][j] - m * A[c][j],  j > c.
 * The basis vector of free position 5 + f (f = 0..3) is y[5 + f] = 1, the other
 * free positions 0, y[i] = (-A[i][5 + f]) / A[i][i] for i < 5, with the column
 * permutation undone.  f = 0..3 are X, Y, Z, W (row-major 3 x 3); no SVD, no
 * orthonormalisation.
 *
 * Constraints.  E = x X + y Y + z Z + W: entry i is the linear polynomial
 * (X[i], Y[i], Z[i], W[i]) over the variables 0 = x, 1 = y, 2 = z, 3 = 1.  A
 * product of two linear polynomials a, b is the quadratic c over the pairs u <= v
 * in lexicographic order: c = 0, then for u = 0..3, v = 0..3 in that order
 *   c[pair(u, v)] = c[pair(u, v)] + a[u] * b[v].
 * A quadratic a times a linear b is the cubic c, likewise from zero over the
 * quadratic's index m = 0..9 and v = 0..3, stored in Nister's column order
 *   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
 * Sums and differences of polynomials are coefficient by coefficient.  The ten
 * rows of the 10 x 20 matrix:
 *   row 0 (det E):  (m0 E00 - m1 E01) + m2 E02  with  m0 = E11 E22 - E12 E21,
 *     m1 = E10 E22 - E12 E20,  m2 = E10 E21 - E11 E20;
 *   G = E E^T:  G[i][j] = (Ei0 Ej0 + Ei1 Ej1) + Ei2 Ej2 for i <= j, G[j][i] = G[i][j];
 *   h = 0.5 * ((G00 + G11) + G22);  L = G with h subtracted on the diagonal;
 *   row 1 + 3 i + j:  (Li0 E0j + Li1 E1j) + Li2 E2j
 * -- the nine entries of (E E^T - tr(E E^T) / 2) E, half of 2 E E^T E - tr(E E^T) E.
 * Gauss-Jordan on the first ten columns with row pivoting: at step c = 0..9 the
 * pivot is the largest |entry| of column c in rows >= c, the scan starting at row
 * c and moving on a strictly larger value only; the same exchange, pivot test
 * and elimination of every other row over the columns j > c.  Rows 4..9 (x^2z,
 * x^2, y^2z, y^2, xyz, xy) then give, with u = row 4 + 2 i and v = row 5 + 2 i,
 * each right-hand entry divided by its row's pivot, row i = u - z v of the 3 x 3
 * polynomial matrix B(z) over (x, y, 1), coefficients ascending in z:
 *   Bi0 = (u[12], u[11] - v[12], u[10] - v[11], -v[10])
 *   Bi1 = (u[15], u[14] - v[15], u[13] - v[14], -v[13])
 *   Bi2 = (u[19], u[18] - v[19], u[17] - v[18], u[16] - v[17], -v[16]).
 * A product of polynomials in z is c = 0, then c[i + j] = c[i + j] + a[i] * b[j]
 * for i over a, j over b.  The degree-10 polynomial is
 *   p = ((B11 B22 - B12 B21) B00 - (B10 B22 - B12 B20) B01) + (B10 B21 - B11 B20) B02
 * with every product in the written order of its factors.
 *
 * Real roots, by the derivative chain.  A p whose p_10 is zero, or with a
 * coefficient that is not finite: no model from this sample.  Each derivative's
 * coefficient is the previous one's times its exponent.  A polynomial c of degree
 * d is evaluated by Horner's rule, acc = c[d], then acc = acc * z + c[k]
 * downwards; at z = +inf its value is c[d] and at z = -inf c[d], negated for an
 * odd d (only the sign is used).  The real line is searched through
 * s = z / (1 + |z|) in [-1, 1], z(s) = s / (1 - |s|): bisection in s needs no
 * root bound and resolves a root of any magnitude to the same relative width.
 * For d = 1..10, with c the derivative of degree d (d = 10: p itself) and the
 * nodes -inf (s = -1), the d - 1 results of level d - 1, +inf (s = 1): bracket
 * i = 0..d-1 is (lo, hi] = (node i, node i + 1] and holds a root when
 * (c(lo) < 0 and c(hi) >= 0) or (c(lo) > 0 and c(hi) <= 0).  Then
 *   a = s(lo), b = s(hi); 48 times: mid = 0.5 * (a + b); when c(z(mid)) has
 *     c(lo)'s strict sign a = mid, else b = mid;
 *   z = z(0.5 * (a + b)), za = z(a), zb = z(b); 3 times: zn = z - c(z) / c'(z),
 *     kept when za <= zn <= zb;
 * and the bracket's result is z, with s = z / (1 + |z|) held into [a, b]; a
 * bracket without a root hands lo on, so the nodes stay sorted and every later
 * bracket is still one on which c is monotonic.  The roots of p are the results
 * of the brackets of level 10 that held one, in bracket order, which is
 * ascending.  No Sturm chain, no companion matrix, no convergence test.
 *
 * Back-substitution.  For root z with b_rc = B_rc(z), on the row pair (u, v) of
 * (0, 1), (0, 2), (1, 2) with the largest |d|, the first on a tie:
 *   d = bu0*bv1 - bu1*bv0;  x = (bu1*bv2 - bu2*bv1) / d;  y = (bu2*bv0 - bu0*bv2) / d
 *   E[i] = ((x*X[i] + y*Y[i]) + z*Z[i]) + W[i]
 *   M = E Kq^-1:  M[r][0] = E[r][0] / fxq;  M[r][1] = E[r][1] / fyq;
 *                 M[r][2] = E[r][2] - (M[r][0]*cxq + M[r][1]*cyq)
 *   F = Kt^-T M:  F[0][c] = M[0][c] / fxt;  F[1][c] = M[1][c] / fyt;
 *                 F[2][c] = M[2][c] - (F[0][c]*cxt + F[1][c]*cyt)
 * scaled to unit Frobenius norm (the squares summed in index order) and rounded
 * to float32.  The r-th root found goes to slot 10 k + r; a root whose F is not
 * finite keeps its slot, zero and invalid; slots past the last root, and every
 * slot of a sample without a model, are zero and invalid.
 *
 * Score, selection and output.  The fundamental rule's over the 10 K slots:
 * `hypothesis` is the winning slot 10 k + r (sample k = hypothesis / 10),
 * valid_hypotheses the number of valid slots, ties go to the lowest slot; n < 5
 * gives the empty result, status success.
 *
 * Scratch.  A verifier serves essential calls after
 * sift_hip_verifier_reserve_essential(v, max_samples), 1 <= max_samples <= 4096,
 * which allocates the samples and the 10-slot model, flag and count arrays for
 * the verifier's max_pairs, once (a second call is SIFT_HIP_ERR_STATE; not
 * capturable).  After it an essential call allocates nothing and is capturable
 * like the rest.  An essential call on a verifier that has not reserved, or with
 * params->hypotheses above the reservation, is SIFT_HIP_ERR_STATE with nothing
 * written; params->hypotheses counts samples and is not bound by the verifier's
 * max_hypotheses.  The other calls and their scratch are untouched.
 *
 * Not here: an essential refit.  sift_hip_refine_fundamental_* on the record is
 * the 8-point least-squares F, accepted when it counts at least as many records;
 * on a near-planar scene that fit is ill-conditioned and can still pass, because
 * it explains the plane.  Planar callers should skip it. */
int sift_hip_verifier_reserve_essential(sift_hip_verifier_t v, int max_samples);
/* The fundamental calls, argument for argument, with the two cameras in front of
 * the params.  The same arguments are refused, with nothing launched, and so are
 * a null camera pointer, fx or fy not > 0 or not finite, cx or cy not finite. */
int sift_hip_verify_essential_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, const sift_hip_camera* cam_query,
                                     const sift_hip_camera* cam_train, const sift_hip_verify_params* params,
                                     sift_hip_verify_result* result, sift_hip_dmatch* out, int* out_count, uint8_t* mask,
                                     void* stream);
int sift_hip_verify_essential_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                   const float* query_xy, int query_stride, int nq, const float* train_xy,
                                   int train_stride, int nt, const sift_hip_camera* cam_query,
                                   const sift_hip_camera* cam_train, const sift_hip_verify_params* params,
                                   sift_hip_verify_result* result_host, sift_hip_dmatch* out_host, uint8_t* mask_host);
/* Pair p under cam_query[p] / cam_train[p] with the seed `seed + p`: its bytes
 * are the single call's. */
int sift_hip_verify_essential_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                             int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                             const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                             const sift_hip_verify_params* params, sift_hip_verify_result* results,
                                             sift_hip_dmatch* out, int* out_counts, uint8_t* mask, void* stream);
int sift_hip_verify_essential_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                           int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                           const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,
                                           const sift_hip_verify_params* params, sift_hip_verify_result* results_host,
                                           sift_hip_dmatch* out_host, uint8_t* mask_host);
/* samples (cap x 5), F (10 cap x 9, zero rows: invalid slots) and counts (10 cap)
 * of the first min(cap, K) samples.  SIFT_HIP_ERR_STATE unless the verifier's
 * last verify call was a single-pair essential call; the other getters refuse
 * after one in the same way. */
int sift_hip_verify_essential_hypotheses_host(sift_hip_verifier_t v, int* samples, float* F, int* counts, int cap);

/* --- Multi-GPU(the reference binds one Detector to the current
 * device, Detector.hh:26-29, and has no multi-GPU path) ----------------------- */

/* Binds the calling host thread to `device` (a thread per GPU drives its own
 * Detector; sift_hip_malloc & co. then allocate there). */
int sift_hip_set_device(int device);
/* Any-to-any device copy (peer or same device) on `stream` (NULL: synchronous). */
int sift_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* Node-local communicator over RCCL (xGMI): one rank per entry of `devices`
 * (distinct GPUs), created with ncclCommInitAll.  RCCL is loaded with dlopen on
 * first use (no link-time dependency). */
typedef struct sift_hip_comm* sift_hip_comm_t;
int sift_hip_comm_create(int ndev, const int* devices, sift_hip_comm_t* out);
int sift_hip_comm_destroy(sift_hip_comm_t c);
int sift_hip_comm_size(sift_hip_comm_t c, int* n);
/* All-gather: recv[k] (device k) receives ndev * bytes, rank r's send[r] at
 * offset r * bytes (the C5 exchange of descriptor sets).  One ncclAllGather per
 * rank inside an ncclGroupStart/End; streams[k] may be NULL for the
 * communicator's own stream, and with streams == NULL the call returns after
 * every rank's copy has completed.  Ordering: the gather runs on streams[k]
 * (or the communicator's non-blocking stream), which is NOT ordered after the
 * stream that produced send[k] -- pass the producer's stream in streams[k], or
 * make send[k] complete (stream/device synchronise) before the call. */
int sift_hip_comm_allgather(sift_hip_comm_t c, const void* const* send, void* const* recv, size_t bytes,
                            void* const* streams);

/* --- Utilities -------------------------------------------------------------- */

/* Deterministic synthetic frame, fp32 0..255 integers. */
int sift_synth_frame(unsigned frame_index, int w, int h, float* out);

/* Device helpers for callers without a HIP toolchain (ctypes tests/bench). */
int sift_hip_device_count(int* n);
int sift_hip_malloc(void** p, size_t bytes);
int sift_hip_free(void* p);
int sift_hip_memcpy_h2d(void* dst, const void* src, size_t bytes);
int sift_hip_memcpy_d2h(void* dst, const void* src, size_t bytes);
int sift_hip_device_sync(void);

#ifdef __cplusplus
}
#endif
#endif
