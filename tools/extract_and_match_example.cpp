// Mirrors /root/reference/tool/extract_and_match_example.cc:38-105: detect on
// consecutive frames and match each frame against the previous one through
// Detector::prev_descriptor + matchBruteForce.  Frames: a synthetic frame and
// copies shifted by (k*dx, k*dy) pixels, so good matches must agree with the shift.
// --pipelined: 8-bit frames through Detector::submit / wait, frame f+1 staged
// and uploaded while frame f computes; prints the same lines as the default
// synchronous Imagef loop.  --exact: Detector::setExactDescriptors(true)
// (OpenCV's descriptor bytes, sift_hip_set_descriptor_mode).  --rootsift:
// Detector::setRootSift(true) (RootSIFT rows from the descriptor kernel, matched
// through their sidecar like the default rows); same lines.  --micro-batch N
// (with --pipelined): Detector::setMicroBatch(N) on 2 lanes, 2N frames
// submitted ahead, so frames run in N-frame launch groups; same lines.
// --ahead N (with --pipelined): N frames submitted past the one waited for
// (default 1, or 2N with --micro-batch); past 2 per lane the default handle
// runs them in automatic launch groups (sift_hip_set_auto_micro_batch).
// --mask-border N (synchronous loop only): every frame is detected with a
// mask that zeroes an N-pixel frame border (cv::SIFT's mask argument,
// Detector::detectAndCompute(image, mask)); no keypoint may come from it.
// --cross-check / --max-distance D: the frame pairs are matched with
// sift_cuda::matchList instead (filter + compaction on the GPU: Lowe's ratio,
// the mutual-nearest-neighbour test with --cross-check, an L2 distance cap of
// D with --max-distance) and its count is printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "sift_cuda/Detector.hh"
#include "sift_hip.h"

int main(int argc, char** argv) {
    int W = 752, H = 480, frames = 4, dx = 3, dy = 2;
    bool pipelined = false, exact = false, rootsift = false;
    int micro = 1, ahead_arg = 0, border = 0;
    bool cross_check = false;
    float max_distance = 0.f;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--pipelined") pipelined = true;
        else if (a == "--exact") exact = true;
        else if (a == "--rootsift") rootsift = true;
        else if (a == "--width" && i + 1 < argc) W = std::atoi(argv[++i]);
        else if (a == "--height" && i + 1 < argc) H = std::atoi(argv[++i]);
        else if (a == "--frames" && i + 1 < argc) frames = std::atoi(argv[++i]);
        else if (a == "--micro-batch" && i + 1 < argc) micro = std::atoi(argv[++i]);
        else if (a == "--ahead" && i + 1 < argc) ahead_arg = std::atoi(argv[++i]);
        else if (a == "--mask-border" && i + 1 < argc) border = std::atoi(argv[++i]);
        else if (a == "--cross-check") cross_check = true;
        else if (a == "--max-distance" && i + 1 < argc) max_distance = (float)std::atof(argv[++i]);
    }
    const int PW = W + frames * dx, PH = H + frames * dy;
    std::vector<float> big((size_t)PW * PH);
    sift_synth_frame(7, PW, PH, big.data());

    CudaSiftConfig config;
    config.upscale = false;
    config.numFeatures = 2000;
    config.col_width = W;
    config.row_width = H;
    sift_cuda::Detector detector(config);
    if (exact) detector.setExactDescriptors(true);  // before the warm-up: part of the captured graphs
    if (rootsift) detector.setRootSift(true);       // likewise
    if (micro > 1) {
        detector.setLanes(2);
        detector.setMicroBatch(micro);
    }
    detector.gpuWarmUpAndAllocate();
    if (border > 0 && pipelined) {
        std::fprintf(stderr, "--mask-border needs the synchronous loop (no pipelined masked variant)\n");
        return 1;
    }
    Image8U mask(H, W);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            mask.at(y, x) = x >= border && x < W - border && y >= border && y < H - border ? 255 : 0;
    int prev_size = 0;
    std::vector<sift_cuda::Float3> prev_kpts;
    int failures = 0;
    auto frame = [&](int f, auto& img) {
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) img.at(y, x) = big[(size_t)(y + f * dy) * PW + x + f * dx];
    };
    std::vector<long long> ticket(frames, -1);
    auto submit = [&](int f) {
        Image8U img(H, W);
        frame(f, img);
        ticket[f] = detector.submit(img);
    };
    const int ahead = ahead_arg > 0 ? ahead_arg : (micro > 1 ? 2 * micro : 1);  // frames past the one waited for
    if (pipelined)
        for (int f = 0; f < ahead && f < frames; f++) submit(f);
    for (int f = 0; f < frames; f++) {
        if (pipelined) {
            if (f + ahead < frames) submit(f + ahead);
            detector.wait(ticket[f]);
        } else {
            Imagef img(H, W);
            frame(f, img);
            if (border > 0)
                detector.detectAndCompute(img, mask);
            else
                detector.detectAndCompute(img);
        }
        detector.copyToHost(false);
        const int curr_size = detector.total_size;
        if (border > 0)
            for (const auto& k : detector.final_kpts)
                if (!mask.at((int)(k.y + 0.5f), (int)(k.x + 0.5f))) {
                    std::printf("frame %d: keypoint (%g, %g) lies in the masked border\n", f, k.x, k.y);
                    failures++;
                    break;
                }
        if (f > 0 && (cross_check || max_distance > 0.f)) {
            sift_cuda::MatchFilter filter;  // ratio 0.8 on squared distances, as matchBruteForce below
            filter.ratio_on_squared = 1;
            filter.cross_check = cross_check;
            filter.max_distance = max_distance;
            const auto list = sift_cuda::matchList(detector.prev_descriptor, prev_size, detector.device_descriptor,
                                                   curr_size, filter);
            int consistent = 0;
            for (const auto& m : list) {
                const auto& a = prev_kpts[m.queryIdx];
                const auto& b = detector.final_kpts[m.trainIdx];
                if (std::fabs((a.x - dx) - b.x) < 1.5f && std::fabs((a.y - dy) - b.y) < 1.5f) consistent++;
            }
            std::printf("frame %d: %d kpts, %zu list matches, %d consistent with the (%d,%d) shift\n", f, curr_size,
                        list.size(), consistent, -dx, -dy);
            if (list.empty() || consistent * 10 < (int)list.size() * 8) failures++;
        } else if (f > 0) {
            const auto matches = sift_cuda::matchBruteForce(detector.prev_descriptor, prev_size,
                                                            detector.device_descriptor, curr_size);
            int good = 0, consistent = 0;
            for (int i = 0; i < prev_size; i++) {
                if (matches[i] < 0) continue;
                good++;
                const auto& a = prev_kpts[i];
                const auto& b = detector.final_kpts[matches[i]];
                if (std::fabs((a.x - dx) - b.x) < 1.5f && std::fabs((a.y - dy) - b.y) < 1.5f) consistent++;
            }
            std::printf("frame %d: %d kpts, %d matches, %d consistent with the (%d,%d) shift\n", f, curr_size, good,
                        consistent, -dx, -dy);
            if (good == 0 || consistent * 10 < good * 8) failures++;
        } else {
            std::printf("frame 0: %d kpts\n", curr_size);
        }
        prev_size = curr_size;
        prev_kpts = detector.final_kpts;
    }
    return failures ? 2 : 0;
}
