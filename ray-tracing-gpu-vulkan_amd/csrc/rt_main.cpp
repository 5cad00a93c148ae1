// rt_main.cpp — command-line front end, the counterpart of the reference's src/main.cpp:10-64
// (target RayTracingGPUVulkan, CMakeLists.txt:47-51). Same flags and defaults, same call into the
// library's ray_trace(); unknown flags are reported and ignored as in the reference (:48-50),
// but a flag missing its value is an error here (the reference reads past argv, :33-46).
//
//   --help  --store  --samples <spp>  --width <w>  --height <h>  --gpus <n>
//   --frames <n> [--animate]: the reference's benchmark frame loop (src/ray_trace.cpp:567-748):
//   n frames back to back, each rebuilding the scene (generateRandomScene(t), t = seconds since
//   start with --animate, else 0) and rendering the image tiled over the GPUs with an RCCL gather
//   to GPU 0 (rt_multi); prints duration_per_frame like the reference (:740-744). Frames are
//   queued asynchronously on ONE rt_multi (one communicator, its streams keep the gathers of
//   successive frames in one order on every device), so the host builds frame k+1's scene while
//   frame k renders.
//   --rng stream|hash: the reference's per-pixel LCG stream (default) or the counter-based
//   RT_RNG_SAMPLE_HASH stream, for --frames and for the single ray_trace() frame alike.
//   --adaptive THRESHOLD[,MIN[,STEP]]: one adaptive frame (rt_render_adaptive_device) on one GPU
//   in the counter-based stream: MIN samples everywhere (default 16), STEP more per pass (default
//   MIN) on the 8x8 tiles noisier than THRESHOLD, at most --samples per pixel.
//   --adaptive ... --frames <n> [--animate] [--replay R]: the frame loop on one GPU with adaptive
//   frames: frame i is an adaptive frame when i % (R + 1) == 0 (R defaults to 0), else a sample-map
//   frame (rt_render_sample_map_device) that replays the latest adaptive frame's per-tile counts
//   without the pass loop, queued asynchronously; duration_per_frame adds the replays and the mean
//   spp. --replay without --adaptive and --frames is refused.
//   --map-launch levels|one: the schedule of the replays (rt_sample_map_set_schedule): one trace
//   launch per distinct count (default), or one launch of a block table for the whole frame.
//   Refused without --replay; duration_per_frame names it.
//   --denoise [F[,ITER]]: one frame on one GPU in the counter-based stream (--rng hash, or an
//   --adaptive frame), then first-hit feature buffers of F samples per pixel (default 16,
//   rt_render_features_device) and the edge-avoiding denoise of ITER iterations (default 3,
//   rt_denoise_device); --store writes the denoised image. Refused with --gpus above 1, with
//   --frames (but for --temporal below), and on the plain path without --rng hash.
//   --denoise-variance [F[,ITER[,PRE]]]: one frame on one GPU in the counter-based stream (--rng
//   hash) rendered as two halves of --samples / 2 (rt_render_device at sample_base 0 and
//   --samples / 2), then the feature buffers of F samples and the variance-guided denoise of PRE
//   prefilter passes (default 2) and ITER iterations (default 3, rt_denoise_variance_device);
//   --store writes the denoised image. Takes --denoise's refusals, and refuses an odd --samples,
//   --adaptive, and --denoise beside it.
//   --temporal [N]: beside --denoise or --denoise-variance and --frames K [--animate], the one pairing
//   of a filter with the frame loop: frame k is rendered at sample_base k x --samples (under
//   --denoise-variance as two halves at k x --samples and k x --samples + --samples / 2), the
//   features at sample_base 0, and the frame is integrated into a per-pixel history of at most N
//   frames (default 8, rt_temporal_accumulate_device) that the filter then reads, everything queued
//   on one stream; prints duration_per_frame; --store writes the last frame's filtered image. Refused
//   without a filter, without --frames, with --gpus above 1, with --adaptive, without --rng hash, and
//   when K x --samples does not fit 32 bits.
//   --reproject: beside --temporal, every frame also renders its motion plane against the frame before
//   (rt_render_motion_device, then rt_motion_keep_current) and the history follows it
//   (rt_temporal_reproject_device in place of rt_temporal_accumulate_device). Refused without --temporal.
//   --camera-step S: frame k's camera stands at (13 + S k, 11, -3 + 2 S k) and looks at the origin
//   (default 0: the reference's camera every frame), with or without --reproject. Refused without
//   --temporal.
//   --adaptive T[,MIN[,STEP]] --samples CAP --frames K --feedback --denoise-variance [F[,ITER[,PRE]]]
//   [--temporal [N] [--reproject] [--camera-step S]] [--animate]: the feedback loop through the filters,
//   the one pairing of noise-driven frames with them. Frame 0 is an adaptive frame and every later frame
//   a feedback frame (min, max, cap and threshold as --feedback derives them), frame k from sample_base
//   k x CAP; each hands its two halves and half counts over (rt_render_adaptive_halves_device,
//   rt_render_sample_map_feedback_halves_device), then the features at sample_base 0, with --reproject
//   the motion pass, with --temporal the stage on the two halves (sample_count = the half counts), and
//   the variance-guided filter (on the stage's outputs at half_spp 1, else on the halves with their
//   counts), all on one stream; --store writes the last frame's filtered image. Refused when K x CAP
//   does not fit 32 bits. Without --feedback, --denoise-variance and --temporal still refuse --adaptive,
//   and --denoise (the plain filter) refuses --frames as before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_mi355x.h"

static bool parse_u32(const char* s, uint32_t& out) {
    const char* end = s + std::strlen(s);
    auto r = std::from_chars(s, end, out);
    return r.ec == std::errc() && r.ptr == end;
}

#define CLI_HIP(x)                                                                      \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
            return 1;                                                                   \
        }                                                                               \
    } while (0)
#define CLI_RT(x)                                                                       \
    do {                                                                                \
        if ((x) != RT_OK) {                                                             \
            std::fprintf(stderr, "%s: %s\n", #x, rt_last_error());                     \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {

int run_frames(uint32_t samples, uint32_t width, uint32_t height, uint32_t gpu_count, uint32_t frames,
               bool animate, bool store, uint32_t rng_mode) {
    // One multi-device renderer: two rt_multi over the same devices would be two RCCL
    // communicators whose grouped gathers could run in different orders on different devices.
    rt_multi* m = nullptr;
    hipStream_t stream = nullptr;   // device 0
    float* accum = nullptr;
    uint8_t* rgba8 = nullptr;
    uint32_t n = 1;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_multi_create(gpu_count, &m));
    CLI_RT(rt_multi_device_count(m, &n));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum, size_t(width) * height * 16));
    CLI_HIP(hipMalloc(&rgba8, size_t(width) * height * 4));
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = rng_mode;
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    const auto t_start = std::chrono::steady_clock::now();
    auto frame = [&]() -> int {
        const float t = animate ? std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count() : 0.0f;
        CLI_RT(rt_generate_scene(t, 11, scene.data(), uint32_t(scene.size()), &cnt));   // scene.h:79
        RenderCallInfo rci;
        CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
        CLI_RT(rt_multi_set_scene(m, scene.data(), cnt));
        CLI_RT(rt_multi_render(m, &rci, &opt, accum, rgba8, stream));
        return 0;
    };
    auto sync_all = [&]() -> int {
        for (uint32_t g = 0; g < n; g++) {
            CLI_HIP(hipSetDevice(int(g)));
            CLI_HIP(hipDeviceSynchronize());
        }
        CLI_HIP(hipSetDevice(0));
        return 0;
    };
    if (int rc = frame()) return rc;   // warm-up: every context has its LPT order
    if (int rc = sync_all()) return rc;
    // Report about once a second, like the reference's ~4 s benchmark windows (:740-748).
    uint32_t done = 0;
    while (done < frames) {
        const auto b = std::chrono::steady_clock::now();
        uint32_t k = 0;
        for (;;) {
            if (int rc = frame()) return rc;
            ++k;
            if (done + k >= frames) break;
            if (std::chrono::steady_clock::now() - b > std::chrono::milliseconds(1000)) break;
        }
        if (int rc = sync_all()) return rc;
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
        done += k;
        std::printf("duration_per_frame: %.3f ms (%u frames, %u GPU, %.1f Msamples/s)\n", sec / k * 1e3, k, n,
                    double(width) * height * samples * k / sec / 1e6);
    }
    if (store) {   // the last frame
        std::vector<uint8_t> img(size_t(width) * height * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_multi_destroy(m);
    (void)hipStreamDestroy(stream);
    (void)hipFree(accum);
    (void)hipFree(rgba8);
    return 0;
}

// One adaptive frame of the canonical scene on device 0.
int run_adaptive(uint32_t samples, uint32_t width, uint32_t height, bool store, const rt_adaptive& ad) {
    rt_context* ctx = nullptr;
    hipStream_t stream = nullptr;
    float* accum = nullptr;
    uint8_t* rgba8 = nullptr;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum, size_t(width) * height * 16));
    CLI_HIP(hipMalloc(&rgba8, size_t(width) * height * 4));
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    CLI_RT(rt_generate_scene(0.0f, 11, scene.data(), uint32_t(scene.size()), &cnt));
    CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
    RenderCallInfo rci;
    CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = RT_RNG_SAMPLE_HASH;
    rt_adaptive_info info;
    CLI_HIP(hipStreamSynchronize(stream));
    const auto b = std::chrono::steady_clock::now();
    CLI_RT(rt_render_adaptive_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt, &ad, &info, stream));
    CLI_HIP(hipStreamSynchronize(stream));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
    const double pixels = double(width) * height;
    std::printf("duration_per_frame: %.3f ms (adaptive, threshold %g: %u passes, mean %.2f spp of at most %u, "
                "%u of %u tiles capped, %.1f Msamples/s)\n",
                sec * 1e3, double(ad.threshold), info.passes, double(info.samples) / pixels, samples, info.tiles_capped,
                info.tiles, double(info.samples) / sec / 1e6);
    if (store) {
        std::vector<uint8_t> img(size_t(width) * height * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    (void)hipFree(accum);
    (void)hipFree(rgba8);
    return 0;
}

// One frame of the canonical scene on device 0, plain (ad == nullptr) or adaptive, then its feature
// buffers and the denoise; the stored image is the denoised one.
int run_denoised(uint32_t samples, uint32_t width, uint32_t height, bool store, const rt_adaptive* ad,
                 uint32_t feature_samples, uint32_t iterations) {
    rt_context* ctx = nullptr;
    hipStream_t stream = nullptr;
    float *accum = nullptr, *feat0 = nullptr, *feat1 = nullptr;
    uint8_t* rgba8 = nullptr;
    uint32_t* counts = nullptr;
    rt_denoise dn = {iterations, 4.0f, 16.0f, 1.0f};
    const size_t texels = size_t(width) * height;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum, texels * 16));
    CLI_HIP(hipMalloc(&feat0, texels * 16));
    CLI_HIP(hipMalloc(&feat1, texels * 16));
    CLI_HIP(hipMalloc(&rgba8, texels * 4));
    if (ad) CLI_HIP(hipMalloc(&counts, texels * 4));
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    CLI_RT(rt_generate_scene(0.0f, 11, scene.data(), uint32_t(scene.size()), &cnt));
    CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
    RenderCallInfo rci;
    CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = RT_RNG_SAMPLE_HASH;
    rt_adaptive_info info;
    std::memset(&info, 0, sizeof(info));
    CLI_HIP(hipStreamSynchronize(stream));
    const auto b = std::chrono::steady_clock::now();
    if (ad) CLI_RT(rt_render_adaptive_device(ctx, &rci, nullptr, width, height, accum, rgba8, counts, &opt, ad, &info, stream));
    else CLI_RT(rt_render_device(ctx, &rci, nullptr, width, height, accum, rgba8, &opt, stream));
    CLI_RT(rt_render_features_device(ctx, &rci, nullptr, width, height, feat0, feat1, feature_samples, &opt, stream));
    CLI_RT(rt_denoise_device(ctx, accum, counts, samples, feat0, feat1, feature_samples, width, height, &dn, nullptr, rgba8,
                             stream));
    CLI_HIP(hipStreamSynchronize(stream));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
    const double spp = ad ? double(info.samples) / double(texels) : double(samples);
    std::printf("duration_per_frame: %.3f ms (%s, mean %.2f spp, denoised: %u feature samples, %u iterations)\n", sec * 1e3,
                ad ? "adaptive" : "plain", spp, feature_samples, iterations);
    if (store) {
        std::vector<uint8_t> img(texels * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    (void)hipFree(accum);
    (void)hipFree(feat0);
    (void)hipFree(feat1);
    (void)hipFree(rgba8);
    (void)hipFree(counts);
    return 0;
}

// One frame of the canonical scene on device 0 as two halves of samples / 2, then its feature
// buffers and the variance-guided denoise; the stored image is the denoised one.
int run_denoised_variance(uint32_t samples, uint32_t width, uint32_t height, bool store, uint32_t feature_samples,
                          const rt_denoise_variance& dn) {
    rt_context* ctx = nullptr;
    hipStream_t stream = nullptr;
    float *accum_a = nullptr, *accum_b = nullptr, *feat0 = nullptr, *feat1 = nullptr;
    uint8_t* rgba8 = nullptr;
    const size_t texels = size_t(width) * height;
    const uint32_t half = samples / 2u;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum_a, texels * 16));
    CLI_HIP(hipMalloc(&accum_b, texels * 16));
    CLI_HIP(hipMalloc(&feat0, texels * 16));
    CLI_HIP(hipMalloc(&feat1, texels * 16));
    CLI_HIP(hipMalloc(&rgba8, texels * 4));
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    CLI_RT(rt_generate_scene(0.0f, 11, scene.data(), uint32_t(scene.size()), &cnt));
    CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
    RenderCallInfo rci, half_rci;
    CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
    half_rci = rci;
    half_rci.samplesPerRenderCall = half;
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = RT_RNG_SAMPLE_HASH;
    rt_options second = opt;
    second.sample_base = half;
    CLI_HIP(hipStreamSynchronize(stream));
    const auto b = std::chrono::steady_clock::now();
    CLI_RT(rt_render_device(ctx, &half_rci, nullptr, width, height, accum_a, rgba8, &opt, stream));
    CLI_RT(rt_render_device(ctx, &half_rci, nullptr, width, height, accum_b, rgba8, &second, stream));
    CLI_RT(rt_render_features_device(ctx, &rci, nullptr, width, height, feat0, feat1, feature_samples, &opt, stream));
    CLI_RT(rt_denoise_variance_device(ctx, accum_a, accum_b, nullptr, half, feat0, feat1, feature_samples, width, height,
                                      &dn, nullptr, rgba8, stream));
    CLI_HIP(hipStreamSynchronize(stream));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
    std::printf("duration_per_frame: %.3f ms (two halves of %u spp, variance-guided denoise: %u feature samples, "
                "%u prefilter passes, %u iterations)\n",
                sec * 1e3, half, feature_samples, dn.prefilter, dn.iterations);
    if (store) {
        std::vector<uint8_t> img(texels * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    (void)hipFree(accum_a);
    (void)hipFree(accum_b);
    (void)hipFree(feat0);
    (void)hipFree(feat1);
    (void)hipFree(rgba8);
    return 0;
}

// The frame loop with adaptive frames, on device 0: frame i is an adaptive frame when
// i % (replay + 1) == 0, else a sample-map frame replaying the latest adaptive frame's counts. One
// stream, the scene rebuilt per frame as run_frames does; the replays are queued without a host wait.
// feedback: frame 0 is the adaptive frame and every later frame a feedback frame:
// it renders the map, measures it and plans the next frame's map on the device; after the one set call
// behind frame 0 the host waits for nothing but the end of a report window.
int run_adaptive_frames(uint32_t samples, uint32_t width, uint32_t height, uint32_t frames, bool animate, bool store,
                        const rt_adaptive& ad, uint32_t replay, uint32_t map_schedule, bool feedback) {
    rt_context* ctx = nullptr;
    rt_sample_map* map = nullptr;
    hipStream_t stream = nullptr;
    float* accum = nullptr;
    uint8_t* rgba8 = nullptr;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_RT(rt_sample_map_create(ctx, width, height, &map));
    // (a feedback loop's one host-planned map may hold any number of distinct counts)
    CLI_RT(rt_sample_map_set_schedule(map, feedback ? RT_SAMPLE_MAP_ONE_LAUNCH : map_schedule, 0));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum, size_t(width) * height * 16));
    CLI_HIP(hipMalloc(&rgba8, size_t(width) * height * 4));
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = RT_RNG_SAMPLE_HASH;
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    uint64_t frame_index = 0, window_samples = 0;
    uint32_t window_replays = 0;
    bool map_stale = true;   // an adaptive frame has run since the map was set
    rt_sample_map_info map_info;
    std::memset(&map_info, 0, sizeof(map_info));
    rt_sample_map_feedback fb;
    std::memset(&fb, 0, sizeof(fb));
    fb.threshold = ad.threshold;
    fb.min_spp = ad.min_spp;
    fb.max_spp = samples;
    const auto t_start = std::chrono::steady_clock::now();
    auto frame = [&]() -> int {
        const float t = animate ? std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count() : 0.0f;
        CLI_RT(rt_generate_scene(t, 11, scene.data(), uint32_t(scene.size()), &cnt));
        RenderCallInfo rci;
        CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
        CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
        if (feedback && frame_index > 0) {
            if (map_stale) CLI_RT(rt_sample_map_set_from_adaptive(map, 0, stream, &map_info));
            map_stale = false;
            CLI_RT(rt_render_sample_map_feedback_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt, map,
                                                        &fb, nullptr, stream));
            ++window_replays;
        } else if (frame_index % (uint64_t(replay) + 1u) == 0) {
            rt_adaptive_info info;
            CLI_RT(rt_render_adaptive_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt, &ad, &info,
                                             stream));
            window_samples += info.samples;
            map_stale = true;
        } else {
            if (map_stale) CLI_RT(rt_sample_map_set_from_adaptive(map, 0, stream, &map_info));
            map_stale = false;
            CLI_RT(rt_render_sample_map_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt, map, stream));
            window_samples += map_info.samples;
            ++window_replays;
        }
        ++frame_index;
        return 0;
    };
    if (int rc = frame()) return rc;   // warm-up: the adaptive buffers exist
    CLI_HIP(hipStreamSynchronize(stream));
    frame_index = 0;
    const double pixels = double(width) * height;
    uint32_t done = 0;
    while (done < frames) {
        const auto b = std::chrono::steady_clock::now();
        uint32_t k = 0;
        window_samples = 0;
        window_replays = 0;
        for (;;) {
            if (int rc = frame()) return rc;
            ++k;
            if (done + k >= frames) break;
            if (std::chrono::steady_clock::now() - b > std::chrono::milliseconds(1000)) break;
        }
        CLI_HIP(hipStreamSynchronize(stream));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
        done += k;
        if (feedback) {   // (the stream is idle: the info call's wait costs nothing)
            if (window_replays) CLI_RT(rt_sample_map_get_info(map, &map_info));
            std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u feedback frames, next map mean %.2f spp "
                        "of at most %u)\n",
                        sec / k * 1e3, k, double(ad.threshold), window_replays, double(map_info.samples) / pixels, samples);
            continue;
        }
        std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u replays, map launch %s, mean %.2f spp "
                    "of at most %u, %.1f Msamples/s)\n",
                    sec / k * 1e3, k, double(ad.threshold), window_replays,
                    map_schedule == RT_SAMPLE_MAP_ONE_LAUNCH ? "one" : "levels", double(window_samples) / pixels / k, samples,
                    double(window_samples) / sec / 1e6);
    }
    if (store) {   // the last frame
        std::vector<uint8_t> img(size_t(width) * height * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_sample_map_destroy(map);
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    (void)hipFree(accum);
    (void)hipFree(rgba8);
    return 0;
}

// The denoised frame loop on device 0 (--temporal with --frames and a filter): frame k renders the
// scene at t from the sample range of its own (sample_base = k x samples; under the variance filter
// as two halves at k x samples and k x samples + samples / 2), the features at sample_base 0 every
// frame, integrates the frame into the temporal state and filters what that call wrote, everything
// queued on one stream. dv: the variance-guided filter's parameters, or nullptr for the plain
// filter's dn. The stored image is the last frame's filtered one.
int run_temporal_frames(uint32_t samples, uint32_t width, uint32_t height, uint32_t frames, bool animate, bool store,
                        uint32_t feature_samples, const rt_denoise& dn, const rt_denoise_variance* dv,
                        const rt_temporal_params& tp, bool reproject, float camera_step) {
    rt_context* ctx = nullptr;
    rt_temporal* temporal = nullptr;
    rt_motion* motion = nullptr;
    float* motion_plane = nullptr;
    hipStream_t stream = nullptr;
    float *accum_a = nullptr, *accum_b = nullptr, *feat0 = nullptr, *feat1 = nullptr, *out_a = nullptr, *out_b = nullptr;
    uint8_t* rgba8 = nullptr;
    const size_t texels = size_t(width) * height;
    const uint32_t half = samples / 2u;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_RT(rt_temporal_create(ctx, width, height, &temporal));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    CLI_HIP(hipMalloc(&accum_a, texels * 16));
    CLI_HIP(hipMalloc(&out_a, texels * 16));
    if (dv) {
        CLI_HIP(hipMalloc(&accum_b, texels * 16));
        CLI_HIP(hipMalloc(&out_b, texels * 16));
    }
    CLI_HIP(hipMalloc(&feat0, texels * 16));
    CLI_HIP(hipMalloc(&feat1, texels * 16));
    CLI_HIP(hipMalloc(&rgba8, texels * 4));
    if (reproject) {
        CLI_RT(rt_motion_create(ctx, width, height, &motion));
        CLI_HIP(hipMalloc(&motion_plane, texels * 16));
    }
    rt_options feat_opt;
    std::memset(&feat_opt, 0, sizeof(feat_opt));
    feat_opt.rng_mode = RT_RNG_SAMPLE_HASH;
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0;
    uint32_t frame_index = 0;
    const auto t_start = std::chrono::steady_clock::now();
    auto frame = [&]() -> int {
        const float t = animate ? std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count() : 0.0f;
        CLI_RT(rt_generate_scene(t, 11, scene.data(), uint32_t(scene.size()), &cnt));
        CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
        RenderCallInfo rci;
        CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
        if (camera_step != 0.0f) {   // frame k of the path; it looks at the origin
            rci.camera_pos.x = 13.0f + camera_step * float(frame_index);
            rci.camera_pos.z = -3.0f + (2.0f * camera_step) * float(frame_index);
            rci.camera_dir = rt_vec4{-rci.camera_pos.x, -rci.camera_pos.y, -rci.camera_pos.z, 0.0f};
        }
        rt_options opt = feat_opt;
        opt.sample_base = frame_index * samples;
        if (dv) {
            RenderCallInfo half_rci = rci;
            half_rci.samplesPerRenderCall = half;
            rt_options second = opt;
            second.sample_base = opt.sample_base + half;
            CLI_RT(rt_render_device(ctx, &half_rci, nullptr, width, height, accum_a, rgba8, &opt, stream));
            CLI_RT(rt_render_device(ctx, &half_rci, nullptr, width, height, accum_b, rgba8, &second, stream));
        } else {
            CLI_RT(rt_render_device(ctx, &rci, nullptr, width, height, accum_a, rgba8, &opt, stream));
        }
        CLI_RT(rt_render_features_device(ctx, &rci, nullptr, width, height, feat0, feat1, feature_samples, &feat_opt, stream));
        if (reproject) {
            CLI_RT(rt_render_motion_device(ctx, motion, &rci, motion_plane, nullptr, stream));
            CLI_RT(rt_motion_keep_current(ctx, motion, &rci, stream));
            CLI_RT(rt_temporal_reproject_device(ctx, temporal, accum_a, accum_b, nullptr, dv ? half : samples, feat0, feat1,
                                                feature_samples, motion_plane, &tp, out_a, out_b, nullptr, nullptr, stream));
        } else {
            CLI_RT(rt_temporal_accumulate_device(ctx, temporal, accum_a, accum_b, nullptr, dv ? half : samples, feat0, feat1,
                                                 feature_samples, &tp, out_a, out_b, nullptr, nullptr, stream));
        }
        if (dv)
            CLI_RT(rt_denoise_variance_device(ctx, out_a, out_b, nullptr, 1, feat0, feat1, feature_samples, width, height, dv,
                                              nullptr, rgba8, stream));
        else
            CLI_RT(rt_denoise_device(ctx, out_a, nullptr, 1, feat0, feat1, feature_samples, width, height, &dn, nullptr, rgba8,
                                     stream));
        ++frame_index;
        return 0;
    };
    if (int rc = frame()) return rc;   // warm-up: the context's band buffers exist
    CLI_RT(rt_temporal_reset(temporal, stream));
    CLI_HIP(hipStreamSynchronize(stream));
    frame_index = 0;
    uint32_t done = 0;
    while (done < frames) {
        const auto b = std::chrono::steady_clock::now();
        uint32_t k = 0;
        for (;;) {
            if (int rc = frame()) return rc;
            ++k;
            if (done + k >= frames) break;
            if (std::chrono::steady_clock::now() - b > std::chrono::milliseconds(1000)) break;
        }
        CLI_HIP(hipStreamSynchronize(stream));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
        done += k;
        std::printf("duration_per_frame: %.3f ms (%u frames, %u spp%s, temporal history %u%s, %s denoise: %u feature samples, "
                    "%.1f Msamples/s)\n",
                    sec / k * 1e3, k, samples, dv ? " in two halves" : "", tp.max_history, reproject ? " reprojected" : "",
                    dv ? "variance-guided" : "plain", feature_samples, double(width) * height * samples * k / sec / 1e6);
    }
    if (store) {   // the last frame
        std::vector<uint8_t> img(texels * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_temporal_destroy(temporal);
    rt_motion_destroy(motion);
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    (void)hipFree(motion_plane);
    (void)hipFree(accum_a);
    (void)hipFree(accum_b);
    (void)hipFree(out_a);
    (void)hipFree(out_b);
    (void)hipFree(feat0);
    (void)hipFree(feat1);
    (void)hipFree(rgba8);
    return 0;
}

// The feedback loop through the filters, on device 0 (--adaptive --frames --feedback --denoise-variance,
// optionally --temporal [--reproject] [--camera-step]): frame 0 is an adaptive halves frame and every
// later frame a feedback halves frame, with the feedback parameters run_adaptive_frames derives; frame k
// renders from sample_base k x samples (the cap), so the frames' noise is independent. Every frame hands
// its two halves and half counts over (rt_half_outputs); then the features at sample_base 0, with tp
// the temporal stage on the halves (reprojected behind the motion pass, or in place) and the
// variance-guided filter: on the stage's outputs at half_spp 1, or on the halves with their counts.
// Everything on one stream; after the one set call behind frame 0 nothing waits but a window's end.
int run_feedback_filtered_frames(uint32_t samples, uint32_t width, uint32_t height, uint32_t frames, bool animate,
                                 bool store, const rt_adaptive& ad, uint32_t feature_samples,
                                 const rt_denoise_variance& dv, const rt_temporal_params* tp, bool reproject,
                                 float camera_step) {
    rt_context* ctx = nullptr;
    rt_sample_map* map = nullptr;
    rt_temporal* temporal = nullptr;
    rt_motion* motion = nullptr;
    hipStream_t stream = nullptr;
    float *accum = nullptr, *accum_a = nullptr, *accum_b = nullptr, *feat0 = nullptr, *feat1 = nullptr;
    float *out_a = nullptr, *out_b = nullptr, *motion_plane = nullptr;
    uint32_t* half_count = nullptr;
    uint8_t* rgba8 = nullptr;
    const size_t texels = size_t(width) * height;
    CLI_HIP(hipSetDevice(0));
    CLI_RT(rt_context_create(0, &ctx));
    CLI_RT(rt_sample_map_create(ctx, width, height, &map));
    CLI_RT(rt_sample_map_set_schedule(map, RT_SAMPLE_MAP_ONE_LAUNCH, 0));
    CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (float** p : {&accum, &accum_a, &accum_b, &feat0, &feat1}) CLI_HIP(hipMalloc(p, texels * 16));
    CLI_HIP(hipMalloc(&half_count, texels * 4));
    CLI_HIP(hipMalloc(&rgba8, texels * 4));
    if (tp) {
        CLI_RT(rt_temporal_create(ctx, width, height, &temporal));
        CLI_HIP(hipMalloc(&out_a, texels * 16));
        CLI_HIP(hipMalloc(&out_b, texels * 16));
    }
    if (reproject) {
        CLI_RT(rt_motion_create(ctx, width, height, &motion));
        CLI_HIP(hipMalloc(&motion_plane, texels * 16));
    }
    const rt_half_outputs halves = {accum_a, accum_b, half_count, nullptr};
    rt_options feat_opt;
    std::memset(&feat_opt, 0, sizeof(feat_opt));
    feat_opt.rng_mode = RT_RNG_SAMPLE_HASH;
    rt_sample_map_feedback fb;
    std::memset(&fb, 0, sizeof(fb));
    fb.threshold = ad.threshold;
    fb.min_spp = ad.min_spp;
    fb.max_spp = samples;
    rt_sample_map_info map_info;
    std::memset(&map_info, 0, sizeof(map_info));
    std::vector<Sphere> scene(488);
    uint32_t cnt = 0, frame_index = 0, window_feedback = 0;
    bool map_stale = true;   // an adaptive frame has run since the map was set
    const auto t_start = std::chrono::steady_clock::now();
    auto frame = [&]() -> int {
        const float t = animate ? std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count() : 0.0f;
        CLI_RT(rt_generate_scene(t, 11, scene.data(), uint32_t(scene.size()), &cnt));
        CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
        RenderCallInfo rci;
        CLI_RT(rt_canonical_render_call_info(samples, width, height, &rci));
        if (camera_step != 0.0f) {   // frame k of the path; it looks at the origin
            rci.camera_pos.x = 13.0f + camera_step * float(frame_index);
            rci.camera_pos.z = -3.0f + (2.0f * camera_step) * float(frame_index);
            rci.camera_dir = rt_vec4{-rci.camera_pos.x, -rci.camera_pos.y, -rci.camera_pos.z, 0.0f};
        }
        rt_options opt = feat_opt;
        opt.sample_base = frame_index * samples;
        if (frame_index == 0) {
            rt_adaptive_info info;
            CLI_RT(rt_render_adaptive_halves_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt, &ad, &info,
                                                    &halves, stream));
            map_stale = true;
        } else {
            if (map_stale) CLI_RT(rt_sample_map_set_from_adaptive(map, 0, stream, &map_info));
            map_stale = false;
            CLI_RT(rt_render_sample_map_feedback_halves_device(ctx, &rci, nullptr, width, height, accum, rgba8, nullptr, &opt,
                                                               map, &fb, nullptr, &halves, stream));
            ++window_feedback;
        }
        CLI_RT(rt_render_features_device(ctx, &rci, nullptr, width, height, feat0, feat1, feature_samples, &feat_opt, stream));
        if (reproject) {
            CLI_RT(rt_render_motion_device(ctx, motion, &rci, motion_plane, nullptr, stream));
            CLI_RT(rt_motion_keep_current(ctx, motion, &rci, stream));
            CLI_RT(rt_temporal_reproject_device(ctx, temporal, accum_a, accum_b, half_count, 0, feat0, feat1, feature_samples,
                                                motion_plane, tp, out_a, out_b, nullptr, nullptr, stream));
        } else if (tp) {
            CLI_RT(rt_temporal_accumulate_device(ctx, temporal, accum_a, accum_b, half_count, 0, feat0, feat1, feature_samples,
                                                 tp, out_a, out_b, nullptr, nullptr, stream));
        }
        if (tp)
            CLI_RT(rt_denoise_variance_device(ctx, out_a, out_b, nullptr, 1, feat0, feat1, feature_samples, width, height, &dv,
                                              nullptr, rgba8, stream));
        else
            CLI_RT(rt_denoise_variance_device(ctx, accum_a, accum_b, half_count, 0, feat0, feat1, feature_samples, width,
                                              height, &dv, nullptr, rgba8, stream));
        ++frame_index;
        return 0;
    };
    if (int rc = frame()) return rc;   // warm-up: the adaptive planes and the filters' band buffers exist
    if (tp) CLI_RT(rt_temporal_reset(temporal, stream));
    CLI_HIP(hipStreamSynchronize(stream));
    frame_index = 0;
    const double pixels = double(width) * height;
    uint32_t done = 0;
    while (done < frames) {
        const auto b = std::chrono::steady_clock::now();
        uint32_t k = 0;
        window_feedback = 0;
        for (;;) {
            if (int rc = frame()) return rc;
            ++k;
            if (done + k >= frames) break;
            if (std::chrono::steady_clock::now() - b > std::chrono::milliseconds(1000)) break;
        }
        CLI_HIP(hipStreamSynchronize(stream));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count();
        done += k;
        if (window_feedback) CLI_RT(rt_sample_map_get_info(map, &map_info));   // (the stream is idle)
        std::string stage;
        if (tp) stage = ", temporal history " + std::to_string(tp->max_history) + (reproject ? " reprojected" : "");
        std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u feedback frames, next map mean %.2f spp "
                    "of at most %u%s, variance-guided denoise: %u feature samples)\n",
                    sec / k * 1e3, k, double(ad.threshold), window_feedback, double(map_info.samples) / pixels, samples,
                    stage.c_str(), feature_samples);
    }
    if (store) {   // the last frame's filtered image
        std::vector<uint8_t> img(texels * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), width, height));
    }
    rt_temporal_destroy(temporal);
    rt_motion_destroy(motion);
    rt_sample_map_destroy(map);
    rt_context_destroy(ctx);
    (void)hipStreamDestroy(stream);
    for (float* p : {accum, accum_a, accum_b, feat0, feat1, out_a, out_b, motion_plane}) (void)hipFree(p);
    (void)hipFree(half_count);
    (void)hipFree(rgba8);
    return 0;
}

// F[,ITER]
bool parse_denoise(const char* s, uint32_t& f, uint32_t& iter) {
    const std::string v = s;
    const size_t comma = v.find(',');
    if (!parse_u32(v.substr(0, comma).c_str(), f)) return false;
    return comma == std::string::npos || parse_u32(v.c_str() + comma + 1, iter);
}

// F[,ITER[,PRE]]
bool parse_denoise_variance(const char* s, uint32_t& f, uint32_t& iter, uint32_t& pre) {
    const std::string v = s;
    const size_t c1 = v.find(',');
    if (!parse_u32(v.substr(0, c1).c_str(), f)) return false;
    if (c1 == std::string::npos) return true;
    const size_t c2 = v.find(',', c1 + 1);
    if (!parse_u32(v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1).c_str(), iter)) return false;
    return c2 == std::string::npos || parse_u32(v.c_str() + c2 + 1, pre);
}

// THRESHOLD[,MIN[,STEP]]
bool parse_adaptive(const char* s, rt_adaptive& ad) {
    std::memset(&ad, 0, sizeof(ad));
    char* end = nullptr;
    ad.threshold = std::strtof(s, &end);
    if (end == s) return false;
    ad.min_spp = 16;
    if (*end == ',') {
        const std::string rest = end + 1;
        const size_t comma = rest.find(',');
        if (!parse_u32(rest.substr(0, comma).c_str(), ad.min_spp)) return false;
        ad.step_spp = ad.min_spp;
        if (comma != std::string::npos && !parse_u32(rest.c_str() + comma + 1, ad.step_spp)) return false;
        return true;
    }
    ad.step_spp = ad.min_spp;
    return *end == '\0';
}

}  // namespace

int main(int argc, const char** argv) {
    uint32_t samples = 10, width = 1920, height = 1080, gpu_count = 1, frames = 0, rng_mode = RT_RNG_PIXEL_STREAM;
    uint32_t replay = 0, map_schedule = RT_SAMPLE_MAP_LEVELS;
    bool rng_explicit = false, replay_given = false, map_launch_given = false;
    bool store = false, animate = false, adaptive = false, feedback = false, denoise = false;
    uint32_t feature_samples = 16, denoise_iterations = 3;
    bool denoise_variance = false;
    uint32_t dv_feature_samples = 16;
    rt_denoise_variance dv = {3u, 2u, 4.0f, 16.0f, 0.25f};
    bool temporal = false;
    rt_temporal_params tp = {8u, 4.0f, 16.0f, 0u};
    bool reproject = false, camera_step_given = false;
    float camera_step = 0.0f;
    rt_adaptive ad;
    std::memset(&ad, 0, sizeof(ad));
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--help") {
            std::puts("--help                            # Show this help information");
            std::puts("--store                           # Store rendered image to render.ppm");
            std::puts("--samples <count>                 # Samples per pixel of the frame");
            std::puts("--width <width>                   # Image width");
            std::puts("--height <height>                 # Image height");
            std::puts("--gpus <count>                    # Max used GPUs count");
            std::puts("--frames <count>                  # Benchmark loop: render count frames, print duration_per_frame");
            std::puts("--animate                         # With --frames: scene time t = seconds since start");
            std::puts("--rng <stream|hash>               # Reference per-pixel LCG stream (default) or counter-based stream");
            std::puts("--adaptive <thr>[,<min>[,<step>]] # One GPU, hash stream: min spp everywhere, step more per pass on");
            std::puts("                                  # tiles noisier than thr, at most --samples per pixel");
            std::puts("--replay <count>                  # With --adaptive and --frames: after each adaptive frame, count");
            std::puts("                                  # frames replay its per-tile sample counts (no pass loop)");
            std::puts("--map-launch <levels|one>         # With --replay: a launch per distinct count (default) or one");
            std::puts("                                  # launch of a block table per replayed frame");
            std::puts("--feedback                        # With --adaptive and --frames: every frame after the first renders");
            std::puts("                                  # the previous frame's map, measures its noise and plans the next");
            std::puts("                                  # map on the GPU (not with --replay); with --denoise-variance, and");
            std::puts("                                  # optionally --temporal, every frame's two halves feed the filters");
            std::puts("--denoise [<F>[,<iter>]]          # One GPU, hash stream, one frame: first-hit features of F samples");
            std::puts("                                  # per pixel (default 16), then iter edge-avoiding filter passes");
            std::puts("                                  # (default 3); --store writes the denoised image");
            std::puts("--denoise-variance [<F>[,<iter>[,<pre>]]]  # One GPU, hash stream, one frame of an even sample count as");
            std::puts("                                  # two halves, features of F samples, then the variance-guided filter:");
            std::puts("                                  # pre prefilter passes (default 2), iter iterations (default 3)");
            std::puts("--temporal [<N>]                  # With --frames and --denoise or --denoise-variance: every frame takes");
            std::puts("                                  # a sample range of its own and is integrated into a per-pixel");
            std::puts("                                  # history of at most N frames (default 8) ahead of the filter");
            std::puts("--reproject                       # With --temporal: a motion pass per frame, and the history follows");
            std::puts("                                  # camera and sphere motion instead of staying in place");
            std::puts("--camera-step <S>                 # With --temporal: frame k's camera at (13 + S k, 11, -3 + 2 S k),");
            std::puts("                                  # looking at the origin (default 0)");
            return 0;
        } else if (a == "--adaptive") {
            if (i + 1 >= argc || !parse_adaptive(argv[i + 1], ad)) {
                std::fprintf(stderr, "--adaptive needs THRESHOLD[,MIN[,STEP]]\n");
                return 2;
            }
            ++i;
            adaptive = true;
        } else if (a == "--denoise") {
            denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_denoise(argv[i + 1], feature_samples, denoise_iterations)) {
                    std::fprintf(stderr, "--denoise takes F[,ITER]\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--denoise-variance") {
            denoise_variance = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_denoise_variance(argv[i + 1], dv_feature_samples, dv.iterations, dv.prefilter)) {
                    std::fprintf(stderr, "--denoise-variance takes F[,ITER[,PRE]]\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--temporal") {
            temporal = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_u32(argv[i + 1], tp.max_history)) {
                    std::fprintf(stderr, "--temporal takes N\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--reproject") {
            reproject = true;
        } else if (a == "--camera-step") {
            char* end = nullptr;
            if (i + 1 < argc) camera_step = std::strtof(argv[i + 1], &end);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(camera_step == camera_step) ||
                camera_step - camera_step != 0.0f) {
                std::fprintf(stderr, "--camera-step needs a finite number\n");
                return 2;
            }
            ++i;
            camera_step_given = true;
        } else if (a == "--store") {
            store = true;
        } else if (a == "--feedback") {
            feedback = true;
        } else if (a == "--animate") {
            animate = true;
        } else if (a == "--rng") {
            if (i + 1 >= argc || (std::strcmp(argv[i + 1], "stream") != 0 && std::strcmp(argv[i + 1], "hash") != 0)) {
                std::fprintf(stderr, "--rng needs stream or hash\n");
                return 2;
            }
            rng_mode = std::strcmp(argv[++i], "hash") == 0 ? RT_RNG_SAMPLE_HASH : RT_RNG_PIXEL_STREAM;
            rng_explicit = true;
        } else if (a == "--map-launch") {
            if (i + 1 >= argc || (std::strcmp(argv[i + 1], "levels") != 0 && std::strcmp(argv[i + 1], "one") != 0)) {
                std::fprintf(stderr, "--map-launch needs levels or one\n");
                return 2;
            }
            map_schedule = std::strcmp(argv[++i], "one") == 0 ? RT_SAMPLE_MAP_ONE_LAUNCH : RT_SAMPLE_MAP_LEVELS;
            map_launch_given = true;
        } else if (a == "--samples" || a == "--width" || a == "--height" || a == "--gpus" || a == "--frames" ||
                   a == "--replay") {
            uint32_t v = 0;
            if (i + 1 >= argc || !parse_u32(argv[i + 1], v)) {
                std::fprintf(stderr, "%s needs an unsigned integer value\n", a.c_str());
                return 2;
            }
            ++i;
            if (a == "--samples") samples = v;
            else if (a == "--width") width = v;
            else if (a == "--height") height = v;
            else if (a == "--frames") frames = v;
            else if (a == "--replay") { replay = v; replay_given = true; }
            else gpu_count = v;
        } else {
            std::fprintf(stderr, "unknown argument: %s\n", argv[i]);
        }
    }
    if (replay_given && !(adaptive && frames > 0)) {
        std::fprintf(stderr, "--replay needs --adaptive and --frames\n");
        return 2;
    }
    if (feedback && !(adaptive && frames > 0)) {
        std::fprintf(stderr, "--feedback needs --adaptive and --frames\n");
        return 2;
    }
    if (feedback && replay_given) {
        std::fprintf(stderr, "--feedback plans every frame's map itself: it cannot run with --replay\n");
        return 2;
    }
    if (map_launch_given && !replay_given) {
        std::fprintf(stderr, "--map-launch needs --replay (with --adaptive and --frames)\n");
        return 2;
    }
    if (adaptive) {   // refused before anything renders
        if (rng_explicit && rng_mode != RT_RNG_SAMPLE_HASH) {
            std::fprintf(stderr, "--adaptive needs the counter-based stream: it cannot run with --rng stream\n");
            return 2;
        }
        if (gpu_count > 1) {
            std::fprintf(stderr, "--adaptive renders on one GPU: it cannot run with --gpus %u\n", gpu_count);
            return 2;
        }
    }
    // the one pairing of noise-driven frames with the filters: the feedback loop hands its halves over
    const bool feedback_filtered = feedback && adaptive && frames > 0 && denoise_variance && !denoise;
    if (reproject && !temporal) {
        std::fprintf(stderr, "--reproject moves the history of --temporal: it needs --temporal\n");
        return 2;
    }
    if (camera_step_given && !temporal) {
        std::fprintf(stderr, "--camera-step moves the camera of the --temporal frame loop: it needs --temporal\n");
        return 2;
    }
    if (temporal) {   // refused before anything renders
        if (!denoise && !denoise_variance) {
            std::fprintf(stderr, "--temporal feeds a filter: it needs --denoise or --denoise-variance\n");
            return 2;
        }
        if (frames == 0) {
            std::fprintf(stderr, "--temporal integrates the frames of a loop: it needs --frames\n");
            return 2;
        }
        if (gpu_count > 1) {
            std::fprintf(stderr, "--temporal runs on one GPU: it cannot run with --gpus %u\n", gpu_count);
            return 2;
        }
        if (adaptive && !feedback_filtered) {
            std::fprintf(stderr, "--temporal renders plain frames: it cannot run with --adaptive\n");
            return 2;
        }
        if (!feedback_filtered && !(rng_explicit && rng_mode == RT_RNG_SAMPLE_HASH)) {
            std::fprintf(stderr, "--temporal needs the counter-based stream: give --rng hash\n");
            return 2;
        }
        if (uint64_t(frames) * samples > 0xffffffffull) {
            std::fprintf(stderr, "--temporal gives every frame a sample range of its own: --frames %u x --samples %u exceeds 32 bits\n",
                         frames, samples);
            return 2;
        }
        if (rt_temporal_check(&tp, width, height, denoise_variance ? dv_feature_samples : feature_samples) != RT_OK) {
            std::fprintf(stderr, "--temporal: %s\n", rt_last_error());
            return 2;
        }
    }
    if (denoise_variance) {   // refused before anything renders
        if (denoise) {
            std::fprintf(stderr, "--denoise-variance is a filter of its own: it cannot run with --denoise\n");
            return 2;
        }
        if (adaptive && !feedback_filtered) {
            std::fprintf(stderr, "--denoise-variance renders two plain halves: it cannot run with --adaptive\n");
            return 2;
        }
        if (gpu_count > 1) {
            std::fprintf(stderr, "--denoise-variance runs on one GPU: it cannot run with --gpus %u\n", gpu_count);
            return 2;
        }
        if (frames > 0 && !temporal && !feedback_filtered) {
            std::fprintf(stderr, "--denoise-variance renders one frame: it cannot run with --frames\n");
            return 2;
        }
        if (feedback_filtered && uint64_t(frames) * samples > 0xffffffffull) {
            std::fprintf(stderr, "--feedback with --denoise-variance gives every frame a sample range of its own: "
                                 "--frames %u x --samples %u exceeds 32 bits\n", frames, samples);
            return 2;
        }
        if (!feedback_filtered && !(rng_explicit && rng_mode == RT_RNG_SAMPLE_HASH)) {
            std::fprintf(stderr, "--denoise-variance needs the counter-based stream: give --rng hash\n");
            return 2;
        }
        if (samples % 2u) {
            std::fprintf(stderr, "--denoise-variance splits the frame in two halves: --samples %u is odd\n", samples);
            return 2;
        }
        if (rt_denoise_variance_check(&dv, width, height, dv_feature_samples) != RT_OK) {
            std::fprintf(stderr, "--denoise-variance: %s\n", rt_last_error());
            return 2;
        }
    }
    if (denoise) {   // refused before anything renders
        if (gpu_count > 1) {
            std::fprintf(stderr, "--denoise runs on one GPU: it cannot run with --gpus %u\n", gpu_count);
            return 2;
        }
        if (frames > 0 && !temporal) {
            std::fprintf(stderr, "--denoise renders one frame: it cannot run with --frames\n");
            return 2;
        }
        if (!adaptive && !(rng_explicit && rng_mode == RT_RNG_SAMPLE_HASH)) {
            std::fprintf(stderr, "--denoise needs the counter-based stream: give --rng hash (or --adaptive)\n");
            return 2;
        }
        const rt_denoise dn = {denoise_iterations, 4.0f, 16.0f, 1.0f};
        if (rt_denoise_check(&dn, width, height, feature_samples) != RT_OK) {
            std::fprintf(stderr, "--denoise: %s\n", rt_last_error());
            return 2;
        }
    }
    int n = 0;
    if (rt_device_count(&n) != RT_OK) {
        std::fprintf(stderr, "%s\n", rt_last_error());
        return 1;
    }
    if (feedback_filtered)
        return run_feedback_filtered_frames(samples, width, height, frames, animate, store, ad, dv_feature_samples, dv,
                                            temporal ? &tp : nullptr, reproject, camera_step);
    if (temporal) {
        const rt_denoise dn = {denoise_iterations, 4.0f, 16.0f, 1.0f};
        return run_temporal_frames(samples, width, height, frames, animate, store,
                                   denoise_variance ? dv_feature_samples : feature_samples, dn,
                                   denoise_variance ? &dv : nullptr, tp, reproject, camera_step);
    }
    if (denoise_variance) return run_denoised_variance(samples, width, height, store, dv_feature_samples, dv);
    if (denoise) return run_denoised(samples, width, height, store, adaptive ? &ad : nullptr, feature_samples, denoise_iterations);
    if (adaptive && frames > 0) return run_adaptive_frames(samples, width, height, frames, animate, store, ad, replay, map_schedule, feedback);
    if (adaptive) return run_adaptive(samples, width, height, store, ad);
    if (frames > 0) return run_frames(samples, width, height, gpu_count, frames, animate, store, rng_mode);
    // ray_trace() keeps the reference's signature; its stream is selected through RT_RNG. An
    // explicit --rng wins over the caller's environment; without it RT_RNG passes through.
    if (rng_explicit) setenv("RT_RNG", rng_mode == RT_RNG_SAMPLE_HASH ? "hash" : "stream", 1);
    ray_trace(samples, store, width, height, gpu_count);
    return 0;
}
