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
#include <initializer_list>
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

using Clock = std::chrono::steady_clock;

// Everything main parses; the modes read it and nothing else.
struct Flags {
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
    rt_adaptive ad = {};

    bool hash_given() const { return rng_explicit && rng_mode == RT_RNG_SAMPLE_HASH; }
    // the one pairing of noise-driven frames with the filters: the feedback loop hands its halves over
    bool feedback_filtered() const { return feedback && adaptive && frames > 0 && denoise_variance && !denoise; }
    // the filter a mode runs is the variance-guided one with --denoise-variance, else the plain one
    rt_denoise dn() const { return {denoise_iterations, 4.0f, 16.0f, 1.0f}; }
    uint32_t filter_features() const { return denoise_variance ? dv_feature_samples : feature_samples; }
    size_t texels() const { return size_t(width) * height; }
};

// Refused before anything renders: 0, or 2 with a message naming the option.
int check_flags(const Flags& f) {
    if (f.replay_given && !(f.adaptive && f.frames > 0)) {
        std::fprintf(stderr, "--replay needs --adaptive and --frames\n");
        return 2;
    }
    if (f.feedback && !(f.adaptive && f.frames > 0)) {
        std::fprintf(stderr, "--feedback needs --adaptive and --frames\n");
        return 2;
    }
    if (f.feedback && f.replay_given) {
        std::fprintf(stderr, "--feedback plans every frame's map itself: it cannot run with --replay\n");
        return 2;
    }
    if (f.map_launch_given && !f.replay_given) {
        std::fprintf(stderr, "--map-launch needs --replay (with --adaptive and --frames)\n");
        return 2;
    }
    if (f.adaptive) {
        if (f.rng_explicit && f.rng_mode != RT_RNG_SAMPLE_HASH) {
            std::fprintf(stderr, "--adaptive needs the counter-based stream: it cannot run with --rng stream\n");
            return 2;
        }
        if (f.gpu_count > 1) {
            std::fprintf(stderr, "--adaptive renders on one GPU: it cannot run with --gpus %u\n", f.gpu_count);
            return 2;
        }
    }
    const bool feedback_filtered = f.feedback_filtered();
    if (f.reproject && !f.temporal) {
        std::fprintf(stderr, "--reproject moves the history of --temporal: it needs --temporal\n");
        return 2;
    }
    if (f.camera_step_given && !f.temporal) {
        std::fprintf(stderr, "--camera-step moves the camera of the --temporal frame loop: it needs --temporal\n");
        return 2;
    }
    if (f.temporal) {
        if (!f.denoise && !f.denoise_variance) {
            std::fprintf(stderr, "--temporal feeds a filter: it needs --denoise or --denoise-variance\n");
            return 2;
        }
        if (f.frames == 0) {
            std::fprintf(stderr, "--temporal integrates the frames of a loop: it needs --frames\n");
            return 2;
        }
        if (f.gpu_count > 1) {
            std::fprintf(stderr, "--temporal runs on one GPU: it cannot run with --gpus %u\n", f.gpu_count);
            return 2;
        }
        if (f.adaptive && !feedback_filtered) {
            std::fprintf(stderr, "--temporal renders plain frames: it cannot run with --adaptive\n");
            return 2;
        }
        if (!feedback_filtered && !f.hash_given()) {
            std::fprintf(stderr, "--temporal needs the counter-based stream: give --rng hash\n");
            return 2;
        }
        if (uint64_t(f.frames) * f.samples > 0xffffffffull) {
            std::fprintf(stderr, "--temporal gives every frame a sample range of its own: --frames %u x --samples %u exceeds 32 bits\n",
                         f.frames, f.samples);
            return 2;
        }
        if (rt_temporal_check(&f.tp, f.width, f.height, f.filter_features()) != RT_OK) {
            std::fprintf(stderr, "--temporal: %s\n", rt_last_error());
            return 2;
        }
    }
    if (f.denoise_variance) {
        if (f.denoise) {
            std::fprintf(stderr, "--denoise-variance is a filter of its own: it cannot run with --denoise\n");
            return 2;
        }
        if (f.adaptive && !feedback_filtered) {
            std::fprintf(stderr, "--denoise-variance renders two plain halves: it cannot run with --adaptive\n");
            return 2;
        }
        if (f.gpu_count > 1) {
            std::fprintf(stderr, "--denoise-variance runs on one GPU: it cannot run with --gpus %u\n", f.gpu_count);
            return 2;
        }
        if (f.frames > 0 && !f.temporal && !feedback_filtered) {
            std::fprintf(stderr, "--denoise-variance renders one frame: it cannot run with --frames\n");
            return 2;
        }
        if (feedback_filtered && uint64_t(f.frames) * f.samples > 0xffffffffull) {
            std::fprintf(stderr, "--feedback with --denoise-variance gives every frame a sample range of its own: "
                                 "--frames %u x --samples %u exceeds 32 bits\n", f.frames, f.samples);
            return 2;
        }
        if (!feedback_filtered && !f.hash_given()) {
            std::fprintf(stderr, "--denoise-variance needs the counter-based stream: give --rng hash\n");
            return 2;
        }
        if (f.samples % 2u) {
            std::fprintf(stderr, "--denoise-variance splits the frame in two halves: --samples %u is odd\n", f.samples);
            return 2;
        }
        if (rt_denoise_variance_check(&f.dv, f.width, f.height, f.dv_feature_samples) != RT_OK) {
            std::fprintf(stderr, "--denoise-variance: %s\n", rt_last_error());
            return 2;
        }
    }
    if (f.denoise) {
        if (f.gpu_count > 1) {
            std::fprintf(stderr, "--denoise runs on one GPU: it cannot run with --gpus %u\n", f.gpu_count);
            return 2;
        }
        if (f.frames > 0 && !f.temporal) {
            std::fprintf(stderr, "--denoise renders one frame: it cannot run with --frames\n");
            return 2;
        }
        if (!f.adaptive && !f.hash_given()) {
            std::fprintf(stderr, "--denoise needs the counter-based stream: give --rng hash (or --adaptive)\n");
            return 2;
        }
        const rt_denoise dn = f.dn();
        if (rt_denoise_check(&dn, f.width, f.height, f.feature_samples) != RT_OK) {
            std::fprintf(stderr, "--denoise: %s\n", rt_last_error());
            return 2;
        }
    }
    return 0;
}

#define CLI_TRY(x)                                                                      \
    do {                                                                                \
        if (int rc_ = (x)) return rc_;                                                  \
    } while (0)

// A device plane and its owner: the one hipMalloc / hipFree pair of this file.
template <class T>
struct Plane {
    T* p = nullptr;
    Plane() = default;
    Plane(const Plane&) = delete;
    Plane& operator=(const Plane&) = delete;
    ~Plane() { (void)hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)); }
    operator T*() const { return p; }
};

// Options of the counter-based stream from sample_base on.
rt_options hash_options(uint32_t sample_base = 0) {
    rt_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.rng_mode = RT_RNG_SAMPLE_HASH;
    opt.sample_base = sample_base;
    return opt;
}

// The feedback frames' parameters, as --feedback derives them from --adaptive and --samples.
rt_sample_map_feedback feedback_params(const Flags& f) {
    rt_sample_map_feedback fb;
    std::memset(&fb, 0, sizeof(fb));
    fb.threshold = f.ad.threshold;
    fb.min_spp = f.ad.min_spp;
    fb.max_spp = f.samples;
    return fb;
}

// The RenderCallInfo of frame k: the canonical one, and with --camera-step frame k of the camera path.
int frame_rci(const Flags& f, uint32_t k, RenderCallInfo* rci) {
    CLI_RT(rt_canonical_render_call_info(f.samples, f.width, f.height, rci));
    if (f.camera_step != 0.0f) {   // it looks at the origin
        rci->camera_pos.x = 13.0f + f.camera_step * float(k);
        rci->camera_pos.z = -3.0f + (2.0f * f.camera_step) * float(k);
        rci->camera_dir = rt_vec4{-rci->camera_pos.x, -rci->camera_pos.y, -rci->camera_pos.z, 0.0f};
    }
    return 0;
}

// Scene time of a frame loop: with --animate the seconds since the loop was set up, else 0.
struct SceneClock {
    bool animate;
    Clock::time_point start = Clock::now();
    float t() const { return animate ? std::chrono::duration<float>(Clock::now() - start).count() : 0.0f; }
};

// The frame loop of every --frames mode. The caller has run its warm-up frame; this renders `frames`
// frames in windows of about a second, like the reference's ~4 s benchmark windows (:740-748): frames
// are queued until the count is reached or 1000 ms have passed, then sync() and report(k, sec).
template <class Frame, class Sync, class Report>
int window_loop(uint32_t frames, Frame frame, Sync sync, Report report) {
    uint32_t done = 0;
    while (done < frames) {
        const auto b = Clock::now();
        uint32_t k = 0;
        for (;;) {
            CLI_TRY(frame());
            ++k;
            if (done + k >= frames) break;
            if (Clock::now() - b > std::chrono::milliseconds(1000)) break;
        }
        CLI_TRY(sync());
        const double sec = std::chrono::duration<double>(Clock::now() - b).count();
        done += k;
        CLI_TRY(report(k, sec));
    }
    return 0;
}

// What every mode holds on device 0: the stream, the device planes (those its mode allocates) and the
// host scene. On every path out the stream goes first, then the planes.
struct Target {
    const Flags& f;
    hipStream_t stream = nullptr;
    Plane<float> accum, accum_a, accum_b, feat0, feat1, out_a, out_b, motion_plane;
    Plane<uint32_t> count;   // an adaptive frame's sample counts, or a halves frame's half counts
    Plane<uint8_t> rgba8;
    std::vector<Sphere> scene = std::vector<Sphere>(488);
    uint32_t cnt = 0;

    explicit Target(const Flags& flags) : f(flags) {}
    ~Target() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    int open() {
        CLI_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        CLI_HIP(rgba8.alloc(f.texels() * 4));
        return 0;
    }
    int float4_planes(std::initializer_list<Plane<float>*> planes) {
        for (Plane<float>* plane : planes) CLI_HIP(plane->alloc(f.texels() * 4));
        return 0;
    }
    int generate_scene(float t) {
        CLI_RT(rt_generate_scene(t, 11, scene.data(), uint32_t(scene.size()), &cnt));   // scene.h:79
        return 0;
    }
    // --store: the image the last call on the stream left in rgba8
    int store() {
        if (!f.store) return 0;
        std::vector<uint8_t> img(f.texels() * 4);
        CLI_HIP(hipMemcpy(img.data(), rgba8, img.size(), hipMemcpyDeviceToHost));
        CLI_RT(rt_store_ppm("render.ppm", img.data(), f.width, f.height));
        return 0;
    }
};

// A frame as the filters read it: two halves (b is null for the plain filter's one accumulator) and
// their per-texel sample counts, or with count null the spp of every texel.
struct Halves {
    const float *a, *b;
    const uint32_t* count;
    uint32_t spp;
};

// The one owner of what a single-GPU mode holds: device 0, the context, optionally a sample map, a
// temporal state and a motion object, and the Target. On every path out, failure included, it waits
// for the device (nothing queued may still write a plane that is about to be freed), destroys the
// map, the temporal state and the motion object, then the context, and then the Target goes.
struct Session : Target {
    rt_context* ctx = nullptr;
    rt_sample_map* map = nullptr;
    rt_temporal* temporal = nullptr;
    rt_motion* motion = nullptr;
    rt_sample_map_info map_info = {};
    bool map_stale = true;   // an adaptive frame has run since the map was set

    using Target::Target;
    ~Session() {
        (void)hipDeviceSynchronize();
        if (map) rt_sample_map_destroy(map);
        rt_temporal_destroy(temporal);
        rt_motion_destroy(motion);
        rt_context_destroy(ctx);
    }
    int open() {
        CLI_HIP(hipSetDevice(0));
        CLI_RT(rt_context_create(0, &ctx));
        return Target::open();
    }
    int add_map(uint32_t schedule) {
        CLI_RT(rt_sample_map_create(ctx, f.width, f.height, &map));
        CLI_RT(rt_sample_map_set_schedule(map, schedule, 0));
        return 0;
    }
    // the temporal state and the planes its stage writes
    int add_temporal(bool two_halves) {
        CLI_RT(rt_temporal_create(ctx, f.width, f.height, &temporal));
        CLI_TRY(float4_planes({&out_a}));
        return two_halves ? float4_planes({&out_b}) : 0;
    }
    int add_motion() {
        CLI_RT(rt_motion_create(ctx, f.width, f.height, &motion));
        return float4_planes({&motion_plane});
    }
    int sync() {
        CLI_HIP(hipStreamSynchronize(stream));
        return 0;
    }
    // The device half of a frame's prologue: the scene at t, built on the host and uploaded.
    int scene_at(float t) {
        CLI_TRY(generate_scene(t));
        CLI_RT(rt_set_scene(ctx, scene.data(), cnt, stream));
        return 0;
    }
    // Ahead of a frame that renders the map: the latest adaptive frame's counts, set once.
    int fresh_map() {
        if (map_stale) CLI_RT(rt_sample_map_set_from_adaptive(map, 0, stream, &map_info));
        map_stale = false;
        return 0;
    }
    // The frame as two plain halves of --samples / 2, at sample_base and sample_base + --samples / 2.
    int render_halves(const RenderCallInfo& rci, uint32_t sample_base) {
        const uint32_t half = f.samples / 2u;
        RenderCallInfo half_rci = rci;
        half_rci.samplesPerRenderCall = half;
        const rt_options first = hash_options(sample_base), second = hash_options(sample_base + half);
        CLI_RT(rt_render_device(ctx, &half_rci, nullptr, f.width, f.height, accum_a, rgba8, &first, stream));
        CLI_RT(rt_render_device(ctx, &half_rci, nullptr, f.width, f.height, accum_b, rgba8, &second, stream));
        return 0;
    }
    // The filter tail of every filtered mode, queued behind the frame `in`: the features at sample_base
    // 0; with `stage` the temporal stage on the frame (with --reproject behind the motion pass and
    // rt_motion_keep_current, else in place), which the filter then reads at spp 1; and the filter,
    // variance-guided under --denoise-variance, else plain. It writes the filtered image to rgba8.
    int filter_tail(const RenderCallInfo& rci, Halves in, bool stage) {
        const uint32_t F = f.filter_features();
        const rt_options feat_opt = hash_options();
        CLI_RT(rt_render_features_device(ctx, &rci, nullptr, f.width, f.height, feat0, feat1, F, &feat_opt, stream));
        if (stage && f.reproject) {
            CLI_RT(rt_render_motion_device(ctx, motion, &rci, motion_plane, nullptr, stream));
            CLI_RT(rt_motion_keep_current(ctx, motion, &rci, stream));
            CLI_RT(rt_temporal_reproject_device(ctx, temporal, in.a, in.b, in.count, in.spp, feat0, feat1, F, motion_plane,
                                                &f.tp, out_a, out_b, nullptr, nullptr, stream));
        } else if (stage) {
            CLI_RT(rt_temporal_accumulate_device(ctx, temporal, in.a, in.b, in.count, in.spp, feat0, feat1, F, &f.tp, out_a,
                                                 out_b, nullptr, nullptr, stream));
        }
        if (stage) in = Halves{out_a, out_b, nullptr, 1};
        if (f.denoise_variance) {
            CLI_RT(rt_denoise_variance_device(ctx, in.a, in.b, in.count, in.spp, feat0, feat1, F, f.width, f.height, &f.dv,
                                              nullptr, rgba8, stream));
        } else {
            const rt_denoise dn = f.dn();
            CLI_RT(rt_denoise_device(ctx, in.a, in.count, in.spp, feat0, feat1, F, f.width, f.height, &dn, nullptr, rgba8,
                                     stream));
        }
        return 0;
    }
};

// run_frames' side of the same: one multi-device renderer in place of the context (two rt_multi over
// the same devices would be two RCCL communicators whose grouped gathers could run in different
// orders on different devices), and every device is waited for.
struct MultiSession : Target {
    rt_multi* m = nullptr;
    uint32_t n = 1;

    using Target::Target;
    ~MultiSession() {
        for (uint32_t g = 0; g < n; g++)
            if (hipSetDevice(int(g)) == hipSuccess) (void)hipDeviceSynchronize();
        (void)hipSetDevice(0);
        rt_multi_destroy(m);
    }
    int open() {
        CLI_HIP(hipSetDevice(0));
        CLI_RT(rt_multi_create(f.gpu_count, &m));
        CLI_RT(rt_multi_device_count(m, &n));
        CLI_TRY(Target::open());   // on device 0
        return float4_planes({&accum});
    }
    int sync() {
        for (uint32_t g = 0; g < n; g++) {
            CLI_HIP(hipSetDevice(int(g)));
            CLI_HIP(hipDeviceSynchronize());
        }
        CLI_HIP(hipSetDevice(0));
        return 0;
    }
};

// --frames: n frames back to back on the rt_multi, each rebuilding the scene; frames are queued
// asynchronously, so the host builds frame k+1's scene while frame k renders.
int run_frames(const Flags& f) {
    MultiSession s(f);
    CLI_TRY(s.open());
    rt_options opt = hash_options();
    opt.rng_mode = f.rng_mode;
    const SceneClock clock{f.animate};
    auto frame = [&]() -> int {
        RenderCallInfo rci;
        CLI_TRY(s.generate_scene(clock.t()));
        CLI_TRY(frame_rci(f, 0, &rci));
        CLI_RT(rt_multi_set_scene(s.m, s.scene.data(), s.cnt));
        CLI_RT(rt_multi_render(s.m, &rci, &opt, s.accum, s.rgba8, s.stream));
        return 0;
    };
    auto sync = [&]() -> int { return s.sync(); };
    CLI_TRY(frame());   // warm-up: every context has its LPT order
    CLI_TRY(sync());
    CLI_TRY(window_loop(f.frames, frame, sync, [&](uint32_t k, double sec) -> int {
        std::printf("duration_per_frame: %.3f ms (%u frames, %u GPU, %.1f Msamples/s)\n", sec / k * 1e3, k, s.n,
                    double(f.width) * f.height * f.samples * k / sec / 1e6);
        return 0;
    }));
    return s.store();
}

// One frame of the canonical scene on device 0 (no --frames): an adaptive frame; with --denoise a
// plain or an adaptive frame and the filter tail; with --denoise-variance two plain halves and the
// filter tail. With a filter the stored image is the filtered one.
int run_frame(const Flags& f) {
    const uint32_t half = f.samples / 2u;
    Session s(f);
    CLI_TRY(s.open());
    if (f.denoise_variance) CLI_TRY(s.float4_planes({&s.accum_a, &s.accum_b, &s.feat0, &s.feat1}));
    else if (f.denoise) CLI_TRY(s.float4_planes({&s.accum, &s.feat0, &s.feat1}));
    else CLI_TRY(s.float4_planes({&s.accum}));
    if (f.denoise && f.adaptive) CLI_HIP(s.count.alloc(f.texels()));
    RenderCallInfo rci;
    CLI_TRY(s.scene_at(0.0f));
    CLI_TRY(frame_rci(f, 0, &rci));
    const rt_options opt = hash_options();
    rt_adaptive_info info = {};
    CLI_TRY(s.sync());
    const auto b = Clock::now();
    if (f.denoise_variance) {
        CLI_TRY(s.render_halves(rci, 0));
        CLI_TRY(s.filter_tail(rci, Halves{s.accum_a, s.accum_b, nullptr, half}, false));
    } else {
        if (f.adaptive)
            CLI_RT(rt_render_adaptive_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, s.count, &opt, &f.ad,
                                             &info, s.stream));
        else
            CLI_RT(rt_render_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, &opt, s.stream));
        if (f.denoise) CLI_TRY(s.filter_tail(rci, Halves{s.accum, nullptr, s.count, f.samples}, false));
    }
    CLI_TRY(s.sync());
    const double sec = std::chrono::duration<double>(Clock::now() - b).count();
    const double pixels = double(f.texels());
    if (f.denoise_variance)
        std::printf("duration_per_frame: %.3f ms (two halves of %u spp, variance-guided denoise: %u feature samples, "
                    "%u prefilter passes, %u iterations)\n",
                    sec * 1e3, half, f.dv_feature_samples, f.dv.prefilter, f.dv.iterations);
    else if (f.denoise)
        std::printf("duration_per_frame: %.3f ms (%s, mean %.2f spp, denoised: %u feature samples, %u iterations)\n", sec * 1e3,
                    f.adaptive ? "adaptive" : "plain", f.adaptive ? double(info.samples) / pixels : double(f.samples),
                    f.feature_samples, f.denoise_iterations);
    else
        std::printf("duration_per_frame: %.3f ms (adaptive, threshold %g: %u passes, mean %.2f spp of at most %u, "
                    "%u of %u tiles capped, %.1f Msamples/s)\n",
                    sec * 1e3, double(f.ad.threshold), info.passes, double(info.samples) / pixels, f.samples,
                    info.tiles_capped, info.tiles, double(info.samples) / sec / 1e6);
    return s.store();
}

// The frame loop with adaptive frames, on device 0: frame i is an adaptive frame when
// i % (replay + 1) == 0, else a sample-map frame replaying the latest adaptive frame's counts. One
// stream, the scene rebuilt per frame as run_frames does; the replays are queued without a host wait.
// --feedback: frame 0 is the adaptive frame and every later frame a feedback frame:
// it renders the map, measures it and plans the next frame's map on the device; after the one set call
// behind frame 0 the host waits for nothing but the end of a report window.
int run_adaptive_frames(const Flags& f) {
    Session s(f);
    CLI_TRY(s.open());
    // (a feedback loop's one host-planned map may hold any number of distinct counts)
    CLI_TRY(s.add_map(f.feedback ? RT_SAMPLE_MAP_ONE_LAUNCH : f.map_schedule));
    CLI_TRY(s.float4_planes({&s.accum}));
    const rt_options opt = hash_options();
    const rt_sample_map_feedback fb = feedback_params(f);
    uint64_t frame_index = 0, window_samples = 0;
    uint32_t window_replays = 0;
    const SceneClock clock{f.animate};
    auto frame = [&]() -> int {
        RenderCallInfo rci;
        CLI_TRY(s.scene_at(clock.t()));
        CLI_TRY(frame_rci(f, 0, &rci));
        if (f.feedback && frame_index > 0) {
            CLI_TRY(s.fresh_map());
            CLI_RT(rt_render_sample_map_feedback_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, nullptr, &opt,
                                                        s.map, &fb, nullptr, s.stream));
            ++window_replays;
        } else if (frame_index % (uint64_t(f.replay) + 1u) == 0) {
            rt_adaptive_info info;
            CLI_RT(rt_render_adaptive_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, nullptr, &opt, &f.ad,
                                             &info, s.stream));
            window_samples += info.samples;
            s.map_stale = true;
        } else {
            CLI_TRY(s.fresh_map());
            CLI_RT(rt_render_sample_map_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, nullptr, &opt, s.map,
                                               s.stream));
            window_samples += s.map_info.samples;
            ++window_replays;
        }
        ++frame_index;
        return 0;
    };
    auto sync = [&]() -> int { return s.sync(); };
    CLI_TRY(frame());   // warm-up: the adaptive buffers exist
    CLI_TRY(sync());
    frame_index = window_samples = window_replays = 0;
    const double pixels = double(f.texels());
    CLI_TRY(window_loop(f.frames, frame, sync, [&](uint32_t k, double sec) -> int {
        if (f.feedback) {   // (the stream is idle: the info call's wait costs nothing)
            if (window_replays) CLI_RT(rt_sample_map_get_info(s.map, &s.map_info));
            std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u feedback frames, next map mean %.2f spp "
                        "of at most %u)\n",
                        sec / k * 1e3, k, double(f.ad.threshold), window_replays, double(s.map_info.samples) / pixels, f.samples);
        } else {
            std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u replays, map launch %s, mean %.2f spp "
                        "of at most %u, %.1f Msamples/s)\n",
                        sec / k * 1e3, k, double(f.ad.threshold), window_replays,
                        f.map_schedule == RT_SAMPLE_MAP_ONE_LAUNCH ? "one" : "levels", double(window_samples) / pixels / k,
                        f.samples, double(window_samples) / sec / 1e6);
        }
        window_samples = window_replays = 0;
        return 0;
    }));
    return s.store();
}

// The filtered frame loops on device 0, everything queued on one stream; frame k renders the scene at
// t from a sample range of its own (sample_base = k x --samples), so the frames' noise is independent,
// and the filter tail follows it. They differ in how a frame's halves are produced:
// --temporal with a filter: plain frames, under --denoise-variance as two halves at k x --samples and
// k x --samples + --samples / 2, under --denoise as one accumulator; the stage always runs.
// --feedback --denoise-variance: frame 0 is an adaptive halves frame and every later frame a feedback
// halves frame (parameters as run_adaptive_frames derives them); each hands its two halves and half
// counts over (rt_half_outputs), and the stage runs with --temporal. After the one set call behind
// frame 0 nothing waits but a window's end.
// The stored image is the last frame's filtered one.
int run_filtered_frames(const Flags& f) {
    const bool fed = f.feedback_filtered(), two = f.denoise_variance;
    Session s(f);
    CLI_TRY(s.open());
    CLI_TRY(s.float4_planes({&s.accum_a, &s.feat0, &s.feat1}));
    if (two) CLI_TRY(s.float4_planes({&s.accum_b}));
    if (fed) {
        CLI_TRY(s.add_map(RT_SAMPLE_MAP_ONE_LAUNCH));
        CLI_TRY(s.float4_planes({&s.accum}));
        CLI_HIP(s.count.alloc(f.texels()));
    }
    if (f.temporal) CLI_TRY(s.add_temporal(two));
    if (f.reproject) CLI_TRY(s.add_motion());
    const rt_half_outputs halves = {s.accum_a, s.accum_b, s.count, nullptr};
    const rt_sample_map_feedback fb = feedback_params(f);
    // what the tail reads: the half counts of a feedback loop's frames, else the spp of a plain frame's planes
    const Halves in = {s.accum_a, s.accum_b, s.count, fed ? 0u : two ? f.samples / 2u : f.samples};
    uint32_t frame_index = 0, window_feedback = 0;
    const SceneClock clock{f.animate};
    auto frame = [&]() -> int {
        RenderCallInfo rci;
        CLI_TRY(s.scene_at(clock.t()));
        CLI_TRY(frame_rci(f, frame_index, &rci));
        const rt_options opt = hash_options(frame_index * f.samples);
        if (fed && frame_index == 0) {
            rt_adaptive_info info;
            CLI_RT(rt_render_adaptive_halves_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, nullptr, &opt,
                                                    &f.ad, &info, &halves, s.stream));
            s.map_stale = true;
        } else if (fed) {
            CLI_TRY(s.fresh_map());
            CLI_RT(rt_render_sample_map_feedback_halves_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum, s.rgba8, nullptr,
                                                               &opt, s.map, &fb, nullptr, &halves, s.stream));
            ++window_feedback;
        } else if (two) {
            CLI_TRY(s.render_halves(rci, opt.sample_base));
        } else {
            CLI_RT(rt_render_device(s.ctx, &rci, nullptr, f.width, f.height, s.accum_a, s.rgba8, &opt, s.stream));
        }
        CLI_TRY(s.filter_tail(rci, in, f.temporal));
        ++frame_index;
        return 0;
    };
    auto sync = [&]() -> int { return s.sync(); };
    CLI_TRY(frame());   // warm-up: the adaptive planes and the filters' band buffers exist
    if (f.temporal) CLI_RT(rt_temporal_reset(s.temporal, s.stream));
    CLI_TRY(sync());
    frame_index = window_feedback = 0;
    const uint32_t F = f.filter_features();
    const double pixels = double(f.texels());
    CLI_TRY(window_loop(f.frames, frame, sync, [&](uint32_t k, double sec) -> int {
        if (fed) {
            if (window_feedback) CLI_RT(rt_sample_map_get_info(s.map, &s.map_info));   // (the stream is idle)
            std::string stage;
            if (f.temporal) stage = ", temporal history " + std::to_string(f.tp.max_history) + (f.reproject ? " reprojected" : "");
            std::printf("duration_per_frame: %.3f ms (%u frames, adaptive, threshold %g: %u feedback frames, next map mean %.2f spp "
                        "of at most %u%s, variance-guided denoise: %u feature samples)\n",
                        sec / k * 1e3, k, double(f.ad.threshold), window_feedback, double(s.map_info.samples) / pixels, f.samples,
                        stage.c_str(), F);
        } else {
            std::printf("duration_per_frame: %.3f ms (%u frames, %u spp%s, temporal history %u%s, %s denoise: %u feature samples, "
                        "%.1f Msamples/s)\n",
                        sec / k * 1e3, k, f.samples, two ? " in two halves" : "", f.tp.max_history, f.reproject ? " reprojected" : "",
                        two ? "variance-guided" : "plain", F, double(f.width) * f.height * f.samples * k / sec / 1e6);
        }
        window_feedback = 0;
        return 0;
    }));
    return s.store();
}

}  // namespace

int main(int argc, const char** argv) {
    Flags f;
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
            if (i + 1 >= argc || !parse_adaptive(argv[i + 1], f.ad)) {
                std::fprintf(stderr, "--adaptive needs THRESHOLD[,MIN[,STEP]]\n");
                return 2;
            }
            ++i;
            f.adaptive = true;
        } else if (a == "--denoise") {
            f.denoise = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_denoise(argv[i + 1], f.feature_samples, f.denoise_iterations)) {
                    std::fprintf(stderr, "--denoise takes F[,ITER]\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--denoise-variance") {
            f.denoise_variance = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_denoise_variance(argv[i + 1], f.dv_feature_samples, f.dv.iterations, f.dv.prefilter)) {
                    std::fprintf(stderr, "--denoise-variance takes F[,ITER[,PRE]]\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--temporal") {
            f.temporal = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // the optional value
                if (!parse_u32(argv[i + 1], f.tp.max_history)) {
                    std::fprintf(stderr, "--temporal takes N\n");
                    return 2;
                }
                ++i;
            }
        } else if (a == "--reproject") {
            f.reproject = true;
        } else if (a == "--camera-step") {
            char* end = nullptr;
            if (i + 1 < argc) f.camera_step = std::strtof(argv[i + 1], &end);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(f.camera_step == f.camera_step) ||
                f.camera_step - f.camera_step != 0.0f) {
                std::fprintf(stderr, "--camera-step needs a finite number\n");
                return 2;
            }
            ++i;
            f.camera_step_given = true;
        } else if (a == "--store") {
            f.store = true;
        } else if (a == "--feedback") {
            f.feedback = true;
        } else if (a == "--animate") {
            f.animate = true;
        } else if (a == "--rng") {
            if (i + 1 >= argc || (std::strcmp(argv[i + 1], "stream") != 0 && std::strcmp(argv[i + 1], "hash") != 0)) {
                std::fprintf(stderr, "--rng needs stream or hash\n");
                return 2;
            }
            f.rng_mode = std::strcmp(argv[++i], "hash") == 0 ? RT_RNG_SAMPLE_HASH : RT_RNG_PIXEL_STREAM;
            f.rng_explicit = true;
        } else if (a == "--map-launch") {
            if (i + 1 >= argc || (std::strcmp(argv[i + 1], "levels") != 0 && std::strcmp(argv[i + 1], "one") != 0)) {
                std::fprintf(stderr, "--map-launch needs levels or one\n");
                return 2;
            }
            f.map_schedule = std::strcmp(argv[++i], "one") == 0 ? RT_SAMPLE_MAP_ONE_LAUNCH : RT_SAMPLE_MAP_LEVELS;
            f.map_launch_given = true;
        } else if (a == "--samples" || a == "--width" || a == "--height" || a == "--gpus" || a == "--frames" ||
                   a == "--replay") {
            uint32_t v = 0;
            if (i + 1 >= argc || !parse_u32(argv[i + 1], v)) {
                std::fprintf(stderr, "%s needs an unsigned integer value\n", a.c_str());
                return 2;
            }
            ++i;
            if (a == "--samples") f.samples = v;
            else if (a == "--width") f.width = v;
            else if (a == "--height") f.height = v;
            else if (a == "--frames") f.frames = v;
            else if (a == "--replay") { f.replay = v; f.replay_given = true; }
            else f.gpu_count = v;
        } else {
            std::fprintf(stderr, "unknown argument: %s\n", argv[i]);
        }
    }
    if (int rc = check_flags(f)) return rc;
    int n = 0;
    if (rt_device_count(&n) != RT_OK) {
        std::fprintf(stderr, "%s\n", rt_last_error());
        return 1;
    }
    if (f.feedback_filtered() || f.temporal) return run_filtered_frames(f);
    if (f.denoise_variance || f.denoise) return run_frame(f);
    if (f.adaptive) return f.frames > 0 ? run_adaptive_frames(f) : run_frame(f);
    if (f.frames > 0) return run_frames(f);
    // ray_trace() keeps the reference's signature; its stream is selected through RT_RNG. An
    // explicit --rng wins over the caller's environment; without it RT_RNG passes through.
    if (f.rng_explicit) setenv("RT_RNG", f.rng_mode == RT_RNG_SAMPLE_HASH ? "hash" : "stream", 1);
    ray_trace(f.samples, f.store, f.width, f.height, f.gpu_count);
    return 0;
}
