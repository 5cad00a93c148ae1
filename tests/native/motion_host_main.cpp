// motion_host_main.cpp — the host half of the motion pass (csrc/rt_motion_host.cpp: the argument
// checks, the camera of a RenderCallInfo, the motion kernel's constants and the plane sizes) as a
// stand-alone program for the sanitizer build of tests/test_motion_host.py: the accept and refusal
// cases of rt_motion_check, each refusal's message naming its field, the band check of
// rt_motion_create, the reference camera's geometry, a projection of the camera's own viewport corners
// back to the image corners, and the sizes up to the largest band. Exits 0 and prints the number of
// checks when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_motion_host.h"

namespace mo = rt::motion;

static int g_checks = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static RenderCallInfo frame(uint32_t w, uint32_t h, float px, float py, float pz) {
    RenderCallInfo r;
    std::memset(&r, 0, sizeof(r));
    r.samplesPerRenderCall = 1;
    r.image_size.x = w;
    r.image_size.y = h;
    r.camera_pos.x = px; r.camera_pos.y = py; r.camera_pos.z = pz;
    r.camera_dir.x = -px; r.camera_dir.y = -py; r.camera_dir.z = -pz;
    return r;
}

static int check(uint32_t w, uint32_t h, const RenderCallInfo* rci, const RenderCallInfo* prev, const char* names = nullptr) {
    const char* err = nullptr;
    const int rc = mo::check(w, h, rci, prev, &err);
    CHECK(err != nullptr);
    CHECK((rc == RT_OK) == (err[0] == '\0'));
    if (names) CHECK(rc == RT_ERR_INVALID_ARGUMENT && std::strstr(err, names) != nullptr);
    return rc;
}

static double dot(const float* a, const float* b) { return double(a[0]) * b[0] + double(a[1]) * b[1] + double(a[2]) * b[2]; }

// A world point through the previous camera, in double: the kernel's projection with the constants.
static void project(const mo::Projection& p, const double q[3], double w, double h, double* sx, double* sy) {
    double r[3], rel[3];
    for (int c = 0; c < 3; c++) r[c] = q[c] - p.lf[c];
    const double den = r[0] * p.wn[0] + r[1] * p.wn[1] + r[2] * p.wn[2];
    const double s = p.k / den;
    for (int c = 0; c < 3; c++) rel[c] = s * r[c] - p.u[c];
    *sx = (rel[0] * p.hor[0] + rel[1] * p.hor[1] + rel[2] * p.hor[2]) * p.ihh * w;
    *sy = -(rel[0] * p.ver[0] + rel[1] * p.ver[1] + rel[2] * p.ver[2]) * p.ivv * h;
}

int main() {
    const RenderCallInfo a = frame(64, 36, 13.0f, 11.0f, -3.0f), b = frame(64, 36, 13.2f, 11.0f, -2.6f);
    // the checks
    CHECK(check(64, 36, &a, nullptr) == RT_OK);
    CHECK(check(37, 19, &a, &b) == RT_OK);
    CHECK(check(65535, 65535, &a, &a) == RT_OK);
    CHECK(check(0, 0, &a, nullptr) == RT_OK);          // an empty band is the call's business, as rt_denoise_check's
    check(65536, 36, &a, nullptr, "width");
    check(64, 65536, &a, nullptr, "height");
    check(64, 36, nullptr, nullptr, "rci");
    check(64, 36, nullptr, &a, "rci");
    const RenderCallInfo zero_w = frame(0, 36, 1, 1, 1), zero_h = frame(64, 0, 1, 1, 1), tall = frame(64, 37, 1, 1, 1);
    check(64, 36, &zero_w, nullptr, "image_size");
    check(64, 36, &zero_h, nullptr, "image_size");
    check(64, 36, &a, &tall, "previous");
    check(64, 36, &tall, &a, "previous");
    // the band of an object
    const char* err = nullptr;
    CHECK(mo::check_band(1, 1, &err) == RT_OK && err[0] == '\0');
    CHECK(mo::check_band(65535, 65535, &err) == RT_OK);
    for (uint32_t bad : {0u, 65536u, 0xffffffffu}) {
        CHECK(mo::check_band(bad, 36, &err) == RT_ERR_INVALID_ARGUMENT && err[0] != '\0');
        CHECK(mo::check_band(64, bad, &err) == RT_ERR_INVALID_ARGUMENT && err[0] != '\0');
    }
    // the camera: hor, ver and the view direction are orthogonal, the viewport has the image's aspect
    // and the height 2 tan(12.5 deg) at the focus distance 10, ulc is its upper left corner
    mo::Camera cam;
    mo::camera(a, &cam);
    const double vh = 2.0 * std::tan(12.5 * 3.14159265358979323846 / 180.0) * 10.0;
    CHECK(std::fabs(dot(cam.hor, cam.ver)) < 1e-5);
    CHECK(std::fabs(std::sqrt(dot(cam.ver, cam.ver)) - vh) < 1e-5);
    CHECK(std::fabs(std::sqrt(dot(cam.hor, cam.hor)) - vh * 64.0 / 36.0) < 1e-5);
    CHECK(cam.lf[0] == 13.0f && cam.lf[1] == 11.0f && cam.lf[2] == -3.0f);
    CHECK(cam.size_x == 64.0f && cam.size_y == 36.0f && cam.inv_size_x == 1.0 / 64.0 && cam.inv_size_y == 1.0 / 36.0);
    float centre[3], fwd[3];
    for (int c = 0; c < 3; c++) centre[c] = cam.ulc[c] + 0.5f * cam.hor[c] - 0.5f * cam.ver[c];
    for (int c = 0; c < 3; c++) fwd[c] = centre[c] - cam.lf[c];
    CHECK(std::fabs(std::sqrt(dot(fwd, fwd)) - 10.0) < 1e-4);
    CHECK(std::fabs(dot(fwd, cam.hor)) < 1e-4 && std::fabs(dot(fwd, cam.ver)) < 1e-4);
    const float to_origin[3] = {-13.0f, -11.0f, 3.0f};
    CHECK(dot(fwd, to_origin) > 0.0);
    // the constants: wn along the view direction, k > 0, and the viewport's own points project to
    // their image coordinates
    mo::Projection pr;
    mo::projection(cam, &pr);
    CHECK(pr.k > 0.0f && dot(pr.wn, fwd) > 0.0);
    CHECK(std::fabs(dot(pr.wn, cam.hor)) < 1e-3 && std::fabs(dot(pr.wn, cam.ver)) < 1e-3);
    CHECK(std::fabs(double(pr.ihh) * dot(cam.hor, cam.hor) - 1.0) < 1e-6);
    CHECK(std::fabs(double(pr.ivv) * dot(cam.ver, cam.ver) - 1.0) < 1e-6);
    for (double fx : {0.0, 0.25, 1.0})
        for (double fy : {0.0, 0.5, 1.0})
            for (double depth : {1.0, 3.5}) {   // a point on the ray through (fx, fy), any distance along it
                double q[3], sx, sy;
                for (int c = 0; c < 3; c++)
                    q[c] = cam.lf[c] + depth * ((cam.ulc[c] + fx * cam.hor[c] - fy * cam.ver[c]) - cam.lf[c]);
                project(pr, q, 64.0, 36.0, &sx, &sy);
                CHECK(std::fabs(sx - fx * 64.0) < 1e-3 && std::fabs(sy - fy * 36.0) < 1e-3);
            }
    // a camera that looks straight down has no right vector: the camera's values are not finite, and
    // nothing else happens
    RenderCallInfo down = frame(64, 36, 0.0f, 5.0f, 0.0f);
    mo::camera(down, &cam);
    mo::projection(cam, &pr);
    CHECK(std::isnan(cam.hor[0]) && std::isnan(pr.k));
    // the sizes: 24 and 8 bytes per texel, no overflow at the largest band
    CHECK(mo::kRayFloats == 6 && mo::kHitWords == 2);
    CHECK(mo::texels(1, 1) == 1 && mo::ray_bytes(1, 1) == 24 && mo::hit_bytes(1, 1) == 8);
    CHECK(mo::ray_bytes(1920, 1080) == 2073600ull * 24ull && mo::hit_bytes(1920, 1080) == 2073600ull * 8ull);
    CHECK(mo::texels(65535, 65535) == 4294836225ull);
    CHECK(mo::ray_bytes(65535, 65535) == 4294836225ull * 24ull && mo::hit_bytes(65535, 65535) == 4294836225ull * 8ull);
    std::printf("%d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
