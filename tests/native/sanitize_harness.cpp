// sanitize_harness.cpp — the path's host C++ under AddressSanitizer + UndefinedBehaviorSanitizer
// (race detection / sanitizers row: the reference runs with its validation layers
// off, src/vulkan.h:51). Test infrastructure: built and run by tests/native/Makefile `sanitize`
// (tests/test_sanitize.py), never shipped.
//
// Driven here, with the scenes of configs 3 and 5 and the edge scenes of
// tests/test_gpu_build.py::test_device_tree_edge_cases:
//   * the host SAH and Morton LBVH builders (csrc/rt_bvh.cpp) and the host uniform grid
//     (csrc/rt_grid.cpp) — what rt_set_scene runs for scenes of up to 1 024 spheres;
//   * the grid layout of the device build (grid_layout, config 5's bounds);
//   * the multi-device partition, balancer and frame plan (csrc/rt_plan.cpp): every device count
//     1-9 over the image heights of the configs and small odd ones, random partitions, random
//     device times and row weights, malformed inputs; the tile-row partition and plan of adaptive
//     frames; every group of every plan through the pairing the logical transport executes
//     (pair_group), and mutilated groups refused;
//   * the closest-hit probe's batch staging (csrc/rt_probe_batch.cpp) and the oracle's closest-hit entries;
//   * the scatter probe's argument checks (the same file) and the oracle's orc_scatter;
//   * the single-device launch plan and the row weights (csrc/rt_launch.cpp): scenes, bands, sample
//     counts, streams, forms and tuning values of tests/test_launch_plan.py plus the extremes (one
//     CU, 1x1 and 65535x65535 bands, 0 samples, no spheres, tuning values up to 2^32), every plan
//     checked against the invariants the kernels rely on;
//   * the CPU oracle (oracle/rt_oracle.cpp): scenes, small frames in both streams, with a rows map
//     and accumulation, the tonemap.
// The geometry contract is driven here too: degenerate finite scenes (negative and
// zero radii, exact duplicates, concentric shells, a 100:1 radius ratio, radii and centres at
// 1e-30 / 1e30 and extents that overflow to inf) must build with every sphere's box inside its
// leaf's and its ancestors' boxes and listed by every grid cell it overlaps; non-finite scenes are
// only shown to first_nonfinite_geometry, which the scene calls refuse them by.
// Every structural property is checked; the process exits non-zero on the first violation (and
// the sanitizers abort on the first error).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/rt_abi.h"
#include "../../include/rt_mi355x.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_bvh.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_grid.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_launch.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_probe_batch.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_plan.h"

extern "C" {
int orc_generate_scene(float t, uint32_t K, Sphere* out, uint32_t capacity, uint32_t* count);
int orc_closest_hits(const Sphere* spheres, uint32_t n, const float* rays6, uint32_t n_rays, int gated,
                     uint32_t* out_id, float* out_t, int threads);
int orc_report_t(const Sphere* spheres, uint32_t n, const float* rays6, uint32_t n_rays, const uint32_t* ids,
                 float* out_t);
int orc_scatter(const Sphere* spheres, uint32_t n, const float* rays6, const uint32_t* ids, const float* t,
                const uint32_t* seeds, uint32_t n_cases, float* out_p, float* out_att, float* out_sd, float* out_dnext,
                uint32_t* out_scatter, uint32_t* out_seed);
int orc_render(const Sphere* spheres, uint32_t n, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_w,
               uint32_t band_h, const rt_options* opt, float* accum, uint8_t* out, uint64_t* stats3, int threads);
int orc_resolve(const float* acc, uint64_t n_texels, uint32_t spp, uint8_t* out);
}

namespace {

int g_checks = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        g_checks++;                                                                          \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

std::vector<Sphere> scene(float t, uint32_t K) {
    uint32_t n = 0;
    orc_generate_scene(t, K, nullptr, 0, &n);
    std::vector<Sphere> s(n);
    CHECK(orc_generate_scene(t, K, s.data(), n, &n) == 0);
    return s;
}

std::vector<Sphere> spheres_at(const std::vector<float>& c, const std::vector<float>& r) {
    const std::vector<Sphere> base = scene(0.0f, 11);
    std::vector<Sphere> s(r.size());
    for (size_t i = 0; i < r.size(); i++) {
        s[i] = base[i % base.size()];
        s[i].geometry = rt_vec4{c[3 * i], c[3 * i + 1], c[3 * i + 2], r[i]};
    }
    return s;
}

// The edge scenes of tests/test_gpu_build.py::test_device_tree_edge_cases.
std::vector<std::vector<Sphere>> edge_scenes() {
    std::mt19937 g(7);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    auto uni = [&](float a, float b) { return a + (b - a) * u(g); };
    std::vector<std::vector<Sphere>> out;
    out.push_back(spheres_at({0, -1000, 1}, {1000}));                                     // one
    out.push_back(spheres_at({0, -1000, 1, 1, 0.2f, 1}, {1000, 0.2f}));                   // two
    {   // five
        std::vector<float> c, r;
        for (int i = 0; i < 5; i++) { c.insert(c.end(), {uni(-3, 3), uni(-3, 3), uni(-3, 3)}); r.push_back(0.2f); }
        out.push_back(spheres_at(c, r));
    }
    {   // dups: coincident centres
        std::vector<float> c, r;
        for (int i = 0; i < 37; i++) {
            const float x = uni(-5, 5), y = uni(-5, 5), z = uni(-5, 5);
            for (int k = 0; k < 7; k++) { c.insert(c.end(), {x, y, z}); r.push_back(uni(0.1f, 0.3f)); }
        }
        out.push_back(spheres_at(c, r));
    }
    out.push_back(spheres_at(std::vector<float>(33 * 3, 0.0f), std::vector<float>(33, 0.5f)));   // all equal
    {   // many big, tied radii
        std::vector<float> c, r;
        for (int i = 0; i < 300; i++) {
            c.insert(c.end(), {uni(-50, 50), uni(-50, 50), uni(-50, 50)});
            r.push_back(i < 200 ? 0.2f : float(3 + (i % 3)));
        }
        out.push_back(spheres_at(c, r));
    }
    {   // flat line
        std::vector<float> c, r;
        for (int i = 0; i < 129; i++) { c.insert(c.end(), {-10.0f + 20.0f * float(i) / 128.0f, 0.0f, 0.0f}); r.push_back(0.05f); }
        out.push_back(spheres_at(c, r));
    }
    // --- degenerate finite geometry: rendered as the oracle renders it ---
    auto with_radii = [](std::vector<Sphere> s, auto&& f) {
        for (size_t i = 0; i < s.size(); i++) s[i].geometry.w = f(i, s[i].geometry.w);
        return s;
    };
    // negative radii among the small spheres (every third) ...
    out.push_back(with_radii(scene(0.0f, 3), [](size_t i, float r) { return i >= 4 && i % 3 == 0 ? -r : r; }));
    // ... as the largest sphere (the ground, -1000) ...
    out.push_back(with_radii(scene(0.0f, 11), [](size_t i, float r) { return i == 0 ? -r : r; }));
    // ... and everywhere
    out.push_back(with_radii(scene(0.0f, 3), [](size_t, float r) { return -r; }));
    // zero radii among real spheres
    out.push_back(with_radii(scene(0.0f, 11), [](size_t i, float r) { return i >= 4 && i % 5 == 0 ? 0.0f : r; }));
    {   // exact duplicates: 20 positions x 9 identical records' geometry (more than one leaf each)
        std::vector<float> c, r;
        for (int i = 0; i < 20; i++) {
            const float x = uni(-5, 5), z = uni(-5, 5);
            for (int k = 0; k < 9; k++) { c.insert(c.end(), {x, 0.3f, z}); r.push_back(0.3f); }
        }
        out.push_back(spheres_at(c, r));
    }
    {   // concentric shells, both signs
        std::vector<float> c, r;
        for (int i = 0; i < 6; i++) {
            const float x = uni(-4, 4), z = uni(-4, 4);
            for (float rad : {1.0f, 0.9f, -0.8f, 0.5f, -0.45f}) { c.insert(c.end(), {x, 1.0f, z}); r.push_back(rad); }
        }
        out.push_back(spheres_at(c, r));
    }
    {   // one sphere 100 x the others, once positive and once negative
        for (float big : {20.0f, -20.0f}) {
            std::vector<float> c, r;
            for (int i = 0; i < 200; i++) { c.insert(c.end(), {uni(-8, 8), 0.2f, uni(-8, 8)}); r.push_back(0.2f); }
            c.insert(c.end(), {0.0f, 20.0f, 30.0f});
            r.push_back(big);
            out.push_back(spheres_at(c, r));
        }
    }
    return out;
}

// Finite extremes: they must build (a refusal is for non-finite input only), with no sanitizer report.
std::vector<std::vector<Sphere>> extreme_scenes() {
    std::vector<std::vector<Sphere>> out;
    auto canon = [](size_t at, float x, float y, float z, float r) {
        std::vector<Sphere> s = scene(0.0f, 3);
        s[at].geometry = rt_vec4{x, y, z, r};
        return s;
    };
    out.push_back(canon(7, 1.0f, 0.2f, 1.0f, 1e-30f));    // a radius far below every rounding step
    out.push_back(canon(7, 1.0f, 0.2f, 1.0f, -1e-30f));
    out.push_back(canon(7, 0.0f, -1e30f, 0.0f, 1e30f));   // a second "ground", 1e30 in size
    out.push_back(canon(7, 1e30f, 0.0f, -1e30f, 0.2f));   // a small sphere 1e30 away: the Morton frame spans it
    {   // every sphere 1e30 in size at +-1e30: no big sphere, finite boxes of 2e30
        std::vector<float> c, r;
        for (int i = 0; i < 9; i++) {
            c.insert(c.end(), {i & 1 ? 1e30f : -1e30f, i & 2 ? 1e30f : -1e30f, i & 4 ? 1e30f : -1e30f});
            r.push_back(i % 3 == 2 ? -1e30f : 1e30f);
        }
        out.push_back(spheres_at(c, r));
    }
    {   // finite spheres whose boxes and Morton / SAH extents overflow to +-inf
        std::vector<float> c, r;
        for (int i = 0; i < 37; i++) {
            c.insert(c.end(), {i & 1 ? 3e38f : -3e38f, i & 2 ? 3e38f : -3e38f, i & 4 ? 3e38f : float(i)});
            r.push_back(1e38f);
        }
        out.push_back(spheres_at(c, r));
    }
    return out;
}

// Non-finite geometry is refused by index (rt_grid.h first_nonfinite_geometry) before any builder
// runs: the builders are never called on these scenes.
void check_nonfinite_refused() {
    const std::vector<Sphere> base = scene(0.0f, 11);
    const uint32_t n = uint32_t(base.size());
    CHECK(rt::first_nonfinite_geometry(base.data(), n) == n);
    CHECK(rt::first_nonfinite_geometry(base.data(), 0) == 0);
    CHECK(rt::first_nonfinite_geometry(nullptr, 0) == 0);
    const float nan = std::nanf(""), inf = INFINITY;
    for (uint32_t at : {0u, n / 2, n - 1}) {
        for (int kind = 0; kind < 6; kind++) {
            std::vector<Sphere> s = base;
            rt_vec4& g = s[at].geometry;
            switch (kind) {
                case 0: g.w = nan; break;    // NaN radius
                case 1: g.y = nan; break;    // NaN centre
                case 2: g.w = inf; break;    // +inf radius
                case 3: g.x = -inf; break;   // -inf centre
                case 4: g.w = -inf; break;
                default: g.z = inf; break;
            }
            CHECK(rt::first_nonfinite_geometry(s.data(), n) == at);
            CHECK(rt::first_nonfinite_geometry(s.data(), at) == at);   // a prefix without it is clean
            s[n - 1].geometry.x = nan;                                // a later one does not hide the first
            CHECK(rt::first_nonfinite_geometry(s.data(), n) == at);
        }
    }
    // finite extremes and negative / zero radii are not refused
    for (const auto& s : extreme_scenes()) CHECK(rt::first_nonfinite_geometry(s.data(), uint32_t(s.size())) == s.size());
    std::vector<Sphere> s = base;
    s[3].geometry.w = -1.0f;
    s[4].geometry.w = 0.0f;
    s[5].geometry.w = -0.0f;
    s[6].geometry.x = 1e-45f;   // a denormal
    CHECK(rt::first_nonfinite_geometry(s.data(), n) == n);
}

// The box the kernels' AABB gate tests for a sphere: centre -/+ |radius|.
void sphere_box(const Sphere& s, float lo[3], float hi[3]) {
    const float c[3] = {s.geometry.x, s.geometry.y, s.geometry.z}, r = std::fabs(s.geometry.w);
    for (int k = 0; k < 3; k++) { lo[k] = c[k] - r; hi[k] = c[k] + r; }
}

// Every sphere of a leaf lies inside the leaf's box and every ancestor's, up to the root.
void check_tree_contains(const std::vector<Sphere>& s, const rt::HostBvh& b) {
    std::vector<uint32_t> chain;   // the inner nodes whose subtree holds node j
    for (uint32_t j = 0; j < b.nodes.size(); j++) {
        while (!chain.empty() && b.nodes[chain.back()].escape <= j) chain.pop_back();   // (the last escapes are ~0u)
        const rt::BvhNode& nd = b.nodes[j];
        if (nd.first_count == 0u) {
            chain.push_back(j);
            continue;
        }
        const uint32_t first = nd.first_count >> 4, count = nd.first_count & 15u;
        CHECK(count >= 1 && count <= 4 && size_t(first) + count <= b.leaf_ids.size());
        chain.push_back(j);
        for (uint32_t k = first; k < first + count; k++) {
            const uint32_t id = b.leaf_ids[k];
            CHECK(id < s.size());
            float lo[3], hi[3];
            sphere_box(s[id], lo, hi);
            for (uint32_t a : chain) {
                const rt::BvhNode& an = b.nodes[a];
                CHECK(lo[0] >= an.lox && lo[1] >= an.loy && lo[2] >= an.loz);
                CHECK(hi[0] <= an.hix && hi[1] <= an.hiy && hi[2] <= an.hiz);
            }
        }
        chain.pop_back();
    }
}

// Every cell a small sphere's box overlaps (no margin) lists the sphere; each cell's ids ascend.
void check_grid_contains(const std::vector<Sphere>& s, const rt::HostBvh& b, const rt::HostGrid& grid) {
    const rt::GridInfo& gi = grid.info;
    for (uint32_t c = 0; c < gi.n_cells; c++)
        for (uint32_t j = grid.cell_start[c] + 1; j < grid.cell_start[c + 1]; j++) CHECK(grid.ids[j - 1] < grid.ids[j]);
    std::vector<char> is_big(s.size(), 0);
    for (uint32_t id : b.big_ids) is_big[id] = 1;
    for (uint32_t i = 0; i < s.size(); i++) {
        if (is_big[i]) continue;
        float lo[3], hi[3];
        sphere_box(s[i], lo, hi);
        uint32_t a[3], z[3];
        for (int k = 0; k < 3; k++) {
            const double x0 = std::floor((double(lo[k]) - gi.gmin[k]) / gi.cs[k]);
            const double x1 = std::floor((double(hi[k]) - gi.gmin[k]) / gi.cs[k]);
            CHECK(x0 <= x1);
            a[k] = uint32_t(std::min<double>(gi.n[k] - 1, std::max(0.0, x0)));
            z[k] = uint32_t(std::min<double>(gi.n[k] - 1, std::max(0.0, x1)));
        }
        for (uint32_t zz = a[2]; zz <= z[2]; zz++)
            for (uint32_t y = a[1]; y <= z[1]; y++)
                for (uint32_t x = a[0]; x <= z[0]; x++) {
                    const uint32_t c = (zz * gi.n[1] + y) * gi.n[0] + x;
                    const uint32_t* f = grid.ids.data() + grid.cell_start[c];
                    const uint32_t* l = grid.ids.data() + grid.cell_start[c + 1];
                    CHECK(std::binary_search(f, l, i));
                }
    }
}

void check_tree(const std::vector<Sphere>& s, bool sah) {
    rt::HostBvh b;
    rt::build_lbvh_host(s.data(), uint32_t(s.size()), b, sah);
    CHECK(!b.nodes.empty() || s.empty());
    CHECK(b.leaf_geom.size() == b.leaf_ids.size());
    std::vector<int> seen(s.size(), 0);
    for (uint32_t id : b.big_ids) {
        CHECK(id < s.size());
        seen[id]++;
    }
    for (size_t k = 0; k < b.leaf_ids.size(); k++) {
        // leaf slots hold the small spheres once each (padding slots repeat an id with radius 0 or
        // sit outside the count; count only slots whose record is the sphere's)
        const uint32_t id = b.leaf_ids[k];
        CHECK(id < s.size() || b.leaf_geom[k].rr <= 0.0f);
        if (id < s.size() && b.leaf_geom[k].cx == s[id].geometry.x && b.leaf_geom[k].cy == s[id].geometry.y &&
            b.leaf_geom[k].cz == s[id].geometry.z && b.leaf_geom[k].rr == s[id].geometry.w)
            seen[id]++;
    }
    for (size_t i = 0; i < s.size(); i++) CHECK(seen[i] >= 1);
    check_tree_contains(s, b);
    rt::HostGrid grid;
    if (rt::build_grid_host(s.data(), uint32_t(s.size()), b.big_ids, 64.0f * 0x1p-24f * 1100.0f, rt::kGridCellScaleHost,
                            1u << 22, grid)) {
        CHECK(grid.cell_start.size() == size_t(grid.info.n_cells) + 1);
        for (size_t c = 0; c + 1 < grid.cell_start.size(); c++) CHECK(grid.cell_start[c] <= grid.cell_start[c + 1]);
        CHECK(grid.cell_start.back() == grid.ids.size() && grid.ids.size() == grid.rec.size());
        for (uint32_t id : grid.ids) CHECK(id < s.size());
        check_grid_contains(s, b, grid);
    }
}

// The groups of a plan under the pairing the logical transport executes (rt_plan.h pair_group):
// every receive pairs with exactly one send of equal count and no send is left over; a group with
// a send removed or a count altered is refused. No transfer stands outside a group.
void check_groups(const rt::plan::FramePlan& p) {
    using namespace rt::plan;
    auto is_send = [](const PlanStep& s) { return s.op == OP_SEND || s.op == OP_SEND_COUNTS; };
    auto is_recv = [](const PlanStep& s) { return s.op == OP_RECV || s.op == OP_RECV_COUNTS; };
    std::vector<std::pair<size_t, size_t>> pairs;
    bool open = false;
    std::vector<PlanStep> group;
    for (const PlanStep& s : p.steps) {
        if (s.op == OP_GROUP_START) {
            CHECK(!open);
            open = true;
            group.clear();
        } else if (s.op == OP_GROUP_END) {
            CHECK(open && !group.empty());
            open = false;
            CHECK(pair_group(group.data(), group.size(), pairs));
            CHECK(2 * pairs.size() == group.size());
            std::vector<int> used(group.size(), 0);
            for (const auto& pr : pairs) {
                CHECK(pr.first < group.size() && pr.second < group.size());
                const PlanStep &r = group[pr.first], &t = group[pr.second];
                CHECK(is_recv(r) && is_send(t) && (r.op == OP_RECV) == (t.op == OP_SEND));
                CHECK(r.count == t.count && r.part == t.part && r.dev == t.peer && r.peer == t.dev);
                used[pr.first]++;
                used[pr.second]++;
            }
            for (int u : used) CHECK(u == 1);
            const size_t a_send = pairs[0].second;
            for (size_t k = 0; k < group.size(); k++) {
                std::vector<PlanStep> cut = group;   // one step removed: a receive without its send, or a send left over
                cut.erase(cut.begin() + std::ptrdiff_t(k));
                CHECK(!pair_group(cut.data(), cut.size(), pairs));
                std::vector<PlanStep> off = group;   // one count altered
                off[k].count += 1;
                CHECK(!pair_group(off.data(), off.size(), pairs));
            }
            std::vector<PlanStep> twice = group;     // a second send for one receive
            twice.push_back(group[a_send]);
            CHECK(!pair_group(twice.data(), twice.size(), pairs));
            CHECK(pair_group(group.data(), 0, pairs) && pairs.empty());
        } else if (open) {
            CHECK(is_send(s) || is_recv(s));
            group.push_back(s);
        } else {
            CHECK(!is_send(s) && !is_recv(s));
        }
    }
    CHECK(!open);
}

void check_plans() {
    using namespace rt::plan;
    std::mt19937 g(2024);
    const uint32_t heights[] = {1, 5, 7, 8, 27, 64, 1080, 2160};
    for (uint32_t n = 1; n <= 9; n++) {
        for (uint32_t H : heights) {
            Parts parts = strip_parts(n, H);
            std::vector<int> seen(H, 0);
            size_t mn = H, mx = 0;
            for (auto& p : parts) {
                for (uint32_t y : p.second) {
                    CHECK(y < H);
                    seen[y]++;
                }
                mn = std::min(mn, p.second.size());
                mx = std::max(mx, p.second.size());
            }
            for (uint32_t y = 0; y < H; y++) CHECK(seen[y] == 1);
            CHECK(mx - mn <= 1);
            for (int acc = 0; acc < 2; acc++) {
                Parts cp = parts;
                const FramePlan p = make_plan(1920, H, std::move(cp), acc != 0);
                const std::vector<uint32_t> v = serialize(p);
                CHECK(v.size() >= 2 && v[0] == p.parts.size() && v[1] == p.steps.size());
                check_groups(p);
            }
            {   // adaptive frames: whole tile rows, every row once, and their plan's groups
                Parts tp = tile_row_parts(n, H);
                CHECK(tp.size() == std::min(n, (H + kStrip - 1) / kStrip));
                std::vector<int> seen_t(H, 0);
                for (auto& p : tp)
                    for (uint32_t y : p.second) {
                        CHECK(y < H);
                        seen_t[y]++;
                    }
                for (uint32_t y = 0; y < H; y++) CHECK(seen_t[y] == 1);
                check_groups(make_adaptive_plan(1920, H, std::move(tp)));
            }
            // balancing: random row costs, random device times and weights, a few rounds
            std::vector<double> cost(H, 0.0);
            std::uniform_real_distribution<float> u(0.5f, 2.0f);
            for (int round = 0; round < 4; round++) {
                std::vector<float> ms(n);
                std::vector<std::vector<double>> w(n);
                for (uint32_t d = 0; d < n; d++) {
                    ms[d] = u(g) * float(parts[d].second.size());
                    if (round % 2) for (size_t k = 0; k < parts[d].second.size(); k++) w[d].push_back(u(g));
                }
                update_costs(parts, ms.data(), cost, round % 2 ? &w : nullptr);
                std::vector<double> loads;
                const double before = imbalance(parts, cost);
                rebalance(parts, cost, 0.0, &loads);
                CHECK(imbalance(parts, cost) <= before + 1e-12);
                std::vector<int> seen2(H, 0);
                for (auto& p : parts)
                    for (uint32_t y : p.second) seen2[y]++;
                for (uint32_t y = 0; y < H; y++) CHECK(seen2[y] == 1);
                std::vector<uint32_t> rows, counts;
                for (auto& p : parts) {
                    counts.push_back(uint32_t(p.second.size()));
                    rows.insert(rows.end(), p.second.begin(), p.second.end());
                }
                CHECK(!row_parts(n, H, rows.data(), counts.data()).empty());
                Parts cp = parts;
                const FramePlan fp = make_plan(64, H, std::move(cp), true);
                CHECK(!fp.steps.empty());
            }
        }
    }
    // malformed partitions and bands are refused, not read out of bounds
    const uint32_t rows_dup[] = {0, 1, 1, 3}, counts2[] = {2, 2};
    CHECK(row_parts(2, 4, rows_dup, counts2).empty());
    const uint32_t rows_big[] = {0, 1, 2, 9};
    CHECK(row_parts(2, 4, rows_big, counts2).empty());
    const uint32_t short_counts[] = {1, 2};
    CHECK(row_parts(2, 4, rows_big, short_counts).empty());
    const uint32_t bad_start[] = {3, 5}, bad_order[] = {0, 7, 5};
    CHECK(band_parts(2, 10, bad_start, 2).empty());
    CHECK(band_parts(2, 10, bad_order, 3).empty());
}

// The launch plan over the matrix of tests/test_launch_plan.py and the extremes of its domain (what
// rt_render_device and rt_debug_tune admit), occupancies from a table: every plan keeps the
// invariants the kernels rely on, or the band is refused as too large.
void check_launch_plans() {
    using namespace rt::launch;
    struct SceneSum { uint32_t n, big, nodes, leaf, grid, gpu, gn[3], cells, refs; float cs[3], rmin, rmax; };
    const float nan = std::nanf("");
    const SceneSum scenes[] = {
        {488, 4, 243, 488, 1, 0, {19, 1, 19}, 361, 836, {1.17204976f, 0.4f, 1.17292404f}, 0.2f, 0.2f},          // configs 2, 3
        {99860, 4, 67955, 135912, 1, 1, {253, 1, 253}, 64009, 0, {1.25018585f, 0.4f, 1.25017834f}, 0.2f, 0.2f}, // config 5
        {1028, 4, 529, 1060, 1, 1, {26, 1, 26}, 676, 0, {1.24084449f, 0.4f, 1.23880279f}, 0.2f, 0.2f},         // device tree
        {0, 0, 0, 0, 0, 0, {0, 0, 0}, 0, 0, {0, 0, 0}, 0.0f, 0.0f},                                            // empty
        {1, 0, 1, 4, 0, 0, {0, 0, 0}, 0, 0, {0, 0, 0}, 1000.0f, 1000.0f},                                      // one sphere
        {488, 4, 243, 488, 0, 0, {0, 0, 0}, 0, 0, {0, 0, 0}, 0.2f, 0.2f},                                      // no grid
        {488, 4, 243, 488, 1, 0, {19, 1, 19}, 361, 836, {1.17204976f, 0.4f, 1.17292404f}, 0.0f, 0.2f},         // r_min 0
        {488, 4, 243, 488, 1, 0, {19, 1, 19}, 361, 836, {1.17204976f, 0.4f, 1.17292404f}, nan, 0.2f},          // r_min NaN
        {0xffffffffu, 64, 0xffffffffu, 0xffffffffu, 1, 1, {1, 1, 1}, 0xffffffffu, 0xffffffffu, {1e-30f, 1e30f, 1.0f}, 1e-30f, 1e30f},
    };
    const uint32_t bands[][3] = {{8, 8, 0}, {64, 36, 0}, {1920, 135, 1}, {1920, 1080, 0}, {3840, 2160, 0}, {65535, 1, 0},
                                 {1, 1, 0}, {1, 65535, 1}, {65535, 65535, 0}, {65528, 65535, 1}};
    const uint32_t spps[] = {0, 1, 2, 7, 100, 1000, 10000, 1u << 19};
    const uint32_t forms[] = {0, 6, 8, 10, 12, 14, 16, 99};   // 99: brute force
    const double tunes[] = {Tuning::kUnset, 0.0, 1.0, 7.0, 4096.0, 2147483648.0, 4294967296.0};
    const uint32_t cus[] = {256, 1};
    CHECK(tuning_value_ok(-1.0) && tuning_value_ok(0.0) && tuning_value_ok(4294967296.0));
    CHECK(!tuning_value_ok(4294967297.0) && !tuning_value_ok(1e30) && !tuning_value_ok(INFINITY));
    CHECK(!tuning_value_ok(-INFINITY) && !tuning_value_ok(nan) && !tuning_value_ok(-0.5));
    CHECK(tuning_field("nope") == nullptr && tuning_key(kTuningKeys) == nullptr);
    uint64_t plans = 0, refused = 0;
    auto run = [&](Inputs& in) {
        for (uint32_t flat = 0; flat < 2; flat++) {
            in.flat_grid = flat;
            Plan p;
            const char* err = "";
            const int rc = make_plan(in, table_device(in), p, &err);
            const uint64_t n_tiles = uint64_t((in.band_w + 7) / 8) * ((in.band_h + 7) / 8);
            if (rc != RT_OK) {
                CHECK(rc == RT_ERR_INVALID_ARGUMENT && std::strcmp(err, "band too large") == 0);
                CHECK(n_tiles * 64u >= (1ull << 32));
                refused++;
                continue;
            }
            plans++;
            CHECK(p.chunks >= 1 && p.chunks <= std::max(1u, std::min(in.spp, 4096u)));
            CHECK(p.head_tiles <= n_tiles);
            const uint64_t units = 64u * (uint64_t(p.head_tiles) * p.head_chunks + (n_tiles - p.head_tiles) * p.chunks);
            CHECK(units < (1ull << 32) && p.n_units == units);
            CHECK(p.n_block_units % 64u == 0 && p.n_block_units <= p.n_units);
            CHECK(p.first_blocks <= p.n_block_units / 64u);
            CHECK(p.isolate_blocks <= p.first_blocks);
            CHECK(!p.head_tiles || p.head_chunks <= p.chunks);
            CHECK(p.grid >= 1 && p.blocks_per_cu >= 1);
            CHECK(p.accel >= 1 && p.accel < rt::ACCEL_COUNT && (p.accel == rt::ACCEL_BRUTE) == (in.accel == RT_ACCEL_BRUTE));
            CHECK(p.rows_lds == rt::kNoRowsLds || (in.has_rows && p.rows_lds % 16u == 0 && p.rows_lds + 4u * in.band_h == p.lds));
            CHECK(p.lds <= 156u * 1024u);
            CHECK(p.cull_abs > 0.0 && p.cull_near_abs > 0.0 && p.cull_near_abs <= p.cull_abs);
        }
    };
    for (const SceneSum& sc : scenes)
        for (const auto& b : bands)
            for (uint32_t spp : spps)
                for (uint32_t mode : {uint32_t(RT_RNG_PIXEL_STREAM), uint32_t(RT_RNG_SAMPLE_HASH)})
                    for (uint32_t form : forms)
                        for (uint32_t cu : cus)
                            for (uint32_t lpt = 0; lpt < 2; lpt++) {
                                Inputs in;
                                in.bytes = sizeof(in);
                                in.n_spheres = sc.n; in.n_big = sc.big; in.n_nodes = sc.nodes; in.n_leaf = sc.leaf;
                                in.has_grid = sc.grid; in.gpu_tree = sc.gpu; in.has_treelet = sc.gpu;
                                for (int k = 0; k < 3; k++) { in.grid_n[k] = sc.gn[k]; in.grid_cs[k] = sc.cs[k]; }
                                in.grid_n_cells = sc.cells; in.grid_n_refs = sc.refs;
                                in.small_rmin = sc.rmin; in.small_rmax = sc.rmax;
                                in.grid_pad_radius = 2120.0; in.cam_r = 17.29;
                                in.cu_count = cu;
                                in.band_w = b[0]; in.band_h = b[1]; in.has_rows = b[2];
                                in.spp = spp; in.rng_mode = mode; in.lpt_valid = lpt; in.pinhole_lf = 1;
                                in.accel = form == 99 ? RT_ACCEL_BRUTE : RT_ACCEL_AUTO;
                                in.reserved1 = form == 99 ? 0 : form;
                                in.reserved0 = lpt;   // the instrumented build with one of the two
                                in.block_brute = 256; in.block_walk = 768;
                                in.n_occ = 3;
                                in.occ[0] = OccRow{rt::ACCEL_BRUTE, 0xffffffffu, 0, 0xffffffffu, 6};
                                in.occ[1] = OccRow{0, 0xffffffffu, 0, 65536, 2};
                                in.occ[2] = OccRow{0, 0xffffffffu, 65537, 0xffffffffu, cu == 1 ? 0u : 1u};   // 0 blocks: planned as 1
                                run(in);
                                if (b[0] > 3840 || spp == 7 || form == 6 || form == 10) continue;   // thin the tuning sweep
                                for (uint32_t k = (spp + form + lpt) % 3; k < kTuningKeys; k += 3)
                                    for (double tv : tunes) {
                                        Inputs t = in;
                                        t.tune.*tuning_field(tuning_key(k)) = tv;
                                        run(t);
                                    }
                            }
    CHECK(plans > 100000 && refused > 0);
    {   // an occupancy the table does not answer fails the plan
        Inputs in;
        in.band_w = in.band_h = 8;
        in.block_brute = 256; in.block_walk = 768;
        Plan p;
        const char* err = "";
        CHECK(make_plan(in, table_device(in), p, &err) == RT_ERR_DEVICE);
    }
    // row weights: hand-made records (tests/test_launch_plan.py works the answers out), odd shapes
    std::vector<double> w;
    const uint32_t cost[] = {1, 2, 3, 4}, order[] = {3, 9, 0, 1};
    row_weights(cost, order, 4, 2, 16, 2, 5, 2, w);
    CHECK(w.size() == 16 && w[0] == 0.75 && w[15] == 4.375);
    row_weights(cost, nullptr, 4, 2, 12, 0, 1, 1, w);
    CHECK(w.size() == 12 && w[7] == 0.375 && w[8] == 1.75);
    row_weights(cost, order, 4, 0, 5, 2, 5, 2, w);
    CHECK(w.size() == 5 && w[4] == 0.0);
    row_weights(cost, order, 4, 3, 100, 4, 5, 2, w);   // 4 tiles do not fill two rows of 3: the last tile is dropped
    CHECK(w.size() == 100 && w[8] == 0.0);
    row_weights(nullptr, nullptr, 0, 7, 9, 0, 1, 1, w);
    CHECK(w.size() == 9 && w[0] == 0.0);
    row_weights(nullptr, nullptr, 0, 0, 0, 0, 0, 0, w);
    CHECK(w.empty());
}

void check_oracle() {
    const std::vector<Sphere> s = scene(0.0f, 11);
    const uint32_t W = 32, H = 18;
    RenderCallInfo rci;
    std::memset(&rci, 0, sizeof(rci));
    rci.samplesPerRenderCall = 2;
    rci.image_size = rt_uvec2{W, H};
    rci.camera_pos = rt_vec4{13.0f, 11.0f, -3.0f, 0.0f};
    rci.camera_dir = rt_vec4{-13.0f, -11.0f, 3.0f, 0.0f};
    for (uint32_t mode : {0u, 1u, 2u}) {
        rt_options o;
        std::memset(&o, 0, sizeof(o));
        o.rng_mode = mode;
        std::vector<float> acc(size_t(W) * H * 4);
        std::vector<uint8_t> out(size_t(W) * H * 4);
        uint64_t st[3] = {0, 0, 0};
        CHECK(orc_render(s.data(), uint32_t(s.size()), &rci, nullptr, W, H, &o, acc.data(), out.data(), st, 4) == 0);
        CHECK(st[1] == uint64_t(W) * H * 2 && st[0] >= st[1]);
        // a rows map (every third row, reversed) and accumulation on top
        std::vector<uint32_t> rows;
        for (int y = int(H) - 1; y >= 0; y -= 3) rows.push_back(uint32_t(y));
        std::vector<float> bacc(rows.size() * W * 4);
        std::vector<uint8_t> bout(rows.size() * W * 4);
        CHECK(orc_render(s.data(), uint32_t(s.size()), &rci, rows.data(), W, uint32_t(rows.size()), &o, bacc.data(),
                         bout.data(), nullptr, 3) == 0);
        for (size_t i = 0; i < rows.size(); i++)
            CHECK(std::memcmp(&bacc[i * W * 4], &acc[size_t(rows[i]) * W * 4], W * 16) == 0);
        o.accumulate = 1;
        o.sample_base = mode ? 2 : 0;
        CHECK(orc_render(s.data(), uint32_t(s.size()), &rci, nullptr, W, H, &o, acc.data(), out.data(), nullptr, 2) == 0);
        std::vector<uint8_t> res(out.size());
        CHECK(orc_resolve(acc.data(), uint64_t(W) * H, 4, res.data()) == 0);
    }
}

// The host half of rt_debug_closest_hits (csrc/rt_probe_batch.cpp): batches that end inside a band
// row, on one and one past it, the refusals, and the oracle's closest-hit entries on the staged band.
void check_probe_batch() {
    using rt::probe::kProbeBandW;
    using rt::probe::stage_batch;
    const std::vector<Sphere> s = scene(0.0f, 11);
    for (uint32_t n : {1u, 63u, kProbeBandW - 1u, kProbeBandW, kProbeBandW + 1u, 3u * kProbeBandW + 7u}) {
        std::vector<float> in(size_t(n) * 6u);   // exactly n rays: a read past them is a heap overflow
        for (uint32_t i = 0; i < n; i++) {
            const float q[6] = {0.01f * float(i), 1.0f, -3.0f + 0.001f * float(i), 0.0f, -0.1f, 1.0f};
            std::memcpy(&in[6u * i], q, sizeof(q));
        }
        in[6u * (n / 2u) + 0] = -40.0f;   // the far origin
        std::vector<float> rays;
        uint32_t band_h = 0;
        float cam_r = -1.0f;
        CHECK(stage_batch(in.data(), n, rays, &band_h, &cam_r) == 0);
        CHECK(band_h == (n + kProbeBandW - 1u) / kProbeBandW && rays.size() == size_t(band_h) * kProbeBandW * 6u);
        CHECK(std::memcmp(rays.data(), in.data(), in.size() * sizeof(float)) == 0);
        for (size_t i = n; i < size_t(band_h) * kProbeBandW; i++)
            CHECK(std::memcmp(&rays[6u * i], in.data(), 6u * sizeof(float)) == 0);
        const float* f = &in[6u * (n / 2u)];
        CHECK(cam_r == std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]));
        // the staged band through the oracle's entries (every texel is a valid ray)
        const uint32_t texels = band_h * kProbeBandW;
        std::vector<uint32_t> ids(texels), ungated(texels);
        std::vector<float> t(texels), t2(texels), raw(texels);
        CHECK(orc_closest_hits(s.data(), uint32_t(s.size()), rays.data(), texels, 1, ids.data(), t.data(), 3) == 0);
        CHECK(orc_closest_hits(s.data(), uint32_t(s.size()), rays.data(), texels, 0, ungated.data(), t2.data(), 1) == 0);
        std::vector<uint32_t> which(texels, 0u);
        CHECK(orc_report_t(s.data(), uint32_t(s.size()), rays.data(), texels, which.data(), raw.data()) == 0);
        for (uint32_t i = 0; i < texels; i++) CHECK(ids[i] == 0xffffffffu || ids[i] < s.size());
        for (int k = 0; k < 6; k++) {   // refusals: the first bad ray's index + 1, nothing staged past it
            std::vector<float> bad = in;
            bad[6u * (n - 1u) + k] = k % 2 ? INFINITY : NAN;
            CHECK(stage_batch(bad.data(), n, rays, &band_h, &cam_r) == n);
        }
        std::vector<float> bad = in;
        bad[3] = 0.0f; bad[4] = -0.0f; bad[5] = 0.0f;
        CHECK(stage_batch(bad.data(), n, rays, &band_h, &cam_r) == 1u);
        bad = in;
        bad[1] = 3e38f;   // finite, |o|^2 overflows
        CHECK(stage_batch(bad.data(), n, rays, &band_h, &cam_r) == 1u);
    }
    CHECK(orc_closest_hits(nullptr, 0, nullptr, 0, 1, nullptr, nullptr, 2) == 0);   // nothing to do
}

// The host half of rt_debug_scatter (csrc/rt_probe_batch.cpp check_scatter_batch, scatter_form_ok):
// arrays of exactly n cases, every refusal at the first and at the last case, and the oracle's
// orc_scatter on the same arrays with every material of the canonical scene.
void check_scatter_batch() {
    using rt::probe::check_scatter_batch;
    using rt::probe::scatter_form_ok;
    const std::vector<Sphere> s = scene(0.0f, 11);
    const uint32_t ns = uint32_t(s.size());
    for (uint32_t n : {1u, 63u, 257u, 1000u}) {
        std::vector<float> rays(size_t(n) * 6u), t(n);
        std::vector<uint32_t> ids(n), seeds(n);
        for (uint32_t i = 0; i < n; i++) {
            const float q[6] = {0.01f * float(i), 1.0f, -3.0f + 0.001f * float(i), 0.0f, -0.1f, 1.0f};
            std::memcpy(&rays[6u * i], q, sizeof(q));
            ids[i] = (i * 7u) % ns;
            t[i] = 0.5f + 0.001f * float(i);
            seeds[i] = 0x9e3779b9u * i;
        }
        CHECK(check_scatter_batch(rays.data(), ids.data(), t.data(), n, ns) == 0);
        std::vector<float> p(size_t(n) * 3u), att(p.size()), sd(p.size()), dn(p.size());
        std::vector<uint32_t> sc(n), after(n);
        CHECK(orc_scatter(s.data(), ns, rays.data(), ids.data(), t.data(), seeds.data(), n, p.data(), att.data(), sd.data(),
                          dn.data(), sc.data(), after.data()) == 0);
        for (uint32_t i = 0; i < n; i++) CHECK(sc[i] <= 1u);
        for (uint32_t at : {0u, n - 1u}) {
            for (int k = 0; k < 6; k++) {
                std::vector<float> bad = rays;
                bad[6u * at + k] = k % 2 ? INFINITY : NAN;
                CHECK(check_scatter_batch(bad.data(), ids.data(), t.data(), n, ns) == at + 1u);
            }
            std::vector<float> bad = rays;
            bad[6u * at + 3] = 0.0f; bad[6u * at + 4] = -0.0f; bad[6u * at + 5] = 0.0f;
            CHECK(check_scatter_batch(bad.data(), ids.data(), t.data(), n, ns) == at + 1u);
            std::vector<float> bad_t = t;
            bad_t[at] = at ? NAN : -INFINITY;
            CHECK(check_scatter_batch(rays.data(), ids.data(), bad_t.data(), n, ns) == at + 1u);
            std::vector<uint32_t> bad_id = ids;
            bad_id[at] = at ? ns : 0xffffffffu;
            CHECK(check_scatter_batch(rays.data(), bad_id.data(), t.data(), n, ns) == at + 1u);
            CHECK(orc_scatter(s.data(), ns, rays.data(), bad_id.data(), t.data(), seeds.data(), n, p.data(), att.data(),
                              sd.data(), dn.data(), sc.data(), after.data()) == -1);
        }
        CHECK(check_scatter_batch(rays.data(), ids.data(), t.data(), n, 0u) == 1u);   // an empty scene holds no id
    }
    CHECK(scatter_form_ok(0u, 0u, 512u) && scatter_form_ok(0u, 100000u, 512u));
    CHECK(scatter_form_ok(1u, 512u, 512u) && !scatter_form_ok(1u, 513u, 512u));
    CHECK(!scatter_form_ok(2u, 1u, 512u) && !scatter_form_ok(0xffffffffu, 1u, 512u));
    CHECK(orc_scatter(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                      nullptr) == 0);   // nothing to do
}

}  // namespace

int main() {
    const float ts[] = {0.0f, 1.3f};
    for (float t : ts) {
        const std::vector<Sphere> s = scene(t, 11);
        CHECK(s.size() == 488);
        check_tree(s, true);
        check_tree(s, false);
    }
    for (uint32_t K : {1u, 2u, 40u}) {
        const std::vector<Sphere> s = scene(0.5f, K);
        check_tree(s, true);
        check_tree(s, false);
    }
    for (const auto& s : edge_scenes()) {
        check_tree(s, true);
        check_tree(s, false);
    }
    for (const auto& s : extreme_scenes()) {
        check_tree(s, true);
        check_tree(s, false);
    }
    check_nonfinite_refused();
    {   // config 5: 99 860 spheres, the Morton tree (the device build's host twin) and the grid layout
        const std::vector<Sphere> s = scene(0.0f, 158);
        CHECK(s.size() == 99860);
        check_tree(s, false);
        const float lo[3] = {-158.0f, 0.0f, -158.0f}, hi[3] = {158.0f, 0.4f, 158.0f};
        rt::GridInfo gi;
        uint64_t bound = 0;
        CHECK(rt::grid_layout(lo, hi, 99856, 0.2f, 64.0f * 0x1p-24f * 330.0f, rt::kGridCellScale, gi, &bound));
        CHECK(gi.n_cells > 0 && bound >= 99856);
    }
    check_plans();
    check_launch_plans();
    check_oracle();
    check_probe_batch();
    check_scatter_batch();
    std::printf("sanitize harness: %d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
