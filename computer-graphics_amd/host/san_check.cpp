// san_check.cpp -- the library's host-side code under AddressSanitizer and
// UBSan (Makefile `sanitize`; no GPU needed): every C-ABI entry that runs on
// the host -- scene builders, the rasteriser's host geometry (camera space,
// shadow volumes, the six clip planes with the plane-6 quirks,
// rasteriser/Source/skeleton.cpp:205-241, 720-1673), the RT column window,
// the opacity maps, glibc rand(), the starfield, and the JPEG parser and
// entropy decoder on the reference's textures and on damaged copies.
//   san_check TEXTURE_DIR [JPEG_DIR]
// JPEG_DIR: every .jpg in it (tests/golden/jpeg_san: baseline, restart
// intervals, one scan per component, gray) is walked like the textures.
#include <dirent.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cg_render.h"

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return v;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void fail(const char *what, int rc)
{
    fprintf(stderr, "%s failed: %d\n", what, rc);
    exit(1);
}

// A crafted JPEG: SOI, the given segments (marker, payload), a few entropy bytes, EOI.
static std::vector<uint8_t> crafted(std::initializer_list<std::pair<int, std::vector<uint8_t>>> segs)
{
    std::vector<uint8_t> j = {0xFF, 0xD8};
    for (const auto &sg : segs) {
        j.push_back(0xFF);
        j.push_back((uint8_t)sg.first);
        const size_t len = sg.second.size() + 2;
        j.push_back((uint8_t)(len >> 8));
        j.push_back((uint8_t)len);
        j.insert(j.end(), sg.second.begin(), sg.second.end());
        if (sg.first == 0xDA)
            for (int k = 0; k < 64; ++k) j.push_back((uint8_t)(0x5A ^ k));
    }
    j.push_back(0xFF);
    j.push_back(0xD9);
    return j;
}

// Malformed headers the damaged-file loop cannot reach: each must
// be rejected (CG_E_INVALID) without reading outside the buffer or using
// undefined tables.
static int malformed_jpegs()
{
    const std::vector<uint8_t> sof1 = {8, 0, 16, 0, 16, 1, 1, 0x11, 0};                // 16x16 gray, tq 0
    std::vector<uint8_t> dqt(65, 1);
    dqt[0] = 0;                                                                        // table 0, 8-bit
    std::vector<uint8_t> dht_dc = {0x00, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // one 1-bit code
    std::vector<uint8_t> dht_dc_bad = dht_dc;
    dht_dc_bad[17] = 20;                                                               // DC category 20 > 15
    std::vector<uint8_t> dht_ac = {0x10, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x00};
    std::vector<uint8_t> dht_over = {0x10, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3};  // 3 1-bit codes
    std::vector<uint8_t> dht_ones = {0x10, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2};     // '1' used
    const std::vector<uint8_t> sos1 = {1, 1, 0x00, 0, 63, 0};
    std::vector<uint8_t> dqt_short(dqt.begin(), dqt.begin() + 20);
    std::vector<uint8_t> dht_short(dht_ac.begin(), dht_ac.begin() + 10);
    std::vector<uint8_t> dht_short_syms = {0x10, 0, 0, 0, 0, 0, 0, 0, 40, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2};
    const std::vector<uint8_t> sof3_short = {8, 0, 16, 0, 16, 3, 1, 0x11, 0};         // 3 components, 1 described
    const std::vector<uint8_t> adobe_short = {'A', 'd', 'o', 'b', 'e', 0, 100, 0, 0, 0};
    const std::vector<std::vector<uint8_t>> cases = {
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc_bad}, {0xC4, dht_ac}, {0xDA, sos1}}),   // DC s > 15
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xDA, sos1}}),                                        // no Huffman tables
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc}, {0xDA, sos1}}),                        // no AC table
        crafted({{0xC0, sof1}, {0xC4, dht_dc}, {0xC4, dht_ac}, {0xDA, sos1}}),                     // no quant table
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc}, {0xC4, dht_over}, {0xDA, sos1}}),      // over-subscribed
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc}, {0xC4, dht_ones}, {0xDA, sos1}}),      // all-ones code
        crafted({{0xDB, dqt_short}, {0xC0, sof1}}),                                                // DQT past its segment
        crafted({{0xC4, dht_short}, {0xC0, sof1}}),                                                // DHT counts cut off
        crafted({{0xC4, dht_short_syms}, {0xC0, sof1}}),                                           // DHT symbols cut off
        crafted({{0xDB, dqt}, {0xC0, sof3_short}}),                                                // SOF shorter than 3 comps
        crafted({{0xDB, dqt}, {0xC0, {8, 0, 16}}}),                                                // SOF cut off
        crafted({{0xDD, {}}, {0xDB, dqt}, {0xC0, sof1}}),                                          // DRI without its value
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC0, sof1}}),                                        // two frame headers
        crafted({{0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc}, {0xC4, dht_ac}, {0xDA, {}}}),          // empty SOS
    };
    int rejected = 0;
    for (const auto &j : cases) {
        if (cg_image_jpeg_check(j.data(), j.size()) != CG_E_INVALID) fail("malformed JPEG accepted", -1);
        ++rejected;
    }
    // an Adobe segment too short for its transform byte is ignored, not read past
    const auto ok = crafted({{0xEE, adobe_short}, {0xDB, dqt}, {0xC0, sof1}, {0xC4, dht_dc}, {0xC4, dht_ac},
                             {0xDA, sos1}});
    if (int rc = cg_image_jpeg_check(ok.data(), ok.size())) fail("well-formed crafted JPEG", rc);
    return rejected;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden/textures";
    // JPEG: the reference's maps, truncated and corrupted copies
    std::vector<std::string> files;
    for (const char *fn : {"Metal_Grill_002_basecolor.jpg", "Metal_Grill_002_opacity.jpg", "Metal_Grill_002_normal.jpg",
                           "woven1024x1024.jpg", "Wood_wicker_003_ambientOcclusion.jpg", "Wood_wicker_003_opacity.jpg",
                           "Wood_wicker_003_normal.jpg"})
        files.push_back(dir + "/" + fn);
    if (argc > 2) {
        const size_t before = files.size();
        DIR *dp = opendir(argv[2]);
        if (!dp) fail("opening the JPEG directory", -1);
        while (const dirent *de = readdir(dp)) {
            const std::string name = de->d_name;
            if (name.size() > 4 && name.compare(name.size() - 4, 4, ".jpg") == 0)
                files.push_back(std::string(argv[2]) + "/" + name);
        }
        closedir(dp);
        if (files.size() == before) fail("no .jpg in the JPEG directory", -1);
    }
    int checked = 0;
    for (const std::string &fn : files) {
        std::vector<uint8_t> j = slurp(fn);
        if (j.empty()) fail(fn.c_str(), -1);
        int w, h, c;
        if (int rc = cg_image_jpeg_info(j.data(), j.size(), &w, &h, &c)) fail("cg_image_jpeg_info", rc);
        if (int rc = cg_image_jpeg_check(j.data(), j.size())) fail("cg_image_jpeg_check", rc);
        for (size_t cut = 2; cut < j.size(); cut = cut * 3 + 5) (void)cg_image_jpeg_check(j.data(), cut);
        std::vector<uint8_t> bad = j;
        for (size_t k = bad.size() / 4; k < bad.size(); k += 1013) bad[k] ^= 0xa5;
        (void)cg_image_jpeg_check(bad.data(), bad.size());
        for (size_t k = 2; k + 1 < bad.size() && k < 700; k += 7) bad[k] = 0xff;   // damaged headers
        (void)cg_image_jpeg_info(bad.data(), bad.size(), &w, &h, &c);
        (void)cg_image_jpeg_check(bad.data(), bad.size());
        ++checked;
    }
    // rasteriser host geometry over cameras inside / outside / behind the near plane, yawed
    cg_rtri room[16], boxes[32];
    int nr = 0, nb = 0;
    if (int rc = cg_rast_load_test_model(room, 16, &nr, boxes, 32, &nb); rc < 0) fail("cg_rast_load_test_model", rc);
    std::vector<cg_rtri> out(32 * (nr + 7 * nb));
    const float cams[][3] = {{0, 0, -3.001f}, {0, 0, -1.2f}, {0.9f, 0.5f, -0.2f}, {-1.8f, 0, -1.6f},
                             {0, 0, 0.95f}, {3, -2, 2}, {0, 0, -0.99f}, {0.3f, 0.99f, -3}};
    long tris = 0;
    for (const auto &cam : cams)
        for (float yaw : {0.0f, 0.174533f, -0.8726650476455688f, 3.0f})
            for (int W : {3, 161, 900}) {
                cg_rast_params p{};
                p.width = W;
                p.height = W * 3 / 4 + 1;
                p.focal = 0.6f * (float)W;
                p.camera = cg_vec4{cam[0], cam[1], cam[2], 1.0f};
                for (int k = 0; k < 16; ++k) p.R[k] = (k % 5 == 0) ? 1.0f : 0.0f;
                p.R[0] = cosf(yaw); p.R[2] = -sinf(yaw); p.R[8] = sinf(yaw); p.R[10] = cosf(yaw);
                p.light_scene = cg_vec4{0, -0.5f, 0, 1};
                p.light_power = cg_vec3{20, 20, 20};
                p.indirect_first = 0.2f;
                p.yaw = yaw;
                cg_vec4 light;
                int n = cg_rast_prepare(&p, room, nr, boxes, nb, out.data(), (int)out.size(), &light);
                if (n < 0) fail("cg_rast_prepare", n);
                tris += n;
            }
    // RT scenes, column windows, lights, rand, opacity, starfield
    cg_tri t[64];
    cg_sphere sph;
    int n = cg_rt_load_test_model(t, 64, &sph);
    if (n < 0) fail("cg_rt_load_test_model", n);
    std::vector<cg_tri> rnd(5000);
    if (int rc = cg_rt_random_scene(0x5EED, 5000, rnd.data()); rc < 0) fail("cg_rt_random_scene", rc);
    for (float z : {-3.0f, -1.5f, 0.0f, 2.0f}) {
        cg_rt_camera cam{};
        cam.width = 1920; cam.height = 1080; cam.focal = 1080.0f;
        cam.camera = cg_vec4{0, 0, z, 1};
        for (int k = 0; k < 16; ++k) cam.R[k] = (k % 5 == 0) ? 1.0f : 0.0f;
        cam.indirect = 0.5f;
        int c0 = 0, c1 = 0;
        (void)cg_rt_frame_columns(t, n, &sph, 1, &cam, &c0, &c1);
        (void)cg_rt_frame_columns(rnd.data(), 5000, nullptr, 0, &cam, &c0, &c1);
        // the ray of a pixel's sub-ray (host-only): the frame's corners, every sub-ray, and the rejected arguments
        for (int s = -1; s <= 9; ++s)
            for (int x : {-1, 0, 1919, 1920})
                for (int y : {-1, 0, 1079, 1080}) {
                    cg_vec4 start{}, dir{};
                    const bool ok = s >= 0 && s <= 8 && x >= 0 && x < 1920 && y >= 0 && y < 1080;
                    if (cg_rt_pixel_ray(&cam, x, y, s, &start, &dir) != (ok ? CG_OK : CG_E_INVALID))
                        fail("cg_rt_pixel_ray", s);
                    if (ok && (dir.z != 1080.0f || dir.w != 1.0f || start.z != z)) fail("cg_rt_pixel_ray ray", s);
                }
        if (cg_rt_pixel_ray(nullptr, 0, 0, 4, nullptr, nullptr) != CG_E_INVALID) fail("cg_rt_pixel_ray null", -1);
        // kernel routes (host-only): identity, a yaw, NaN and huge entries, shards, large scenes
        const cg_rt_shard shards[3] = {{0, 1, 15, 0, 0, 0, 0}, {1, 3, 8, 0, 0, 0, 0}, {0, 1, 15, 135, 270, 0, 0}};
        for (int variant = 0; variant < 4; ++variant) {
            cg_rt_camera rc = cam;
            if (variant == 1) { rc.R[0] = 0.98f; rc.R[2] = -0.17f; rc.R[8] = 0.17f; rc.R[10] = 0.98f; }
            if (variant == 2) rc.R[0] = __builtin_nanf("");
            if (variant == 3) rc.R[8] = 1e30f;
            for (const cg_rt_shard &sh : shards)
                for (int nt : {28, 1000000})
                    for (int nl : {1, 64, 81})
                        if (cg_rt_route(&rc, nt, 1, nl, &sh) < 0) fail("cg_rt_route", -1);
        }
    }
    {
        // a sequence's runs (host-only): route changes, every cap from none to more than the runs,
        // the output arrays exactly cap and cap + 1 long
        std::vector<cg_rt_camera> seq(9);
        for (size_t f = 0; f < seq.size(); ++f) {
            cg_rt_camera &c = seq[f];
            c = cg_rt_camera{};
            c.width = 1920; c.height = 1080; c.focal = 1080.0f + 10.0f * (float)f;
            c.camera = cg_vec4{0, 0, -3, 1};
            for (int k = 0; k < 16; ++k) c.R[k] = (k % 5 == 0) ? 1.0f : 0.0f;
            if (f % 3 == 1) { c.R[0] = 0.98f; c.R[2] = -0.17f; c.R[8] = 0.17f; c.R[10] = 0.98f; }
            if (f == 5) c.R[5] = 0.9f;
            c.indirect = 0.5f;
        }
        for (int nt : {28, 1000000})
            for (int cap = 0; cap <= 10; ++cap) {
                std::vector<int> start((size_t)cap + 1), route((size_t)cap);
                const int runs = cg_rt_sequence_runs(seq.data(), (int)seq.size(), nt, 1, 1, nullptr, start.data(),
                                                     cap ? route.data() : nullptr, cap);
                if (runs < 1 || runs > (int)seq.size()) fail("cg_rt_sequence_runs", runs);
            }
        if (cg_rt_sequence_runs(seq.data(), -1, 28, 1, 1, nullptr, nullptr, nullptr, 0) != CG_E_INVALID)
            fail("cg_rt_sequence_runs accepted n_frames < 0", -1);
    }
    {
        // the scene grid's sizing rule (host-only): ordinary, flat in one axis, a single point (near
        // the origin and far from it, where the +-1e-4f widening rounds away), infinite, lo > hi
        const float inf = __builtin_inff(), nan = __builtin_nanf("");
        const float bounds[][6] = {{-1.02f, -1.02f, -1.02f, 1.02f, 1.02f, 1.02f},
                                   {-1, -1, 0.5f, 1, 1, 0.5f},
                                   {0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f},
                                   {1e9f, 1e9f, 1e9f, 1e9f, 1e9f, 1e9f},
                                   {-inf, -1, -1, 1, 1, inf},
                                   {inf, inf, inf, -inf, -inf, -inf},
                                   {nan, 0, 0, 1, 1, 1},
                                   {1, 1, 1, -1, -1, -1},
                                   {3.4e38f, -3.4e38f, 0, 3.4e38f, 3.4e38f, 1},
                                   {0, 0, 0, 1000, 1e-3f, 1e-3f}};
        for (const auto &b : bounds)
            for (int n : {0, 1, 4194304}) {
                float lo[3], h, inv_h;
                int res[3];
                const int rc = cg_rt_grid_dims(b, b + 3, n, lo, &h, &inv_h, res);
                if (rc != 0 && rc != 1) fail("cg_rt_grid_dims", rc);
                if (n == 0 && rc != 0) fail("cg_rt_grid_dims built a grid of no triangles", rc);
                if (rc == 1)
                    for (int k = 0; k < 3; ++k)
                        if (res[k] < 1 || res[k] > 512) fail("cg_rt_grid_dims resolution", res[k]);
            }
        float lo[3], h, inv_h;
        if (cg_rt_grid_dims(nullptr, bounds[0], 1, lo, &h, &inv_h, nullptr) != CG_E_INVALID)
            fail("cg_rt_grid_dims accepted null arguments", -1);
    }
    cg_light centre{{0, -0.5f, -0.7f, 1}, {14, 14, 14}}, area[64];
    if (int rc = cg_rt_area_lights(&centre, 0.1f, 8, area, 64); rc < 0) fail("cg_rt_area_lights", rc);
    std::vector<int32_t> r(4096);
    if (int rc = cg_glibc_rand(0, 4096, r.data())) fail("cg_glibc_rand", rc);
    if (int rc = cg_glibc_rand(11999000, 4096, r.data())) fail("cg_glibc_rand", rc);
    std::vector<uint8_t> bgr(3 * 4096), op(4096);
    for (size_t i = 0; i < bgr.size(); ++i) bgr[i] = (uint8_t)(i * 37);
    if (int rc = cg_rast_opacity_map(bgr.data(), 4096, op.data())) fail("cg_rast_opacity_map", rc);
    std::vector<float> stars(3 * 1000);
    if (int rc = cg_starfield_init(stars.data(), 1000)) fail("cg_starfield_init", rc);
    for (int k = 0; k < 100; ++k) cg_starfield_update(stars.data(), 1000, 16.0f);
    cg_rt_shard sh{1, 3, 15, 0, 0, 0, 0};
    (void)cg_rt_shard_rows(1080, &sh);
    if (cg_pix_bytes(CG_PIX_ARGB8888) != 4 || cg_pix_bytes(CG_PIX_RGB24) != 3 || cg_pix_bytes(CG_PIX_RGBA_F32) != 16 ||
        cg_pix_bytes(3) != CG_E_INVALID || cg_pix_bytes(-1) != CG_E_INVALID)
        fail("cg_pix_bytes", -1);
    // the exposure chain's host-only restatements: every bin, a two-frame chain, the refusals
    for (int b = 0; b < CG_HDR_BINS; ++b)
        if (cg_hdr_bin(cg_hdr_bin_edge(b)) != (b < CG_HDR_BINS - 1 ? b + 1 : b)) fail("cg_hdr_bin", b);
    if (cg_hdr_bin(0.0f) != -1 || cg_hdr_bin_edge(-1) != 0.0f || cg_hdr_bin_edge(CG_HDR_BINS) != 0.0f ||
        cg_hdr_luminance(1.0f, 1.0f, 1.0f) != 1.0f || cg_hdr_tone(CG_TONE_REINHARD, 1.0f, 1.0f) != 0.5f ||
        cg_hdr_tone(CG_TONE_REINHARD_WHITE, 1.0f, 4.0f) != 0.625f)
        fail("cg_hdr helpers", -1);
    {
        std::vector<uint32_t> hist(2 * CG_HDR_BINS, 0u);
        hist[127] = 7u;                    // t = 1
        hist[CG_HDR_BINS + 135] = 7u;      // t = 0.5
        cg_hdr_exposure_params ep{990, 1.0f, 1.0f / 65536.0f, 65536.0f, 0.25f};
        float scales[2] = {0.f, 0.f}, prev = 4.0f;
        if (cg_hdr_exposure(hist.data(), 2, &ep, nullptr, scales) != CG_OK || scales[0] != 1.0f || scales[1] != 0.875f)
            fail("cg_hdr_exposure", -1);
        if (cg_hdr_exposure(hist.data(), 2, &ep, &prev, scales) != CG_OK || scales[0] != 4.0f || scales[1] != 3.125f)
            fail("cg_hdr_exposure with a previous scale", -1);
        ep.permille = 1001;
        if (cg_hdr_exposure(hist.data(), 2, &ep, nullptr, scales) != CG_E_INVALID ||
            cg_hdr_exposure(hist.data(), 0, nullptr, nullptr, nullptr) != CG_E_INVALID)
            fail("cg_hdr_exposure refusals", -1);
    }
    // the bloom pyramid's host-only restatements, in buffers of exactly the sizes the layout names
    // (the index clamps at odd sizes and 1 x 1 levels are where host code could read outside them):
    // layout, pyramid and composite on 1 x 1, 2 x 1, 5 x 4 and 33 x 17 with levels 1 and 6, the
    // contract's two hand pins, the refusals
    {
        const int sizes[4][2] = {{1, 1}, {2, 1}, {5, 4}, {33, 17}};
        for (const auto &sz : sizes)
            for (int levels : {1, 6}) {
                const int W = sz[0], H = sz[1];
                std::vector<int> ws(levels), hs(levels);
                std::vector<size_t> off(levels);
                size_t total = 0;
                if (cg_hdr_bloom_layout(W, H, levels, ws.data(), hs.data(), off.data(), &total) != levels)
                    fail("cg_hdr_bloom_layout", levels);
                size_t run = 0;
                for (int k = 0, w = W, h = H; k < levels; ++k) {
                    w = (w + 1) / 2, h = (h + 1) / 2;
                    if (ws[k] != w || hs[k] != h || off[k] != run) fail("cg_hdr_bloom_layout level", k);
                    run += (size_t)w * h;
                }
                if (run != total) fail("cg_hdr_bloom_layout total", (int)total);
                std::vector<float> rgba((size_t)W * H * 4, 2.0f), pyr(total * 4, -1.0f);   // bright pass: 1.0 everywhere
                std::vector<uint32_t> argb((size_t)W * H, 0u);
                cg_hdr_bloom_params bp{levels, 1.0f, 64.0f, 0.25f};
                if (int rc = cg_hdr_bloom(rgba.data(), W, H, 1.0f, &bp, pyr.data())) fail("cg_hdr_bloom", rc);
                for (int k = 0; k < levels; ++k)   // a constant 1.0 gives U_k == levels - k + 1 exactly
                    for (size_t i = 0; i < (size_t)ws[k] * hs[k]; ++i) {
                        const float *p = &pyr[(off[k] + i) * 4];
                        const float want = (float)(levels - k);
                        if (p[0] != want || p[1] != want || p[2] != want || p[3] != 0.0f) fail("cg_hdr_bloom constant plane", k);
                    }
                for (int rule : {CG_BLOOM_RULE_RT, CG_BLOOM_RULE_RAST})
                    for (int op : {CG_TONE_LINEAR, CG_TONE_REINHARD, CG_TONE_REINHARD_WHITE}) {
                        if (int rc = cg_hdr_bloom_pack(rgba.data(), pyr.data(), W, H, 1.0f, &bp, rule, op, 4.0f, argb.data()))
                            fail("cg_hdr_bloom_pack", rc);
                        if ((argb[0] >> 24) != 128u || argb.back() != argb[0]) fail("cg_hdr_bloom_pack of a constant frame", rule);
                    }
            }
        // 16 x 16, bright 4.0 on (8..9, 8..9), one level: U_1[2..6][2..6] = 4 outer(k, k), k = (1, 4, 6, 4, 1) / 16
        std::vector<float> rgba(16 * 16 * 4, 0.0f), pyr(8 * 8 * 4);
        for (size_t i = 0; i < 256; ++i) rgba[i * 4 + 3] = 1.0f;
        for (int y = 8; y < 10; ++y)
            for (int x = 8; x < 10; ++x)
                for (int c = 0; c < 3; ++c) rgba[((size_t)y * 16 + x) * 4 + c] = 4.0f;
        cg_hdr_bloom_params one{1, 0.0f, 64.0f, 0.0f};
        if (int rc = cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, &one, pyr.data())) fail("cg_hdr_bloom", rc);
        const float k5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sum = 0.0f;
        for (int y = 0; y < 8; ++y)
            for (int x = 0; x < 8; ++x) {
                const bool in = x >= 2 && x < 7 && y >= 2 && y < 7;
                const float want = in ? 4.0f * (k5[y - 2] * k5[x - 2]) : 0.0f;
                if (pyr[((size_t)y * 8 + x) * 4] != want) fail("cg_hdr_bloom binomial pin", y * 8 + x);
                sum += pyr[((size_t)y * 8 + x) * 4];
            }
        if (pyr[(4 * 8 + 4) * 4] != 0.5625f || sum != 4.0f) fail("cg_hdr_bloom binomial centre and sum", -1);
        // a single bright pixel of 4.0 at (8, 8): U_1(4, 4) = 0.140625 with one level, 0.17016602 with two
        for (int y = 8; y < 10; ++y)
            for (int x = 8; x < 10; ++x)
                for (int c = 0; c < 3; ++c) rgba[((size_t)y * 16 + x) * 4 + c] = x == 8 && y == 8 ? 4.0f : 0.0f;
        std::vector<float> pyr2((8 * 8 + 4 * 4) * 4);
        cg_hdr_bloom_params two{2, 0.0f, 64.0f, 0.0f};
        if (cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, &one, pyr.data()) || pyr[(4 * 8 + 4) * 4] != 0.140625f ||
            cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, &two, pyr2.data()) || pyr2[(4 * 8 + 4) * 4] != 0.17016602f)
            fail("cg_hdr_bloom single pixel pin", -1);
        // refusals
        uint32_t px = 0;
        const float nan = std::nanf("");
        cg_hdr_bloom_params bad[] = {{0, 1, 64, 0.25f}, {7, 1, 64, 0.25f}, {4, -1, 64, 0.25f}, {4, nan, 64, 0.25f},
                                     {4, 1, 0, 0.25f}, {4, 1, nan, 0.25f}, {4, 1, 0x1p+65f, 0.25f}, {4, 1, 64, -1},
                                     {4, 1, 64, nan}, {4, 1, 64, 0x1p+33f}};
        for (const auto &b : bad)
            if (cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, &b, pyr2.data()) != CG_E_INVALID ||
                cg_hdr_bloom_pack(rgba.data(), pyr2.data(), 16, 16, 1.0f, &b, 0, 0, 1.0f, &px) != CG_E_INVALID)
                fail("bloom parameters accepted", b.levels);
        if (cg_hdr_bloom(nullptr, 16, 16, 1.0f, &one, pyr.data()) != CG_E_INVALID ||
            cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, nullptr, pyr.data()) != CG_E_INVALID ||
            cg_hdr_bloom(rgba.data(), 16, 16, 1.0f, &one, nullptr) != CG_E_INVALID ||
            cg_hdr_bloom(rgba.data(), 0, 16, 1.0f, &one, pyr.data()) != CG_E_INVALID ||
            cg_hdr_bloom_pack(rgba.data(), pyr.data(), 1, 1, 1.0f, &one, 2, 0, 1.0f, &px) != CG_E_INVALID ||
            cg_hdr_bloom_pack(rgba.data(), pyr.data(), 1, 1, 1.0f, &one, 0, 3, 1.0f, &px) != CG_E_INVALID ||
            cg_hdr_bloom_pack(rgba.data(), pyr.data(), 1, 1, 1.0f, &one, 0, 2, 0.0f, &px) != CG_E_INVALID ||
            cg_hdr_bloom_pack(rgba.data(), pyr.data(), 1, 1, 1.0f, &one, 0, 0, 1.0f, nullptr) != CG_E_INVALID ||
            cg_hdr_bloom_pack(rgba.data(), nullptr, 1, 1, 1.0f, &one, 0, 0, 1.0f, &px) != CG_E_INVALID ||
            cg_hdr_bloom_layout(0, 1, 1, nullptr, nullptr, nullptr, nullptr) != CG_E_INVALID ||
            cg_hdr_bloom_layout(1, 1, 0, nullptr, nullptr, nullptr, nullptr) != CG_E_INVALID ||
            cg_hdr_bloom_layout(1, 1, 7, nullptr, nullptr, nullptr, nullptr) != CG_E_INVALID ||
            cg_hdr_bloom_layout(33, 17, 6, nullptr, nullptr, nullptr, nullptr) != 6)
            fail("bloom refusals", -1);
    }
    // the JPEG encoder's host-only entries, in buffers of exactly the sizes they are told: sizes that
    // are all padding, end inside a block and inside an MCU (dummy blocks at 4:2:0) and run over
    // more than 8 restart intervals, a row stride, every capacity from 0 to the file's length on the
    // smallest, one byte short on the others; the parser takes every product back
    int encoded = 0;
    {
        const int sizes[][2] = {{1, 1}, {3, 2}, {8, 8}, {16, 16}, {33, 17}, {35, 20}, {24, 88}, {40, 150}};
        uint32_t seed = 12345u;
        for (const auto &sz : sizes)
            for (int sub : {CG_JPEG_444, CG_JPEG_420})
                for (int q : {1, 50, 100}) {
                    const int W = sz[0], H = sz[1];
                    const size_t stride = (size_t)W + 3;
                    std::vector<uint32_t> px(stride * H);   // exactly H rows: the last row's stride is not read past
                    for (auto &v : px) v = (seed = seed * 1103515245u + 12345u) >> ((seed >> 28) & 7);
                    const cg_jpeg_params prm{q, sub};
                    size_t need = 0, n = 0;
                    if (cg_image_encode_jpeg_host(px.data(), W, H, stride, &prm, nullptr, 0, &need) != CG_E_CAPACITY || !need)
                        fail("cg_image_encode_jpeg_host length query", q);
                    if ((long long)need > cg_image_jpeg_bound(W, H, sub)) fail("cg_image_jpeg_bound", (int)need);
                    std::vector<uint8_t> file(need);
                    if (int rc = cg_image_encode_jpeg_host(px.data(), W, H, stride, &prm, file.data(), need, &n))
                        fail("cg_image_encode_jpeg_host", rc);
                    int w = 0, h = 0, c = 0;
                    if (n != need || cg_image_jpeg_check(file.data(), n) || cg_image_jpeg_info(file.data(), n, &w, &h, &c) ||
                        w != W || h != H || c != 3)
                        fail("the parser on an encoded file", (int)n);
                    for (size_t cap = W == 1 ? 0 : need - 1; cap < need; ++cap) {
                        std::vector<uint8_t> part(cap);
                        if (cg_image_encode_jpeg_host(px.data(), W, H, stride, &prm, part.data(), cap, &n) != CG_E_CAPACITY ||
                            n != need || (cap && memcmp(part.data(), file.data(), cap)))
                            fail("cg_image_encode_jpeg_host capacity", (int)cap);
                    }
                    std::vector<uint8_t> hdr(629);
                    if (cg_image_jpeg_header(W, H, &prm, hdr.data(), 629) != 629 || memcmp(hdr.data(), file.data(), 629) ||
                        cg_image_jpeg_header(W, H, &prm, hdr.data(), 628) != CG_E_CAPACITY)
                        fail("cg_image_jpeg_header", W);
                    ++encoded;
                }
        const cg_jpeg_params ok{75, CG_JPEG_420}, bad_q{0, CG_JPEG_420}, bad_s{75, 1};
        uint32_t one = 0;
        uint8_t byte = 0;
        size_t n = 0;
        if (cg_image_encode_jpeg_host(&one, 0, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 1, 65536, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 1, 1, 0, &bad_q, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 1, 1, 0, &bad_s, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(nullptr, 1, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 1, 1, 0, &ok, nullptr, 1, &n) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 1, 1, 0, &ok, &byte, 1, nullptr) != CG_E_INVALID ||
            cg_image_encode_jpeg_host(&one, 2, 1, 1, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_jpeg_header(1, 1, nullptr, &byte, 1) != CG_E_INVALID ||
            cg_image_jpeg_header(1, 1, &ok, nullptr, 629) != CG_E_INVALID || cg_image_jpeg_bound(0, 1, 0) != CG_E_INVALID ||
            cg_image_jpeg_bound(1, 1, 1) != CG_E_INVALID || cg_image_jpeg_bound(65535, 65535, CG_JPEG_444) <= 0)
            fail("jpeg encoder refusals", -1);
    }
    // the PNG encoder's host-only entries the same way: tiny sizes around a band of 16 rows, both
    // colours, adaptive and fixed filters, noise (stored bands) and runs (matches), a row stride, the
    // length query with no buffer, every capacity on the smallest and one byte short on the others;
    // then the code-length rule at both limits
    int png_encoded = 0;
    {
        const int sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {5, 15}, {5, 16}, {5, 17}, {7, 33}, {70, 3}};
        uint32_t seed = 54321u;
        for (const auto &sz : sizes)
            for (int colour : {CG_PNG_RGB, CG_PNG_RGBA})
                for (int filter : {CG_PNG_FILTER_ADAPTIVE, 0, 4})
                    for (int noisy : {0, 1}) {
                        const int W = sz[0], H = sz[1];
                        const size_t stride = (size_t)W + 3;
                        std::vector<uint32_t> px(stride * H);   // exactly H rows
                        for (size_t i = 0; i < px.size(); ++i)
                            px[i] = noisy ? (seed = seed * 1103515245u + 12345u) : 0x01010101u * (uint32_t)(i / 23);
                        const cg_png_params prm{colour, filter};
                        size_t need = 0, n = 0;
                        if (cg_image_encode_png_host(px.data(), W, H, stride, &prm, nullptr, 0, &need) != CG_E_CAPACITY || !need)
                            fail("cg_image_encode_png_host length query", W);
                        if ((long long)need > cg_image_png_bound(W, H, colour)) fail("cg_image_png_bound", (int)need);
                        std::vector<uint8_t> file(need);
                        if (int rc = cg_image_encode_png_host(px.data(), W, H, stride, &prm, file.data(), need, &n))
                            fail("cg_image_encode_png_host", rc);
                        if (n != need || memcmp(file.data(), "\x89PNG\r\n\x1a\n", 8)) fail("the encoded PNG", (int)n);
                        for (size_t cap = W * H <= 2 ? 0 : need - 1; cap < need; ++cap) {
                            std::vector<uint8_t> part(cap);
                            if (cg_image_encode_png_host(px.data(), W, H, stride, &prm, part.data(), cap, &n) != CG_E_CAPACITY ||
                                n != need || (cap && memcmp(part.data(), file.data(), cap)))
                                fail("cg_image_encode_png_host capacity", (int)cap);
                        }
                        ++png_encoded;
                    }
        // Fibonacci frequencies run the limiter; exactly n entries are read and written
        for (int limit : {15, 7})
            for (int n : {1, 2, 19, 30, 286}) {
                std::vector<uint32_t> freq((size_t)n);
                uint32_t a = 1, b = 1;
                for (int i = 0; i < n; ++i) {
                    freq[(size_t)i] = i < 40 ? a : 1u + (uint32_t)i % 3u;
                    const uint32_t c = a + b;
                    a = b, b = c;
                }
                std::vector<uint8_t> len((size_t)n);
                const int rc = cg_image_png_code_lengths(freq.data(), n, limit, len.data());
                if (n > (1 << limit) ? rc != CG_E_INVALID : rc != CG_OK) fail("cg_image_png_code_lengths", n);
                unsigned long long kraft = 0;
                for (int i = 0; i < n && !rc; ++i) {
                    if (!len[(size_t)i] || len[(size_t)i] > limit) fail("a code length", i);
                    kraft += 1ull << (limit - len[(size_t)i]);
                }
                if (!rc && n > 1 && kraft != 1ull << limit) fail("the Kraft sum", n);
            }
        const cg_png_params ok{CG_PNG_RGB, CG_PNG_FILTER_ADAPTIVE}, bad_c{4, 0}, bad_f{CG_PNG_RGB, 5};
        uint32_t one = 0;
        uint8_t byte = 0;
        size_t n = 0;
        if (cg_image_encode_png_host(&one, 0, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 1, 65536, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 1, 1, 0, &bad_c, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 1, 1, 0, &bad_f, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(nullptr, 1, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 1, 1, 0, &ok, nullptr, 1, &n) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 1, 1, 0, &ok, &byte, 1, nullptr) != CG_E_INVALID ||
            cg_image_encode_png_host(&one, 2, 1, 1, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_png_code_lengths(nullptr, 1, 15, &byte) != CG_E_INVALID ||
            cg_image_png_code_lengths(&one, 1, 16, &byte) != CG_E_INVALID || cg_image_png_bound(0, 1, CG_PNG_RGB) != CG_E_INVALID ||
            cg_image_png_bound(1, 1, 3) != CG_E_INVALID || cg_image_png_bound(65535, 65535, CG_PNG_RGBA) <= 0)
            fail("png encoder refusals", -1);
    }
    // the EXR encoder's host-only entries: odd sizes around a chunk of 16 scanlines, both channel sets,
    // types and compressions, smooth pictures (deflated chunks), noise (the raw fallback) and float
    // specials, a row stride, NULL params, the length query with no buffer, every capacity on the
    // smallest and one byte short on the others; then the half rule alone and the refusals
    int exr_encoded = 0;
    {
        const int sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 15}, {3, 16}, {5, 17}, {7, 33}, {70, 3}};
        const uint32_t specials[] = {0x7F800001u, 0x7FC00000u, 0xFF800000u, 0x00000001u, 0x807FFFFFu, 0x33000000u,
                                     0x33000001u, 0x387FC000u, 0x477FEFFFu, 0x477FF000u, 0xFFFFFFFFu};
        uint32_t seed = 97531u;
        int raw_files = 0;
        for (const auto &sz : sizes)
            for (int channels : {CG_EXR_RGB, CG_EXR_RGBA})
                for (int type : {CG_EXR_HALF, CG_EXR_FLOAT})
                    for (int compression : {CG_EXR_NONE, CG_EXR_ZIP})
                        for (int content : {0, 1, 2}) {
                            const int W = sz[0], H = sz[1];
                            const size_t stride = (size_t)W + 3;
                            std::vector<float> px(stride * H * 4);   // exactly H rows
                            for (size_t i = 0; i < px.size(); ++i) {
                                const uint32_t bits = content == 1   ? (seed = seed * 1103515245u + 12345u)
                                                      : content == 2 ? specials[i % (sizeof specials / sizeof specials[0])]
                                                                     : 0x3F000000u + 0x2000u * (uint32_t)(i / 29);
                                memcpy(&px[i], &bits, 4);
                            }
                            const cg_exr_params prm{channels, type, compression, content ? 1.0f : 0.5f};
                            const bool dflt = channels == CG_EXR_RGBA && type == CG_EXR_HALF && compression == CG_EXR_ZIP && content;
                            const cg_exr_params *pp = dflt ? nullptr : &prm;   // NULL is RGBA, HALF, ZIP, scale 1
                            size_t need = 0, n = 0;
                            if (cg_image_encode_exr_host(px.data(), W, H, stride, pp, nullptr, 0, &need) != CG_E_CAPACITY || !need)
                                fail("cg_image_encode_exr_host length query", W);
                            const long long bound = cg_image_exr_bound(W, H, channels, type);
                            if ((long long)need > bound || (compression == CG_EXR_NONE && (long long)need != bound))
                                fail("cg_image_exr_bound", (int)need);
                            if (compression == CG_EXR_ZIP && (long long)need == bound) ++raw_files;   // every chunk fell back
                            std::vector<uint8_t> file(need);
                            if (int rc = cg_image_encode_exr_host(px.data(), W, H, stride, pp, file.data(), need, &n))
                                fail("cg_image_encode_exr_host", rc);
                            if (n != need || memcmp(file.data(), "\x76\x2f\x31\x01", 4)) fail("the encoded EXR", (int)n);
                            for (size_t cap = W * H <= 2 ? 0 : need - 1; cap < need; ++cap) {
                                std::vector<uint8_t> part(cap);
                                if (cg_image_encode_exr_host(px.data(), W, H, stride, pp, part.data(), cap, &n) != CG_E_CAPACITY ||
                                    n != need || (cap && memcmp(part.data(), file.data(), cap)))
                                    fail("cg_image_encode_exr_host capacity", (int)cap);
                            }
                            ++exr_encoded;
                        }
        if (!raw_files) fail("no EXR file took the raw fallback", 0);
        std::vector<float> v(sizeof specials / sizeof specials[0]);
        memcpy(v.data(), specials, sizeof specials);
        std::vector<uint16_t> hv(v.size());
        if (cg_image_exr_half(v.data(), (int)v.size(), hv.data()) || hv[0] != 0x7C01 || hv[6] != 0x0001 || hv[9] != 0x7C00)
            fail("cg_image_exr_half", hv[0]);
        uint8_t hdr[331];
        size_t n = 0;
        if (cg_image_exr_header(7, 33, nullptr, hdr, sizeof hdr, &n) || n != 331) fail("cg_image_exr_header", (int)n);
        const cg_exr_params ok{CG_EXR_RGB, CG_EXR_HALF, CG_EXR_ZIP, 1.0f}, bad_c{2, 1, 3, 1.0f}, bad_t{3, 3, 3, 1.0f},
            bad_z{3, 1, 2, 1.0f}, bad_a{4, 1, 3, INFINITY};
        float one[4] = {0, 0, 0, 0};
        uint8_t byte = 0;
        if (cg_image_encode_exr_host(one, 0, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 65536, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &bad_c, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &bad_t, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &bad_z, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &bad_a, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(nullptr, 1, 1, 0, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &ok, nullptr, 1, &n) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 1, 1, 0, &ok, &byte, 1, nullptr) != CG_E_INVALID ||
            cg_image_encode_exr_host(one, 2, 1, 1, &ok, &byte, 1, &n) != CG_E_INVALID ||
            cg_image_exr_header(1, 1, &ok, hdr, 312, &n) != CG_E_CAPACITY || n != 313 ||
            cg_image_exr_half(nullptr, 1, hv.data()) != CG_E_INVALID || cg_image_exr_bound(0, 1, CG_EXR_RGB, CG_EXR_HALF) != CG_E_INVALID ||
            cg_image_exr_bound(1, 1, 5, CG_EXR_HALF) != CG_E_INVALID || cg_image_exr_bound(65535, 65535, CG_EXR_RGBA, CG_EXR_FLOAT) <= 0)
            fail("exr encoder refusals", -1);
    }
    const int malformed = malformed_jpegs();
    printf("sanitized host code: %d JPEGs, %d malformed JPEGs rejected, %d JPEGs encoded, %d PNGs encoded, "
           "%d EXRs encoded, %ld clipped triangles, clean\n",
           checked, malformed, encoded, png_encoded, exr_encoded, tris);
    return 0;
}
