// rasteriser.cpp -- headless drop-in for rasteriser/Source/skeleton.cpp
// (texture mode 0, colour mode 0).
//
// Same globals (focalLength, cameraPos, yaw, R, sceneCoordinatesLightPos,
// lightPower, indirectLightPowerPerArea, originalroom/originalbox), same
// main loop and Draw(screen*) -> screen->buffer, same screenshot.bmp.  The
// whole Draw runs on the GPU (cg_rast_draw): geometry (camera space, shadow
// volumes, clipping), span setup, ordered fill and post-pass.  (cg_rast_prepare
// + cg_rast_render keep the host-geometry split available.)  Scripted keys as
// in Update() (:311-417): w s a d q e =
// light, 1 2 = indirect, U D L R z x = camera, n m = yaw, f g = focal,
// ' ' (SPACE) = colour mode, ESC = 'X'.
// Texture modes (TestModelH.h:9-10 setting / settingBoxes, skeleton.cpp:135-170):
// --setting / --setting-boxes pick the room's / boxes' texture, --textures DIR
// holds the reference's JPEG maps under their own file names (Textures/ in the
// reference tree); they are decoded like cv::imread does (cg_image_decode_jpeg).
//
//   rasteriser [--width W] [--height H] [--focal F] [--keys KEYS] [--out FILE]
//              [--setting S] [--setting-boxes B] [--textures DIR] [--batch] [--pfm FILE]
//              [--auto-exposure PERMILLE[,TARGET]] [--tonemap linear|reinhard|reinhard-white:W]
//              [--bloom THRESHOLD,INTENSITY[,LEVELS[,CAP]]]
//              [--jpeg FILE [--quality 1..100] [--subsampling 444|420]]
//              [--png FILE [--png-colour rgb|rgba] [--png-filter adaptive|0..4]]
//              [--exr FILE [--exr-type half|float] [--exr-compression zip|none] [--exr-colour rgb|rgba]]
//
// --batch: Update() runs over the whole key script first, each frame's globals
// are recorded as a cg_rast_params, and one cg_rast_draw_sequence call renders
// every frame (the rand() call index chained on the device); the screenshot is
// the last frame and randCalls the closing record, as without the flag.  What
// Draw carries from frame to frame besides, indirectLightPowerPerArea, follows
// Draw's own rule while recording, with the frame's clipped triangle count
// from cg_rast_prepare.
// --pfm FILE: the last frame's picture before PutPixelSDL clamps it (cg_rast_draw_picture), as a
// little-endian colour PFM: "PF", the size, "-1.0", then rows bottom-up of three floats a pixel.
// --auto-exposure PERMILLE[,TARGET]: the run's frames go through one cg_rast_draw_exposed call (as
// --batch records them): each frame's scale puts the upper edge of the luminance bin that holds its
// PERMILLE-th thousandth of lit pixels at TARGET (default 1), no adaptation; the screenshot is the
// last exposed frame and the scale of every frame is printed.
// --tonemap: the curve between the scaled picture and PutPixelSDL (default linear; reinhard-white:W
// maps W to white); with --tonemap alone the scale is 1.  Without these flags nothing changes.
// --bloom THRESHOLD,INTENSITY[,LEVELS[,CAP]]: the run goes through cg_rast_draw_exposed_bloom -- glare
// around what exceeds THRESHOLD after the scale, added INTENSITY times before the curve (levels 4 and
// cap 64 unless given); without --auto-exposure every scale is 1.
// --jpeg FILE: the frame --out writes, as a baseline JPEG encoded on the device (cg_image_encode_jpeg;
// quality 75 and 4:2:0 unless --quality / --subsampling say otherwise).  With --batch, every frame of
// the run, the files one after the other (a motion-JPEG stream): through cg_rast_draw_sequence_jpeg,
// or with the exposure flags each exposed frame through the encoder.
// --png FILE: the frame --out writes, as a lossless PNG encoded on the device (cg_image_encode_png; RGB
// and adaptive filters unless --png-colour / --png-filter say otherwise): it decodes to exactly the
// pixels of --out.  With --batch, also frame k of the run as FILE with .%04d before its extension:
// through cg_rast_draw_sequence_png, or with the exposure flags each exposed frame through the encoder.
// --exr FILE: the picture --pfm writes, as an OpenEXR file encoded on the device (cg_image_encode_exr;
// RGBA halves under ZIP unless --exr-type / --exr-compression / --exr-colour say otherwise).  With
// --batch, also frame k's picture as FILE with .%04d before its extension, through
// cg_rast_draw_sequence_exr; the exposure flags do not change them.
#include <cmath>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "SDLauxiliary.h"
#include "TestModelH.h"
#include "bloom_arg.h"
#include "cg_render.h"
#include "exr_arg.h"
#include "jpeg_arg.h"
#include "png_arg.h"

using namespace std;
using glm::mat4;
using glm::vec3;
using glm::vec4;

int SCREEN_WIDTH = 900, SCREEN_HEIGHT = 720;                 // :21-22
float focalLength = 512;                                      // :30
vec4 cameraPos(0, 0, -3.001, 1);                              // :31
float yaw = 0.0;                                              // :34
mat4 R(1.0f);                                                 // :35
vec4 sceneCoordinatesLightPos(0, -0.5, 0, 1);                 // :52
vec3 lightPower = 20.0f * vec3(1, 1, 1);                      // :53
vec3 indirectLightPowerPerArea = 0.15f * vec3(1, 1, 1);       // :54
int randColourSelect = 0;                                     // :81
uint64_t randCalls = 0;                                       // glibc rand() calls so far (never seeded)
vector<rast::Triangle> originalroom;                          // :84
vector<rast::Triangle> originalbox;                           // :85

static cg_ctx *g_ctx = nullptr;
static string g_keys;
static size_t g_frame = 0;
static cg_rast_params g_last;                                 // the latest frame drawn (--pfm)
static bool g_drawn = false;

static void die(int rc, const char *what)
{
    cerr << what << " failed (" << rc << "): " << (g_ctx ? cg_last_error(g_ctx) : "") << endl;
    exit(1);
}

// the globals as Draw hands them to the library
static cg_rast_params CurrentParams(const screen *screen)
{
    cg_rast_params p;
    p.width = screen->width;
    p.height = screen->height;
    p.focal = focalLength;
    p.camera = cg_vec4{cameraPos.x, cameraPos.y, cameraPos.z, cameraPos.w};
    memcpy(p.R, R.data(), sizeof(p.R));
    p.light_scene = cg_vec4{sceneCoordinatesLightPos.x, sceneCoordinatesLightPos.y,
                            sceneCoordinatesLightPos.z, sceneCoordinatesLightPos.w};
    p.light_power = cg_vec3{lightPower.x, lightPower.y, lightPower.z};
    p.indirect_first = indirectLightPowerPerArea.x;
    p.colour_mode = randColourSelect;
    p.yaw = yaw;
    p.rand_offset = randCalls;
    return p;
}

// skeleton.cpp:203-308
void Draw(screen *screen)
{
    const cg_rast_params p = CurrentParams(screen);
    g_last = p;
    g_drawn = true;
    // geometry (shadow volumes + clip), fill and post-pass all on the GPU
    cg_stats st;
    int rc = cg_rast_draw(g_ctx, &p, screen->buffer, nullptr, nullptr, &st);
    if (rc) die(rc, "cg_rast_draw");
    if (randColourSelect == 0) {
        // PixelShader leaves the global at 0.2 after the first shaded fragment (:585)
        if (st.n_tris > 0) indirectLightPowerPerArea = 0.2f * vec3(1, 1, 1);
    } else {
        randCalls += 3 * (uint64_t)st.n_shaded;              // :649-651 / :657-659 per fragment
    }
}

// --pfm, --exr: the picture of the latest frame's parameters, unclamped
static vector<float> Picture()
{
    vector<float> rgba((size_t)g_last.width * g_last.height * 4);
    int rc = cg_rast_draw_picture(g_ctx, &g_last, rgba.data(), nullptr);
    if (rc) die(rc, "cg_rast_draw_picture");
    return rgba;
}

static void SavePicturePFM(const char *path)
{
    const int W = g_last.width, H = g_last.height;
    const vector<float> rgba = Picture();
    ofstream f(path, ios::binary);
    f << "PF\n" << W << " " << H << "\n-1.0\n";
    vector<float> row((size_t)W * 3);
    for (int y = H - 1; y >= 0; --y) {   // bottom row first
        for (int x = 0; x < W; ++x) memcpy(&row[3 * x], &rgba[((size_t)y * W + x) * 4], 3 * sizeof(float));
        f.write(reinterpret_cast<const char *>(row.data()), row.size() * sizeof(float));
    }
    if (!f) {
        cerr << "cannot write " << path << endl;
        exit(1);
    }
}

// skeleton.cpp:311-417 with scripted keys
bool Update()
{
    if (g_frame >= g_keys.size()) return g_frame++ == 0;
    char key = g_keys[g_frame++];
    switch (key) {
    case 'w': sceneCoordinatesLightPos += vec4(0, 0, 0.1, 0); break;
    case 's': sceneCoordinatesLightPos += vec4(0, 0, -0.1, 0); break;
    case 'a': sceneCoordinatesLightPos += vec4(-0.1, 0, 0, 0); break;
    case 'd': sceneCoordinatesLightPos += vec4(0.1, 0, 0, 0); break;
    case 'q': sceneCoordinatesLightPos += vec4(0, -0.1, 0, 0); break;
    case 'e': sceneCoordinatesLightPos += vec4(0, 0.1, 0, 0); break;
    case '1': indirectLightPowerPerArea -= vec3(0.005f, 0.005f, 0.005f); break;
    case '2': indirectLightPowerPerArea += vec3(0.005f, 0.005f, 0.005f); break;
    case 'U': cameraPos += vec4(0, 0, 0.1, 0); break;
    case 'D': cameraPos += vec4(0, 0, -0.1, 0); break;
    case 'L': cameraPos += vec4(-0.1, 0, 0, 0); break;
    case 'R': cameraPos += vec4(0.1, 0, 0, 0); break;
    case 'z': cameraPos += vec4(0, -0.1, 0, 0); break;
    case 'x': cameraPos += vec4(0, 0.1, 0, 0); break;
    case 'n':
    case 'm':
        if (key == 'n') yaw -= 0.174533;
        else yaw += 0.174533;
        R[0][0] = cos(yaw); R[0][1] = 0; R[0][2] = -sin(yaw);
        R[1][0] = 0;        R[1][1] = 1; R[1][2] = 0;
        R[2][0] = sin(yaw); R[2][1] = 0; R[2][2] = cos(yaw);
        break;
    case ' ': randColourSelect = (randColourSelect + 1) % 3; break;   // SPACE (:406-409)
    case 'f': focalLength += 5; break;
    case 'g': focalLength -= 5; break;
    case 'X': return false;
    default: break;
    }
    return true;
}

// cv::imread(DIR/FILE, CV_LOAD_IMAGE_UNCHANGED) (:135-146) for a map of
// side n: BGR bytes, or empty if the file is absent (the reference then holds
// an empty Mat and must not render that texture).
static vector<uint8_t> read_map(const string &dir, const char *file, int n)
{
    vector<uint8_t> bytes, v;
    FILE *f = fopen((dir + "/" + file).c_str(), "rb");
    if (!f) return v;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
    fclose(f);
    int w = 0, h = 0, ch = 0;
    int rc = cg_image_jpeg_info(bytes.data(), bytes.size(), &w, &h, &ch);
    if (rc) die(rc, file);
    if (w != n || h != n || ch != 3) {
        cerr << file << ": " << w << "x" << h << "x" << ch << ", the reference indexes it as " << n << "x" << n
             << " BGR" << endl;
        exit(1);
    }
    v.resize((size_t)n * n * 3);
    rc = cg_image_decode_jpeg(g_ctx, bytes.data(), bytes.size(), v.data(), v.size());
    if (rc) die(rc, "cg_image_decode_jpeg");
    return v;
}

int main(int argc, char *argv[])
{
    string out = "screenshot.bmp", tex_dir, pfm;
    int setting = 0, setting_boxes = 0;
    bool batch = false, exposed = false;
    cg_hdr_exposure_params expo{990, 1.0f, 1.0f, 1.0f, 1.0f};   // --tonemap alone: every scale is 1
    int tone = CG_TONE_LINEAR;
    float white2 = 1.0f;
    bool bloomed = false;
    cg_hdr_bloom_params bloom{4, 1.0f, 64.0f, 0.25f};          // --bloom: levels and cap unless given
    JpegArg jpeg;                                              // --jpeg: quality 75, 4:2:0 unless given
    vector<uint8_t> jpeg_bytes;
    PngArg png;                                                // --png: RGB, adaptive filters unless given
    ExrArg exr;                                                // --exr: RGBA halves under ZIP unless given
    for (int i = 1; i < argc; i += 2) {
        string a = argv[i];
        if (a == "--batch") {
            batch = true;
            --i;
            continue;
        }
        if (i + 1 >= argc) {
            if (a == "--bloom") {   // a flag without its value
                cerr << BLOOM_USAGE << endl;
                return 1;
            }
            if (ParseJpegArg(a, nullptr, &jpeg)) {
                cerr << JPEG_USAGE << endl;
                return 1;
            }
            if (ParsePngArg(a, nullptr, &png)) {
                cerr << PNG_USAGE << endl;
                return 1;
            }
            if (ParseExrArg(a, nullptr, &exr)) {
                cerr << EXR_USAGE << endl;
                return 1;
            }
            break;
        }
        if (const int j = ParseJpegArg(a, argv[i + 1], &jpeg)) {
            if (j < 0) {
                cerr << JPEG_USAGE << endl;
                return 1;
            }
            continue;
        }
        if (const int j = ParsePngArg(a, argv[i + 1], &png)) {
            if (j < 0) {
                cerr << PNG_USAGE << endl;
                return 1;
            }
            continue;
        }
        if (const int j = ParseExrArg(a, argv[i + 1], &exr)) {
            if (j < 0) {
                cerr << EXR_USAGE << endl;
                return 1;
            }
            continue;
        }
        if (a == "--width") SCREEN_WIDTH = atoi(argv[i + 1]);
        else if (a == "--height") SCREEN_HEIGHT = atoi(argv[i + 1]);
        else if (a == "--focal") focalLength = (float)atof(argv[i + 1]);
        else if (a == "--keys") g_keys = argv[i + 1];
        else if (a == "--out") out = argv[i + 1];
        else if (a == "--setting") setting = atoi(argv[i + 1]);
        else if (a == "--setting-boxes") setting_boxes = atoi(argv[i + 1]);
        else if (a == "--textures") tex_dir = argv[i + 1];
        else if (a == "--pfm") pfm = argv[i + 1];
        else if (a == "--auto-exposure") {
            const string v = argv[i + 1];
            const size_t comma = v.find(',');
            expo.permille = atoi(v.substr(0, comma).c_str());
            expo.target = comma == string::npos ? 1.0f : (float)atof(v.substr(comma + 1).c_str());
            expo.scale_min = 1.0f / 65536.0f;
            expo.scale_max = 65536.0f;
            exposed = true;
        } else if (a == "--tonemap") {
            const string v = argv[i + 1];
            if (v == "linear") tone = CG_TONE_LINEAR;
            else if (v == "reinhard") tone = CG_TONE_REINHARD;
            else if (v.rfind("reinhard-white:", 0) == 0) {
                const float w = (float)atof(v.c_str() + 15);
                tone = CG_TONE_REINHARD_WHITE;
                white2 = w * w;
            } else {
                cerr << "--tonemap linear|reinhard|reinhard-white:W" << endl;
                return 1;
            }
            exposed = true;
        } else if (a == "--bloom") {
            if (!ParseBloomArg(argv[i + 1], &bloom)) {
                cerr << BLOOM_USAGE << endl;
                return 1;
            }
            bloomed = exposed = true;
        }
    }
    int rc = cg_create(0, &g_ctx);
    if (rc) die(rc, "cg_create");
    screen *screen = InitializeSDL(SCREEN_WIDTH, SCREEN_HEIGHT, false);
    rast::LoadTestModel(originalroom, originalbox);          // :131
    for (auto &t : originalroom) t.texture = setting;         // TestModelH.h:85-129
    for (auto &t : originalbox) t.texture = setting_boxes;    // TestModelH.h:148-260
    vector<uint8_t> maps[8];
    if (!tex_dir.empty()) {                                   // :135-170
        const char *files[8] = {"Marble2000x2000.jpg", "woven1024x1024.jpg",
                                "Wood_wicker_003_ambientOcclusion.jpg", "Wood_wicker_003_opacity.jpg",
                                "Wood_wicker_003_normal.jpg", "Metal_Grill_002_basecolor.jpg",
                                "Metal_Grill_002_opacity.jpg", "Metal_Grill_002_normal.jpg"};
        for (int k = 0; k < 8; ++k) maps[k] = read_map(tex_dir, files[k], k ? 1024 : 2000);
        auto ptr = [&](int k) { return maps[k].empty() ? nullptr : maps[k].data(); };
        cg_rast_textures tx = {ptr(0), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), ptr(7)};
        rc = cg_rast_set_textures(g_ctx, &tx);
        if (rc) die(rc, "cg_rast_set_textures");
        if (tx.marble) randCalls = 3ull * 2000 * 2000;       // normalMap_marble's rand() calls (:158-170)
    }
    rc = cg_rast_set_scene(g_ctx, reinterpret_cast<const cg_rtri *>(originalroom.data()), (int)originalroom.size(),
                           reinterpret_cast<const cg_rtri *>(originalbox.data()), (int)originalbox.size());
    if (rc) die(rc, "cg_rast_set_scene");
    if (batch || exposed) {
        // the main loop's frames in one call: each Update()'s globals recorded, then every Draw()
        vector<cg_rast_params> ps;
        while (Update()) {
            ps.push_back(CurrentParams(screen));
            if (randColourSelect == 0) {   // Draw's rule (:585), the count without a buffer
                const int n = cg_rast_prepare(&ps.back(), reinterpret_cast<const cg_rtri *>(originalroom.data()),
                                              (int)originalroom.size(),
                                              reinterpret_cast<const cg_rtri *>(originalbox.data()),
                                              (int)originalbox.size(), nullptr, 0, nullptr);
                if (n < 0) die(n, "cg_rast_prepare");
                if (n > 0) indirectLightPowerPerArea = 0.2f * vec3(1, 1, 1);
            }
        }
        if (!ps.empty()) {
            const size_t px = (size_t)screen->width * screen->height;
            vector<uint32_t> frames(ps.size() * px);
            vector<cg_rast_seq_frame> info(ps.size() + 1);
            if (exposed) {
                vector<float> scales(ps.size());
                if (bloomed) {
                    rc = cg_rast_draw_exposed_bloom(g_ctx, ps.data(), (int)ps.size(), &expo, nullptr, tone, white2, &bloom,
                                                    frames.data(), 0, scales.data(), info.data(), nullptr);
                    if (rc) die(rc, "cg_rast_draw_exposed_bloom");
                } else {
                    rc = cg_rast_draw_exposed(g_ctx, ps.data(), (int)ps.size(), &expo, nullptr, tone, white2,
                                              frames.data(), 0, scales.data(), info.data(), nullptr);
                    if (rc) die(rc, "cg_rast_draw_exposed");
                }
                for (size_t f = 0; f < scales.size(); ++f) cout << "Exposure scale : " << scales[f] << endl;
            } else {
                rc = cg_rast_draw_sequence(g_ctx, ps.data(), (int)ps.size(), frames.data(), nullptr, nullptr, 0, 0,
                                           info.data(), nullptr);
                if (rc) die(rc, "cg_rast_draw_sequence");
                if (!jpeg.path.empty() && batch) {   // the same frames again, delivered compressed
                    rc = JpegDeliver(
                        [&](uint8_t *o, size_t cap, size_t *offsets) {
                            return cg_rast_draw_sequence_jpeg(g_ctx, ps.data(), (int)ps.size(), &jpeg.params, o, cap,
                                                              offsets, 0, nullptr, nullptr);
                        },
                        ps.size(), screen->width, screen->height, &jpeg_bytes);
                    if (rc) die(rc, "cg_rast_draw_sequence_jpeg");
                }
                if (!png.path.empty() && batch) {   // the same frames again, delivered exact
                    rc = PngDeliver(
                        [&](uint8_t *o, size_t cap, size_t *offsets) {
                            return cg_rast_draw_sequence_png(g_ctx, ps.data(), (int)ps.size(), &png.params, o, cap, offsets,
                                                             0, nullptr, nullptr);
                        },
                        ps.size(), screen->width, screen->height, png.path);
                    if (rc) die(rc, "cg_rast_draw_sequence_png");
                }
            }
            if (!jpeg.path.empty() && batch && exposed) {
                rc = JpegEncodeFrames(g_ctx, frames.data(), ps.size(), screen->width, screen->height, jpeg.params,
                                      &jpeg_bytes);
                if (rc) die(rc, "cg_image_encode_jpeg");
            }
            if (!png.path.empty() && batch && exposed) {
                rc = PngEncodeFrames(g_ctx, frames.data(), ps.size(), screen->width, screen->height, png.params,
                                     [&](size_t f) { return PngFramePath(png.path, f); });
                if (rc) die(rc, "cg_image_encode_png");
            }
            if (!exr.path.empty() && batch) {   // the frames' float pictures, delivered as files
                rc = ExrDeliver(
                    [&](uint8_t *o, size_t cap, size_t *offsets) {
                        return cg_rast_draw_sequence_exr(g_ctx, ps.data(), (int)ps.size(), &exr.params, o, cap, offsets, 0,
                                                         nullptr, nullptr);
                    },
                    ps.size(), screen->width, screen->height, exr.path);
                if (rc) die(rc, "cg_rast_draw_sequence_exr");
            }
            randCalls = info.back().rand_offset;
            g_last = ps.back();                               // the last frame, at its chained index
            g_last.rand_offset = info[ps.size() - 1].rand_offset;
            g_drawn = true;
            memcpy(screen->buffer, frames.data() + (ps.size() - 1) * px, px * sizeof(uint32_t));
            SDL_Renderframe(screen);
        }
    } else {
        while (Update()) {
            Draw(screen);
            SDL_Renderframe(screen);
        }
    }
    SDL_SaveImage(screen, out.c_str());
    if (!jpeg.path.empty()) {
        if (jpeg_bytes.empty() && g_drawn) {   // the frame the screenshot holds
            rc = JpegEncodeFrames(g_ctx, screen->buffer, 1, screen->width, screen->height, jpeg.params, &jpeg_bytes);
            if (rc) die(rc, "cg_image_encode_jpeg");
        }
        if (!JpegSave(jpeg.path, jpeg_bytes)) {
            cerr << "cannot write " << jpeg.path << endl;
            return 1;
        }
    }
    if (!png.path.empty() && g_drawn) {   // the frame the screenshot holds
        rc = PngEncodeFrames(g_ctx, screen->buffer, 1, screen->width, screen->height, png.params,
                             [&](size_t) { return png.path; });
        if (rc) die(rc, "cg_image_encode_png");
    }
    if (!pfm.empty() && g_drawn) SavePicturePFM(pfm.c_str());
    if (!exr.path.empty() && g_drawn) {
        rc = ExrEncodePicture(g_ctx, Picture().data(), g_last.width, g_last.height, exr.params, exr.path);
        if (rc) die(rc, "cg_image_encode_exr");
    }
    KillSDL(screen);
    cg_destroy(g_ctx);
    return 0;
}
