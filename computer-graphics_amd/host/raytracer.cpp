// raytracer.cpp -- headless drop-in for raytracer/Source/skeleton.cpp.
//
// Same globals (focalLength, cameraPos, lights, yaw, R), same main loop
// `while (Update()) { Draw(screen); SDL_Renderframe(screen); }`, same
// Draw(screen*) writing ARGB into screen->buffer, same screenshot.bmp on
// exit.  Keyboard input is replaced by a scripted key string (one key per
// frame, letters as in Update(): w s a d q e = light, U D L R = camera
// arrows, n m = yaw, i o = focal, x = ESC).  The per-pixel loop runs on the
// GPU through the C-ABI (include/cg_render.h).
//
//   raytracer [--width W] [--height H] [--focal F] [--keys KEYS] [--out FILE] [--batch] [--pfm FILE]
//             [--auto-exposure PERMILLE[,TARGET]] [--tonemap linear|reinhard|reinhard-white:W]
//             [--bloom THRESHOLD,INTENSITY[,LEVELS[,CAP]]]
//             [--jpeg FILE [--quality 1..100] [--subsampling 444|420]]
//             [--png FILE [--png-colour rgb|rgba] [--png-filter adaptive|0..4]]
//             [--exr FILE [--exr-type half|float] [--exr-compression zip|none] [--exr-colour rgb|rgba]]
//
// --batch: Update() runs over the whole key script first, each frame's globals
// are recorded, and one cg_rt_render_sequence call renders every frame; the
// screenshot is the last frame, as without the flag.
// --pfm FILE: the last frame's pixelColour / 9.0f before PutPixelSDL clamps it
// (cg_rt_render_radiance), as a little-endian colour PFM: "PF", the size, "-1.0",
// then rows bottom-up of three floats a pixel.
// --auto-exposure PERMILLE[,TARGET]: the run's frames go through one cg_rt_render_exposed call
// (as --batch records them): each frame's scale puts the upper edge of the luminance bin that
// holds its PERMILLE-th thousandth of lit pixels at TARGET (default 1), no adaptation; the
// screenshot is the last exposed frame and the scale of every frame is printed.
// --tonemap: the curve between the scaled radiance and PutPixelSDL (default linear; reinhard-white:W
// maps radiance W to white); with --tonemap alone the scale is 1.
// --bloom THRESHOLD,INTENSITY[,LEVELS[,CAP]]: the run goes through cg_rt_render_exposed_bloom -- glare
// around what exceeds THRESHOLD after the scale, added INTENSITY times before the curve (levels 4 and
// cap 64 unless given); without --auto-exposure every scale is 1.  Without the flag nothing changes.
// --jpeg FILE: the frame --out writes, as a baseline JPEG encoded on the device (cg_image_encode_jpeg;
// quality 75 and 4:2:0 unless --quality / --subsampling say otherwise).  With --batch, every frame of
// the run, the files one after the other (a motion-JPEG stream): through cg_rt_render_sequence_jpeg,
// or with the exposure flags each exposed frame through the encoder.
// --png FILE: the frame --out writes, as a lossless PNG encoded on the device (cg_image_encode_png; RGB
// and adaptive filters unless --png-colour / --png-filter say otherwise): it decodes to exactly the
// pixels of --out.  With --batch, also frame k of the run as FILE with .%04d before its extension:
// through cg_rt_render_sequence_png, or with the exposure flags each exposed frame through the encoder.
// --exr FILE: the picture --pfm writes, as an OpenEXR file encoded on the device (cg_image_encode_exr;
// RGBA halves under ZIP unless --exr-type / --exr-compression / --exr-colour say otherwise).  A is the
// share of the pixel's nine sub-rays that hit, w / 9.  With --batch, also frame k's picture as FILE with
// .%04d before its extension, through cg_rt_render_sequence_exr; the exposure flags do not change them.
#include <chrono>
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

// skeleton.cpp:40-50
struct Intersection {
    vec4 position;
    float distance;
    int triangleIndex;
    int sphereIndex;
};
struct Light {
    vec4 position;
    vec3 colour;
};
static_assert(sizeof(Intersection) == sizeof(cg_isect), "Intersection layout");
static_assert(sizeof(Light) == sizeof(cg_light), "Light layout");

// skeleton.cpp:56-60
int SCREEN_WIDTH = 320, SCREEN_HEIGHT = 256;
float focalLength = 256;
vec4 cameraPos(0.0, 0.0, -3.0, 1.0);
vector<Light> lights;
float yaw = 0.0;
mat4 R(1.0f);

static cg_ctx *g_ctx = nullptr;
static string g_keys;
static size_t g_frame = 0;

bool Update();
void Draw(screen *screen);

static void die(int rc, const char *what)
{
    cerr << what << " failed (" << rc << "): " << (g_ctx ? cg_last_error(g_ctx) : "") << endl;
    exit(1);
}

// LoadTestModel every frame as the reference does (:113-116); the scene
// is constant, so it is uploaded to the device once.
static void UploadScene()
{
    static bool uploaded = false;
    vector<rt::Triangle> triangles;
    vector<rt::Sphere> spheres;
    rt::LoadTestModel(triangles, spheres);
    if (!uploaded) {
        int rc = cg_rt_set_scene(g_ctx, reinterpret_cast<const cg_tri *>(triangles.data()),
                                 (int)triangles.size(),
                                 reinterpret_cast<const cg_sphere *>(spheres.data()),
                                 (int)spheres.size());
        if (rc) die(rc, "cg_rt_set_scene");
        uploaded = true;
    }
}

// the globals as Draw hands them to the library
static cg_rt_camera CurrentCamera(const screen *screen)
{
    cg_rt_camera cam;
    cam.width = screen->width;
    cam.height = screen->height;
    cam.focal = focalLength;
    cam.camera = cg_vec4{cameraPos.x, cameraPos.y, cameraPos.z, cameraPos.w};
    memcpy(cam.R, R.data(), sizeof(cam.R));
    cam.indirect = 0.5f;                                              // :110
    return cam;
}

// skeleton.cpp:104-169: the pixel loop runs in rt_pixel_kernel.
void Draw(screen *screen)
{
    memset(screen->buffer, 0, screen->height * screen->width * sizeof(uint32_t));
    UploadScene();
    const cg_rt_camera cam = CurrentCamera(screen);
    int rc = cg_rt_render(g_ctx, reinterpret_cast<const cg_light *>(lights.data()),
                          (int)lights.size(), &cam, screen->buffer, nullptr);
    if (rc) die(rc, "cg_rt_render");
}

// --pfm, --exr: the frame Draw would render from the current globals, unclamped
static vector<float> Radiance(const screen *screen)
{
    UploadScene();
    const cg_rt_camera cam = CurrentCamera(screen);
    vector<float> rgba((size_t)cam.width * cam.height * 4);
    int rc = cg_rt_render_radiance(g_ctx, reinterpret_cast<const cg_light *>(lights.data()), (int)lights.size(), &cam,
                                   rgba.data(), nullptr);
    if (rc) die(rc, "cg_rt_render_radiance");
    return rgba;
}

static void SaveRadiancePFM(const screen *screen, const char *path)
{
    const cg_rt_camera cam = CurrentCamera(screen);
    const vector<float> rgba = Radiance(screen);
    ofstream f(path, ios::binary);
    f << "PF\n" << cam.width << " " << cam.height << "\n-1.0\n";
    vector<float> row((size_t)cam.width * 3);
    for (int y = cam.height - 1; y >= 0; --y) {   // bottom row first
        for (int x = 0; x < cam.width; ++x)
            memcpy(&row[3 * x], &rgba[((size_t)y * cam.width + x) * 4], 3 * sizeof(float));
        f.write(reinterpret_cast<const char *>(row.data()), row.size() * sizeof(float));
    }
    if (!f) {
        cerr << "cannot write " << path << endl;
        exit(1);
    }
}

// skeleton.cpp:172-260 with scripted keys
bool Update()
{
    static auto t = chrono::steady_clock::now();
    auto t2 = chrono::steady_clock::now();
    float dt = chrono::duration<float, milli>(t2 - t).count();
    t = t2;
    cout << "Render time : " << dt << " ms." << endl;
    if (g_frame >= g_keys.size()) return g_frame++ == 0;   // no keys: render one frame
    char key = g_keys[g_frame++];
    switch (key) {
    case 'w': lights[0].position += vec4(0, 0, 0.1, 0); break;
    case 's': lights[0].position += vec4(0, 0, -0.1, 0); break;
    case 'a': lights[0].position += vec4(-0.1, 0, 0, 0); break;
    case 'd': lights[0].position += vec4(0.1, 0, 0, 0); break;
    case 'q': lights[0].position += vec4(0, -0.1, 0, 0); break;
    case 'e': lights[0].position += vec4(0, 0.1, 0, 0); break;
    case 'U': cameraPos += vec4(0, 0, 0.1, 0); break;
    case 'D': cameraPos += vec4(0, 0, -0.1, 0); break;
    case 'L': cameraPos += vec4(-0.1, 0, 0, 0); break;
    case 'R': cameraPos += vec4(0.1, 0, 0, 0); break;
    case 'n':
    case 'm':
        if (key == 'n') yaw -= 0.174533;   // double literal, narrowed (:235, :241)
        else yaw += 0.174533;
        R[0][0] = cos(yaw); R[0][1] = 0; R[0][2] = -sin(yaw);
        R[1][0] = 0;        R[1][1] = 1; R[1][2] = 0;
        R[2][0] = sin(yaw); R[2][1] = 0; R[2][2] = cos(yaw);
        break;
    case 'i': focalLength += 10; break;
    case 'o': focalLength -= 10; break;
    case 'x': return false;
    default: break;
    }
    return true;
}

int main(int argc, char *argv[])
{
    string out = "screenshot.bmp", pfm;
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
    exr.params.alpha_scale = 1.0f / 9.0f;                      // w counts the sub-rays of nine that hit
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
    Light light1;                                                     // :86-89
    light1.position = vec4(0, -0.5, -0.7, 1.0);
    light1.colour = 14.f * vec3(1, 1, 1);
    lights.push_back(light1);
    size_t drawn = 0;
    if (batch || exposed) {
        // the main loop's frames in one call: each Update()'s globals recorded, then every Draw()
        vector<cg_rt_camera> cams;
        vector<Light> seq;   // frame-major, lights.size() per frame
        while (Update()) {
            cams.push_back(CurrentCamera(screen));
            seq.insert(seq.end(), lights.begin(), lights.end());
        }
        if (!cams.empty()) {
            UploadScene();
            const size_t px = (size_t)screen->width * screen->height;
            vector<uint32_t> frames(cams.size() * px);
            if (exposed) {
                vector<float> scales(cams.size());
                if (bloomed) {
                    rc = cg_rt_render_exposed_bloom(g_ctx, reinterpret_cast<const cg_light *>(seq.data()),
                                                    (int)lights.size(), cams.data(), (int)cams.size(), 1, &expo, nullptr,
                                                    tone, white2, &bloom, frames.data(), 0, scales.data(), nullptr);
                    if (rc) die(rc, "cg_rt_render_exposed_bloom");
                } else {
                    rc = cg_rt_render_exposed(g_ctx, reinterpret_cast<const cg_light *>(seq.data()), (int)lights.size(),
                                              cams.data(), (int)cams.size(), 1, &expo, nullptr, tone, white2,
                                              frames.data(), 0, scales.data(), nullptr);
                    if (rc) die(rc, "cg_rt_render_exposed");
                }
                for (size_t f = 0; f < scales.size(); ++f) cout << "Exposure scale : " << scales[f] << endl;
            } else {
                rc = cg_rt_render_sequence(g_ctx, reinterpret_cast<const cg_light *>(seq.data()), (int)lights.size(),
                                           cams.data(), (int)cams.size(), frames.data(), 0, 0, nullptr);
                if (rc) die(rc, "cg_rt_render_sequence");
                if (!jpeg.path.empty() && batch) {   // the same frames again, delivered compressed
                    rc = JpegDeliver(
                        [&](uint8_t *o, size_t cap, size_t *offsets) {
                            return cg_rt_render_sequence_jpeg(g_ctx, reinterpret_cast<const cg_light *>(seq.data()),
                                                              (int)lights.size(), cams.data(), (int)cams.size(),
                                                              &jpeg.params, o, cap, offsets, 0, nullptr);
                        },
                        cams.size(), screen->width, screen->height, &jpeg_bytes);
                    if (rc) die(rc, "cg_rt_render_sequence_jpeg");
                }
                if (!png.path.empty() && batch) {   // the same frames again, delivered exact
                    rc = PngDeliver(
                        [&](uint8_t *o, size_t cap, size_t *offsets) {
                            return cg_rt_render_sequence_png(g_ctx, reinterpret_cast<const cg_light *>(seq.data()),
                                                             (int)lights.size(), cams.data(), (int)cams.size(), &png.params,
                                                             o, cap, offsets, 0, nullptr);
                        },
                        cams.size(), screen->width, screen->height, png.path);
                    if (rc) die(rc, "cg_rt_render_sequence_png");
                }
            }
            if (!jpeg.path.empty() && batch && exposed) {
                rc = JpegEncodeFrames(g_ctx, frames.data(), cams.size(), screen->width, screen->height, jpeg.params,
                                      &jpeg_bytes);
                if (rc) die(rc, "cg_image_encode_jpeg");
            }
            if (!png.path.empty() && batch && exposed) {
                rc = PngEncodeFrames(g_ctx, frames.data(), cams.size(), screen->width, screen->height, png.params,
                                     [&](size_t f) { return PngFramePath(png.path, f); });
                if (rc) die(rc, "cg_image_encode_png");
            }
            if (!exr.path.empty() && batch) {   // the frames' float pictures, delivered as files
                rc = ExrDeliver(
                    [&](uint8_t *o, size_t cap, size_t *offsets) {
                        return cg_rt_render_sequence_exr(g_ctx, reinterpret_cast<const cg_light *>(seq.data()),
                                                         (int)lights.size(), cams.data(), (int)cams.size(), &exr.params, o,
                                                         cap, offsets, 0, nullptr);
                    },
                    cams.size(), screen->width, screen->height, exr.path);
                if (rc) die(rc, "cg_rt_render_sequence_exr");
            }
            memcpy(screen->buffer, frames.data() + (cams.size() - 1) * px, px * sizeof(uint32_t));
            SDL_Renderframe(screen);
        }
        drawn = cams.size();
    } else {
        while (Update()) {
            Draw(screen);
            SDL_Renderframe(screen);
            ++drawn;
        }
    }
    SDL_SaveImage(screen, out.c_str());
    if (!jpeg.path.empty()) {
        if (jpeg_bytes.empty() && drawn > 0) {   // the frame the screenshot holds
            rc = JpegEncodeFrames(g_ctx, screen->buffer, 1, screen->width, screen->height, jpeg.params, &jpeg_bytes);
            if (rc) die(rc, "cg_image_encode_jpeg");
        }
        if (!JpegSave(jpeg.path, jpeg_bytes)) {
            cerr << "cannot write " << jpeg.path << endl;
            return 1;
        }
    }
    if (!png.path.empty() && drawn > 0) {   // the frame the screenshot holds
        rc = PngEncodeFrames(g_ctx, screen->buffer, 1, screen->width, screen->height, png.params,
                             [&](size_t) { return png.path; });
        if (rc) die(rc, "cg_image_encode_png");
    }
    // Update() changes nothing on the turn it ends the loop: the globals are the last frame's
    if (!pfm.empty() && drawn > 0) SaveRadiancePFM(screen, pfm.c_str());
    if (!exr.path.empty() && drawn > 0) {
        rc = ExrEncodePicture(g_ctx, Radiance(screen).data(), screen->width, screen->height, exr.params, exr.path);
        if (rc) die(rc, "cg_image_encode_exr");
    }
    KillSDL(screen);
    cg_destroy(g_ctx);
    return 0;
}
