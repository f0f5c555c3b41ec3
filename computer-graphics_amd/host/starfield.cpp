// starfield.cpp -- headless drop-in for starfield/Source/skeleton.cpp.
//
// Same main: the star set-up (:40-51), then while (frames left) { Draw(screen);
// Update(); SDL_Renderframe(screen); } and SDL_SaveImage.  The stars live on
// the GPU (cg_starfield_set): Draw is a run of one frame with no update into
// screen->buffer, Update is cg_starfield_advance_device with the scripted
// frame time, which stands in for the reference's SDL_GetTicks difference
// (:84-87).  --batch renders the whole script with one cg_starfield_run and
// keeps its last frame: the same image.
//
//   starfield [--width W] [--height H] [--stars N] [--dts "0,16,17,..."]
//             [--frames N --dt MS] [--out FILE] [--batch]
#include <cstring>
#include <string>
#include <vector>

#include "SDLauxiliary.h"
#include "cg_render.h"

using namespace std;
using glm::vec3;

int SCREEN_WIDTH = 320, SCREEN_HEIGHT = 256;                  // :12-13
vector<float> stars(3 * 1000);                                // :22, (x, y, z) triples

static cg_ctx *g_ctx = nullptr;
static vector<float> g_dts;                                   // frame time of each Update, ms
static size_t g_frame = 0;

static void die(int rc, const char *what)
{
    cerr << what << " failed (" << rc << "): " << (g_ctx ? cg_last_error(g_ctx) : "") << endl;
    exit(1);
}

// float -> int as the reference's build converts (cvttss2si)
static int f2i(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000u; }

// skeleton.cpp:66-79
void Draw(screen *screen)
{
    int rc = cg_starfield_run(g_ctx, nullptr, 0, 1, screen->width, screen->height, screen->buffer, 0, 0, nullptr);
    if (rc) die(rc, "cg_starfield_run");
}

// skeleton.cpp:82-104 with the scripted frame time
void Update()
{
    float dt = g_dts[g_frame++];
    int rc = cg_starfield_advance_device(g_ctx, &dt, 1, nullptr);
    if (rc) die(rc, "cg_starfield_advance_device");
}

int main(int argc, char *argv[])
{
    string out = "screenshot.bmp", dts;
    int n_stars = 1000, frames = -1;
    float dt = 16;
    bool batch = false;
    for (int i = 1; i < argc; ++i) {
        string a = argv[i];
        if (a == "--batch") {
            batch = true;
            continue;
        }
        if (i + 1 >= argc) break;
        const char *v = argv[++i];
        if (a == "--width") SCREEN_WIDTH = atoi(v);
        else if (a == "--height") SCREEN_HEIGHT = atoi(v);
        else if (a == "--stars") n_stars = atoi(v);
        else if (a == "--dts") dts = v;
        else if (a == "--frames") frames = atoi(v);
        else if (a == "--dt") dt = (float)atof(v);
        else if (a == "--out") out = v;
    }
    if (!dts.empty()) {
        const char *p = dts.c_str();
        while (*p) {
            char *end;
            float v = strtof(p, &end);
            if (end == p) break;
            g_dts.push_back(v);
            p = *end == ',' ? end + 1 : end;
        }
    } else {
        g_dts.assign(frames < 0 ? 1 : frames, dt);
    }
    if (n_stars < 0 || SCREEN_WIDTH <= 0 || SCREEN_HEIGHT <= 0) {
        cerr << "bad --stars / --width / --height" << endl;
        return 1;
    }
    int rc = cg_create(0, &g_ctx);
    if (rc) die(rc, "cg_create");
    screen *screen = InitializeSDL(SCREEN_WIDTH, SCREEN_HEIGHT, false);
    memset(screen->buffer, 0, screen->height * screen->width * sizeof(uint32_t));   // :38

    vec3 white(1, 1, 1);                                      // :40
    stars.resize(3 * (size_t)n_stars);
    rc = cg_starfield_init(stars.data(), n_stars);            // :42-45 (glibc rand(), never seeded)
    if (rc) die(rc, "cg_starfield_init");
    for (int i = 0; i < n_stars; i++) {                       // :47-50, without PutPixelSDL's "apa" lines
        float u = (SCREEN_WIDTH / 2) * (stars[3 * i] / stars[3 * i + 2]) + (SCREEN_WIDTH / 2);
        float v = (SCREEN_HEIGHT / 2) * (stars[3 * i + 1] / stars[3 * i + 2]) + (SCREEN_HEIGHT / 2);
        int x = f2i(u), y = f2i(v);
        if (x >= 0 && x < screen->width && y >= 0 && y < screen->height) PutPixelSDL(screen, x, y, white);
    }
    rc = cg_starfield_set(g_ctx, stars.data(), n_stars);
    if (rc) die(rc, "cg_starfield_set");

    if (batch && !g_dts.empty()) {
        const int n = (int)g_dts.size();
        const size_t px = (size_t)screen->width * screen->height;
        vector<uint32_t> all(n * px);
        rc = cg_starfield_run(g_ctx, g_dts.data(), n, n, screen->width, screen->height, all.data(), 0, 0, nullptr);
        if (rc) die(rc, "cg_starfield_run");
        memcpy(screen->buffer, all.data() + (n - 1) * px, px * sizeof(uint32_t));
        SDL_Renderframe(screen);
    } else {
        while (g_frame < g_dts.size()) {                      // :53-57
            Draw(screen);
            Update();
            SDL_Renderframe(screen);
        }
    }

    SDL_SaveImage(screen, out.c_str());                       // :59
    KillSDL(screen);
    cg_destroy(g_ctx);
    return 0;
}
