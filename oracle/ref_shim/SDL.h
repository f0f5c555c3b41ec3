/* TEST INFRASTRUCTURE ONLY -- headless stand-in for <SDL.h>.
 *
 * The reference programs (raytracer, rasteriser, starfield) compile unmodified against this
 * header instead of SDL2 (recipe: oracle/ref_build.py).  Nothing here draws a window: the
 * header scripts the keyboard and the clock, and records what the program computes.
 *
 *   CG_REF_KEYS / CG_REF_KEYS_FILE   key script, one key per Update(): U D L R = arrows,
 *                                    ' ' = SPACE, '.' = a frame with no key, every other
 *                                    character is the key of that name.  When the script is
 *                                    spent the program receives ESC.
 *   CG_REF_TICKS                     comma-separated values that SDL_GetTicks returns in turn;
 *                                    after the list (default: from 0) each call adds 16 ms.
 *   CG_REF_FRAMES                    file that receives every presented frame: the ARGB buffer,
 *                                    then (-DCG_REF_RAST) depthBuffer and shadowBuffer.
 *   CG_REF_STATE                     file that receives the program's own globals, raw float
 *                                    bits, each time SDL_PollEvent reports an empty queue, i.e.
 *                                    the state the next Draw() uses.  Layout per program below.
 *   CG_REF_SETTING / CG_REF_SETTING_BOXES   (-DCG_REF_RAST) the rasteriser's texture modes.
 *   CG_REF_BOX_INDEX                 (-DCG_REF_RAST) value for the one Triangle::index that the
 *                                    reference leaves uninitialised (see below); unset = untouched.
 *   CG_REF_CAM / CG_REF_FOCAL / CG_REF_LIGHT   (-DCG_REF_RT, -DCG_REF_RAST) start values of cameraPos
 *                                    ("x,y,z"), focalLength and the light's position ("x,y,z":
 *                                    lights[0].position / sceneCoordinatesLightPos), given to the
 *                                    program's globals before the first key is handled; unset =
 *                                    untouched.  For the scene-loading builds (ref_shim/scene/).
 *
 * Build with exactly one of -DCG_REF_RT, -DCG_REF_RAST, -DCG_REF_STAR.  glm is included before
 * this header by all three programs, so their globals can be declared extern here.
 */
#ifndef CG_REF_SHIM_SDL_H
#define CG_REF_SHIM_SDL_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <string>

typedef struct SDL_Window { int unused; } SDL_Window;
typedef struct SDL_Renderer { int unused; } SDL_Renderer;
typedef struct SDL_Texture { int w, h; } SDL_Texture;
typedef struct SDL_Surface { const void *pixels; int w, h, pitch; } SDL_Surface;
typedef struct SDL_version { uint8_t major, minor, patch; } SDL_version;
typedef struct SDL_Rect { int x, y, w, h; } SDL_Rect;
typedef struct SDL_Keysym { int sym; } SDL_Keysym;
typedef struct SDL_KeyboardEvent { uint32_t type; SDL_Keysym keysym; } SDL_KeyboardEvent;
typedef union SDL_Event { uint32_t type; SDL_KeyboardEvent key; } SDL_Event;

enum { SDL_QUIT = 0x100, SDL_KEYDOWN = 0x300 };
enum { SDLK_ESCAPE = 27, SDLK_SPACE = ' ', SDLK_1 = '1', SDLK_2 = '2',
       SDLK_a = 'a', SDLK_d = 'd', SDLK_e = 'e', SDLK_f = 'f', SDLK_g = 'g', SDLK_i = 'i',
       SDLK_m = 'm', SDLK_n = 'n', SDLK_o = 'o', SDLK_q = 'q', SDLK_s = 's', SDLK_w = 'w',
       SDLK_x = 'x', SDLK_z = 'z',
       SDLK_RIGHT = 0x4000004F, SDLK_LEFT = 0x40000050, SDLK_DOWN = 0x40000051, SDLK_UP = 0x40000052 };

#define SDL_LIL_ENDIAN 1234
#define SDL_BIG_ENDIAN 4321
#define SDL_BYTEORDER SDL_LIL_ENDIAN
#define SDL_INIT_TIMER 0x1u
#define SDL_INIT_VIDEO 0x20u
#define SDL_WINDOW_OPENGL 0x2u
#define SDL_WINDOW_FULLSCREEN_DESKTOP 0x1001u
#define SDL_WINDOWPOS_UNDEFINED 0x1FFF0000
#define SDL_RENDERER_ACCELERATED 0x2u
#define SDL_RENDERER_PRESENTVSYNC 0x4u
#define SDL_HINT_RENDER_SCALE_QUALITY "SDL_RENDER_SCALE_QUALITY"
#define SDL_PIXELFORMAT_ARGB8888 0x16362004u
#define SDL_TEXTUREACCESS_STATIC 0
#define SDL_VERSION(v) do { (v)->major = 2; (v)->minor = 0; (v)->patch = 0; } while (0)

/* ---- the programs' own globals (external linkage, defined after this header) ---- */
#if defined(CG_REF_RT)
/* state record: cameraPos[4] yaw R[16] focalLength lights[0].position[4]  (26 words) */
extern glm::vec4 cameraPos;
extern float yaw;
extern glm::mat4 R;
extern float focalLength;
struct Light;
extern std::vector<Light> lights;
#elif defined(CG_REF_RAST)
/* state record: cameraPos[4] yaw R[16] focalLength sceneCoordinatesLightPos[4]
 * indirectLightPowerPerArea.x randColourSelect(int)  (28 words) */
extern glm::vec4 cameraPos;
extern float yaw;
extern glm::mat4 R;
extern float focalLength;
extern glm::vec4 sceneCoordinatesLightPos;
extern glm::vec3 indirectLightPowerPerArea;
extern int randColourSelect;
extern int setting;
extern int settingBoxes;
#define CG_REF_RAST_W 900
#define CG_REF_RAST_H 720
extern float depthBuffer[CG_REF_RAST_H][CG_REF_RAST_W];
extern int shadowBuffer[CG_REF_RAST_H][CG_REF_RAST_W];
/* The reference never assigns `index` of the last box triangle (the second top face of the tall
 * block: its line sets the first top face's index twice), and findU / findV read it whenever the
 * boxes are textured: undefined behaviour, whose outcome is whatever the stack held.  With
 * CG_REF_BOX_INDEX set, that one field is given the value before the first frame, so that the run
 * is defined.  Triangle is complete only after this header: reach it through a dependent name. */
class Triangle;
extern std::vector<Triangle> originalbox;
template <class V> static inline void cg_ref_shim_define_box_index(V &boxes)
{
    const char *v = getenv("CG_REF_BOX_INDEX");
    if (v && !boxes.empty())
        boxes.back().index = atoi(v);
}
#elif defined(CG_REF_STAR)
/* state record: stars[n][3] */
extern std::vector<glm::vec3> stars;
#else
#error "define one of CG_REF_RT, CG_REF_RAST, CG_REF_STAR"
#endif

struct cg_ref_shim_state {
    std::string keys;
    size_t key_pos;
    bool key_given;          /* a key was delivered in the current Update() */
    std::vector<uint32_t> ticks;
    size_t tick_pos;
    uint32_t tick_last;
    FILE *frames, *state;
    bool ready;
};

static inline cg_ref_shim_state &cg_ref_shim()
{
    static cg_ref_shim_state s;
    if (s.ready)
        return s;
    s.ready = true;
    s.key_pos = s.tick_pos = 0;
    s.key_given = false;
    s.tick_last = 0;
    if (const char *k = getenv("CG_REF_KEYS")) {
        s.keys = k;
    } else if (const char *kf = getenv("CG_REF_KEYS_FILE")) {
        if (FILE *f = fopen(kf, "rb")) {
            int c;
            while ((c = fgetc(f)) != EOF)
                if (c != '\n' && c != '\r')
                    s.keys.push_back((char)c);
            fclose(f);
        }
    }
    if (const char *t = getenv("CG_REF_TICKS")) {
        while (*t) {
            char *end;
            unsigned long v = strtoul(t, &end, 10);
            if (end == t)
                break;
            s.ticks.push_back((uint32_t)v);
            t = (*end == ',') ? end + 1 : end;
        }
    }
    const char *fr = getenv("CG_REF_FRAMES"), *st = getenv("CG_REF_STATE");
    s.frames = fr ? fopen(fr, "wb") : 0;
    s.state = st ? fopen(st, "wb") : 0;
    return s;
}

#if defined(CG_REF_RT)
/* Light is complete only after this header: reach its member through a dependent name. */
template <class V> static inline void cg_ref_shim_put_light(const V &v, FILE *f)
{
    fwrite(&v[0].position, sizeof(float), 4, f);
}
template <class V> static inline void cg_ref_shim_set_light(V &v, const float *xyz)
{
    if (!v.empty()) {
        v[0].position.x = xyz[0]; v[0].position.y = xyz[1]; v[0].position.z = xyz[2];
    }
}
#endif

#if defined(CG_REF_RT) || defined(CG_REF_RAST)
static inline bool cg_ref_shim_xyz(const char *name, float *xyz)
{
    const char *v = getenv(name);
    if (!v)
        return false;
    if (sscanf(v, "%f,%f,%f", &xyz[0], &xyz[1], &xyz[2]) != 3) {
        fprintf(stderr, "%s: expected x,y,z\n", name);
        exit(3);
    }
    return true;
}

/* Start values for the programs' globals, at the first SDL_PollEvent: the model is loaded (and the
 * raytracer's light exists), nothing is drawn and no key is handled yet.  w stays 1. */
static inline void cg_ref_shim_start_values()
{
    float v[3];
    if (cg_ref_shim_xyz("CG_REF_CAM", v)) {
        cameraPos.x = v[0]; cameraPos.y = v[1]; cameraPos.z = v[2];
    }
    if (const char *f = getenv("CG_REF_FOCAL"))
        focalLength = strtof(f, 0);
    if (cg_ref_shim_xyz("CG_REF_LIGHT", v)) {
#if defined(CG_REF_RT)
        cg_ref_shim_set_light(lights, v);
#else
        sceneCoordinatesLightPos.x = v[0]; sceneCoordinatesLightPos.y = v[1]; sceneCoordinatesLightPos.z = v[2];
#endif
    }
}
#endif

static inline void cg_ref_shim_dump_state()
{
    FILE *f = cg_ref_shim().state;
    if (!f)
        return;
#if defined(CG_REF_RT) || defined(CG_REF_RAST)
    fwrite(&cameraPos, sizeof(float), 4, f);
    fwrite(&yaw, sizeof(float), 1, f);
    fwrite(&R, sizeof(float), 16, f);
    fwrite(&focalLength, sizeof(float), 1, f);
#endif
#if defined(CG_REF_RT)
    cg_ref_shim_put_light(lights, f);
#elif defined(CG_REF_RAST)
    fwrite(&sceneCoordinatesLightPos, sizeof(float), 4, f);
    fwrite(&indirectLightPowerPerArea, sizeof(float), 1, f);
    fwrite(&randColourSelect, sizeof(int), 1, f);
#elif defined(CG_REF_STAR)
    if (!stars.empty())
        fwrite(&stars[0], sizeof(float), 3 * stars.size(), f);
#endif
    fflush(f);
}

static inline int SDL_Init(uint32_t)
{
    cg_ref_shim();
#if defined(CG_REF_RAST)
    if (const char *v = getenv("CG_REF_SETTING"))
        setting = atoi(v);
    if (const char *v = getenv("CG_REF_SETTING_BOXES"))
        settingBoxes = atoi(v);
#endif
    return 0;
}

static inline int SDL_PollEvent(SDL_Event *e)
{
    cg_ref_shim_state &s = cg_ref_shim();
#if defined(CG_REF_RAST)
    if (s.key_pos == 0 && !s.key_given)     /* first Update(): the model is loaded, nothing drawn yet */
        cg_ref_shim_define_box_index(originalbox);
#endif
#if defined(CG_REF_RT) || defined(CG_REF_RAST)
    if (s.key_pos == 0 && !s.key_given)
        cg_ref_shim_start_values();
#endif
    if (s.key_given) {                  /* second call of this Update(): queue empty */
        s.key_given = false;
        cg_ref_shim_dump_state();
        return 0;
    }
    memset(e, 0, sizeof *e);
    e->type = SDL_KEYDOWN;
    if (s.key_pos >= s.keys.size()) {
        e->key.keysym.sym = SDLK_ESCAPE;
        return 1;
    }
    const char c = s.keys[s.key_pos++];
    if (c == '.') {
        cg_ref_shim_dump_state();
        return 0;
    }
    e->key.keysym.sym = c == 'U' ? SDLK_UP : c == 'D' ? SDLK_DOWN : c == 'L' ? SDLK_LEFT
                      : c == 'R' ? SDLK_RIGHT : (int)(unsigned char)c;
    s.key_given = true;
    return 1;
}

static inline uint32_t SDL_GetTicks()
{
    cg_ref_shim_state &s = cg_ref_shim();
    if (s.tick_pos < s.ticks.size())
        s.tick_last = s.ticks[s.tick_pos];
    else if (s.tick_pos > 0)
        s.tick_last += 16;
    ++s.tick_pos;
    return s.tick_last;
}

static inline int SDL_UpdateTexture(SDL_Texture *t, const SDL_Rect *, const void *pixels, int pitch)
{
    FILE *f = cg_ref_shim().frames;
    if (!f)
        return 0;
    for (int y = 0; y < t->h; ++y)
        fwrite((const char *)pixels + (size_t)y * pitch, 4, t->w, f);
#if defined(CG_REF_RAST)
    fwrite(depthBuffer, sizeof(float), CG_REF_RAST_W * CG_REF_RAST_H, f);
    fwrite(shadowBuffer, sizeof(int), CG_REF_RAST_W * CG_REF_RAST_H, f);
#endif
    fflush(f);
    return 0;
}

static inline SDL_Surface *SDL_CreateRGBSurfaceFrom(void *pixels, int w, int h, int, int pitch,
                                                    uint32_t, uint32_t, uint32_t, uint32_t)
{
    SDL_Surface *s = new SDL_Surface;
    s->pixels = pixels; s->w = w; s->h = h; s->pitch = pitch;
    return s;
}

/* 32-bit BI_RGB bitmap, rows bottom-up. */
static inline int SDL_SaveBMP(SDL_Surface *s, const char *path)
{
    FILE *f = fopen(path, "wb");
    if (!f)
        return -1;
    const uint32_t size = 4u * s->w * s->h;
    uint8_t h[54];
    memset(h, 0, sizeof h);
    h[0] = 'B'; h[1] = 'M';
    const uint32_t words[] = { 54 + size, 0, 54, 40, (uint32_t)s->w, (uint32_t)s->h, 1u | (32u << 16), 0, size };
    memcpy(h + 2, words, sizeof words);
    fwrite(h, 1, sizeof h, f);
    for (int y = s->h - 1; y >= 0; --y)
        fwrite((const char *)s->pixels + (size_t)y * s->pitch, 4, s->w, f);
    fclose(f);
    return 0;
}

static inline const char *SDL_GetError() { return "headless stand-in"; }
static inline void SDL_GetVersion(SDL_version *v) { SDL_VERSION(v); }
static inline SDL_Window *SDL_CreateWindow(const char *, int, int, int, int, uint32_t) { return new SDL_Window; }
static inline SDL_Renderer *SDL_CreateRenderer(SDL_Window *, int, uint32_t) { return new SDL_Renderer; }
static inline SDL_Texture *SDL_CreateTexture(SDL_Renderer *, uint32_t, int, int w, int h)
{
    SDL_Texture *t = new SDL_Texture;
    t->w = w; t->h = h;
    return t;
}
static inline int SDL_SetHint(const char *, const char *) { return 1; }
static inline int SDL_RenderSetLogicalSize(SDL_Renderer *, int, int) { return 0; }
static inline int SDL_RenderClear(SDL_Renderer *) { return 0; }
static inline int SDL_RenderCopy(SDL_Renderer *, SDL_Texture *, const SDL_Rect *, const SDL_Rect *) { return 0; }
static inline void SDL_RenderPresent(SDL_Renderer *) {}
static inline void SDL_DestroyTexture(SDL_Texture *t) { delete t; }
static inline void SDL_DestroyRenderer(SDL_Renderer *r) { delete r; }
static inline void SDL_DestroyWindow(SDL_Window *w) { delete w; }
static inline void SDL_Quit()
{
    cg_ref_shim_state &s = cg_ref_shim();
    if (s.frames) fclose(s.frames);
    if (s.state) fclose(s.state);
    s.frames = s.state = 0;
}

#endif
