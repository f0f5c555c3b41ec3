// png_arg.h -- the --png / --png-colour / --png-filter flags of the headless raytracer and
// rasteriser apps, and the writers behind them.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "cg_render.h"

#define PNG_USAGE "--png FILE [--png-colour rgb|rgba] [--png-filter adaptive|0..4]"

struct PngArg {
    std::string path;                          // empty: no --png
    cg_png_params params{CG_PNG_RGB, CG_PNG_FILTER_ADAPTIVE};
};

// 0: `flag` is none of the three; 1: taken into *p; -1: a missing or invalid value
inline int ParsePngArg(const std::string &flag, const char *value, PngArg *p)
{
    if (flag != "--png" && flag != "--png-colour" && flag != "--png-filter") return 0;
    if (!value) return -1;
    const std::string v = value;
    if (flag == "--png") {
        p->path = v;
        return v.empty() ? -1 : 1;
    }
    if (flag == "--png-colour") {
        if (v != "rgb" && v != "rgba") return -1;
        p->params.colour = v == "rgba" ? CG_PNG_RGBA : CG_PNG_RGB;
        return 1;
    }
    if (v == "adaptive") {
        p->params.filter = CG_PNG_FILTER_ADAPTIVE;
        return 1;
    }
    if (v.size() != 1 || v[0] < '0' || v[0] > '4') return -1;
    p->params.filter = v[0] - '0';
    return 1;
}

// FILE with .%04d before its extension: frame k of a --batch run
inline std::string PngFramePath(const std::string &path, size_t k)
{
    char num[32];
    snprintf(num, sizeof num, ".%04zu", k);
    const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + num;
    return path.substr(0, dot) + num + path.substr(dot);
}

inline bool PngSave(const std::string &path, const uint8_t *bytes, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(bytes), (std::streamsize)n);
    return (bool)f;
}

// n frames of w x h pixels, one after the other in host memory, each through the device encoder
// (cg_image_encode_png) into name(f).  Returns the library's status, CG_E_INVALID for a file that
// cannot be written.
inline int PngEncodeFrames(cg_ctx *ctx, const uint32_t *argb, size_t n, int w, int h, const cg_png_params &p,
                           const std::function<std::string(size_t)> &name)
{
    const long long bound = cg_image_png_bound(w, h, p.colour);
    if (bound < 0) return (int)bound;
    std::vector<uint8_t> file((size_t)bound);
    for (size_t f = 0; f < n; ++f) {
        size_t len = 0;
        const int rc = cg_image_encode_png(ctx, argb + f * (size_t)w * h, w, h, 0, &p, file.data(), file.size(), &len);
        if (rc) return rc;
        if (!PngSave(name(f), file.data(), len)) return CG_E_INVALID;
    }
    return CG_OK;
}

// A delivery call (cg_rt_render_sequence_png / cg_rast_draw_sequence_png bound to its scene
// arguments): n frames' files into PngFramePath(path, f), the call repeated once at the capacity
// it asks for when the first guess was short.
inline int PngDeliver(const std::function<int(uint8_t *, size_t, size_t *)> &call, size_t n, int w, int h,
                      const std::string &path)
{
    std::vector<size_t> offsets(n + 1, 0);
    std::vector<uint8_t> bytes(n * (size_t)w * h + 4096);
    int rc = call(bytes.data(), bytes.size(), offsets.data());
    if (rc == CG_E_CAPACITY) {
        bytes.resize(offsets[n]);
        rc = call(bytes.data(), bytes.size(), offsets.data());
    }
    if (rc) return rc;
    for (size_t f = 0; f < n; ++f)
        if (!PngSave(PngFramePath(path, f), bytes.data() + offsets[f], offsets[f + 1] - offsets[f])) return CG_E_INVALID;
    return CG_OK;
}
