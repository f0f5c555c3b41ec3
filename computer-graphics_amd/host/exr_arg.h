// exr_arg.h -- the --exr / --exr-type / --exr-compression / --exr-colour flags of the headless
// raytracer and rasteriser apps, and the writers behind them.
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "cg_render.h"
#include "png_arg.h"   // PngFramePath, PngSave: the numbered names and the file writer

#define EXR_USAGE "--exr FILE [--exr-type half|float] [--exr-compression zip|none] [--exr-colour rgb|rgba]"

struct ExrArg {
    std::string path;                          // empty: no --exr
    cg_exr_params params{CG_EXR_RGBA, CG_EXR_HALF, CG_EXR_ZIP, 1.0f};
};

// 0: `flag` is none of the four; 1: taken into *p; -1: a missing or invalid value
inline int ParseExrArg(const std::string &flag, const char *value, ExrArg *p)
{
    if (flag != "--exr" && flag != "--exr-type" && flag != "--exr-compression" && flag != "--exr-colour") return 0;
    if (!value) return -1;
    const std::string v = value;
    if (flag == "--exr") {
        p->path = v;
        return v.empty() ? -1 : 1;
    }
    if (flag == "--exr-type") {
        if (v != "half" && v != "float") return -1;
        p->params.type = v == "float" ? CG_EXR_FLOAT : CG_EXR_HALF;
        return 1;
    }
    if (flag == "--exr-compression") {
        if (v != "zip" && v != "none") return -1;
        p->params.compression = v == "none" ? CG_EXR_NONE : CG_EXR_ZIP;
        return 1;
    }
    if (v != "rgb" && v != "rgba") return -1;
    p->params.channels = v == "rgb" ? CG_EXR_RGB : CG_EXR_RGBA;
    return 1;
}

// One w x h picture of four floats a pixel in host memory through the device encoder
// (cg_image_encode_exr) into `path`.  Returns the library's status, CG_E_INVALID for a file that
// cannot be written.
inline int ExrEncodePicture(cg_ctx *ctx, const float *rgba, int w, int h, const cg_exr_params &p, const std::string &path)
{
    const long long bound = cg_image_exr_bound(w, h, p.channels, p.type);
    if (bound < 0) return (int)bound;
    std::vector<uint8_t> file((size_t)bound);
    size_t len = 0;
    const int rc = cg_image_encode_exr(ctx, rgba, w, h, 0, &p, file.data(), file.size(), &len);
    if (rc) return rc;
    return PngSave(path, file.data(), len) ? CG_OK : CG_E_INVALID;
}

// A delivery call (cg_rt_render_sequence_exr / cg_rast_draw_sequence_exr bound to its scene
// arguments): n frames' files into PngFramePath(path, f), the call repeated once at the capacity
// it asks for when the first guess was short.
inline int ExrDeliver(const std::function<int(uint8_t *, size_t, size_t *)> &call, size_t n, int w, int h,
                      const std::string &path)
{
    std::vector<size_t> offsets(n + 1, 0);
    std::vector<uint8_t> bytes(n * (size_t)w * h * 4 + 4096);
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
