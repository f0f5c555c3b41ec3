// jpeg_arg.h -- the --jpeg / --quality / --subsampling flags of the headless raytracer and
// rasteriser apps, and the writers behind them.
#pragma once

#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

#include "cg_render.h"

#define JPEG_USAGE "--jpeg FILE [--quality 1..100] [--subsampling 444|420]"

struct JpegArg {
    std::string path;                          // empty: no --jpeg
    cg_jpeg_params params{75, CG_JPEG_420};
};

// 0: `flag` is none of the three; 1: taken into *j; -1: a missing or invalid value
inline int ParseJpegArg(const std::string &flag, const char *value, JpegArg *j)
{
    if (flag != "--jpeg" && flag != "--quality" && flag != "--subsampling") return 0;
    if (!value) return -1;
    const std::string v = value;
    if (flag == "--jpeg") {
        j->path = v;
        return v.empty() ? -1 : 1;
    }
    if (flag == "--quality") {
        j->params.quality = atoi(value);
        return j->params.quality >= 1 && j->params.quality <= 100 ? 1 : -1;
    }
    if (v != "444" && v != "420") return -1;
    j->params.subsampling = v == "444" ? CG_JPEG_444 : CG_JPEG_420;
    return 1;
}

inline bool JpegSave(const std::string &path, const std::vector<uint8_t> &bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(bytes.data()), (std::streamsize)bytes.size());
    return (bool)f;
}

// n frames of w x h pixels, one after the other in host memory, each through the device encoder
// (cg_image_encode_jpeg); the files concatenated into *bytes.  Returns the library's status.
inline int JpegEncodeFrames(cg_ctx *ctx, const uint32_t *argb, size_t n, int w, int h, const cg_jpeg_params &p,
                            std::vector<uint8_t> *bytes)
{
    const long long bound = cg_image_jpeg_bound(w, h, p.subsampling);
    if (bound < 0) return (int)bound;
    std::vector<uint8_t> file((size_t)bound);
    for (size_t f = 0; f < n; ++f) {
        size_t len = 0;
        const int rc = cg_image_encode_jpeg(ctx, argb + f * (size_t)w * h, w, h, 0, &p, file.data(), file.size(), &len);
        if (rc) return rc;
        bytes->insert(bytes->end(), file.begin(), file.begin() + (std::ptrdiff_t)len);
    }
    return CG_OK;
}

// A delivery call (cg_rt_render_sequence_jpeg / cg_rast_draw_sequence_jpeg bound to its scene
// arguments) into *bytes: n frames' files back to back, the call repeated once at the capacity it
// asks for when the first guess was short.
inline int JpegDeliver(const std::function<int(uint8_t *, size_t, size_t *)> &call, size_t n, int w, int h,
                       std::vector<uint8_t> *bytes)
{
    std::vector<size_t> offsets(n + 1, 0);
    bytes->resize(n * (size_t)w * h / 4 + 4096);
    int rc = call(bytes->data(), bytes->size(), offsets.data());
    if (rc == CG_E_CAPACITY) {
        bytes->resize(offsets[n]);
        rc = call(bytes->data(), bytes->size(), offsets.data());
    }
    if (rc == CG_OK) bytes->resize(offsets[n]);
    return rc;
}
