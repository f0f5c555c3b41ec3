// bloom_arg.h -- the --bloom flag of the headless raytracer and rasteriser apps.
#pragma once

#include <cstdlib>
#include <string>
#include <vector>

#include "cg_render.h"

#define BLOOM_USAGE "--bloom THRESHOLD,INTENSITY[,LEVELS[,CAP]]"

// THRESHOLD,INTENSITY[,LEVELS[,CAP]] into *b (levels and cap keep their values unless given);
// false for a missing value (NULL) or a list of fewer than two or more than four parts
inline bool ParseBloomArg(const char *value, cg_hdr_bloom_params *b)
{
    if (!value) return false;
    const std::string v = value;
    std::vector<std::string> part;
    for (size_t at = 0;;) {
        const size_t comma = v.find(',', at);
        part.push_back(v.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    if (part.size() < 2 || part.size() > 4) return false;
    b->threshold = (float)atof(part[0].c_str());
    b->intensity = (float)atof(part[1].c_str());
    if (part.size() > 2) b->levels = atoi(part[2].c_str());
    if (part.size() > 3) b->cap = (float)atof(part[3].c_str());
    return true;
}
