/* TEST INFRASTRUCTURE ONLY -- the reference rasteriser's model header, with a scene from a file.
 *
 * The rasteriser names "TestModelH.h" in quotes; the generated copy of its skeleton.cpp lies in a
 * directory without that file and finds this one first on the -I path (recipe:
 * oracle/ref_build.py).  This header takes in the reference's own header whole, through the path
 * macro CG_REF_MODEL_HEADER, with its LoadTestModel renamed, and defines a LoadTestModel that
 *
 *   CG_REF_SCENE unset    calls the renamed original;
 *   CG_REF_SCENE = file   reads int32 n_room, int32 n_boxes, then n_room + n_boxes records of 84
 *                         bytes (v0[4] v1[4] v2[4] normal[4] color[3] as floats, int32 texture,
 *                         int32 index; the normal is not read: the reference's constructor
 *                         computes it), room records first.  texture and index are set from the
 *                         record, so no field of a Triangle is left uninitialised;
 *   CG_REF_SCENE_NORMALS  receives, once, the normals the reference's ComputeNormal gave
 *                         ((n_room + n_boxes) x 4 floats).
 *
 * Triangle and everything it does stay the reference's code.
 */
#ifndef CG_REF_SHIM_SCENE_RAST_MODEL_H
#define CG_REF_SHIM_SCENE_RAST_MODEL_H

#ifndef CG_REF_MODEL_HEADER
#error "give the reference's model header as -DCG_REF_MODEL_HEADER='\"<path>/TestModelH.h\"'"
#endif

#define LoadTestModel cg_ref_shim_original_LoadTestModel
#include CG_REF_MODEL_HEADER
#undef LoadTestModel

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline void cg_ref_shim_scene_fail(const char *path, const char *what)
{
    fprintf(stderr, "CG_REF_SCENE %s: %s\n", path, what);
    exit(3);
}

void LoadTestModel(std::vector<Triangle> &room, std::vector<Triangle> &boxes)
{
    const char *path = getenv("CG_REF_SCENE");
    if (!path) {
        cg_ref_shim_original_LoadTestModel(room, boxes);
        return;
    }
    room.clear();
    boxes.clear();
    FILE *f = fopen(path, "rb");
    if (!f)
        cg_ref_shim_scene_fail(path, "cannot open");
    int32_t counts[2];
    if (fread(counts, sizeof(int32_t), 2, f) != 2 || counts[0] < 0 || counts[1] < 0)
        cg_ref_shim_scene_fail(path, "bad header");
    for (int32_t i = 0; i < counts[0] + counts[1]; ++i) {
        float r[19];
        int32_t ti[2];
        if (fread(r, sizeof(float), 19, f) != 19 || fread(ti, sizeof(int32_t), 2, f) != 2)
            cg_ref_shim_scene_fail(path, "short triangle record");
        Triangle t(glm::vec4(r[0], r[1], r[2], r[3]), glm::vec4(r[4], r[5], r[6], r[7]),
                   glm::vec4(r[8], r[9], r[10], r[11]), glm::vec3(r[16], r[17], r[18]));
        t.texture = ti[0];
        t.index = ti[1];
        (i < counts[0] ? room : boxes).push_back(t);
    }
    fclose(f);
    if (const char *np = getenv("CG_REF_SCENE_NORMALS")) {
        FILE *g = fopen(np, "wb");
        if (!g)
            cg_ref_shim_scene_fail(np, "cannot write the normals");
        for (size_t i = 0; i < room.size(); ++i)
            fwrite(&room[i].normal, sizeof(float), 4, g);
        for (size_t i = 0; i < boxes.size(); ++i)
            fwrite(&boxes[i].normal, sizeof(float), 4, g);
        fclose(g);
    }
}

#endif
