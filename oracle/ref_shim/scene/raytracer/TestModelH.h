/* TEST INFRASTRUCTURE ONLY -- the reference raytracer's model header, with a scene from a file.
 *
 * The raytracer names "TestModelH.h" in quotes; a byte-identical copy of its skeleton.cpp in a
 * directory without that file finds this one first on the -I path (recipe: oracle/ref_build.py).
 * This header takes in the reference's own header whole, through the path macro
 * CG_REF_MODEL_HEADER, with its LoadTestModel renamed, and defines a LoadTestModel that
 *
 *   CG_REF_SCENE unset    calls the renamed original;
 *   CG_REF_SCENE = file   reads int32 n_tris, int32 n_spheres, n_tris records of 19 floats
 *                         (v0[4] v1[4] v2[4] normal[4] color[3]; the normal is not read: the
 *                         reference's constructor computes it), then n_spheres records of 7
 *                         floats (centre[3] radius color[3]);
 *   CG_REF_SCENE_NORMALS  receives, once, the normals the reference's ComputeNormal gave
 *                         (n_tris x 4 floats).
 *
 * Triangle, Sphere and everything they do stay the reference's code.
 */
#ifndef CG_REF_SHIM_SCENE_RT_MODEL_H
#define CG_REF_SHIM_SCENE_RT_MODEL_H

#ifndef CG_REF_MODEL_HEADER
#error "give the reference's model header as -DCG_REF_MODEL_HEADER='\"<path>/TestModelH.h\"'"
#endif

#define LoadTestModel cg_ref_shim_original_LoadTestModel
#include CG_REF_MODEL_HEADER
#undef LoadTestModel

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

struct cg_ref_shim_rt_scene {
    bool tried, loaded;
    std::vector<Triangle> triangles;
    std::vector<Sphere> spheres;
};

static inline void cg_ref_shim_scene_fail(const char *path, const char *what)
{
    fprintf(stderr, "CG_REF_SCENE %s: %s\n", path, what);
    exit(3);
}

static inline cg_ref_shim_rt_scene &cg_ref_shim_rt_scene_get()
{
    static cg_ref_shim_rt_scene s;
    if (s.tried)
        return s;
    s.tried = true;
    const char *path = getenv("CG_REF_SCENE");
    if (!path)
        return s;
    FILE *f = fopen(path, "rb");
    if (!f)
        cg_ref_shim_scene_fail(path, "cannot open");
    int32_t counts[2];
    if (fread(counts, sizeof(int32_t), 2, f) != 2 || counts[0] < 0 || counts[1] < 0)
        cg_ref_shim_scene_fail(path, "bad header");
    for (int32_t i = 0; i < counts[0]; ++i) {
        float r[19];
        if (fread(r, sizeof(float), 19, f) != 19)
            cg_ref_shim_scene_fail(path, "short triangle record");
        s.triangles.push_back(Triangle(glm::vec4(r[0], r[1], r[2], r[3]), glm::vec4(r[4], r[5], r[6], r[7]),
                                       glm::vec4(r[8], r[9], r[10], r[11]), glm::vec3(r[16], r[17], r[18])));
    }
    for (int32_t i = 0; i < counts[1]; ++i) {
        float r[7];
        if (fread(r, sizeof(float), 7, f) != 7)
            cg_ref_shim_scene_fail(path, "short sphere record");
        s.spheres.push_back(Sphere(glm::vec3(r[0], r[1], r[2]), r[3], glm::vec3(r[4], r[5], r[6])));
    }
    fclose(f);
    if (const char *np = getenv("CG_REF_SCENE_NORMALS")) {
        FILE *g = fopen(np, "wb");
        if (!g)
            cg_ref_shim_scene_fail(np, "cannot write the normals");
        for (size_t i = 0; i < s.triangles.size(); ++i)
            fwrite(&s.triangles[i].normal, sizeof(float), 4, g);
        fclose(g);
    }
    s.loaded = true;
    return s;
}

void LoadTestModel(std::vector<Triangle> &triangles, std::vector<Sphere> &spheres)
{
    cg_ref_shim_rt_scene &s = cg_ref_shim_rt_scene_get();
    if (!s.loaded) {
        cg_ref_shim_original_LoadTestModel(triangles, spheres);
        return;
    }
    triangles = s.triangles;
    spheres = s.spheres;
}

#endif
