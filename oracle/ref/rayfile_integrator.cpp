// oracle/ref/rayfile_integrator.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// A SurfaceIntegrator plugin (interface core/transport.h:35-50; factory symbol
// CreateSurfaceIntegrator as in integrators/whitted.cpp:141) that holds rays a
// FILE names against the scene, not the camera's: Preprocess (called once at
// core/scene.cpp:38, before the first camera sample) reads records of 8 floats
// o[3] d[3] mint maxt, calls Scene::Intersect on a fresh Ray of those values and
// Scene::IntersectP on another fresh Ray of the same values, and writes the probe
// plugin's record per ray.
//   SurfaceIntegrator "rayfile" "string rays" ["rays.bin"] "string dump" ["hits.bin"]
// record = 20 floats: o[3] d[3] mint maxt | hit t p[3] nn[3] u v | occluded pad
// `occluded` = IntersectP of the ray ITSELF (probe_integrator.cpp: of a shadow
// segment).  t = the Ray's maxt after Intersect.  Li returns black: the film of
// such a run (2 x 2) means nothing.
#include "pbrt.h"
#include "transport.h"
#include "scene.h"
#include "paramset.h"
class RayFileIntegrator : public SurfaceIntegrator {
public:
    RayFileIntegrator(const string &r, const string &d) : rays(r), dump(d) {}
    void Preprocess(const Scene *scene) {
        FILE *in = fopen(rays.c_str(), "rb");
        FILE *out = fopen(dump.c_str(), "wb");
        if (!in || !out) Severe("rayfile: cannot open \"%s\" / \"%s\"", rays.c_str(), dump.c_str());
        float r[8];
        while (fread(r, sizeof(float), 8, in) == 8) {
            float rec[20]; memset(rec, 0, sizeof rec);
            memcpy(rec, r, sizeof r);
            Ray closest(Point(r[0], r[1], r[2]), Vector(r[3], r[4], r[5]), r[6], r[7]);
            Intersection isect;
            if (scene->Intersect(closest, &isect)) {
                rec[8] = 1.f; rec[9] = closest.maxt;
                rec[10] = isect.dg.p.x; rec[11] = isect.dg.p.y; rec[12] = isect.dg.p.z;
                rec[13] = isect.dg.nn.x; rec[14] = isect.dg.nn.y; rec[15] = isect.dg.nn.z;
                rec[16] = isect.dg.u; rec[17] = isect.dg.v;
            }
            Ray any(Point(r[0], r[1], r[2]), Vector(r[3], r[4], r[5]), r[6], r[7]);
            rec[18] = scene->IntersectP(any) ? 1.f : 0.f;
            fwrite(rec, sizeof(float), 20, out);
        }
        fclose(in);
        fclose(out);
    }
    Spectrum Li(const Scene *, const RayDifferential &, const Sample *, float *alpha) const {
        if (alpha) *alpha = 0.f;
        return Spectrum(0.f);
    }
private:
    string rays, dump;
};
extern "C" DLLEXPORT SurfaceIntegrator *CreateSurfaceIntegrator(const ParamSet &params) {
    return new RayFileIntegrator(params.FindOneString("rays", "rays.bin"), params.FindOneString("dump", "rayfile_hits.bin"));
}
