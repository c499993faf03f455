// tests/golden/bsdf_probe.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Built and run only by tests/golden/make_bsdf_golden.py.
//
// A SurfaceIntegrator plugin for the reference renderer (interface core/transport.h:35-50; factory symbol CreateSurfaceIntegrator as in
// integrators/whitted.cpp:141) that asks of a hit what an integrator asks: Preprocess (called once at core/scene.cpp:38, before the first camera
// sample) reads query records from a file, and for each one calls Scene::Intersect on a fresh Ray, Intersection::GetBSDF, then BSDF::f, BSDF::Pdf,
// BSDF::Sample_f and BSDF::NumComponents with wo = -d, and Intersection::Le(wo), and writes what they returned.
//   SurfaceIntegrator "bsdfprobe" "string queries" ["queries.bin"] "string dump" ["bsdf.bin"]
// query  = 16 words: o[3] d[3] mint maxt | wi[3] | u1 u2 u3 | flags (int32) | pad
// answer = 36 floats: hit t | dg.p[3] dg.nn[3] dg.u dg.v | bsdf->dgShading.nn[3] bsdf->dgShading.dpdu[3] | f[3] pdf | s_wi[3] s_f[3] s_pdf s_type |
//          NumComponents(flags) | Le[3] | NumComponents() | pad[3]
// A miss leaves everything behind `hit` zero.  A failed sample (pdf == 0) leaves s_wi and s_f zero.  Li returns black: the film of such a run means nothing.
#include "pbrt.h"
#include "transport.h"
#include "scene.h"
#include "reflection.h"
#include "paramset.h"
#include <stdint.h>
static void rgb(const Spectrum &s, float *out) {
    // COLOR_SAMPLES floats are a Spectrum's only data (core/color.h:205)
    typedef char spectrum_is_three_floats[sizeof(Spectrum) == 3 * sizeof(float) ? 1 : -1];
    memcpy(out, &s, 3 * sizeof(float));
}
class BsdfProbe : public SurfaceIntegrator {
public:
    BsdfProbe(const string &q, const string &d) : queries(q), dump(d) {}
    void Preprocess(const Scene *scene) {
        FILE *in = fopen(queries.c_str(), "rb");
        FILE *out = fopen(dump.c_str(), "wb");
        if (!in || !out) Severe("bsdfprobe: cannot open \"%s\" / \"%s\"", queries.c_str(), dump.c_str());
        float r[16];
        while (fread(r, sizeof(float), 16, in) == 16) {
            float rec[36]; memset(rec, 0, sizeof rec);
            int32_t flags; memcpy(&flags, &r[14], sizeof flags);
            RayDifferential ray(Point(r[0], r[1], r[2]), Vector(r[3], r[4], r[5]));
            ray.mint = r[6]; ray.maxt = r[7];
            Intersection isect;
            if (scene->Intersect(ray, &isect)) {
                rec[0] = 1.f; rec[1] = ray.maxt;
                rec[2] = isect.dg.p.x; rec[3] = isect.dg.p.y; rec[4] = isect.dg.p.z;
                rec[5] = isect.dg.nn.x; rec[6] = isect.dg.nn.y; rec[7] = isect.dg.nn.z;
                rec[8] = isect.dg.u; rec[9] = isect.dg.v;
                BSDF *bsdf = isect.GetBSDF(ray);
                const DifferentialGeometry &dgs = bsdf->dgShading;
                rec[10] = dgs.nn.x; rec[11] = dgs.nn.y; rec[12] = dgs.nn.z;
                rec[13] = dgs.dpdu.x; rec[14] = dgs.dpdu.y; rec[15] = dgs.dpdu.z;
                const Vector wo = -ray.d, wi(r[8], r[9], r[10]);
                rgb(bsdf->f(wo, wi, BxDFType(flags)), &rec[16]);
                rec[19] = bsdf->Pdf(wo, wi, BxDFType(flags));
                Vector swi(0, 0, 0); float spdf = 0.f; BxDFType stype = BxDFType(0);
                const Spectrum sf = bsdf->Sample_f(wo, &swi, r[11], r[12], r[13], &spdf, BxDFType(flags), &stype);
                if (spdf != 0.f) {
                    rec[20] = swi.x; rec[21] = swi.y; rec[22] = swi.z;
                    rgb(sf, &rec[23]);
                    rec[26] = spdf; rec[27] = float(int(stype));
                }
                rec[28] = float(bsdf->NumComponents(BxDFType(flags)));
                rgb(isect.Le(wo), &rec[29]);
                rec[32] = float(bsdf->NumComponents());
                BSDF::FreeAll();
            }
            fwrite(rec, sizeof(float), 36, out);
        }
        fclose(in);
        fclose(out);
    }
    Spectrum Li(const Scene *, const RayDifferential &, const Sample *, float *alpha) const {
        if (alpha) *alpha = 0.f;
        return Spectrum(0.f);
    }
private:
    string queries, dump;
};
extern "C" DLLEXPORT SurfaceIntegrator *CreateSurfaceIntegrator(const ParamSet &params) {
    return new BsdfProbe(params.FindOneString("queries", "queries.bin"), params.FindOneString("dump", "bsdf.bin"));
}
