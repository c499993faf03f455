// tests/golden/light_probe.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Built and run only by tests/golden/make_light_golden.py.
//
// A SurfaceIntegrator plugin for the reference renderer (interface core/transport.h:35-50; factory symbol CreateSurfaceIntegrator as in
// integrators/whitted.cpp:141) that asks of a light what EstimateDirect asks (core/transport.cpp): Preprocess (called once at core/scene.cpp:38,
// before the first camera sample) reads query records from a file, and for each one sets the keyed random stream (oracle/ref/keyed_rng.cpp) to
// the record's key, burns `counter` draws, and calls scene->lights[l]->Sample_L -- with the normal or without, as the record says --, Pdf, Le and
// IsDeltaLight, and writes what they returned.
//   SurfaceIntegrator "lightprobe" "string queries" ["queries.bin"] "string dump" ["light.bin"]
// query  = 16 words: p[3] n[3] | light (int32) with_normal (int32) | u1 u2 | key counter (uint32) | wi[3] | pad
// answer = 24 floats: s_wi[3] s_L[3] s_pdf | vis.r: o[3] d[3] mint maxt | draws made by Sample_L | Pdf | Le[3] | IsDeltaLight | pad[3]
// Li returns black: the film of such a run means nothing.
#include "pbrt.h"
#include "transport.h"
#include "scene.h"
#include "light.h"
#include "paramset.h"
#include <stdint.h>
extern "C" void keyed_rng_set_key(uint32_t key);
extern "C" uint32_t keyed_rng_counter();
static void rgb(const Spectrum &s, float *out) {
    // COLOR_SAMPLES floats are a Spectrum's only data (core/color.h:205)
    typedef char spectrum_is_three_floats[sizeof(Spectrum) == 3 * sizeof(float) ? 1 : -1];
    memcpy(out, &s, 3 * sizeof(float));
}
class LightProbe : public SurfaceIntegrator {
public:
    LightProbe(const string &q, const string &d) : queries(q), dump(d) {}
    void Preprocess(const Scene *scene) {
        FILE *in = fopen(queries.c_str(), "rb");
        FILE *out = fopen(dump.c_str(), "wb");
        if (!in || !out) Severe("lightprobe: cannot open \"%s\" / \"%s\"", queries.c_str(), dump.c_str());
        float r[16];
        while (fread(r, sizeof(float), 16, in) == 16) {
            float rec[24]; memset(rec, 0, sizeof rec);
            int32_t l, with_normal; uint32_t key, counter;
            memcpy(&l, &r[6], 4); memcpy(&with_normal, &r[7], 4); memcpy(&key, &r[10], 4); memcpy(&counter, &r[11], 4);
            if (l < 0 || l >= int(scene->lights.size())) Severe("lightprobe: light %d of %d", l, int(scene->lights.size()));
            const Light *light = scene->lights[l];
            const Point p(r[0], r[1], r[2]);
            const Normal n(r[3], r[4], r[5]);
            const Vector wi(r[12], r[13], r[14]);
            keyed_rng_set_key(key);
            for (uint32_t k = 0; k < counter; ++k) RandomFloat();
            Vector swi(0, 0, 0); float spdf = 0.f; VisibilityTester vis;
            const Spectrum sL = with_normal ? light->Sample_L(p, n, r[8], r[9], &swi, &spdf, &vis) : light->Sample_L(p, r[8], r[9], &swi, &spdf, &vis);
            const uint32_t draws = keyed_rng_counter() - counter;
            rec[0] = swi.x; rec[1] = swi.y; rec[2] = swi.z;
            rgb(sL, &rec[3]);
            rec[6] = spdf;
            rec[7] = vis.r.o.x; rec[8] = vis.r.o.y; rec[9] = vis.r.o.z;
            rec[10] = vis.r.d.x; rec[11] = vis.r.d.y; rec[12] = vis.r.d.z;
            rec[13] = vis.r.mint; rec[14] = vis.r.maxt;
            rec[15] = float(draws);
            rec[16] = with_normal ? light->Pdf(p, n, wi) : light->Pdf(p, wi);
            rgb(light->Le(RayDifferential(p, wi)), &rec[17]);
            rec[20] = light->IsDeltaLight() ? 1.f : 0.f;
            fwrite(rec, sizeof(float), 24, out);
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
    return new LightProbe(params.FindOneString("queries", "queries.bin"), params.FindOneString("dump", "light.bin"));
}
