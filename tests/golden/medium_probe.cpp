// tests/golden/medium_probe.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Built and run only by tests/golden/make_medium_golden.py.
//
// A SurfaceIntegrator plugin for the reference renderer (interface core/transport.h:35-50; factory symbol CreateSurfaceIntegrator as in
// integrators/whitted.cpp:141) that asks of scene->volumeRegion and of the scene's volume integrator what an integrator asks: Preprocess (called
// once at core/scene.cpp:38, before the first camera sample) reads query records from a file and writes what the region's sigma_a / sigma_s /
// sigma_t / Lve / p / IntersectP / Tau, the volume integrator's Transmittance with a sample, Scene::Transmittance(ray) and the volume
// integrator's Li returned.  The last two run under the keyed random stream (oracle/ref/keyed_rng.cpp) set to the record's key with `counter`
// draws burnt, each from that same position.  The Sample handed to Transmittance and Li is one built here for this integrator (which requests
// nothing) and the scene's volume integrator: its two one-value requests, tau and scatter, are filled from the record.
//   SurfaceIntegrator "mediumprobe" "string queries" ["queries.bin"] "string dump" ["medium.bin"] "float stepsize" [s]
// query  = 24 words: p[3] w[3] wp[3] | o[3] d[3] mint maxt | u u_scatter | key counter (uint32) | pad[3]
// answer = 32 floats: sigma_a[3] sigma_s[3] sigma_t[3] Lve[3] p | hit t0 t1 | Tau[3] | Transmittance(sample)[3] | Scene::Transmittance[3] its draws |
//                     Li[3] its draws | pad[2]
// Li returns black: the film of such a run means nothing.
#include "pbrt.h"
#include "transport.h"
#include "scene.h"
#include "volume.h"
#include "sampling.h"
#include "paramset.h"
#include <stdint.h>
extern "C" void keyed_rng_set_key(uint32_t key);
extern "C" uint32_t keyed_rng_counter();
static void rgb(const Spectrum &s, float *out) {
    // COLOR_SAMPLES floats are a Spectrum's only data (core/color.h:205)
    typedef char spectrum_is_three_floats[sizeof(Spectrum) == 3 * sizeof(float) ? 1 : -1];
    memcpy(out, &s, 3 * sizeof(float));
}
class MediumProbe : public SurfaceIntegrator {
public:
    MediumProbe(const string &q, const string &d, float s) : queries(q), dump(d), step(s) {}
    void Preprocess(const Scene *scene) {
        FILE *in = fopen(queries.c_str(), "rb");
        FILE *out = fopen(dump.c_str(), "wb");
        if (!in || !out) Severe("mediumprobe: cannot open \"%s\" / \"%s\"", queries.c_str(), dump.c_str());
        VolumeRegion *vr = scene->volumeRegion;
        if (!vr) Severe("mediumprobe: the scene has no volume region");
        Sample sample(this, scene->volumeIntegrator, scene);          // RequestSamples again: the same two offsets, 0 and 1
        if (sample.n1D.size() != 2 || sample.n1D[0] != 1 || sample.n1D[1] != 1) Severe("mediumprobe: the volume integrator's requests are not tau, scatter");
        float r[24];
        while (fread(r, sizeof(float), 24, in) == 24) {
            float rec[32]; memset(rec, 0, sizeof rec);
            uint32_t key, counter;
            memcpy(&key, &r[19], 4); memcpy(&counter, &r[20], 4);
            const Point p(r[0], r[1], r[2]);
            const Vector w(r[3], r[4], r[5]), wp(r[6], r[7], r[8]);
            const Ray ray(Point(r[9], r[10], r[11]), Vector(r[12], r[13], r[14]), r[15], r[16]);
            rgb(vr->sigma_a(p, w), &rec[0]);
            rgb(vr->sigma_s(p, w), &rec[3]);
            rgb(vr->sigma_t(p, w), &rec[6]);
            rgb(vr->Lve(p, w), &rec[9]);
            rec[12] = vr->p(p, w, wp);
            float t0 = 0.f, t1 = 0.f;
            const bool hit = vr->IntersectP(ray, &t0, &t1);
            rec[13] = hit ? 1.f : 0.f; rec[14] = hit ? t0 : 0.f; rec[15] = hit ? t1 : 0.f;
            rgb(vr->Tau(ray, step, r[17]), &rec[16]);
            sample.oneD[0][0] = r[17]; sample.oneD[1][0] = r[18];
            rgb(scene->volumeIntegrator->Transmittance(scene, ray, &sample, NULL), &rec[19]);
            keyed_rng_set_key(key);
            for (uint32_t k = 0; k < counter; ++k) RandomFloat();
            rgb(scene->Transmittance(ray), &rec[22]);
            rec[25] = float(keyed_rng_counter() - counter);
            keyed_rng_set_key(key);
            for (uint32_t k = 0; k < counter; ++k) RandomFloat();
            rgb(scene->volumeIntegrator->Li(scene, RayDifferential(ray), &sample, NULL), &rec[26]);
            rec[29] = float(keyed_rng_counter() - counter);
            fwrite(rec, sizeof(float), 32, out);
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
    float step;
};
extern "C" DLLEXPORT SurfaceIntegrator *CreateSurfaceIntegrator(const ParamSet &params) {
    return new MediumProbe(params.FindOneString("queries", "queries.bin"), params.FindOneString("dump", "medium.bin"), params.FindOneFloat("stepsize", 1.f));
}
