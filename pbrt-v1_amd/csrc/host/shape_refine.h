// shape_refine.h -- the reference's three CanIntersect() == false shapes, refined on the host into the one triangle mesh each of them hands to
// MakeShape("trianglemesh") inside Refine: shapes/heightfield.cpp:65-107, shapes/nurbs.cpp:224-298, shapes/loopsubdiv.cpp:246-438.
//
// The vertices, uvs, normals and the index order are the reference's bit for bit: every rule below keeps the reference's float operations in
// their order (the cited lines), and this file is compiled with the reference's own flags (no x87, no contraction) against the same libm.
// A statement the reference would assert on, crash on or walk garbage for is an Error here and gives no mesh.
#pragma once
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "paramset.h"

namespace pbrthip {

struct RefinedMesh {                       // what the reference's Refine puts into the ParamSet of its trianglemesh
    std::vector<int> indices;
    std::vector<Float3> P, N;              // N: empty (heightfield) or one per vertex
    std::vector<float> uv;                 // empty (loopsubdiv) or two per vertex
};

namespace refine {
inline Float3 mul(float f, Float3 p) { return Float3{f * p.x, f * p.y, f * p.z}; }              // geometry.h:129-131, :57-59
inline Float3 add(Float3 a, Float3 b) { return Float3{a.x + b.x, a.y + b.y, a.z + b.z}; }
inline Float3 sub(Float3 a, Float3 b) { return Float3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline Float3 cross(Float3 a, Float3 b) {                                                      // geometry.h:306-310
    return Float3{(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)};
}
// two triangles per cell of an nx x ny vertex grid, vertex (x, y) at x + y * nx (heightfield.cpp:84-97, nurbs.cpp:270-282)
inline void gridIndices(int nx, int ny, std::vector<int> &out) {
    out.clear(); out.reserve(size_t(6) * size_t(nx - 1) * size_t(ny - 1));
    for (int y = 0; y < ny - 1; ++y)
        for (int x = 0; x < nx - 1; ++x) {
            const int v00 = x + y * nx, v10 = v00 + 1, v11 = v10 + nx, v01 = v00 + nx;
            const int cell[6] = {v00, v10, v11, v00, v11, v01};
            out.insert(out.end(), cell, cell + 6);
        }
}
}  // namespace refine

// ------------------------------------------------------------------ heightfield (heightfield.cpp:65-117)
inline bool RefineHeightfield(const ParamSet &ps, RefinedMesh *out) {
    const int nx = ps.FindOneInt("nu", -1), ny = ps.FindOneInt("nv", -1);
    int nitems = 0;
    const float *z = ps.FindFloat("Pz", &nitems);
    // the reference asserts on these (:114-115) and, under NDEBUG, reads past "Pz"
    if (nx == -1 || ny == -1 || !z) { Error("Shape \"heightfield\" needs \"integer nu\", \"integer nv\" and \"float Pz\"; shape ignored"); return false; }
    if (nx < 2 || ny < 2) { Error("Shape \"heightfield\": nu = %d, nv = %d, both must be at least 2; shape ignored", nx, ny); return false; }
    if ((long long)nx * ny != (long long)nitems) { Error("Shape \"heightfield\" has %d \"Pz\" values but nu*nv = %lld; shape ignored", nitems, (long long)nx * ny); return false; }
    out->P.resize(size_t(nitems)); out->uv.resize(size_t(nitems) * 2); out->N.clear();
    size_t pos = 0;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x, ++pos) {                                                   // :75-82
            const float u = (float)x / (float)(nx - 1), v = (float)y / (float)(ny - 1);
            out->P[pos] = Float3{u, v, z[pos]};
            out->uv[2 * pos] = u; out->uv[2 * pos + 1] = v;
        }
    refine::gridIndices(nx, ny, out->indices);
    return true;
}

// ------------------------------------------------------------------ nurbs (nurbs.cpp:52-153, :224-332)
namespace refine {
struct H3 { float x, y, z, w; };
// nurbs.cpp:52-62.  For t inside [knot[order-1], knot[np]] the walk ends below np by itself; the bound keeps any other t inside the array.
inline int knotOffset(const float *knot, int order, int np, float t) {
    int k = order - 1;
    while (k + 1 < np && t > knot[k + 1]) ++k;
    return k;
}
// nurbs.cpp:73-123: de Boor's recurrence on `order` homogeneous control points, cp[(first + i - base) * stride]; deriv: the Cartesian derivative
inline H3 evaluate(int order, const float *knot, const H3 *cp, int base, int np, int stride, float t, Float3 *deriv, std::vector<H3> &work) {
    const int off = knotOffset(knot, order, np, t);
    knot += off;
    const int first = off - order + 1;
    work.resize(size_t(order));
    for (int i = 0; i < order; ++i) work[size_t(i)] = cp[size_t(first + i - base) * size_t(stride)];
    float alpha;
    for (int i = 0; i < order - 2; ++i)
        for (int j = 0; j < order - 1 - i; ++j) {
            alpha = (knot[1 + j] - t) / (knot[1 + j] - knot[j + 2 - order + i]);
            H3 &a = work[size_t(j)]; const H3 &b = work[size_t(j) + 1];
            a.x = a.x * alpha + b.x * (1 - alpha);
            a.y = a.y * alpha + b.y * (1 - alpha);
            a.z = a.z * alpha + b.z * (1 - alpha);
            a.w = a.w * alpha + b.w * (1 - alpha);
        }
    alpha = (knot[1] - t) / (knot[1] - knot[0]);
    const H3 c0 = work[0], c1 = work[1];
    const H3 val = {c0.x * alpha + c1.x * (1 - alpha), c0.y * alpha + c1.y * (1 - alpha), c0.z * alpha + c1.z * (1 - alpha), c0.w * alpha + c1.w * (1 - alpha)};
    if (deriv) {
        const float factor = (order - 1) / (knot[1] - knot[0]);
        const H3 delta = {(c1.x - c0.x) * factor, (c1.y - c0.y) * factor, (c1.z - c0.z) * factor, (c1.w - c0.w) * factor};
        deriv->x = delta.x / val.w - (val.x * delta.w / (val.w * val.w));
        deriv->y = delta.y / val.w - (val.y * delta.w / (val.w * val.w));
        deriv->z = delta.z / val.w - (val.z * delta.w / (val.w * val.w));
    }
    return val;
}
}  // namespace refine

// One direction's parameters (CreateShape nurbs.cpp:301-316).  Returns false after an Error.
inline bool nurbsDirection(const ParamSet &ps, const char *d, int *n, int *order, const float **knots, float *t0, float *t1) {
    const std::string s(d);
    *n = ps.FindOneInt("n" + s, -1); *order = ps.FindOneInt(s + "order", -1);
    int nknots = 0;
    *knots = ps.FindFloat(s + "knots", &nknots);
    if (*n == -1 || *order == -1 || !*knots) { Error("Shape \"nurbs\" needs \"integer n%s\", \"integer %sorder\" and \"float %sknots\"; shape ignored", d, d, d); return false; }
    if (*order < 2 || *n < *order) { Error("Shape \"nurbs\": %sorder = %d, n%s = %d: the order must be at least 2 and at most the number of control points; shape ignored", d, *order, d, *n); return false; }
    if (nknots != *n + *order) { Error("Shape \"nurbs\" has %d \"%sknots\" but n%s + %sorder = %d; shape ignored", nknots, d, d, d, *n + *order); return false; }
    const float lo = (*knots)[*order - 1], hi = (*knots)[*n];
    *t0 = ps.FindOneFloat(s + "0", lo); *t1 = ps.FindOneFloat(s + "1", hi);
    // outside the knot range the reference's KnotOffset walks past the knot vector
    if (!(*t0 >= lo && *t0 <= hi && *t1 >= lo && *t1 <= hi)) { Error("Shape \"nurbs\": [%s0, %s1] = [%g, %g] leaves the knot range [%g, %g]; shape ignored", d, d, *t0, *t1, lo, hi); return false; }
    return true;
}

inline bool RefineNurbs(const ParamSet &ps, RefinedMesh *out) {
    int nu, uorder, nv, vorder; const float *uknot, *vknot; float umin, umax, vmin, vmax;
    if (!nurbsDirection(ps, "u", &nu, &uorder, &uknot, &umin, &umax)) return false;
    if (!nurbsDirection(ps, "v", &nv, &vorder, &vknot, &vmin, &vmax)) return false;
    int npts = 0;
    std::vector<refine::H3> Pw;
    if (const Float3 *P = ps.FindPoint("P", &npts)) {                                           // :242-250
        Pw.resize(size_t(npts));
        for (int i = 0; i < npts; ++i) Pw[size_t(i)] = refine::H3{P[i].x, P[i].y, P[i].z, 1.f};
    } else if (const float *w = ps.FindFloat("Pw", &npts)) {
        npts /= 4;
        Pw.resize(size_t(npts));
        for (int i = 0; i < npts; ++i) Pw[size_t(i)] = refine::H3{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    } else return false;                                                                        // :321-324: no shape, and no message
    if ((long long)npts != (long long)nu * nv) { Error("Shape \"nurbs\" has %d control points but nu*nv = %lld; shape ignored", npts, (long long)nu * nv); return false; }

    const int diceu = 30, dicev = 30;                                                           // :226
    float ueval[diceu], veval[dicev];
    for (int i = 0; i < diceu; ++i) { const float t = (float)i / (float)(diceu - 1); ueval[i] = (1.f - t) * umin + t * umax; }   // Lerp pbrt.h:549-551
    for (int i = 0; i < dicev; ++i) { const float t = (float)i / (float)(dicev - 1); veval[i] = (1.f - t) * vmin + t * vmax; }
    out->P.resize(size_t(diceu * dicev)); out->N.resize(size_t(diceu * dicev)); out->uv.resize(size_t(2 * diceu * dicev));
    std::vector<refine::H3> iso(size_t(std::max(uorder, vorder))), work;
    for (int v = 0; v < dicev; ++v)
        for (int u = 0; u < diceu; ++u) {
            const size_t at = size_t(v * diceu + u);
            const float tu = ueval[u], tv = veval[v];
            out->uv[2 * at] = tu; out->uv[2 * at + 1] = tv;
            // NURBSEvaluateSurface :124-153: iso-curve in v through the uorder control columns that matter, then along u with dPdu ...
            const int uFirst = refine::knotOffset(uknot, uorder, nu, tu) - uorder + 1;
            for (int i = 0; i < uorder; ++i) iso[size_t(i)] = refine::evaluate(vorder, vknot, &Pw[size_t(uFirst + i)], 0, nv, nu, tv, nullptr, work);
            const int vFirst = refine::knotOffset(vknot, vorder, nv, tv) - vorder + 1;
            Float3 dPdu, dPdv;
            const refine::H3 p = refine::evaluate(uorder, uknot, iso.data(), uFirst, nu, 1, tu, &dPdu, work);
            // ... and the other way round for dPdv
            for (int i = 0; i < vorder; ++i) iso[size_t(i)] = refine::evaluate(uorder, uknot, &Pw[size_t(vFirst + i) * size_t(nu)], 0, nu, 1, tu, nullptr, work);
            (void)refine::evaluate(vorder, vknot, iso.data(), vFirst, nv, 1, tv, &dPdv, work);
            out->P[at] = Float3{p.x / p.w, p.y / p.w, p.z / p.w};
            const Float3 n = refine::cross(dPdu, dPdv);                                         // :262 Normalize: v / Length, geometry.h:65-69
            const float inv = 1.f / sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);
            out->N[at] = Float3{n.x * inv, n.y * inv, n.z * inv};
        }
    refine::gridIndices(diceu, dicev, out->indices);
    return true;
}

// ------------------------------------------------------------------ loopsubdiv (loopsubdiv.cpp:161-226, :246-494)
// The reference's SDVertex / SDFace pointers are indices here: a level is the faces' three vertices and three neighbours (-1: none) and a
// vertex's startFace / boundary / regular.  One level of subdivision is a few linear passes over these arrays; nothing in the output
// depends on an address (the reference orders an edge's end points by pointer value, but only adds fl(c*a) + fl(c*b), which commutes).
namespace refine {
struct SubdivLevel {
    std::vector<Float3> P;
    std::vector<int> fv, fn, startFace;                  // fv, fn: 3 per face
    std::vector<uint8_t> boundary, regular;
    int nverts() const { return int(P.size()); }
    int nfaces() const { return int(fv.size() / 3); }
    static int next(int i) { return (i + 1) % 3; }
    static int prev(int i) { return (i + 2) % 3; }
    int vnum(int f, int v) const { return fv[3 * f] == v ? 0 : (fv[3 * f + 1] == v ? 1 : 2); }
    int nextFace(int f, int v) const { return fn[3 * f + vnum(f, v)]; }
    int prevFace(int f, int v) const { return fn[3 * f + prev(vnum(f, v))]; }
    int nextVert(int f, int v) const { return fv[3 * f + next(vnum(f, v))]; }
    int prevVert(int f, int v) const { return fv[3 * f + prev(vnum(f, v))]; }
    int otherVert(int f, int a, int b) const {                                                  // :83-89
        for (int i = 0; i < 3; ++i) if (fv[3 * f + i] != a && fv[3 * f + i] != b) return fv[3 * f + i];
        return a;
    }
    // SDVertex::oneRing :449-469 into `ring`; its size is SDVertex::valence :140-159
    int oneRing(int v, std::vector<Float3> &ring) const {
        ring.clear();
        int f = startFace[v];
        if (!boundary[v]) {
            do { ring.push_back(P[nextVert(f, v)]); f = nextFace(f, v); } while (f != startFace[v]);
        } else {
            int f2;
            while ((f2 = nextFace(f, v)) != -1) f = f2;
            ring.push_back(P[nextVert(f, v)]);
            do { ring.push_back(P[prevVert(f, v)]); f = prevFace(f, v); } while (f != -1);
        }
        return int(ring.size());
    }
    int valence(int v, std::vector<Float3> &ring) const { return oneRing(v, ring); }
    Float3 weightOneRing(int v, float beta, std::vector<Float3> &ring) const {                 // :439-448
        const int valence = oneRing(v, ring);
        Float3 p = mul(1 - valence * beta, P[v]);
        for (int i = 0; i < valence; ++i) p = add(p, mul(beta, ring[size_t(i)]));
        return p;
    }
    Float3 weightBoundary(int v, float beta, std::vector<Float3> &ring) const {                // :470-480
        const int valence = oneRing(v, ring);
        Float3 p = mul(1 - 2 * beta, P[v]);
        p = add(p, mul(beta, ring[0]));
        p = add(p, mul(beta, ring[size_t(valence) - 1]));
        return p;
    }
};
const float kPi = 3.14159265358979323846f;                                                               // pbrt.h:204: M_PI redefined as a float
inline float loopBeta(int valence) { return valence == 3 ? 3.f / 16.f : 3.f / (8.f * valence); }          // :125-128
inline float loopGamma(int valence) { return 1.f / (valence + 3.f / (8.f * loopBeta(valence))); }         // :131-133

// LoopSubdiv constructor :161-226.  Returns false after an Error for what the reference cannot represent.
inline bool buildControlMesh(const int *vi, int nfaces, const Float3 *P, int nverts, SubdivLevel &m) {
    m.P.assign(P, P + nverts);
    m.fv.assign(vi, vi + size_t(nfaces) * 3);
    m.fn.assign(size_t(nfaces) * 3, -1);
    m.startFace.assign(size_t(nverts), -1);
    m.boundary.assign(size_t(nverts), 0); m.regular.assign(size_t(nverts), 0);
    for (int f = 0; f < nfaces; ++f)
        for (int j = 0; j < 3; ++j) {
            const int v = vi[3 * f + j];
            if (v < 0 || v >= nverts) { Error("Shape \"loopsubdiv\" has out of-bounds vertex index %d (%d \"P\" values were given); shape ignored", v, nverts); return false; }
            m.startFace[size_t(v)] = f;                                                         // :178-187: the LAST face that names it
        }
    for (int f = 0; f < nfaces; ++f)
        if (vi[3 * f] == vi[3 * f + 1] || vi[3 * f + 1] == vi[3 * f + 2] || vi[3 * f + 2] == vi[3 * f]) {
            Error("Shape \"loopsubdiv\": face %d names a vertex twice; shape ignored", f); return false;
        }
    for (int v = 0; v < nverts; ++v)
        if (m.startFace[size_t(v)] < 0) { Error("Shape \"loopsubdiv\": vertex %d is in no face (the reference dereferences its NULL startFace); shape ignored", v); return false; }
    // Neighbours :188-210.  The reference keeps the open edges in a std::set ordered by the end points' addresses and only ever looks one up;
    // a hash map keyed on the two indices finds the same face.  value: 3 * face + edge of the first face on the edge, -2 once two faces share it
    std::unordered_map<uint64_t, int> open;
    open.reserve(size_t(nfaces) * 3);
    for (int f = 0; f < nfaces; ++f)
        for (int e = 0; e < 3; ++e) {
            const int a = vi[3 * f + e], b = vi[3 * f + SubdivLevel::next(e)];
            const uint64_t key = (uint64_t(uint32_t(std::min(a, b))) << 32) | uint32_t(std::max(a, b));
            auto it = open.find(key);
            if (it == open.end()) { open.emplace(key, 3 * f + e); continue; }
            if (it->second == -2) { Error("Shape \"loopsubdiv\": the edge (%d, %d) is shared by more than two faces; shape ignored", a, b); return false; }
            const int f0 = it->second / 3, e0 = it->second % 3;
            if (vi[3 * f0 + e0] == a) { Error("Shape \"loopsubdiv\": faces %d and %d run along the edge (%d, %d) in the same direction (inconsistent winding); shape ignored", f0, f, a, b); return false; }
            m.fn[size_t(3 * f0 + e0)] = f; m.fn[size_t(3 * f + e)] = f0;
            it->second = -2;
        }
    std::vector<Float3> ring;
    for (int v = 0; v < nverts; ++v) {                                                          // :211-225
        int f = m.startFace[size_t(v)];
        do { f = m.nextFace(f, v); } while (f != -1 && f != m.startFace[size_t(v)]);
        m.boundary[size_t(v)] = f == -1;
        const int valence = m.valence(v, ring);
        m.regular[size_t(v)] = (!m.boundary[size_t(v)] && valence == 6) || (m.boundary[size_t(v)] && valence == 4);
    }
    return true;
}

// one pass of the loop :253-358: `m` becomes its subdivided mesh.  Vertices: the even children in parent order, then the odd vertices in the
// order the face loop creates them; faces: the four children of each face in face order.
inline void subdivideOnce(SubdivLevel &m, std::vector<Float3> &ring) {
    const int nv = m.nverts(), nf = m.nfaces();
    SubdivLevel c;
    c.P.resize(size_t(nv)); c.P.reserve(size_t(nv) + size_t(nf) * 3 / 2 + 3);
    c.boundary = m.boundary; c.regular = m.regular;                                             // :258-263
    c.startFace.resize(size_t(nv));
    for (int v = 0; v < nv; ++v) {                                                              // even vertices :271-284
        if (!m.boundary[size_t(v)])
            c.P[size_t(v)] = m.regular[size_t(v)] ? m.weightOneRing(v, 1.f / 16.f, ring) : m.weightOneRing(v, loopBeta(m.valence(v, ring)), ring);
        else
            c.P[size_t(v)] = m.weightBoundary(v, 1.f / 8.f, ring);
    }
    // Odd vertices :286-316.  The reference finds an edge's vertex in a std::map keyed on the end points' addresses; here the face that creates it
    // writes its index into its own edge slot and into its neighbour's, so the look-up is an array read.
    std::vector<int> edgeVert(size_t(nf) * 3, -1);
    for (int f = 0; f < nf; ++f)
        for (int k = 0; k < 3; ++k) {
            if (edgeVert[size_t(3 * f + k)] >= 0) continue;
            const int a = m.fv[size_t(3 * f + k)], b = m.fv[size_t(3 * f + SubdivLevel::next(k))], f2 = m.fn[size_t(3 * f + k)];
            const int vert = int(c.P.size());
            Float3 p;
            if (f2 == -1) {
                p = mul(0.5f, m.P[size_t(a)]);
                p = add(p, mul(0.5f, m.P[size_t(b)]));
            } else {
                p = mul(3.f / 8.f, m.P[size_t(a)]);
                p = add(p, mul(3.f / 8.f, m.P[size_t(b)]));
                p = add(p, mul(1.f / 8.f, m.P[size_t(m.otherVert(f, a, b))]));
                p = add(p, mul(1.f / 8.f, m.P[size_t(m.otherVert(f2, a, b))]));
                for (int k2 = 0; k2 < 3; ++k2)
                    if (m.fn[size_t(3 * f2 + k2)] == f && m.fv[size_t(3 * f2 + k2)] == b && m.fv[size_t(3 * f2 + SubdivLevel::next(k2))] == a) edgeVert[size_t(3 * f2 + k2)] = vert;
            }
            edgeVert[size_t(3 * f + k)] = vert;
            c.P.push_back(p);
            c.regular.push_back(1); c.boundary.push_back(f2 == -1); c.startFace.push_back(4 * f + 3);
        }
    for (int v = 0; v < nv; ++v) {                                                              // :319-324
        const int sf = m.startFace[size_t(v)];
        c.startFace[size_t(v)] = 4 * sf + m.vnum(sf, v);
    }
    c.fv.assign(size_t(nf) * 12, -1); c.fn.assign(size_t(nf) * 12, -1);
    for (int f = 0; f < nf; ++f)
        for (int k = 0; k < 3; ++k) {
            const int nk = SubdivLevel::next(k), pk = SubdivLevel::prev(k), ck = 4 * f + k, c3 = 4 * f + 3, v = m.fv[size_t(3 * f + k)];
            c.fn[size_t(3 * c3 + k)] = 4 * f + nk;                                              // :326-340
            c.fn[size_t(3 * ck + nk)] = c3;
            int f2 = m.fn[size_t(3 * f + k)];
            c.fn[size_t(3 * ck + k)] = f2 != -1 ? 4 * f2 + m.vnum(f2, v) : -1;
            f2 = m.fn[size_t(3 * f + pk)];
            c.fn[size_t(3 * ck + pk)] = f2 != -1 ? 4 * f2 + m.vnum(f2, v) : -1;
            const int vert = edgeVert[size_t(3 * f + k)];                                       // :342-354
            c.fv[size_t(3 * ck + k)] = v;
            c.fv[size_t(3 * ck + nk)] = vert;
            c.fv[size_t(3 * (4 * f + nk) + k)] = vert;
            c.fv[size_t(3 * c3 + k)] = vert;
        }
    m = std::move(c);
}
}  // namespace refine

inline bool RefineLoopSubdiv(const ParamSet &ps, RefinedMesh *out) {
    using namespace refine;
    const int nlevels = ps.FindOneInt("nlevels", 3);                                            // CreateShape :481-494
    int nps = 0, nIndices = 0;
    const int *vi = ps.FindInt("indices", &nIndices);
    const Float3 *P = ps.FindPoint("P", &nps);
    if (!vi || !P) return false;
    ps.FindOneString("scheme", "loop");                                                         // "don't actually use this for now..."
    long long nfinal = nIndices / 3;                                                            // faces and vertices are ints here, as in the reference
    for (int i = 0; i < nlevels && nfinal <= (1LL << 28); ++i) nfinal *= 4;
    if (nfinal > (1LL << 28)) { Error("Shape \"loopsubdiv\": %d faces at nlevels %d are more than 2^28 triangles; shape ignored", nIndices / 3, nlevels); return false; }
    SubdivLevel m;
    if (!buildControlMesh(vi, nIndices / 3, P, nps, m)) return false;
    std::vector<Float3> ring;
    for (int i = 0; i < nlevels; ++i) subdivideOnce(m, ring);
    // limit positions :360-370, from the last level's positions; the tangents below read the limit positions
    const int nv = m.nverts();
    std::vector<Float3> limit((size_t(nv)));
    for (int v = 0; v < nv; ++v)
        limit[size_t(v)] = m.boundary[size_t(v)] ? m.weightBoundary(v, 1.f / 5.f, ring) : m.weightOneRing(v, loopGamma(m.valence(v, ring)), ring);
    m.P = limit;
    out->N.resize(size_t(nv)); out->uv.clear();
    for (int v = 0; v < nv; ++v) {                                                              // :376-415
        Float3 S{0, 0, 0}, T{0, 0, 0};
        const int valence = m.oneRing(v, ring);
        const Float3 *R = ring.data();
        if (!m.boundary[size_t(v)]) {
            for (int k = 0; k < valence; ++k) {                                                 // float throughout: the reference's M_PI is a float (pbrt.h:204)
                S = add(S, mul(cosf(2.f * kPi * k / valence), R[k]));
                T = add(T, mul(sinf(2.f * kPi * k / valence), R[k]));
            }
        } else {
            S = sub(R[valence - 1], R[0]);
            if (valence == 2) T = sub(add(R[0], R[1]), mul(2, m.P[size_t(v)]));
            else if (valence == 3) T = sub(R[1], m.P[size_t(v)]);
            else if (valence == 4)
                T = add(add(add(add(mul(-1, R[0]), mul(2, R[1])), mul(2, R[2])), mul(-1, R[3])), mul(-2, m.P[size_t(v)]));
            else {
                const float theta = kPi / float(valence - 1);
                T = mul(sinf(theta), add(R[0], R[valence - 1]));
                for (int k = 1; k < valence - 1; ++k) {
                    const float wt = (2 * cosf(theta) - 2) * sinf(k * theta);
                    T = add(T, mul(wt, R[k]));
                }
                T = Float3{-T.x, -T.y, -T.z};
            }
        }
        out->N[size_t(v)] = cross(S, T);                                                        // :414: not normalised
    }
    out->P.swap(m.P);
    out->indices.swap(m.fv);
    return true;
}

}  // namespace pbrthip
