// hit_attributes_sanitize.cpp -- the host arbiter of the hit attributes (arctic-renderer_amd/csrc/hit_attributes.cpp, hit_attributes.h, on
// ray_query.h) under -fsanitize=address,undefined, in a program of its own (tests/test_hit_reference.py builds and runs it; it is never loaded
// into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/hit_attributes_sanitize.cpp \
//       arctic-renderer_amd/csrc/hit_attributes.cpp
// With two arguments it reads a scene the test wrote -- per object its mesh, trs and material, then the sun's matrix and the hit records -- chains
// arctic_interpolate_hits over the objects and writes attributes and materials for the test to compare with tests/hit_reference.py.  In either
// mode it runs its own cases first: no hit, no mesh, every index out of range, prims below and beyond the object's range, NaN and infinite
// vertices, u and v, coordinates of 1e30, zero-length frame vectors; buffers are sized exactly, so a read or write past an end is caught.  Then
// the refusals, each of which must leave the outputs untouched.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/hit_attributes.h"
#include "../../include/arctic_hip.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
static void bad(const std::string &name, const char *why) { std::printf("BAD %s: %s\n", name.c_str(), why); ++failures; }
static const float p_inf = std::numeric_limits<float>::infinity(), q_nan = std::numeric_limits<float>::quiet_NaN();
static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

struct Object { std::vector<ArcticVertex> v; std::vector<uint32_t> ix; float trs[16]; uint32_t material; };

// the chain the header describes: outputs start as zeros and 0xFFFFFFFF, every object fills the hits of its own prims
static bool chain(const std::vector<Object> &objs, const float *lpv, const std::vector<ArcticHit> &hits, std::vector<float> &attrs, std::vector<uint32_t> &mat) {
    attrs.assign(hits.size() * 18, 0.0f);
    mat.assign(hits.size(), 0xFFFFFFFFu);
    uint64_t prim = 0;
    for (const Object &o : objs) {
        if (arctic_interpolate_hits(o.v.data(), o.v.size(), o.ix.data(), o.ix.size(), o.trs, lpv, o.material, prim, hits.data(), hits.size(), attrs.data(), mat.data()) != ARCTIC_OK)
            return false;
        prim += o.ix.size() / 3;
    }
    return true;
}

static Object random_object(std::mt19937 &g, size_t n_vertices, size_t n_triangles, float scale, uint32_t material) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    Object o;
    o.v.resize(n_vertices);
    for (ArcticVertex &v : o.v) {
        float *f = v.position;
        for (int k = 0; k < 14; ++k) f[k] = u(g);
        for (int k = 0; k < 3; ++k) f[k] *= scale;
    }
    o.ix.resize(3 * n_triangles);
    for (uint32_t &i : o.ix) i = n_vertices ? (uint32_t)(g() % n_vertices) : 0u;
    for (int k = 0; k < 16; ++k) o.trs[k] = identity[k] + 0.3f * u(g) * (k % 4 != 3);
    o.material = material;
    return o;
}

static void run(const std::string &name, std::vector<Object> objs, size_t n_hits, bool odd) {
    std::mt19937 g(777);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    uint64_t n_prims = 0;
    for (const Object &o : objs) n_prims += o.ix.size() / 3;
    std::vector<ArcticHit> hits(n_hits);
    for (size_t k = 0; k < n_hits; ++k) {
        ArcticHit &h = hits[k];
        h.t = 1.0f; h.u = u(g); h.v = (1.0f - h.u) * u(g);
        h.prim = n_prims ? (uint32_t)(g() % n_prims) : 0u;
        switch (odd ? k % 8 : 99) {
        case 0: h.prim = 0xFFFFFFFFu; break;
        case 1: h.prim = (uint32_t)n_prims; break;
        case 2: h.prim = 0xFFFFFFFEu; break;
        case 3: h.u = q_nan; break;
        case 4: h.v = p_inf; break;
        case 5: h.u = -3.0f; h.v = 7.0f; break;
        default: break;
        }
    }
    float lpv[16];
    for (int k = 0; k < 16; ++k) lpv[k] = identity[k] * 0.05f;
    std::vector<float> attrs;
    std::vector<uint32_t> mat;
    if (!chain(objs, lpv, hits, attrs, mat)) return bad(name, "refused");
    size_t resolved = 0;
    for (size_t k = 0; k < n_hits; ++k) {
        const bool none = mat[k] == 0xFFFFFFFFu;
        resolved += !none;
        if (hits[k].prim >= n_prims && !none) return bad(name, "a prim the scene does not have resolved");
        if (none) for (int j = 0; j < 18; ++j) if (std::memcmp(&attrs[18 * k + j], &identity[1], 4) != 0) return bad(name, "an unresolved hit has attributes");
    }
    std::printf("ok %s: %zu hits, %zu resolved, %llu prims\n", name.c_str(), n_hits, resolved, (unsigned long long)n_prims);
}

template <class T> static bool get(std::FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static void from_file(const char *in, const char *out) {
    std::FILE *f = std::fopen(in, "rb");
    if (!f) return bad("scene", "cannot open the input");
    uint64_t n_obj = 0, n_hits = 0;
    bool ok = get(f, &n_obj, 1);
    std::vector<Object> objs((size_t)n_obj);
    for (Object &o : objs) {
        uint64_t nv = 0, ni = 0;
        ok = ok && get(f, &nv, 1) && get(f, &ni, 1) && get(f, o.trs, 16) && get(f, &o.material, 1);
        if (!ok) break;
        o.v.resize((size_t)nv); o.ix.resize((size_t)ni);
        ok = get(f, o.v.data(), o.v.size()) && get(f, o.ix.data(), o.ix.size());
    }
    float lpv[16];
    ok = ok && get(f, lpv, 16) && get(f, &n_hits, 1);
    std::vector<ArcticHit> hits(ok ? (size_t)n_hits : 0);
    ok = ok && get(f, hits.data(), hits.size());
    std::fclose(f);
    if (!ok) return bad("scene", "the input is short");
    std::vector<float> attrs;
    std::vector<uint32_t> mat;
    if (!chain(objs, lpv, hits, attrs, mat)) return bad("scene", "refused");
    std::FILE *o = std::fopen(out, "wb");
    if (!o || std::fwrite(attrs.data(), 4, attrs.size(), o) != attrs.size() || std::fwrite(mat.data(), 4, mat.size(), o) != mat.size()) bad("scene", "cannot write the output");
    if (o) std::fclose(o);
    if (!failures) std::printf("ok scene: %llu objects, %llu hits\n", (unsigned long long)n_obj, (unsigned long long)n_hits);
}

int main(int argc, char **argv) {
    std::mt19937 g(99);
    run("empty", {}, 100, true);
    run("no-hits", {random_object(g, 10, 10, 1.0f, 0)}, 0, false);
    run("one-triangle", {random_object(g, 3, 1, 1.0f, 5)}, 64, true);
    run("three-objects", {random_object(g, 50, 80, 1.0f, 0), random_object(g, 7, 3, 1.0f, 1), random_object(g, 200, 400, 1.0f, 2)}, 2000, true);
    run("large-20000", {random_object(g, 30000, 20000, 1.0f, 3)}, 5000, false);
    run("no-vertices", {random_object(g, 0, 10, 1.0f, 0)}, 100, true);   // every index is out of range: nothing resolves, nothing is read
    { Object o = random_object(g, 20, 30, 1.0f, 1); for (size_t k = 0; k < o.ix.size(); k += 7) o.ix[k] = 20u + (uint32_t)k; run("indices-out-of-range", {o, random_object(g, 9, 9, 1.0f, 2)}, 500, true); }
    { Object o = random_object(g, 40, 60, 1.0f, 0); for (size_t k = 0; k < o.v.size(); k += 3) { o.v[k].position[k % 3] = (k % 2) ? q_nan : p_inf; o.v[k].normal[0] = q_nan; } run("nan-and-inf-vertices", {o}, 500, true); }
    { Object o = random_object(g, 40, 60, 1.0f, 0); for (ArcticVertex &v : o.v) v.tangent[0] = v.tangent[1] = v.tangent[2] = 0.0f; run("zero-length-frames", {o}, 300, false); }
    run("huge-1e30", {random_object(g, 100, 100, 1e30f, 0)}, 300, true);
    { Object o = random_object(g, 3, 1, 1.0f, 0); o.ix.push_back(0); o.ix.push_back(1); run("index-count-not-a-multiple-of-3", {o}, 64, true); }

    // refusals: each leaves the outputs as they were
    const Object one = random_object(g, 3, 1, 1.0f, 4);
    const ArcticHit hit = {1.0f, 0.25f, 0.25f, 0u};
    float a[18];
    uint32_t m = 77;
    for (float &x : a) x = 77.0f;
    int refused = 0, tried = 0;
    auto untouched = [&]() { bool same = m == 77; for (float x : a) same = same && x == 77.0f; return same; };
    auto expect = [&](int rc, int want) { ++tried; refused += rc == want && untouched(); };
    const ArcticVertex *v = one.v.data();
    const uint32_t *ix = one.ix.data();
    expect(arctic_interpolate_hits(nullptr, 3, ix, 3, one.trs, identity, 4, 0, &hit, 1, a, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, nullptr, 3, one.trs, identity, 4, 0, &hit, 1, a, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, ix, 3, nullptr, identity, 4, 0, &hit, 1, a, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, nullptr, 4, 0, &hit, 1, a, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 0, nullptr, 1, a, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 0, &hit, 1, nullptr, &m), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 0, &hit, 1, a, nullptr), ARCTIC_E_INVALID);
    expect(arctic_interpolate_hits(v, 0x100000000ull, ix, 3, one.trs, identity, 4, 0, &hit, 1, a, &m), ARCTIC_E_CAPACITY);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 0xFFFFFFFEull, &hit, 1, a, &m), ARCTIC_E_CAPACITY);
    expect(arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 1, &hit, 1, a, &m), ARCTIC_OK);   // another object's prim: accepted, and left as it is
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    if (arctic_interpolate_hits(nullptr, 0, nullptr, 0, one.trs, identity, 0, 0, nullptr, 0, nullptr, nullptr) != ARCTIC_OK) bad("nothing-to-do", "refused");
    else std::printf("ok nothing-to-do\n");
    if (arctic_interpolate_hits(v, 3, ix, 3, one.trs, identity, 4, 0, &hit, 1, a, &m) != ARCTIC_OK || m != 4 || a[0] == 77.0f) bad("the-good-call", "nothing written");
    else std::printf("ok the-good-call\n");
    if (argc == 3) from_file(argv[1], argv[2]);
    return failures ? 1 : 0;
}
