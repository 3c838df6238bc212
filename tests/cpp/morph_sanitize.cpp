// Sanitizer driver for the morph targets, sparse accessors and weights animations of the scene-loader stand-in (glTF files are untrusted input).
// Built by tests/test_gltf_morph_malformed.py with -fsanitize=address,undefined from host/gltf_loader.cpp itself (the two renderer entry points
// arctic_gltf_upload needs are stubbed: no HIP library, CPU only).  Every argument is a glTF file: it is loaded, every mesh's delta records are
// read through, and every mesh's weights are evaluated under every animation (and at rest) at times before, inside and after the samplers'
// range.  A file must either be refused with a message -- by the loader or by the evaluation -- or give finite deltas and weights; prints one
// line per file, and exits 1 on anything else.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/arctic_gltf.h"

extern "C" {
int arctic_create_material(ArcticRenderer *, const void *, uint32_t, uint32_t, const void *, uint32_t, uint32_t, const void *, uint32_t, uint32_t) { return -1; }
int arctic_create_mesh(ArcticRenderer *, const ArcticVertex *, uint64_t, const uint32_t *, uint64_t, uint64_t) { return -1; }
}

int main(int argc, char **argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        char err[512] = "";
        ArcticGltf *g = arctic_gltf_load(argv[i], err, sizeof err);
        if (!g) {
            std::printf("refused %s %s\n", argv[i], err);
            if (!err[0]) { std::printf("BAD: refused without a message\n"); ++bad; }
            continue;
        }
        std::string refusal;
        uint64_t evaluated = 0, morphed = 0;
        for (uint64_t m = 0; m < arctic_gltf_mesh_count(g); ++m) {
            const ArcticMorphDelta *deltas = nullptr;
            uint64_t n = 0; uint32_t n_targets = 0;
            if (arctic_gltf_mesh_morph(g, m, &deltas, &n, &n_targets) != 0) { std::printf("BAD: mesh_morph failed\n"); ++bad; continue; }
            const ArcticVertex *v = nullptr; const uint32_t *ix = nullptr;
            uint64_t nv = 0, ni = 0, mat = 0;
            if (arctic_gltf_mesh(g, m, &v, &nv, &ix, &ni, &mat) != 0) { std::printf("BAD: mesh failed\n"); ++bad; continue; }
            if (!n_targets) continue;
            ++morphed;
            if (n != nv || !deltas) { std::printf("BAD: mesh %llu: %llu delta records per target for %llu vertices\n", (unsigned long long)m, (unsigned long long)n, (unsigned long long)nv); ++bad; continue; }
            const float *f = reinterpret_cast<const float *>(deltas);   // the records the loader hands out must be the library's idea of valid
            for (uint64_t k = 0; k < (uint64_t)n_targets * n * 12; ++k) if (!std::isfinite(f[k])) { std::printf("BAD: mesh %llu: a delta is not finite\n", (unsigned long long)m); ++bad; break; }
            std::vector<float> out(n_targets);
            for (int64_t a = -1; a < (int64_t)arctic_gltf_animation_count(g); ++a) {
                const double d = a < 0 ? 0.0 : arctic_gltf_animation_duration(g, (uint64_t)a);
                for (double t : {-1.0, 0.0, 0.37 * d, 0.5 * d, d, d + 5.0}) {
                    for (float &x : out) x = NAN;
                    if (arctic_gltf_morph_weights(g, m, a, t, out.data()) != 0) {
                        refusal = arctic_gltf_last_error(g);
                        if (refusal.empty()) { std::printf("BAD: weights refused without a message\n"); ++bad; }
                        continue;
                    }
                    ++evaluated;
                    for (float x : out) if (!std::isfinite(x)) { std::printf("BAD: mesh %llu animation %lld time %g: not finite\n", (unsigned long long)m, (long long)a, t); ++bad; break; }
                }
            }
        }
        if (!refusal.empty()) std::printf("refused %s (weights) %s\n", argv[i], refusal.c_str());
        else std::printf("ok      %s %llu morphed meshes, %llu evaluations\n", argv[i], (unsigned long long)morphed, (unsigned long long)evaluated);
        arctic_gltf_free(g);
    }
    return bad ? 1 : 0;
}
