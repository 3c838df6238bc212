// Sanitizer driver for the skins and animations of the scene-loader stand-in (glTF files are untrusted input).
// Built by tests/test_gltf_skins_malformed.py with -fsanitize=address,undefined from host/gltf_loader.cpp itself (the two renderer entry points
// arctic_gltf_upload needs are stubbed: no HIP library, CPU only).  Every argument is a glTF file: it is loaded, and every skin is posed with
// every animation (and at rest) at times before, inside and after the samplers' range.  A file must either be refused with a message -- by the
// loader or by the pose -- or give finite matrices; prints one line per file, and exits 1 on a pose that is neither.
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
        uint64_t posed = 0;
        for (uint64_t m = 0; m < arctic_gltf_mesh_count(g); ++m) {   // the records the loader hands out must be the library's idea of valid
            const ArcticSkinVertex *skin = nullptr;
            uint64_t n = 0; int64_t k = -1; uint32_t n_joints = 0;
            if (arctic_gltf_mesh_skin(g, m, &skin, &n, &k, &n_joints) != 0) { std::printf("BAD: mesh_skin failed\n"); ++bad; continue; }
            if (k < 0) continue;
            for (uint64_t v = 0; v < n; ++v)
                for (int c = 0; c < 4; ++c)
                    if (skin[v].joints[c] >= n_joints || !std::isfinite(skin[v].weights[c])) { std::printf("BAD: mesh %llu vertex %llu\n", (unsigned long long)m, (unsigned long long)v); ++bad; }
        }
        for (uint64_t s = 0; s < arctic_gltf_skin_count(g); ++s) {
            std::vector<float> out(16 * arctic_gltf_skin_joint_count(g, s));
            for (int64_t a = -1; a < (int64_t)arctic_gltf_animation_count(g); ++a) {
                const double d = a < 0 ? 0.0 : arctic_gltf_animation_duration(g, (uint64_t)a);
                for (double t : {-1.0, 0.0, 0.37 * d, 0.5 * d, d, d + 5.0}) {
                    for (float &x : out) x = NAN;
                    if (arctic_gltf_pose(g, s, a, t, out.data()) != 0) {
                        refusal = arctic_gltf_last_error(g);
                        if (refusal.empty()) { std::printf("BAD: a pose refused without a message\n"); ++bad; }
                        continue;
                    }
                    ++posed;
                    for (float x : out) if (!std::isfinite(x)) { std::printf("BAD: skin %llu animation %lld time %g: not finite\n", (unsigned long long)s, (long long)a, t); ++bad; break; }
                }
            }
        }
        if (!refusal.empty()) std::printf("refused %s (pose) %s\n", argv[i], refusal.c_str());
        else std::printf("ok      %s %llu poses\n", argv[i], (unsigned long long)posed);
        arctic_gltf_free(g);
    }
    return bad ? 1 : 0;
}
