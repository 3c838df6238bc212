// What arctic_gltf_upload asks of a renderer, in order: built by tests/test_gltf_materials.py from host/gltf_loader.cpp itself with the two
// renderer entry points it may call replaced by recorders (any other renderer symbol would fail to link).  Prints one line per call.
#include <cstdio>

#include "../../include/arctic_gltf.h"

static int n_materials = 0, n_meshes = 0;

extern "C" {
int arctic_create_material(ArcticRenderer *, const void *d, uint32_t dw, uint32_t dh, const void *n, uint32_t nw, uint32_t nh, const void *m, uint32_t mw, uint32_t mh) {
    std::printf("create_material %u %u %u %u %u %u %d\n", dw, dh, nw, nh, mw, mh, d && n && m ? 1 : 0);
    return n_materials++;
}
int arctic_create_mesh(ArcticRenderer *, const ArcticVertex *, uint64_t nv, const uint32_t *, uint64_t ni, uint64_t material) {
    std::printf("create_mesh %llu %llu %llu\n", (unsigned long long)nv, (unsigned long long)ni, (unsigned long long)material);
    return n_meshes++;
}
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    char err[512] = "";
    ArcticGltf *g = arctic_gltf_load(argv[1], err, sizeof err);
    if (!g) { std::printf("refused %s\n", err); return 1; }
    int dummy = 0;   // the loader hands the handle through, it never looks inside
    const int rc = arctic_gltf_upload(g, reinterpret_cast<ArcticRenderer *>(&dummy));
    std::printf("upload %d\n", rc);
    arctic_gltf_free(g);
    return 0;
}
